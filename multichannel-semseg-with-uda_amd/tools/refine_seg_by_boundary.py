#!/usr/bin/env python3
"""Refine label PNGs by boundary PNGs -- the reference's three commands (sample_scripts/refine_seg_by_boundary.sh:15-17:
tools/binalize_boundary.py, MATLAB's bwboundaries through tools/apply_bwboundary.m, tools/refine_seg_by_bwboundary.py) as one, with
the labelling and the vote on the MI355X (``ops.refine_labels_by_boundary``).

    python tools/refine_seg_by_boundary.py SEGDIR BOUNDARY_DIR [--thre 50] [--min_thre 500] [--max_thre 79333]
                                           [--gt_dir DIR --n_class K] [-b N]

writes ``refined_label/<name>`` next to SEGDIR for every file of SEGDIR (refine_seg_by_bwboundary.py:13-16) and, with ``--gt_dir``
(label PNGs of the same names and size, background 255), ``eval_result_refined.json`` = {"before": ..., "after": ...} beside it.  The
palette images (``refined_vis/``) are outside this build."""
import argparse
import os
import sys

import numpy as np

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if PKG not in sys.path:
    sys.path.insert(0, PKG)


def get_parser():
    parser = argparse.ArgumentParser(description="Refine segmentation results by boundary detection results")
    parser.add_argument("segdir", type=str, help="Directory that contains segmentation results")
    parser.add_argument("boundary_dir", type=str, help="Raw boundary directory name")
    parser.add_argument("--thre", type=int, default=50, help="threshold to binalize. Set from 0 to 255")
    parser.add_argument("--min_thre", type=int, default=500, help="the minimum number of pixel in a region")
    parser.add_argument("--max_thre", type=int, default=79333, help="the maximum number of pixel in a region")  # 425 * 560 / 3
    parser.add_argument("--gt_dir", type=str, default=None, help="ground-truth label PNGs: also write eval_result_refined.json")
    parser.add_argument("--n_class", type=int, default=None, help="number of classes of the evaluation (with --gt_dir)")
    parser.add_argument("-b", "--batch_size", type=int, default=8, help="images of equal size refined per call")
    return parser


def _read(path, what):
    from PIL import Image
    arr = np.array(Image.open(path))
    if arr.ndim != 2 or arr.dtype != np.uint8:
        raise ValueError("%s %s is not an 8-bit single-channel image" % (what, path))
    return arr


def main(argv=None):
    args = get_parser().parse_args(argv)
    if args.gt_dir is not None and (args.n_class is None or args.n_class <= 0):
        raise SystemExit("--gt_dir needs --n_class")
    if args.batch_size <= 0:
        raise SystemExit("--batch_size must be positive")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("this tool runs on an MI355X: the HIP kernels are the only implementation (no CPU fallback)")
    import boundary_refine
    dev = torch.device("cuda", torch.cuda.current_device())
    base = os.path.split(os.path.normpath(args.segdir))[0]
    refiner = boundary_refine.BoundaryRefiner(base, args.thre, args.min_thre, args.max_thre, args.n_class, dev)
    print("Result will be saved in %s" % refiner.outdir)

    batch = []  # (name, labels, boundary, ground truth or None), all of one size

    def flush():
        if not batch:
            return
        seg, bd = np.stack([b[1] for b in batch]), np.stack([b[2] for b in batch])
        seg_dev = torch.from_numpy(seg).to(dev)
        refined = refiner.refine(seg_dev, bd)
        refiner.save(refined, [b[0] for b in batch])
        if args.gt_dir is not None:
            refiner.update(seg_dev, refined, np.stack([b[3] for b in batch]))
        del batch[:]

    for name in sorted(os.listdir(args.segdir)):
        seg = _read(os.path.join(args.segdir, name), "label image")
        bd_fn = os.path.join(args.boundary_dir, name)
        if not os.path.exists(bd_fn):
            raise OSError("no boundary image for %s: %s does not exist" % (name, bd_fn))
        bd = _read(bd_fn, "boundary image")
        if bd.shape != seg.shape:
            raise ValueError("boundary image %s is %d x %d, its label image %d x %d" % (bd_fn, bd.shape[1], bd.shape[0], seg.shape[1], seg.shape[0]))
        gt = None
        if args.gt_dir is not None:
            gt = _read(os.path.join(args.gt_dir, name), "ground truth")
            if gt.shape != seg.shape:
                raise ValueError("ground truth %s is %d x %d, its label image %d x %d"
                                 % (os.path.join(args.gt_dir, name), gt.shape[1], gt.shape[0], seg.shape[1], seg.shape[0]))
        if batch and (len(batch) >= args.batch_size or batch[0][1].shape != seg.shape):
            flush()
        batch.append((name, seg, bd, gt))
    flush()
    refiner.finish()
    print("Finished!!!")
    return refiner.outdir


if __name__ == "__main__":
    main()
