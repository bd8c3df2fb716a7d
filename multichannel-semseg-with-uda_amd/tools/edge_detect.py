#!/usr/bin/env python3
"""Laplacian, Canny and Sobel edge maps of RGB images -- the reference's tools/edge_detect.py with its command line, the maps formed on
the MI355X (``ops.edge_maps``: OpenCV's published 8-bit algorithm, all integer; DESIGN.md section 4.15 -- equality with a particular
OpenCV build is not claimed).

    python tools/edge_detect.py RGBDIR [--min_canny_thre 100] [--max_canny_thre 200] [--kinds laplacian canny sobel]
                                [--outdir DIR] [-b 8]
                                [--refine SEGDIR [--thre 50 --min_thre 500 --max_thre 79333 --gt_dir DIR --n_class K]]

writes ``<parent of RGBDIR>/edges/{laplacian,canny,sobel}/<stem>.png`` (edge_detect.py:19-23; ``--outdir`` replaces the ``edges``
directory) for every file of RGBDIR.  Always PNG: the reference keeps the file's name, so a ``.jpg`` input is re-encoded lossily there,
which is not reproduced.

The thresholds do what the flags say: low = ``--min_canny_thre``, high = ``--max_canny_thre``.  The reference's own call,
``cv2.Canny(imgY, cv2.CV_64F, min, max)`` (edge_detect.py:44), passes its arguments one position too far: as far as the OpenCV binding
can be read, threshold1 becomes 6 (the value of CV_64F), threshold2 ``min_canny_thre``, and ``max_canny_thre`` lands in the ``edges``
slot.  That reading could not be verified; the reference's apparent behaviour stays reachable as
``--min_canny_thre 6 --max_canny_thre 100``.

With ``--refine SEGDIR`` the Canny maps stay on the device and go straight into the boundary refinement together with the label PNGs
``SEGDIR/<stem>.png`` -- sample_scripts/refine_seg_by_boundary.sh in one command: ``refined_label/`` and (with ``--gt_dir``)
``eval_result_refined.json`` are written next to SEGDIR exactly as ``tools/refine_seg_by_boundary.py SEGDIR <edges/canny>`` writes
them."""
import argparse
import os
import sys

import numpy as np

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if sys.path[:1] != [PKG]:  # in FRONT of this file's own directory: ``import edge_detect`` below is the package's module, not this tool
    sys.path.insert(0, PKG)

KINDS = ("laplacian", "canny", "sobel")


def get_parser():
    parser = argparse.ArgumentParser(description="Edge Detection (OpenCV's Laplacian, Canny and Sobel definitions on the device)")
    parser.add_argument("rgbdir", type=str, help="Directory contains rgb images")
    parser.add_argument("--min_canny_thre", type=int, default=100)
    parser.add_argument("--max_canny_thre", type=int, default=200)
    parser.add_argument("--kinds", type=str, nargs="+", default=list(KINDS), help="which maps to write: laplacian canny sobel")
    parser.add_argument("--outdir", type=str, default=None, help="directory of the maps (default: <parent of RGBDIR>/edges)")
    parser.add_argument("-b", "--batch_size", type=int, default=8, help="images of equal size per call")
    parser.add_argument("--refine", type=str, default=None, metavar="SEGDIR", help="also refine the label PNGs of SEGDIR by the Canny maps")
    parser.add_argument("--thre", type=int, default=50, help="threshold to binalize. Set from 0 to 255")
    parser.add_argument("--min_thre", type=int, default=500, help="the minimum number of pixel in a region")
    parser.add_argument("--max_thre", type=int, default=79333, help="the maximum number of pixel in a region")
    parser.add_argument("--gt_dir", type=str, default=None, help="ground-truth label PNGs: also write eval_result_refined.json")
    parser.add_argument("--n_class", type=int, default=None, help="number of classes of the evaluation (with --gt_dir)")
    return parser


def check_args(args):
    """the refusals that need no device; returns the kinds in the order of the reference's directories"""
    if args.batch_size <= 0:
        raise SystemExit("--batch_size must be positive")
    unknown = [k for k in args.kinds if k not in KINDS]
    if unknown:
        raise SystemExit("unknown kind %s: --kinds takes some of %s" % (", ".join(unknown), " ".join(KINDS)))
    if args.gt_dir is not None and args.refine is None:
        raise SystemExit("--gt_dir needs --refine")
    if args.gt_dir is not None and (args.n_class is None or args.n_class <= 0):
        raise SystemExit("--gt_dir needs --n_class")
    return tuple(k for k in KINDS if k in args.kinds)


def _read_label(path, what, like, of):
    from PIL import Image
    arr = np.array(Image.open(path))
    if arr.ndim != 2 or arr.dtype != np.uint8:
        raise ValueError("%s %s is not an 8-bit single-channel image" % (what, path))
    if arr.shape != like:
        raise ValueError("%s %s is %d x %d, the edge map of %s %d x %d" % (what, path, arr.shape[1], arr.shape[0], of, like[1], like[0]))
    return arr


def main(argv=None):
    args = get_parser().parse_args(argv)
    kinds = check_args(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("this tool runs on an MI355X: the HIP kernels are the only implementation (no CPU fallback)")
    import edge_detect
    dev = torch.device("cuda", torch.cuda.current_device())
    rgbdir = os.path.normpath(args.rgbdir)
    edge_dir = args.outdir if args.outdir is not None else os.path.join(os.path.split(rgbdir)[0], "edges")
    computed = kinds if (args.refine is None or "canny" in kinds) else kinds + ("canny",)
    detector = edge_detect.EdgeDetector(args.min_canny_thre, args.max_canny_thre, computed, dev)
    print("Result will be saved in %s" % edge_dir)
    refiner = None
    if args.refine is not None:
        import boundary_refine
        base = os.path.split(os.path.normpath(args.refine))[0]
        refiner = boundary_refine.BoundaryRefiner(base, args.thre, args.min_thre, args.max_thre, args.n_class, dev)
        print("Refined labels will be saved in %s" % refiner.outdir)

    paths = [os.path.join(rgbdir, fn) for fn in sorted(os.listdir(rgbdir))]
    for stems, rgb in edge_detect.batches(paths, args.batch_size):
        maps = detector.detect(rgb)
        detector.save({k: maps[k] for k in kinds}, stems, edge_dir)
        if refiner is None:
            continue
        shape = tuple(rgb.shape[1:3])
        names = [stem + ".png" for stem in stems]
        seg = np.stack([_read_label(os.path.join(args.refine, name), "label image", shape, stem) for name, stem in zip(names, stems)])
        seg_dev = torch.from_numpy(seg).to(dev)
        refined = refiner.refine(seg_dev, maps["canny"])
        refiner.save(refined, names)
        if args.gt_dir is not None:
            gt = np.stack([_read_label(os.path.join(args.gt_dir, name), "ground truth", shape, stem) for name, stem in zip(names, stems)])
            refiner.update(seg_dev, refined, gt)
    if refiner is not None:
        refiner.finish()
    print("Finished!!!")
    return edge_dir


if __name__ == "__main__":
    main()
