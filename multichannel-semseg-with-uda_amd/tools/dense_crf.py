#!/usr/bin/env python3
"""Dense-CRF post-processing of saved logits -- the reference's tools/crf.py with its command line, the mean-field passes on the
MI355X (``ops.dense_crf``: the pairwise sums are exact, not pydensecrf's lattice approximation of them).

    python tools/dense_crf.py PROB_INDIR OUTDIR [--prob_outdir DIR] [--outimg_shape W H] [--raw_img_indir DIR]
                              [--n_iters 10] [--sxy_gaussian 1 1] [--compat_gaussian 4] [--sxy_bilateral 49 49]
                              [--srgb_bilateral 13 13 13] [--compat_bilateral 5] [--n_used K] [--gt_dir DIR --n_class K] [-b N]

reads every ``<name>.npy`` of PROB_INDIR (fp32 logits [C,H,W], what the testers write under ``--saves_prob``) and writes
``OUTDIR/<name>.png``.  Where the reference's defaults are particular to its data they are options here:
``--outimg_shape`` keeps the size of the logits unless given (the reference resizes to 1280 x 720, crf.py:77), ``--n_used`` takes the
arg-max over all classes unless given (the reference over the first 19, crf.py:112).  ``--raw_img_indir`` holds ``<name>.png``, resized
NEAREST to the logits' size (crf.py:101-107); without it only the Gaussian term is used.  With ``--gt_dir`` (label PNGs of the same names at
the logits' size, background 255) ``eval_result_crf.json`` = {"before": ..., "after": ...} is written beside OUTDIR."""
import argparse
import os
import sys

import numpy as np

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if sys.path[:1] != [PKG]:  # in FRONT of this file's own directory: ``import dense_crf`` below is the package's module, not this tool
    sys.path.insert(0, PKG)


def get_parser():
    parser = argparse.ArgumentParser(description="Postprocessing CRF")
    parser.add_argument("prob_indir", type=str, help="input directory that contains npys in which probability tensors exist")
    parser.add_argument("outdir", type=str, help="output directory that contains predicted labels(pngs)")
    parser.add_argument("--prob_outdir", default=None, help="also save the refined probabilities [C,H,W] as npy here")
    parser.add_argument("--outimg_shape", default=None, nargs=2, type=int, help="W H of the label PNGs (default: the logits' size)")
    parser.add_argument("--raw_img_indir", type=str, default=None, help="input directory that contains raw imgs: the bilateral term")
    parser.add_argument("--n_iters", type=int, default=10)
    parser.add_argument("--sxy_gaussian", type=float, nargs=2, default=(1, 1))
    parser.add_argument("--compat_gaussian", type=float, default=4)
    parser.add_argument("--sxy_bilateral", type=float, nargs=2, default=(49, 49))
    parser.add_argument("--srgb_bilateral", type=float, nargs=3, default=(13, 13, 13))
    parser.add_argument("--compat_bilateral", type=float, default=5)
    parser.add_argument("--n_used", type=int, default=None, help="arg-max over the first K classes (default: all)")
    parser.add_argument("--gt_dir", type=str, default=None, help="ground-truth label PNGs: also write eval_result_crf.json")
    parser.add_argument("--n_class", type=int, default=None, help="number of classes of the evaluation (with --gt_dir)")
    parser.add_argument("-b", "--batch_size", type=int, default=1, help="images of equal size refined per call")
    return parser


def main(argv=None):
    args = get_parser().parse_args(argv)
    if args.gt_dir is not None and (args.n_class is None or args.n_class <= 0):
        raise SystemExit("--gt_dir needs --n_class")
    if args.batch_size <= 0:
        raise SystemExit("--batch_size must be positive")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("this tool runs on an MI355X: the HIP kernels are the only implementation (no CPU fallback)")
    from PIL import Image
    import dense_crf
    dev = torch.device("cuda", torch.cuda.current_device())
    crf = dense_crf.DenseCRF(args.outdir, args.prob_outdir, args.outimg_shape, args.n_used, args.n_class, dev, n_iters=args.n_iters,
                             sxy_gaussian=tuple(args.sxy_gaussian), compat_gaussian=args.compat_gaussian,
                             sxy_bilateral=tuple(args.sxy_bilateral), srgb_bilateral=tuple(args.srgb_bilateral),
                             compat_bilateral=args.compat_bilateral)
    print("Result will be saved in %s" % crf.outdir)

    batch = []  # (name, logits, rgb or None, ground truth or None), all of one size

    def flush():
        if not batch:
            return
        logits = torch.from_numpy(np.stack([b[1] for b in batch])).to(dev)
        rgb = np.stack([b[2] for b in batch]) if args.raw_img_indir else None
        q, labels = crf.refine(logits, rgb)
        crf.save(labels, [b[0] for b in batch], q)
        if args.gt_dir is not None:
            crf.update(crf.plain_labels(logits), labels, np.stack([b[3] for b in batch]))
        del batch[:]

    for one_file in sorted(os.listdir(args.prob_indir)):
        if not one_file.endswith(".npy"):
            continue
        name = one_file[:-4]
        z = np.load(os.path.join(args.prob_indir, one_file))
        if z.ndim != 3:
            raise ValueError("%s holds an array of shape %s, not logits [C,H,W]" % (os.path.join(args.prob_indir, one_file), z.shape))
        z = np.ascontiguousarray(z, dtype=np.float32)
        _, h, w = z.shape
        rgb = None
        if args.raw_img_indir:
            img = Image.open(os.path.join(args.raw_img_indir, name + ".png")).convert("RGB").resize((w, h), Image.NEAREST)
            rgb = np.array(img, dtype=np.uint8)
        gt = None
        if args.gt_dir is not None:
            gt = np.array(Image.open(os.path.join(args.gt_dir, name + ".png")))
            if gt.shape != (h, w) or gt.dtype != np.uint8:
                raise ValueError("ground truth %s is not an 8-bit %d x %d label image" % (os.path.join(args.gt_dir, name + ".png"), w, h))
        if batch and (len(batch) >= args.batch_size or batch[0][1].shape != z.shape):
            flush()
        batch.append((name, z, rgb, gt))
    flush()
    crf.finish()
    print("Finished!!!")
    return crf.outdir


if __name__ == "__main__":
    main()
