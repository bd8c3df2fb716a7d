#!/usr/bin/env python3
"""Fill the holes of raw depth maps by colorization guided by the RGB image, on the MI355X (``ops.fill_depth``; the definition is
DESIGN.md section 4.16) -- the NYU toolbox's ``fill_depth_colorization`` step, which stands in front of the HHA encoding.

    python tools/fill_depth.py DEPTH_DIR RGB_DIR OUT_DIR [--unit_m 0.001] [--alpha 1] [--rtol 1e-10] [--max_iter 4000]
                               [--max_valid_m M] [--keep_known] [-b N]

reads every 16-bit single-channel ``<name>.png`` of DEPTH_DIR (a value is ``--unit_m`` metres; 0 is a missing measurement; with
``--max_valid_m`` a value of at least that many metres is missing too) and the RGB image of the same stem in RGB_DIR (.png, .jpg, .jpeg
or .ppm), and writes ``OUT_DIR/<name>.png`` as a 16-bit PNG in the input's unit: ``floor(cm / (100 unit_m) + 0.5)`` clipped to 65535.
Files of equal size are solved ``-b`` at a time.  Prints ``name iterations residual status`` per file and exits 1 after the last file if
an image was neither ``converged`` nor ``empty``."""
import argparse
import os
import sys

import numpy as np

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if sys.path[:1] != [PKG]:
    sys.path.insert(0, PKG)

RGB_SUFFIXES = (".png", ".jpg", ".jpeg", ".ppm")


def add_solver_arguments(parser):
    """the flags tools/depth_to_hha.py --fill shares"""
    parser.add_argument("--alpha", type=float, default=1.0, help="weight of the measured depth in the system (the toolbox's is 1)")
    parser.add_argument("--rtol", type=float, default=1e-10, help="stop when the true residual is at most rtol |b|")
    parser.add_argument("--max_iter", type=int, default=4000, help="iteration limit per image")
    parser.add_argument("--max_valid_m", type=float, default=None, help="a depth of at least this many metres counts as missing")
    parser.add_argument("--keep_known", action="store_true", help="known pixels keep their measured value")


def solver_kwargs(args):
    """the keyword arguments of ``ops.fill_depth`` the flags stand for; SystemExit on values it would refuse"""
    if not (args.alpha > 0 and args.rtol > 0 and args.max_iter >= 0):
        raise SystemExit("--alpha and --rtol must be positive, --max_iter not negative")
    if args.max_valid_m is not None and not args.max_valid_m > 0:
        raise SystemExit("--max_valid_m must be positive")
    return dict(alpha=args.alpha, rtol=args.rtol, max_iter=args.max_iter, keep_known=args.keep_known,
                max_valid_cm=None if args.max_valid_m is None else 100.0 * args.max_valid_m)


def get_parser():
    parser = argparse.ArgumentParser(description="Fill the holes of depth maps (16-bit PNGs), guided by their RGB images")
    parser.add_argument("depth_dir", type=str, help="input directory of 16-bit single-channel depth PNGs")
    parser.add_argument("rgb_dir", type=str, help="directory of the RGB images (same stems)")
    parser.add_argument("out_dir", type=str, help="output directory of the filled depth maps (16-bit PNGs of the same names)")
    parser.add_argument("--unit_m", type=float, default=0.001, help="metres per depth unit (0.001: millimetres)")
    add_solver_arguments(parser)
    parser.add_argument("-b", "--batch_size", type=int, default=1, help="files of equal size solved per call")
    return parser


def read_depth(path):
    """a 16-bit single-channel PNG as uint16 [H,W]"""
    from PIL import Image
    img = Image.open(path)
    if img.mode not in ("I;16", "I;16B", "I;16L", "I"):
        raise ValueError("%s is not a 16-bit single-channel image (mode %s)" % (path, img.mode))
    arr = np.array(img)
    if arr.ndim != 2 or arr.min() < 0 or arr.max() > 65535:
        raise ValueError("%s does not hold 16-bit depth values" % path)
    return arr.astype(np.uint16)


def read_rgb(rgb_dir, depth_name, shape):
    """the RGB image that goes with a depth file, uint8 [H,W,3]"""
    from PIL import Image
    stem = os.path.splitext(depth_name)[0]
    for suffix in RGB_SUFFIXES:
        for name in (stem + suffix, stem + suffix.upper()):
            path = os.path.join(rgb_dir, name)
            if os.path.exists(path):
                arr = np.array(Image.open(path).convert("RGB"))
                if arr.shape[:2] != tuple(shape):
                    raise ValueError("%s is %d x %d, its depth map %d x %d" % ((path,) + arr.shape[:2] + tuple(shape)))
                return arr
    raise FileNotFoundError("no RGB image %s.{png,jpg,jpeg,ppm} in %s" % (stem, rgb_dir))


def to_units(filled_cm, unit_m):
    """fp32 centimetres -> uint16 in units of ``unit_m`` metres: floor(cm / (100 unit_m) + 0.5), clipped to [0, 65535]"""
    return np.clip(np.floor(np.asarray(filled_cm, np.float64) / (100.0 * unit_m) + 0.5), 0, 65535).astype(np.uint16)


def batches(depth_dir, rgb_dir, batch_size):
    """lists of (file name, uint16 depth [H,W], uint8 RGB [H,W,3] or None without ``rgb_dir``), each of one size, in name order"""
    batch = []
    for one_file in sorted(os.listdir(depth_dir)):
        if not one_file.lower().endswith(".png"):
            continue
        d = read_depth(os.path.join(depth_dir, one_file))
        if batch and (len(batch) >= batch_size or batch[0][1].shape != d.shape):
            yield batch
            batch = []
        batch.append((one_file, d, read_rgb(rgb_dir, one_file, d.shape) if rgb_dir else None))
    if batch:
        yield batch


def main(argv=None):
    args = get_parser().parse_args(argv)
    if args.batch_size <= 0:
        raise SystemExit("--batch_size must be positive")
    if not args.unit_m > 0:
        raise SystemExit("--unit_m must be positive")
    kw = solver_kwargs(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("this tool runs on an MI355X: the HIP kernels are the only implementation (no CPU fallback)")
    from PIL import Image
    from mcdseg import ops
    dev = torch.device("cuda", torch.cuda.current_device())
    os.makedirs(args.out_dir, exist_ok=True)
    failed = 0
    for batch in batches(args.depth_dir, args.rgb_dir, args.batch_size):
        depth = torch.from_numpy(np.stack([b[1] for b in batch]).astype(np.int32)).to(dev)
        rgb = torch.from_numpy(np.stack([b[2] for b in batch])).to(dev)
        filled, parts = ops.fill_depth(rgb, depth, unit_m=args.unit_m, return_parts=True, **kw)
        units = to_units(filled.cpu().numpy(), args.unit_m)
        for k, (name, _, _) in enumerate(batch):
            Image.fromarray(units[k]).save(os.path.join(args.out_dir, name))
            status = int(parts["status"][k])
            print("%s %d %.3e %s" % (name, int(parts["iterations"][k]), float(parts["residual"][k]), ops.FILL_STATUS_NAMES[status]))
            failed += status not in (ops.FILL_CONVERGED, ops.FILL_EMPTY)
    if failed:
        raise SystemExit(1)
    return args.out_dir


if __name__ == "__main__":
    main()
