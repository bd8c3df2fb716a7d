#!/usr/bin/env python3
"""HHA images (horizontal disparity, height above ground, angle with gravity) from raw depth maps, on the MI355X (``ops.depth_to_hha``;
the definition is DESIGN.md section 4.13) -- the step the reference leaves to a third-party MATLAB release.

    python tools/depth_to_hha.py DEPTH_DIR OUT_DIR --camera FX FY CX CY [--unit_m 0.001] [-b N]

reads every 16-bit single-channel ``<name>.png`` of DEPTH_DIR (a value is ``--unit_m`` metres, 0.001 for NYUDv2 and Kinect PNGs; 0 is a
missing measurement) and writes ``OUT_DIR/<name>.png`` as an RGB PNG whose channels are disparity, height and angle.  ``--camera`` is the
pinhole model in pixels, for all files.  Files of equal size are encoded ``-b`` at a time.  Prints the estimated gravity direction (camera
coordinates, Y down the image) per file."""
import argparse
import os
import sys

import numpy as np

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if sys.path[:1] != [PKG]:
    sys.path.insert(0, PKG)


def get_parser():
    parser = argparse.ArgumentParser(description="Depth maps (16-bit PNGs) to HHA images")
    parser.add_argument("depth_dir", type=str, help="input directory of 16-bit single-channel depth PNGs")
    parser.add_argument("out_dir", type=str, help="output directory of the HHA images (RGB PNGs of the same names)")
    parser.add_argument("--camera", type=float, nargs=4, required=True, metavar=("FX", "FY", "CX", "CY"), help="pinhole camera, in pixels")
    parser.add_argument("--unit_m", type=float, default=0.001, help="metres per depth unit (0.001: millimetres)")
    parser.add_argument("-b", "--batch_size", type=int, default=1, help="files of equal size encoded per call")
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


def main(argv=None):
    args = get_parser().parse_args(argv)
    if args.batch_size <= 0:
        raise SystemExit("--batch_size must be positive")
    if not (args.unit_m > 0 and args.camera[0] > 0 and args.camera[1] > 0):
        raise SystemExit("--unit_m, FX and FY must be positive")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("this tool runs on an MI355X: the HIP kernels are the only implementation (no CPU fallback)")
    from PIL import Image
    from mcdseg import ops
    dev = torch.device("cuda", torch.cuda.current_device())
    os.makedirs(args.out_dir, exist_ok=True)

    batch = []  # (file name, uint16 [H,W]), all of one size

    def flush():
        if not batch:
            return
        depth = torch.from_numpy(np.stack([b[1] for b in batch]).astype(np.int32)).to(dev)
        hha, parts = ops.depth_to_hha(depth, tuple(args.camera), unit_m=args.unit_m, return_parts=True)
        hha, g = hha.cpu().numpy(), parts["gravity"].cpu().numpy()
        for k, (name, _) in enumerate(batch):
            Image.fromarray(hha[k], "RGB").save(os.path.join(args.out_dir, name))
            print("%s gravity %.6f %.6f %.6f" % (name, g[k, 0], g[k, 1], g[k, 2]))
        del batch[:]

    for one_file in sorted(os.listdir(args.depth_dir)):
        if not one_file.lower().endswith(".png"):
            continue
        d = read_depth(os.path.join(args.depth_dir, one_file))
        if batch and (len(batch) >= args.batch_size or batch[0][1].shape != d.shape):
            flush()
        batch.append((one_file, d))
    flush()
    return args.out_dir


if __name__ == "__main__":
    main()
