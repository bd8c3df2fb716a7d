#!/usr/bin/env python3
"""HHA images (horizontal disparity, height above ground, angle with gravity) from raw depth maps, on the MI355X (``ops.depth_to_hha``;
the definition is DESIGN.md section 4.13) -- the step the reference leaves to a third-party MATLAB release.

    python tools/depth_to_hha.py DEPTH_DIR OUT_DIR --camera FX FY CX CY [--unit_m 0.001] [-b N]
                                 [--fill RGB_DIR [--alpha 1] [--rtol 1e-10] [--max_iter 4000] [--max_valid_m M] [--keep_known]]

reads every 16-bit single-channel ``<name>.png`` of DEPTH_DIR (a value is ``--unit_m`` metres, 0.001 for NYUDv2 and Kinect PNGs; 0 is a
missing measurement) and writes ``OUT_DIR/<name>.png`` as an RGB PNG whose channels are disparity, height and angle.  ``--camera`` is the
pinhole model in pixels, for all files.  Files of equal size are encoded ``-b`` at a time.  Prints the estimated gravity direction (camera
coordinates, Y down the image) per file.

``--fill RGB_DIR`` inpaints the holes of each depth map first, guided by the RGB image of the same stem (``ops.fill_depth``: DESIGN.md
section 4.16; the flags are those of tools/fill_depth.py), and encodes the filled centimetres as they leave the solver: fill and encoding
both happen on the device, with no round trip through 16-bit values.  Each line then also carries ``fill iterations residual status``,
and the tool exits 1 after the last file if an image was neither ``converged`` nor ``empty``."""
import argparse
import os
import sys

import numpy as np

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if sys.path[:1] != [PKG]:
    sys.path.insert(0, PKG)


def _fill_tool():
    """tools/fill_depth.py, whose solver flags and RGB reader ``--fill`` shares"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("fill_depth_tool", os.path.join(PKG, "tools", "fill_depth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def get_parser():
    parser = argparse.ArgumentParser(description="Depth maps (16-bit PNGs) to HHA images")
    parser.add_argument("depth_dir", type=str, help="input directory of 16-bit single-channel depth PNGs")
    parser.add_argument("out_dir", type=str, help="output directory of the HHA images (RGB PNGs of the same names)")
    parser.add_argument("--camera", type=float, nargs=4, required=True, metavar=("FX", "FY", "CX", "CY"), help="pinhole camera, in pixels")
    parser.add_argument("--unit_m", type=float, default=0.001, help="metres per depth unit (0.001: millimetres)")
    parser.add_argument("-b", "--batch_size", type=int, default=1, help="files of equal size encoded per call")
    parser.add_argument("--fill", type=str, default=None, metavar="RGB_DIR", help="inpaint the depth first, guided by the RGB images here")
    _fill_tool().add_solver_arguments(parser)
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
    fill = _fill_tool() if args.fill is not None else None
    fill_kw = fill.solver_kwargs(args) if fill else None
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("this tool runs on an MI355X: the HIP kernels are the only implementation (no CPU fallback)")
    from PIL import Image
    from mcdseg import ops
    dev = torch.device("cuda", torch.cuda.current_device())
    os.makedirs(args.out_dir, exist_ok=True)

    batch = []  # (file name, uint16 [H,W]), all of one size
    failed = []

    def flush():
        if not batch:
            return
        depth = torch.from_numpy(np.stack([b[1] for b in batch]).astype(np.int32)).to(dev)
        if fill:
            rgb = torch.from_numpy(np.stack([fill.read_rgb(args.fill, name, d.shape) for name, d in batch])).to(dev)
            filled, solved = ops.fill_depth(rgb, depth, unit_m=args.unit_m, return_parts=True, **fill_kw)
            hha, parts = ops.depth_to_hha(filled, tuple(args.camera), return_parts=True)
        else:
            hha, parts = ops.depth_to_hha(depth, tuple(args.camera), unit_m=args.unit_m, return_parts=True)
        hha, g = hha.cpu().numpy(), parts["gravity"].cpu().numpy()
        for k, (name, _) in enumerate(batch):
            Image.fromarray(hha[k], "RGB").save(os.path.join(args.out_dir, name))
            line = "%s gravity %.6f %.6f %.6f" % (name, g[k, 0], g[k, 1], g[k, 2])
            if fill:
                status = int(solved["status"][k])
                line += " fill %d %.3e %s" % (int(solved["iterations"][k]), float(solved["residual"][k]), ops.FILL_STATUS_NAMES[status])
                if status not in (ops.FILL_CONVERGED, ops.FILL_EMPTY):
                    failed.append(name)
            print(line)
        del batch[:]

    for one_file in sorted(os.listdir(args.depth_dir)):
        if not one_file.lower().endswith(".png"):
            continue
        d = read_depth(os.path.join(args.depth_dir, one_file))
        if batch and (len(batch) >= args.batch_size or batch[0][1].shape != d.shape):
            flush()
        batch.append((one_file, d))
    flush()
    if failed:
        raise SystemExit(1)
    return args.out_dir


if __name__ == "__main__":
    main()
