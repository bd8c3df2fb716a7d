#!/usr/bin/env python3
"""Milliseconds per image of the edge maps (Laplacian, Sobel, Canny), on one GPU:

    kernels   (a) ``ops.edge_maps`` alone -- the front end's one launch and the hysteresis passes -- on images that already lie on the
                  device (device events)
    device    (b) upload of the RGB batch from pinned memory + the kernels + download of the three maps into pinned memory (host clock
                  around a call that ends in a synchronise)
    cpu       (c) the numpy / scipy oracle of the definition (tests/edge_ref.py) on the same arrays: the only other implementation there
                  is -- it is written for clarity, not for speed, and OpenCV is not installed

480 x 640, batch 16 by default, images synthesised in memory; no file is read or written in any of the three.  The forms alternate
within a repetition, so that what else runs on the machine meets all of them.  The outputs of (b) are compared with those of (c) bit
for bit (``"equal"``).  Prints one JSON line.

    python tools/time_edge_detect.py --reps 20 --warmup 3
"""
import argparse
import json
import os
import statistics
import sys
import time

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, PKG)
sys.path.insert(1, os.path.join(os.path.dirname(PKG), "tests"))  # edge_ref.py: the CPU baseline is the tests' oracle, not a copy

KINDS = ("laplacian", "sobel", "canny")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", type=int, nargs=2, default=(640, 480), metavar=("W", "H"))
    ap.add_argument("-b", "--batch_size", type=int, default=16)
    ap.add_argument("--min_canny_thre", type=int, default=100)
    ap.add_argument("--max_canny_thre", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernel_calls", type=int, default=20, help="calls inside one timed window of (a)")
    ap.add_argument("--cpu_reps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1234)
    args = ap.parse_args(argv)

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("this measurement runs on an MI355X: there is no CPU fallback")
    import edge_ref as R
    from mcdseg import ops

    start = time.monotonic()
    dev = torch.device("cuda", torch.cuda.current_device())
    w, h = args.shape
    b, low, high = args.batch_size, args.min_canny_thre, args.max_canny_thre
    rgb = R.make_rgb("smooth", b, h, w, seed=args.seed)
    host = torch.from_numpy(rgb).pin_memory()
    resident = host.to(dev)
    staged = torch.empty_like(resident)
    back = {k: torch.empty((b, h, w), dtype=torch.uint8).pin_memory() for k in KINDS}

    def form_kernels():
        torch.cuda.synchronize()
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.kernel_calls):
            ops.edge_maps(resident, low, high, KINDS)
        e.record()
        torch.cuda.synchronize()
        return a.elapsed_time(e) / args.kernel_calls / b

    def form_device():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        staged.copy_(host, non_blocking=True)
        maps = ops.edge_maps(staged, low, high, KINDS)
        for k in KINDS:
            back[k].copy_(maps[k], non_blocking=True)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / b

    cpu_out = {}

    def form_cpu():
        t0 = time.perf_counter()
        cpu_out["maps"] = R.edge_maps(rgb, low, high)
        return (time.perf_counter() - t0) * 1e3 / b

    times = {"kernels": [], "device": [], "cpu": []}
    equal, got = None, None
    for rep in range(args.warmup + args.reps):
        for form, fn in (("kernels", form_kernels), ("device", form_device), ("cpu", form_cpu)):
            if form == "cpu" and not (rep >= args.warmup and len(times["cpu"]) < args.cpu_reps):
                continue
            t = fn()
            if rep >= args.warmup:
                times[form].append(t)
            if form == "device" and rep == args.warmup:
                got = {k: v.numpy().copy() for k, v in back.items()}
            if form == "cpu" and equal is None:
                equal = bool(all(np.array_equal(got[k], cpu_out["maps"][k]) for k in KINDS))
    nbytes = 3 * b * h * w + b * h * w * (3 + 1 + 1 + 4 * 4)  # rgb in; three maps + the class map out and in again; the label passes
    result = {"shape_wh": [w, h], "batch": b, "thresholds": [low, high], "kinds": list(KINDS), "warmup": args.warmup,
              "kernel_calls_per_window": args.kernel_calls, "edge_pixel_share": round(float((cpu_out["maps"]["canny"] == 255).mean()), 4),
              "algorithmic_MB_per_image": round(nbytes / b / 1e6, 2), "equal": equal, "wall_s": round(time.monotonic() - start, 1)}
    for form, t in times.items():
        result[form] = {"reps": len(t), "ms_per_image_median": round(statistics.median(t), 4) if t else None,
                        "ms_per_image_min_max": [round(min(t), 4), round(max(t), 4)] if t else None}
    if times["device"] and times["cpu"]:
        result["cpu_over_device"] = round(statistics.median(times["cpu"]) / statistics.median(times["device"]), 2)
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
