#!/usr/bin/env python3
"""Milliseconds per image of ensembling K saved maps, on one GPU, for both methods:

    kernels   (a) ``ops.ensemble_probs`` + ``ops.label_resize_colorize`` alone, on maps that already lie on the device (device events)
    device    (b) upload of the K maps from pinned memory + the two kernels + download of the combined map, the labels and the palette
                  image into pinned memory (host clock around a call that ends in a synchronise)
    cpu       (c) the reference's procedure restated with numpy and Pillow (tests/ensemble_ref.py ``ensemble_predict``) on the same arrays

41 classes at 480 x 640, K = 3 by default (the suncg / nyu test shape), maps synthesised in memory; no file is read or written in any of
the three.  The forms alternate within a repetition, so that what else runs on the machine meets all of them.  The outputs of (b) are
compared with those of (c) bit for bit (``"equal"``).  Prints one JSON line.

    python tools/time_ensemble.py --reps 20 --warmup 3
"""
import argparse
import json
import os
import statistics
import sys
import time

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, PKG)
sys.path.insert(1, os.path.join(os.path.dirname(PKG), "tests"))  # ensemble_ref.py: the CPU baseline is the tests' oracle, not a copy


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", type=int, nargs=2, default=(640, 480), metavar=("W", "H"))
    ap.add_argument("--out_shape", type=int, nargs=2, default=None, metavar=("W", "H"), help="size of the PNG arrays (default: the maps')")
    ap.add_argument("--n_class", type=int, default=41)
    ap.add_argument("--n_used", type=int, default=None)
    ap.add_argument("-k", "--members", type=int, default=3)
    ap.add_argument("-b", "--batch_size", type=int, default=1)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernel_calls", type=int, default=20, help="calls inside one timed window of (a)")
    ap.add_argument("--cpu_reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1234)
    args = ap.parse_args(argv)

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("this measurement runs on an MI355X: there is no CPU fallback")
    import ensemble
    import ensemble_ref as R
    from mcdseg import ops

    start = time.monotonic()
    dev = torch.device("cuda", torch.cuda.current_device())
    w, h = args.shape
    k, b, c = args.members, args.batch_size, args.n_class
    n_used = c if args.n_used is None else args.n_used
    wh = (w, h) if args.out_shape is None else tuple(args.out_shape)
    maps = R.make_maps("random", k, b, c, h, w, seed=args.seed)
    palette = ensemble.default_palette(min(n_used + 1, 256))
    pal_dev = torch.from_numpy(palette).to(dev)
    host = [torch.from_numpy(m).pin_memory() for m in maps]
    resident = [t.to(dev) for t in host]
    staged = [torch.empty_like(t) for t in resident]
    back = {"prob": torch.empty((b, c, h, w), dtype=torch.float32).pin_memory(),
            "label": torch.empty((b, wh[1], wh[0]), dtype=torch.uint8).pin_memory(),
            "vis": torch.empty((b, wh[1], wh[0], 3), dtype=torch.uint8).pin_memory()}

    def kernels(method, src):
        prob, lab = ops.ensemble_probs(src, method, n_used)
        out, vis = ops.label_resize_colorize(lab, wh, pal_dev)
        return prob, out, vis

    def form_kernels(method):
        torch.cuda.synchronize()
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.kernel_calls):
            kernels(method, resident)
        e.record()
        torch.cuda.synchronize()
        return a.elapsed_time(e) / args.kernel_calls / b

    def form_device(method):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for d, s in zip(staged, host):
            d.copy_(s, non_blocking=True)
        prob, out, vis = kernels(method, staged)
        back["prob"].copy_(prob, non_blocking=True)
        back["label"].copy_(out, non_blocking=True)
        back["vis"].copy_(vis, non_blocking=True)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / b

    cpu_out = {}

    def form_cpu(method):
        t0 = time.perf_counter()
        cpu_out[method] = [R.ensemble_predict([m[i] for m in maps], method, n_used, wh, palette) for i in range(b)]
        return (time.perf_counter() - t0) * 1e3 / b

    times = {m: {"kernels": [], "device": [], "cpu": []} for m in R.METHODS}
    equal = {}
    for rep in range(args.warmup + args.reps):
        for method in R.METHODS:
            for form, fn in (("kernels", form_kernels), ("device", form_device), ("cpu", form_cpu)):
                if form == "cpu" and not (rep >= args.warmup and len(times[method]["cpu"]) < args.cpu_reps):
                    continue
                t = fn(method)
                if rep >= args.warmup:
                    times[method][form].append(t)
                if form == "device" and rep == args.warmup:
                    got = {key: v.numpy().copy() for key, v in back.items()}
                if form == "cpu" and method not in equal:
                    want = cpu_out[method]
                    equal[method] = bool(all(R.bits(got["prob"][i]).tobytes() == R.bits(R.canon(want[i][0])).tobytes() and
                                             np.array_equal(got["label"][i], want[i][1]) and np.array_equal(got["vis"][i], want[i][2])
                                             for i in range(b)))
    nbytes = 4 * b * c * h * w * (k + 1) + b * h * w + 5 * b * wh[0] * wh[1]
    result = {"shape_wh": [w, h], "out_shape_wh": list(wh), "n_class": c, "n_used": n_used, "members": k, "batch": b, "warmup": args.warmup,
              "kernel_calls_per_window": args.kernel_calls, "algorithmic_MB_per_image": round(nbytes / b / 1e6, 2),
              "wall_s": round(time.monotonic() - start, 1)}
    for method in R.METHODS:
        entry = {"equal": equal.get(method)}
        for form, t in times[method].items():
            entry[form] = {"reps": len(t), "ms_per_image_median": round(statistics.median(t), 4) if t else None,
                           "ms_per_image_min_max": [round(min(t), 4), round(max(t), 4)] if t else None}
        if times[method]["kernels"]:
            entry["kernels_GB_per_s"] = round(nbytes / b / 1e6 / statistics.median(times[method]["kernels"]), 1)
        if times[method]["device"] and times[method]["cpu"]:
            entry["cpu_over_device"] = round(statistics.median(times[method]["cpu"]) / statistics.median(times[method]["device"]), 2)
        result[method] = entry
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
