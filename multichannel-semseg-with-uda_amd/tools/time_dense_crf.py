#!/usr/bin/env python3
"""Seconds per image of ``ops.dense_crf`` in its two forms, on one GPU:

    fused     the kernels of csrc/crf.hip (the default)
    composed  MCDSEG_FUSED_CRF=0: the same definition from torch, row chunks of exp(-0.5 * cdist^2) @ (n * Q) for both terms

480 x 640, C = 41, 10 iterations, with an image, by default (the suncg / nyu test shape).  One call per repetition on a fixed synthetic
image, bracketed by device events after ``--warmup`` calls; the two forms alternate, so that what else runs on the machine meets both.
Peak memory is torch's allocator peak over a form's calls (inputs included).  The whole measurement runs under ``--time_limit``
seconds: no further call is started once it is used up, an alarm ends a call that overruns it, and what was measured until then is
reported (``"cut_short": true``).  The composed form takes minutes per call at the default size.  Prints one JSON line.

    python tools/time_dense_crf.py --reps 2 --warmup 1
"""
import argparse
import json
import os
import signal
import statistics
import sys
import time

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, PKG)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", type=int, nargs=2, default=(640, 480), metavar=("W", "H"))
    ap.add_argument("--n_class", type=int, default=41)
    ap.add_argument("--n_iters", type=int, default=10)
    ap.add_argument("-b", "--batch_size", type=int, default=1)
    ap.add_argument("--no_image", action="store_true", help="the Gaussian term alone")
    ap.add_argument("--sxy_bilateral", type=float, nargs=2, default=(49, 49))
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--forms", nargs="+", default=("fused", "composed"), choices=("fused", "composed"))
    ap.add_argument("--time_limit", type=int, default=900, help="seconds for the whole measurement")
    ap.add_argument("--seed", type=int, default=1234)
    args = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("this measurement runs on an MI355X: there is no CPU fallback")
    from mcdseg import ops

    start = time.monotonic()

    class Overrun(Exception):
        pass

    def overrun(signum, frame):
        raise Overrun()

    signal.signal(signal.SIGALRM, overrun)
    signal.alarm(args.time_limit)
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(args.seed)
    w, h = args.shape
    b, c = args.batch_size, args.n_class
    blobs = torch.randint(0, c, (b, 1, (h + 3) // 4, (w + 3) // 4), device=dev)
    lab = blobs.repeat_interleave(4, 2).repeat_interleave(4, 3)[:, :, :h, :w]
    logits = 1.5 * torch.randn(b, c, h, w, device=dev)
    logits.scatter_add_(1, lab, torch.full_like(lab, 1.5, dtype=torch.float32))
    palette = torch.randint(0, 256, (c, 3), device=dev).float()
    rgb = None
    if not args.no_image:
        rgb = (palette[lab[:, 0]] + 12 * torch.randn(b, h, w, 3, device=dev)).round().clamp(0, 255).to(torch.uint8)

    def call(form):
        os.environ["MCDSEG_FUSED_CRF"] = "1" if form == "fused" else "0"
        return ops.dense_crf(logits, rgb, n_iters=args.n_iters, sxy_bilateral=tuple(args.sxy_bilateral))

    times = {f: [] for f in args.forms}
    peak = {f: 0 for f in args.forms}
    out = {}
    cut_short = False
    try:
        for rep in range(args.warmup + args.reps):
            for form in args.forms:
                if time.monotonic() - start > args.time_limit:
                    raise Overrun()
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                out[form] = call(form)
                e.record()
                torch.cuda.synchronize()
                peak[form] = max(peak[form], torch.cuda.max_memory_allocated())
                print("%s %s: %.3f s" % ("warmup" if rep < args.warmup else "rep %d" % (rep - args.warmup), form, a.elapsed_time(e) / 1e3),
                      file=sys.stderr, flush=True)
                if rep >= args.warmup:
                    times[form].append(a.elapsed_time(e) / 1e3 / b)
    except Overrun:
        cut_short = True
        torch.cuda.synchronize()
        print("the time limit of %d s ran out" % args.time_limit, file=sys.stderr, flush=True)
    signal.alarm(0)
    os.environ.pop("MCDSEG_FUSED_CRF", None)
    result = {"shape_wh": [w, h], "n_class": c, "n_iters": args.n_iters, "batch": b, "image": rgb is not None,
              "sxy_bilateral": list(args.sxy_bilateral), "warmup": args.warmup, "cut_short": cut_short, "wall_s": round(time.monotonic() - start, 1)}
    for form in args.forms:
        t = times[form]
        result[form] = {"reps": len(t), "s_per_image_median": round(statistics.median(t), 4) if t else None,
                        "s_per_image_min_max": [round(min(t), 4), round(max(t), 4)] if t else None,
                        "peak_memory_MiB": round(peak[form] / 2 ** 20, 1)}
    if len(times) == 2 and all(times.values()) and not cut_short:
        result["speedup"] = round(statistics.median(times["composed"]) / statistics.median(times["fused"]), 2)
        q1, q2 = out["fused"][0], out["composed"][0]
        result["max_abs_q_difference"] = float((q1 - q2).abs().max())
        result["labels_that_differ"] = int((out["fused"][1] != out["composed"][1]).sum())
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
