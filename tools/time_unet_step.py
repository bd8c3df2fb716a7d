#!/usr/bin/env python3
"""Times one MCD step of the U-Net (``--net unet``) on the kernels of csrc/unet.hip and on the composed torch path
(MCDSEG_FUSED_UNET=0: F.max_pool2d, F.conv_transpose2d + torch.cat, torch.relu, mcdseg_split_cb), and the three ops alone.

    python tools/time_unet_step.py [--batch 16] [--shape 640 480] [--warmup 2] [--steps 5] [--what step ops]

``step``  whole steps of ``adapt_trainer.py suncg nyu --synthetic --input_ch 6 --net unet``, as tools/time_fusenet_step.py times them: the
          trainer's own ``main``, a host clock and a device synchronisation on either side of every ``MCDSolver.step``.  The two forms
          alternate, ``--rounds`` times, on the same box back to back.
``ops``   ``ops.max_pool2``, ``ops.up_join`` and ``ops.relu`` alone, forward and backward, at the shapes they meet in the network at that
          size, both forms, HIP events around ``--reps`` calls: the table that says which kernel is behind when a step is.
"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multichannel-semseg-with-uda_amd"))
os.environ["MCDSEG_PRETRAINED"] = "0"
FORMS = (("fused", "1"), ("composed", "0"))


def trainer_args(a, tmp, total):
    return ["suncg", "nyu", "--base_outdir", tmp, "--net", "unet", "--input_ch", "6", "-b", str(a.batch), "--train_img_shape", str(a.shape[0]),
            str(a.shape[1]), "--synthetic", "--synthetic_len", str(a.batch * total), "--no_tflog", "--epochs", "1", "--max_iter", str(total)]


def time_steps(a):
    import torch
    import adapt_trainer
    from solvers.solver import MCDSolver
    plain = MCDSolver.step
    total = a.warmup + a.steps
    means = {name: [] for name, _ in FORMS}
    for rnd in range(a.rounds):
        for name, env in FORMS:
            times = []

            def timed(self, *args, **kw):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = plain(self, *args, **kw)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
                return out
            MCDSolver.step = timed
            os.environ["MCDSEG_FUSED_UNET"] = env
            torch.cuda.reset_peak_memory_stats()
            try:
                with tempfile.TemporaryDirectory() as tmp:
                    rc = adapt_trainer.main(trainer_args(a, tmp, total))
            finally:
                MCDSolver.step = plain
                os.environ.pop("MCDSEG_FUSED_UNET", None)
            if rc != 0 or len(times) != total:
                sys.exit("trainer returned %r after %d steps" % (rc, len(times)))
            t = times[a.warmup:]
            means[name].append(sum(t) / len(t))
            print("STEP round=%d form=%s steps ms: %s  mean %.1f  min %.1f  peak MiB %.0f"
                  % (rnd, name, " ".join("%.1f" % v for v in t), sum(t) / len(t), min(t), torch.cuda.max_memory_allocated() / 2 ** 20), flush=True)
            torch.cuda.empty_cache()
    f, c = (sum(means[k]) / len(means[k]) for k in ("fused", "composed"))
    print("STEP unet batch %d at %d x %d: fused %.1f ms, composed %.1f ms per MCD step (composed / fused %.3f)"
          % (a.batch, a.shape[0], a.shape[1], f, c, c / f), flush=True)


def time_ops(a):
    import torch
    from mcdseg import ops
    dev = torch.device("cuda:0")
    w, h = a.shape
    filters = (16, 32, 64, 128, 256)

    def with_bound(t):
        t._mcd_cb = (None, ops.absmax(t), t._version, t.data_ptr())
        return t

    def clock(fn):
        for _ in range(2):
            fn()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(a.reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) * 1e3 / a.reps

    def both(label, make, call):
        """forward alone (under grad mode) and forward + backward, in both forms"""
        line = []
        for name, env in FORMS:
            os.environ["MCDSEG_FUSED_UNET"] = env
            leaves = make()
            y = call(*leaves)
            dy = torch.randn_like(y)
            fwd = clock(lambda: call(*leaves))

            def fb():
                for t in leaves:
                    t.grad = None
                call(*leaves).backward(dy)
            line.append("%s fwd %8.1f us  fwd+bwd %8.1f us" % (name, fwd, clock(fb)))
            del leaves, y, dy
        print("OPS %-34s %s  %s" % (label, ops.CONV_MATH, "   ".join(line)), flush=True)

    try:
        for k in range(4):  # the pools behind conv1 .. conv4
            shape = (a.batch, filters[k], h >> k, w >> k)
            both("max_pool2 %s" % "x".join(map(str, shape)), lambda: [with_bound(torch.randn(shape, device=dev).relu_().requires_grad_(True))],
                 ops.max_pool2)
        for k in range(3, -1, -1):  # up_concat4 .. up_concat1, and the ReLU behind their convolutions
            cs, cin = filters[k], filters[k + 1]
            hh, wh = h >> (k + 1), w >> (k + 1)

            def make():
                return [torch.randn(a.batch, cs, 2 * hh, 2 * wh, device=dev).requires_grad_(True),
                        torch.randn(a.batch, cin, hh, wh, device=dev).requires_grad_(True),
                        (torch.randn(cin, cs, 2, 2, device=dev) * 0.1).requires_grad_(True), torch.randn(cs, device=dev).requires_grad_(True)]
            both("up_join %d+%d at %dx%d" % (cs, cs, 2 * hh, 2 * wh), make, ops.up_join)
            shape = (a.batch, cs, 2 * hh, 2 * wh)
            both("relu %s" % "x".join(map(str, shape)), lambda: [with_bound(torch.randn(shape, device=dev).requires_grad_(True))], ops.relu)
    finally:
        os.environ.pop("MCDSEG_FUSED_UNET", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--shape", type=int, nargs=2, default=[640, 480], metavar=("W", "H"))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--what", nargs="+", default=["step", "ops"], choices=["step", "ops"])
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_unet_step.py needs an MI355X: a time taken anywhere else says nothing")
    for what, fn in (("ops", time_ops), ("step", time_steps)):
        if what in a.what:
            fn(a)


if __name__ == "__main__":
    main()
