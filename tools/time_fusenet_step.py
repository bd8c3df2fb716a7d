#!/usr/bin/env python3
"""Times the middle fusion (``--net drn_d_38_fusenet``) beside the early fusion (``--net drn_d_38``), and its stage join alone.

    python tools/time_fusenet_step.py [--batch 16] [--shape 640 480] [--warmup 2] [--steps 5] [--what step join aten]

``step``  whole steps of ``adapt_trainer.py suncg nyu --synthetic --input_ch 6`` for both networks, as tools/time_steps.py times them: the
          trainer's own ``main``, a host clock and a device synchronisation on either side of every ``MCDSolver.step``.
``join``  ``ops.stage_join`` alone at the nine stage shapes of drn_d_38 at that size, HIP events around ``--reps`` calls: the fused kernel
          (16 B per element with f16x3: 8 read, 4 + 4 written), the composed form with the known bound (MCDSEG_FUSED_JOIN=0: torch.add and
          mcdseg_split_cb, 20 B) and the composition from before the kernel, which measures the bound (torch.add, mcdseg_absmax,
          mcdseg_split_cb: 24 B).  Prints microseconds and the bytes of that count over the time.
``aten``  the ATen kernels left on one step of each network (torch's profiler: device kernels whose names are not this library's), by name.
"""
import argparse
import collections
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multichannel-semseg-with-uda_amd"))
os.environ["MCDSEG_PRETRAINED"] = "0"
NETS = ("drn_d_38_fusenet", "drn_d_38")


def trainer_args(a, net, tmp, total):
    return ["suncg", "nyu", "--base_outdir", tmp, "--net", net, "--input_ch", "6", "-b", str(a.batch), "--train_img_shape", str(a.shape[0]),
            str(a.shape[1]), "--synthetic", "--synthetic_len", str(a.batch * total), "--no_pretrained", "--no_tflog", "--epochs", "1",
            "--max_iter", str(total)]


def time_steps(a):
    import torch
    import adapt_trainer
    from solvers.solver import MCDSolver
    plain = MCDSolver.step
    total = a.warmup + a.steps
    for rnd in range(a.rounds):  # (the two networks alternate: other work shares the machine)
        for net in NETS:
            times = []

            def timed(self, *args, **kw):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = plain(self, *args, **kw)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
                return out
            MCDSolver.step = timed
            torch.cuda.reset_peak_memory_stats()
            try:
                with tempfile.TemporaryDirectory() as tmp:
                    rc = adapt_trainer.main(trainer_args(a, net, tmp, total))
            finally:
                MCDSolver.step = plain
            if rc != 0 or len(times) != total:
                sys.exit("trainer returned %r after %d steps" % (rc, len(times)))
            t = times[a.warmup:]
            print("STEP round=%d net=%s steps ms: %s  mean %.1f  min %.1f  peak MiB %.0f"
                  % (rnd, net, " ".join("%.1f" % v for v in t), sum(t) / len(t), min(t), torch.cuda.max_memory_allocated() / 2 ** 20), flush=True)
            torch.cuda.empty_cache()


def stage_shapes(batch, w, h):
    """(N, C, H, W) of main_layer0 .. main_layer8 of drn_d_38"""
    from models.drn import CHANNELS
    chans = (CHANNELS[0],) + tuple(CHANNELS)
    div = (1, 1, 2, 4, 8, 8, 8, 8, 8)
    return [(batch, c, h // d, w // d) for c, d in zip(chans, div)]


def time_joins(a):
    import torch
    from mcdseg import ops
    dev = torch.device("cuda:0")
    piece_bytes = 2 * ops.PIECES.get(ops.CONV_MATH, 0)

    def with_bound(t):
        b = ops.absmax(t)
        t._mcd_cb = (None, b, t._version, t.data_ptr())
        return t

    def fused(x, y):
        os.environ["MCDSEG_FUSED_JOIN"] = "1"
        return ops.stage_join(x, y)

    def composed(x, y):
        os.environ["MCDSEG_FUSED_JOIN"] = "0"
        return ops.stage_join(x, y)

    def measured(x, y):
        s = x + y
        return s, ops.split_companion(s)

    forms = (("fused", fused, 12 + piece_bytes), ("composed", composed, 16 + piece_bytes), ("measured", measured, 20 + piece_bytes))
    try:
        with torch.no_grad():
            for k, shape in enumerate(stage_shapes(a.batch, a.shape[0], a.shape[1])):
                x, y = with_bound(torch.randn(shape, device=dev)), with_bound(torch.randn(shape, device=dev))
                line = []
                for name, fn, per_elem in forms:
                    for _ in range(3):
                        fn(x, y)
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    t0.record()
                    for _ in range(a.reps):
                        fn(x, y)
                    t1.record()
                    torch.cuda.synchronize()
                    us = t0.elapsed_time(t1) * 1e3 / a.reps
                    line.append("%s %8.1f us %5.2f TB/s (%d B/elem)" % (name, us, x.numel() * per_elem / us / 1e6, per_elem))
                print("JOIN main_layer%d %-20s %s  %s" % (k, "x".join(map(str, shape)), ops.CONV_MATH, "  ".join(line)), flush=True)
                del x, y
    finally:
        os.environ.pop("MCDSEG_FUSED_JOIN", None)


def count_aten(a):
    import torch
    import adapt_trainer
    from solvers.solver import MCDSolver
    from torch.profiler import ProfilerActivity, profile
    plain = MCDSolver.step
    for net in NETS:
        seen = {"n": 0, "prof": None}

        def profiled(self, *args, **kw):
            seen["n"] += 1
            if seen["n"] != 3:
                return plain(self, *args, **kw)
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                out = plain(self, *args, **kw)
                torch.cuda.synchronize()
            seen["prof"] = prof
            return out
        MCDSolver.step = profiled
        try:
            with tempfile.TemporaryDirectory() as tmp:
                adapt_trainer.main(trainer_args(a, net, tmp, 3))
        finally:
            MCDSolver.step = plain
        ours, aten = 0, collections.Counter()
        for ev in seen["prof"].events():
            if str(getattr(ev, "device_type", "")).endswith("CUDA"):
                if "at::" in ev.name or "Memcpy" in ev.name or "Memset" in ev.name or "elementwise" in ev.name:
                    aten[ev.name.split("<")[0].split("(")[0][:70]] += 1
                else:
                    ours += 1
        print("ATEN net=%s one step: %d device launches of this library, %d ATen kernels / copies:" % (net, ours, sum(aten.values())), flush=True)
        for name, n in aten.most_common():
            print("ATEN   %5d  %s" % (n, name), flush=True)
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--shape", type=int, nargs=2, default=[640, 480], metavar=("W", "H"))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--what", nargs="+", default=["step", "join", "aten"], choices=["step", "join", "aten"])
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_fusenet_step.py needs an MI355X: a time taken anywhere else says nothing")
    for what, fn in (("join", time_joins), ("step", time_steps), ("aten", count_aten)):
        if what in a.what:
            fn(a)


if __name__ == "__main__":
    main()
