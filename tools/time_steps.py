#!/usr/bin/env python3
"""Times whole steps of ``adapt_trainer.py suncg nyu --synthetic`` as the command line runs them (6 x 480 x 640, batch 16 by default): the
trainer's own ``main`` with a host clock and a device synchronisation on either side of every three-step update, whichever route the
trainer takes for the flags (``MCDSolver.step`` or ``dropin_step``).  Prints one line: the timed steps, their mean and minimum, peak
allocated memory.
    python tools/time_steps.py --d_loss symkl [--tree OTHER_CHECKOUT] [--batch 16] [--warmup 2] [--steps 5] [-- extra trainer arguments]
``--tree``: a built checkout of another commit to time instead of this one (for A/B runs: alternate the two in separate processes)."""
import argparse
import os
import sys
import tempfile
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--d_loss", default="diff")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--shape", type=int, nargs=2, default=[640, 480], metavar=("W", "H"))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("extra", nargs="*")
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    sys.path.insert(0, os.path.join(tree, "multichannel-semseg-with-uda_amd"))
    os.environ["MCDSEG_PRETRAINED"] = "0"
    import torch
    import adapt_trainer
    from solvers.solver import MCDSolver
    assert adapt_trainer.__file__.startswith(tree), adapt_trainer.__file__
    times, route = [], []

    def wrap(fn, tag):
        def inner(*args, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*args, **kw)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
            route.append(tag)
            return out
        return inner
    adapt_trainer.dropin_step = wrap(adapt_trainer.dropin_step, "dropin_step")
    MCDSolver.step = wrap(MCDSolver.step, "MCDSolver.step")
    total = a.warmup + a.steps
    with tempfile.TemporaryDirectory() as tmp:
        rc = adapt_trainer.main(["suncg", "nyu", "--base_outdir", tmp, "--input_ch", "6", "-b", str(a.batch), "--train_img_shape", str(a.shape[0]),
                                 str(a.shape[1]), "--synthetic", "--synthetic_len", str(a.batch * total), "--no_pretrained", "--no_tflog",
                                 "--epochs", "1", "--max_iter", str(total), "--d_loss", a.d_loss] + a.extra)
    if rc != 0 or len(times) != total:
        sys.exit("trainer returned %r after %d steps" % (rc, len(times)))
    t = times[a.warmup:]
    print("STEP tree=%s d_loss=%s route=%s steps ms: %s  mean %.1f  min %.1f  peak MiB %.0f"
          % ("this" if tree == os.path.dirname(os.path.dirname(os.path.abspath(__file__))) else "other", a.d_loss, route[-1], " ".join("%.1f" % v for v in t), sum(t) / len(t), min(t),
             torch.cuda.max_memory_allocated() / 2 ** 20), flush=True)


if __name__ == "__main__":
    main()
