#!/usr/bin/env python3
"""Times the loss kernels at the benchmark shape (N=16, 41 classes, 60x80 scores -> 480x640): the fused up-sampler + loss
kernel against up8_fwd x 2 + the plain loss kernel.  ``--dist NAME`` (a ``--d_loss`` name other than diff; repeatable): three legs for
that distance, alternating in one process -- (a) the fused kernel of that distance, (b) the L1 fused kernel of the same build, (c) the
route the flag took before the distance was a kernel: two ``up8`` forwards and the criterion's torch expression, forward and backward,
on the materialised logits (with its peak memory).  Development tool."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multichannel-semseg-with-uda_amd"))
import torch  # noqa: E402

from mcdseg import ops  # noqa: E402


def timed(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def dist_legs(name, s, w1, w2, rounds=3):
    """(a), (b), (c) of the module docstring for one distance: ``rounds`` alternating passes, the median of each leg"""
    import loss as loss_mod
    crit = loss_mod.get_prob_distance_criterion(name, n_class=s.shape[1])

    def fused():
        ops.up8_mcd_losses(s, w1, s, w2, None, None, diff_coef=1.0, dist=name)

    def fused_l1():
        ops.up8_mcd_losses(s, w1, s, w2, None, None, diff_coef=1.0)

    def torch_route():
        z1, z2 = ops.up8(s, w1).requires_grad_(), ops.up8(s, w2).requires_grad_()
        on_kernel, loss_mod._on_kernel = loss_mod._on_kernel, (lambda *a, **k: False)
        try:
            crit(z1, z2).backward()
        finally:
            loss_mod._on_kernel = on_kernel
    legs = {"a": [], "b": [], "c": []}
    peak = {}
    for _ in range(rounds):
        for key, fn, reps in (("a", fused, 20), ("b", fused_l1, 20), ("c", torch_route, 5)):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            legs[key].append(timed(fn, reps))
            peak[key] = torch.cuda.max_memory_allocated() / 2 ** 20
    med = {k: sorted(v)[len(v) // 2] for k, v in legs.items()}
    print("%-11s (a) fused %.3f ms [%s]  (b) fused L1 %.3f ms  (c) up8 x 2 + torch criterion fwd+bwd %.3f ms   a/b %.2f  c/a %.1f   "
          "peak MiB a %.0f  c %.0f   all rounds a %s b %s c %s"
          % (name, med["a"], ops.up8_loss_kernel_name(*s.shape, True, False, dist=name), med["b"], med["c"], med["a"] / med["b"],
             med["c"] / med["a"], peak["a"], peak["c"], *(" ".join("%.3f" % t for t in legs[k]) for k in "abc")), flush=True)


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--dist", action="append", default=[], choices=[k for k in ops.DIST_KINDS if k != "diff"])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, c, hi, wi = 16, int(os.environ.get("NC", "41")), 60, 80
    g = torch.Generator().manual_seed(0)
    s = torch.randn(n, c, hi, wi, generator=g).to(dev)
    w1 = (torch.randn(c, 1, 16, 16, generator=g) * 0.1).to(dev)
    w2 = (torch.randn(c, 1, 16, 16, generator=g) * 0.1).to(dev)
    lab = torch.randint(0, c, (n, 8 * hi, 8 * wi), generator=g).to(dev)
    cw = torch.ones(c, device=dev)
    if args.dist:
        s2 = (2 * torch.randn(n, c, hi, wi, generator=g)).to(dev)  # (spread 2: the heads disagree, as early in training)
        for name in args.dist:
            dist_legs(name, s2, w1, w2)
        return
    for name, labels, kw in (("CE+CE", lab, dict(ce_coef=1.0)), ("Diff", None, dict(diff_coef=1.0))):
        t_f = timed(lambda: ops.up8_mcd_losses(s, w1, s, w2, labels, cw if labels is not None else None, **kw))
        t_2 = timed(lambda: ops.mcd_losses(ops.up8(s, w1), ops.up8(s, w2), labels, cw if labels is not None else None, **kw))
        t_v = timed(lambda: ops.up8_mcd_losses(s, w1, s, w2, labels, cw if labels is not None else None, want_grad=False, **kw))
        print("%-6s fused %.3f ms (values only, no gradient stores: %.3f ms)   two-pass %.3f ms" % (name, t_f, t_v, t_2), flush=True)


if __name__ == "__main__":
    main()
