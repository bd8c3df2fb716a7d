"""Development probe (GPU): ``ops.seg2bd_bce`` forward + backward against the unfused composition it replaces -- ``ops.bilinear8`` ->
torch ``conv2d`` (5x5, padding 2) -> sigmoid -> ``ops.bce2d``, both heads -- at the trainer's size (N = 16, C = 41, 60 x 80 -> 480 x 640).
Device events around each forward + backward, three warm-up rounds, the two versions alternated in one process; the peak of
``torch.cuda.max_memory_allocated`` over one forward + backward of each, above what the inputs hold.  Prints one JSON line.

    python tools/probes/seg2bd_ab.py [--n 16] [--reps 10]"""
import argparse
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "multichannel-semseg-with-uda_amd"))
from mcdseg import ops  # noqa: E402


def fused(z1, z2, w, b, t):
    l1, l2 = ops.seg2bd_bce(z1, z2, w, b, t)
    return l1 + l2


def unfused(z1, z2, w, b, t):
    return sum(ops.bce2d(torch.sigmoid(F.conv2d(ops.bilinear8(z), w, b, padding=2)), t) for z in (z1, z2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--c", type=int, default=41)
    ap.add_argument("--hi", type=int, default=60)
    ap.add_argument("--wi", type=int, default=80)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seg2bd_ab: needs the GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    z1, z2 = (2 * torch.randn(a.n, a.c, a.hi, a.wi, generator=g) for _ in range(2))
    w = torch.randn(1, a.c, 5, 5, generator=g) * 0.5 / math.sqrt(25 * a.c)
    b = torch.zeros(1)
    wide = torch.randn(a.n, 7, 8 * a.hi, 8 * a.wi, generator=g)
    wide[:, 6] = (wide[:, 6] > 1.0).float()
    z1, z2, w, b, wide = (x.to(dev) for x in (z1, z2, w, b, wide))
    for x in (z1, z2, w, b):
        x.requires_grad_()
    t = wide[:, 6:]  # the trainer's target: channel 6 of the source batch, read in place by both versions' loss kernels

    def once(fn, timed=True):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        grads = torch.autograd.grad(fn(z1, z2, w, b, t.contiguous() if fn is unfused else t), [z1, z2, w, b])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), grads

    forms = {"fused": fused, "unfused": unfused}
    res = {k: [] for k in forms}
    for r in range(a.reps + 3):
        for name, fn in forms.items():  # alternated
            ms, _ = once(fn)
            if r >= 3:
                res[name].append(ms)
    peaks = {}
    for name, fn in forms.items():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        once(fn)
        peaks[name] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    gf, gu = once(fused)[1], once(unfused)[1]
    diff = [float((x - y).abs().max() / y.abs().max()) for x, y in zip(gf, gu)]
    out = {"shape": [a.n, a.c, a.hi, a.wi], "reps": a.reps}
    for name in forms:
        v = sorted(res[name])
        out[name] = {"ms_median": v[len(v) // 2], "ms_min": v[0], "ms_max": v[-1], "peak_MiB_above_inputs": peaks[name]}
    out["speedup_median"] = out["unfused"]["ms_median"] / out["fused"]["ms_median"]
    out["grad_rel_diff_dz1_dz2_dw_db"] = diff
    print(json.dumps(out))


if __name__ == "__main__":
    main()
