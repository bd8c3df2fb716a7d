#!/usr/bin/env python3
"""The three-step MCD trace "mcd_small" of traces.json (drn_d_38, 6 channels, 2 x 6 x 64 x 96, two iterations) with the classifier
discrepancies ``--d_loss jsd | symkl | mis_symkl``: ``oracle.ref_mcd.mcd_step`` on the CPU oracle's modules with the REFERENCE's own
criterion objects (its ``CrossEntropyLoss2d`` and ``get_prob_distance_criterion(name)``, imported in memory by the shim of
make_golden.py), once in fp64 -- the truth the fused solver is held to -- and once in fp32.  Only data is written:
tests/golden/dist_traces.json with, per name, the fp64 losses per iteration and the fp64 final state as traces.json stores it (sum and
L2 norm per tensor), and under "f32_distance" how far the fp32 run of the same loop is from the fp64 one in each quantity the tests
bound (relative c_loss / d_loss per iteration; the state as ``_check_state`` measures it): where that distance is itself outside a
test's bar, the test holds the quantity to twice the distance instead.
Run once in this container:  python tests/golden/make_golden_dist_trace.py
"""
import json
import os
import sys
import warnings

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from make_golden import load_reference  # noqa: E402
from recipe import fill_state_, make_batch, state_checksums  # noqa: E402

NC = 41
NAMES = ["jsd", "symkl", "mis_symkl"]


def run(ref_loss, name, dtype, tr):
    from oracle import ref_mcd, ref_models
    n, ch, h, w = tr["shape"]
    s, l, t = make_batch(tr["seed_batch"], n, ch, h, w, NC)
    g, f1, f2 = ref_models.get_models("drn_d_38", ch, NC)
    for m, seed in ((g, 11), (f1, 12), (f2, 13)):
        fill_state_(m, seed)
        m.to(dtype).train()
    og = ref_models.get_optimizer(g.parameters(), "sgd", 1e-3, 0.9, 2e-5)
    of = ref_models.get_optimizer(list(f1.parameters()) + list(f2.parameters()), "sgd", 1e-3, 0.9, 2e-5)
    cw = torch.ones(NC, dtype=dtype)
    cw[NC - 1] = 0
    crit = ref_loss.CrossEntropyLoss2d(cw)
    critd = ref_loss.get_prob_distance_criterion(name, n_class=NC)  # (the reference's trainer passes no n_class and fails for symkl)
    iters = []
    for _ in range(len(tr["iters"])):
        c, d = ref_mcd.mcd_step(g, f1, f2, og, of, crit, critd, s.to(dtype), l, t.to(dtype), num_k=4, num_multiply_d_loss=1)
        iters.append({"c_loss": c, "d_loss": d})
    return iters, {"g": state_checksums(g), "f1": state_checksums(f1), "f2": state_checksums(f2)}, \
        {"g": {k: v.numel() for k, v in g.state_dict().items()}, "f1": {k: v.numel() for k, v in f1.state_dict().items()},
         "f2": {k: v.numel() for k, v in f2.state_dict().items()}}


def state_distance(a, b, numel):
    """the largest ratio ``_check_state`` (tests/test_model_gpu.py) would have to allow as rtol between two sets of checksums"""
    worst = 0.0
    for k, (s, l2) in b.items():
        scale = max(abs(l2), 1e-6)
        worst = max(worst, abs(a[k][1] - l2) / scale, abs(a[k][0] - s) / (scale * max(numel[k], 1) ** 0.5))
    return worst


def main():
    warnings.simplefilter("ignore")
    ref_loss = load_reference()[0]
    with open(os.path.join(HERE, "traces.json")) as fh:
        tr = json.load(fh)["mcd_small"]
    out = {}
    for name in NAMES:
        i64, s64, numel = run(ref_loss, name, torch.float64, tr)
        i32, s32, _ = run(ref_loss, name, torch.float32, tr)
        rel = lambda a, b: abs(a - b) / abs(b)  # noqa: E731
        out[name] = {"shape": tr["shape"], "seed_batch": tr["seed_batch"], "iters": i64, "g": s64["g"], "f1": s64["f1"], "f2": s64["f2"],
                     "iters_f32": i32,
                     "f32_distance": {"c_loss": [rel(a["c_loss"], b["c_loss"]) for a, b in zip(i32, i64)],
                                      "d_loss": [rel(a["d_loss"], b["d_loss"]) for a, b in zip(i32, i64)],
                                      "state": {m: state_distance(s32[m], s64[m], numel[m]) for m in ("g", "f1", "f2")}}}
        print("  %-10s fp64 %s\n             fp32 %s\n             fp32 - fp64: %s" % (name, i64, i32, out[name]["f32_distance"]), flush=True)
    with open(os.path.join(HERE, "dist_traces.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
    print("dist_traces.json written")


if __name__ == "__main__":
    main()
