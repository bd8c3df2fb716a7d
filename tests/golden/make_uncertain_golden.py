#!/usr/bin/env python3
"""Generate tests/golden/uncertain_small.npz by running the REAL reference's ``UncertainDRNSeg.get_loss`` in memory, the way
make_golden.py does (same loader: lib2to3 on the reference's text, nothing copied).

    python tests/golden/make_uncertain_golden.py            # needs the reference checkout make_golden.py loads

The reference's class is built on drn_d_22 and its ``base`` and ``seg`` are then replaced by ``nn.Identity()``: ``get_loss`` is fed the
1/8-resolution score maps themselves, so everything behind the trunk -- Dropout2d, both up-samplers, the T-pass loop, its losses -- is
the reference's own code.  Two cases ("a": N=2, C=5, 3x5 scores, T=3; "b": N=1, C=41, 2x9, T=10 -- a 72-pixel row crosses the kernel's
64-column segment, and 41 classes have a kernel instantiation of their own).  Per case, under "<case>/":
  s, w_up, w_std, labels, cw      the inputs (tests/uncertain_ref.make_inputs; the class weight of the last class is zero)
  keep                            uint8 [T,N,C]: 1 where the reference's Dropout2d kept the channel, from a forward hook on ``dropout``
  r                               the T values of np.random.rand() the reference drew, replayed from the numpy seed
  gb, gu, lam                     the upstream gradients the backward pass was run with, and uncertain_weight
  f32/..., f64/...                B, U (per sample), ds, dw_up, dw_std: the reference's losses and the gradients of gb B + sum_n gu_n U_n
"keys": the state-dict keys of the reference's UncertainDRNSeg(drn_d_22, 5 classes, criterion=None) with their shapes, as JSON.

What the installed torch does not run, and what was done instead: CrossEntropyLoss2d sits on nn.NLLLoss2d, which torch removed; the
criterion is ``F.cross_entropy(., weight=cw)``, the same log_softmax + weighted-mean NLL (make_triple_golden.py does the same).

While generating, tests/uncertain_ref.one_pass (the formulas the HIP kernel implements) and .literal are asserted against the
reference in fp64, and the conditions of the GPU tests (uncertain_ref.conditions) on the inputs.
"""
import json
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import load_reference  # noqa: E402
import uncertain_ref as R  # noqa: E402

CASES = {"a": dict(seed=5, n=2, c=5, hi=3, wi=5, t=3, gb=0.7, gu=[1.3, -0.4]),
         "b": dict(seed=41, n=1, c=41, hi=2, wi=9, t=10, gb=1.0, gu=[0.6])}
LAM = 0.1


def run_reference(dfcn, d, spec, dtype, torch_seed, numpy_seed):
    """the reference's get_loss on the score maps; returns (results, keep bits seen by the hook)"""
    cw = torch.as_tensor(d["cw"]).to(dtype)
    model = dfcn.UncertainDRNSeg("drn_d_22", spec["c"], pretrained=False, criterion=lambda p, t: F.cross_entropy(p, t, weight=cw),
                                 n_dropout_exp=spec["t"], uncertain_weight=LAM)
    model.base, model.seg = nn.Identity(), nn.Identity()
    model.to(dtype)
    with torch.no_grad():
        model.up.weight.copy_(torch.as_tensor(d["w_up"]).to(dtype))
        model.up_std.weight.copy_(torch.as_tensor(d["w_std"]).to(dtype))
    seen = []
    model.dropout.register_forward_hook(lambda mod, inp, out: seen.append(((out != 0).flatten(2).any(2)).to(torch.uint8).numpy()))
    x = torch.as_tensor(d["s"]).to(dtype).requires_grad_(True)
    torch.manual_seed(torch_seed)
    np.random.seed(numpy_seed)
    base, unc = model.get_loss(x, torch.as_tensor(d["labels"]).long(), separately_returning=True)
    (base * spec["gb"] + (unc * torch.tensor(spec["gu"], dtype=dtype)).sum()).backward()
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    res = {"B": base.detach().numpy().astype(np_dt), "U": unc.detach().numpy().astype(np_dt), "ds": x.grad.numpy().astype(np_dt),
           "dw_up": model.up.weight.grad.numpy().astype(np_dt), "dw_std": model.up_std.weight.grad.numpy().astype(np_dt)}
    return res, np.stack(seen)


def main(path=os.path.join(HERE, "uncertain_small.npz")):
    warnings.simplefilter("ignore")
    _, _, dfcn, _, _ = load_reference()
    out = {}
    ref_model = dfcn.UncertainDRNSeg("drn_d_22", 5, pretrained=False, criterion=None)
    out["keys"] = np.array(json.dumps([[k, list(v.shape)] for k, v in ref_model.state_dict().items()]))
    for name, spec in CASES.items():
        d = R.make_inputs(spec["seed"], spec["n"], spec["c"], spec["hi"], spec["wi"], spec["t"])
        r64, keep = run_reference(dfcn, d, spec, torch.float64, 100 + spec["seed"], 200 + spec["seed"])
        r32, keep32 = run_reference(dfcn, d, spec, torch.float32, 100 + spec["seed"], 200 + spec["seed"])
        assert (keep == keep32).all(), "the fp32 and fp64 runs drew different dropout masks"
        assert 0 < keep.mean() < 1 and (keep.min(2) == 0).any()  # (some channel of some draw is dropped)
        np.random.seed(200 + spec["seed"])
        d["keep"], d["r"] = keep, np.array([np.random.rand() for _ in range(spec["t"])], np.float64)
        R.conditions(d)
        for form in (R.one_pass, R.literal):  # the one-pass formulas ARE the reference's loop: fp64, to rounding
            mine = form(d["s"], d["w_up"], d["w_std"], d["labels"], d["cw"], keep, d["r"], lam=LAM, gb=spec["gb"], gu=spec["gu"])
            for k in ("B", "U", "ds", "dw_up", "dw_std"):
                err = R.rel_to_max(mine[k], r64[k])
                assert err < 1e-12, (name, form.__name__, k, err)
                print("%s %-8s %-6s rel. to max %.2e   (fp32 reference: %.2e)" % (name, form.__name__, k, err, R.rel_to_max(r32[k], r64[k])))
        for k in ("s", "w_up", "w_std", "cw"):
            out["%s/%s" % (name, k)] = np.asarray(d[k], np.float32)
        out[name + "/labels"], out[name + "/keep"], out[name + "/r"] = d["labels"].astype(np.int64), keep, d["r"]
        out[name + "/gb"], out[name + "/gu"], out[name + "/lam"] = np.float64(spec["gb"]), np.array(spec["gu"], np.float64), np.float64(LAM)
        for tag, res in (("f32", r32), ("f64", r64)):
            for k, v in res.items():
                out["%s/%s/%s" % (name, tag, k)] = v
    np.savez_compressed(path, **out)
    return path


if __name__ == "__main__":
    print(main(), os.path.getsize(os.path.join(HERE, "uncertain_small.npz")), "bytes")
