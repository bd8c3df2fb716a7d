#!/usr/bin/env python3
"""Generate tests/golden/dann_small.npz by running the REAL reference's ``DownConv`` and ``DRNSegDomainClassifier`` in memory, the way
make_golden.py does (same loader: lib2to3 on the reference's text, nothing copied), in fp32 and in fp64.

    python tests/golden/make_dann_golden.py            # needs the reference checkout make_golden.py loads

Cases (inputs from tests/dann_ref.make_inputs; every case stores its inputs, and "<case>/f32/...", "<case>/f64/..." results):
  down/a     N=2, Cin=5, Cout=10, 7x9     odd both ways: the pooling drops a row and a column, a halo on every side
  down/b     N=1, Cin=41, Cout=10, 19x19  one 16-pixel tile of csrc/dann.hip + 3 each way: both halos come from a neighbour tile; 41
                                          is the largest channel count
  down/c     N=2, Cin=10, Cout=1, 6x6     the second DownConv's shape
  down/wide  N=1, Cin=1, Cout=1, 68x68    25 tiles: the second stage of the parameter gradients sums more than its 16 interleaved
                                          rows' worth of workgroup partials (the trainer's geometry has 320 per domain)
  down/ties  Cin=1, 4x4, identity kernels  windows with two and four exactly equal positive maxima, and an all-zero window
  down/ties_odd  the same on 5x5           ... plus a dropped row and column, whose input gradient is exactly zero
             results: y, dx, dw1, db1, dw2, db2 for the stored upstream gradient dy
  tail/a     G=2, n=2, F=6, labels (1,0);  tail/b  G=2, n=3, F=1089;  tail/eval  G=2, n=2, F=6 with the BatchNorm fixed (training = 0)
             the reference's classifier with conv1 / conv2 replaced by nn.Identity() and fc1 built at the case's F is called once per
             group (domain); the loss is sum_g up[g] * CrossEntropyLoss(logits_g, label_g).  results: loss [G], logits, running_mean,
             running_var (after the calls), dh, dw1, db1, dgamma, dbeta, dw2, db2; "db1_scale": the scale db1 is measured against
             in training mode, where it is a sum that cancels to zero (dann_ref.rel_to_max)
  step       two full iterations of the dann_trainer.py loop (tests/dann_ref.step, the loop of :273-326) over a 1x1-convolution
             stand-in for G (3 -> 5 channels) on a 2x3x16x24 image pair (drawn so that every batch variance D's BatchNorm1d
             sees stays above 1e-2, "step/<f32|f64>/min_variance"), the reference's DRNSegPixelClassifier(5) and
             DRNSegDomainClassifier(5) with fc1 at 24 = (16//4) (24//4), SGD from the reference's get_optimizer (lr 0.01, momentum 0.9,
             weight decay 2e-5).  "step/init/<m>.<key>": the initial state; "step/<f32|f64>/i<k>u1/{g,f}.<key>" and ".../i<k>u2/d.<key>":
             what update 1 / update 2 of iteration k changed; ".../c_loss", ".../d_loss" [2]; ".../d_alone/d.<key>": D after a FIRST
             iteration in which its gradient was zeroed before update 2 -- NOT what the reference does, stored to show the difference.
"keys": the state-dict keys of the reference's DRNSegDomainClassifier(5) with their shapes, as JSON.

What the installed torch does not run, and what was done instead: CrossEntropyLoss2d sits on nn.NLLLoss2d, which torch removed; the
criterion is ``F.cross_entropy(., weight=cw)``, the same log_softmax + weighted-mean NLL (make_uncertain_golden.py does the same).

While generating, tests/dann_ref's formulas are asserted against the reference in fp64 (1e-12 relative to max), and
dann_ref.conditions on the inputs.
"""
import copy
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
import dann_ref as R  # noqa: E402

DOWN = {"a": dict(seed=3, kind="down", n=2, cin=5, cout=10, h=7, w=9),
        "b": dict(seed=4, kind="down", n=1, cin=41, cout=10, h=19, w=19),
        "c": dict(seed=5, kind="down", n=2, cin=10, cout=1, h=6, w=6),
        "wide": dict(seed=10, kind="down", n=1, cin=1, cout=1, h=68, w=68),
        "ties": dict(seed=0, kind="ties", h=4, w=4),
        "ties_odd": dict(seed=0, kind="ties", h=5, w=5)}
TAIL = {"a": dict(seed=6, kind="tail", groups=2, n=2, f=6, labels=(1, 0)),
        "b": dict(seed=7, kind="tail", groups=2, n=3, f=1089, labels=(1, 0)),
        "eval": dict(seed=8, kind="tail", groups=2, n=2, f=6, labels=(1, 0), training=0)}
STEP = dict(seed=9, n=2, cin=3, n_class=5, h=16, w=24, lr=0.01, momentum=0.9, weight_decay=2e-5, gain=40.0, fc1_gain=60.0)


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a)).to(dtype)


def run_down(dfcn, d, dtype):
    cout, cin = d["w1"].shape[:2]
    m = dfcn.DownConv(cin, cout).to(dtype)
    with torch.no_grad():
        for p, k in ((m.conv1.weight, "w1"), (m.conv1.bias, "b1"), (m.conv2.weight, "w2"), (m.conv2.bias, "b2")):
            p.copy_(_t(d[k], dtype))
    x = _t(d["x"], dtype).requires_grad_(True)
    y = m(x)
    y.backward(_t(d["dy"], dtype))
    return {"y": y.detach().numpy(), "dx": x.grad.numpy(), "dw1": m.conv1.weight.grad.numpy(), "db1": m.conv1.bias.grad.numpy(),
            "dw2": m.conv2.weight.grad.numpy(), "db2": m.conv2.bias.grad.numpy()}


def run_tail(dfcn, ref_mu, d, dtype):
    groups, f = int(d["groups"]), d["h"].shape[1]
    n = d["h"].shape[0] // groups
    m = dfcn.DRNSegDomainClassifier(5)
    m.conv1, m.conv2, m.fc1 = nn.Identity(), nn.Identity(), nn.Linear(f, 10)
    m.to(dtype).train()
    if not int(d.get("training", 1)):
        ref_mu.fix_batchnorm_when_training(m)
    with torch.no_grad():
        for p, k in ((m.fc1.weight, "w1"), (m.fc1.bias, "b1"), (m.bn1.weight, "gamma"), (m.bn1.bias, "beta"), (m.bn1.running_mean, "rm"),
                     (m.bn1.running_var, "rv"), (m.fc2.weight, "w2"), (m.fc2.bias, "b2")):
            p.copy_(_t(d[k], dtype))
    h = _t(d["h"], dtype).requires_grad_(True)
    losses, logits = [], []
    for g in range(groups):
        out = m(h[g * n:(g + 1) * n].view(n, 1, 1, f))
        logits.append(out)
        losses.append(nn.CrossEntropyLoss()(out, torch.full((n,), int(d["labels"][g]), dtype=torch.long)))
    sum(float(u) * l for u, l in zip(d["up"], losses)).backward()
    return {"loss": torch.stack(losses).detach().numpy(), "logits": torch.cat(logits).detach().numpy(),
            "running_mean": m.bn1.running_mean.numpy().copy(), "running_var": m.bn1.running_var.numpy().copy(), "dh": h.grad.numpy(),
            "dw1": m.fc1.weight.grad.numpy(), "db1": m.fc1.bias.grad.numpy(), "dgamma": m.bn1.weight.grad.numpy(),
            "dbeta": m.bn1.bias.grad.numpy(), "dw2": m.fc2.weight.grad.numpy(), "db2": m.fc2.bias.grad.numpy()}


def step_inputs(spec, attempt=0):
    """the two samples of a domain differ in gain and offset, the images are large (``gain``) and D's fc1 starts wide (``fc1_gain``): D's
    BatchNorm1d then sees batch variances above 1e-2 in every feature (asserted in ``main`` at every call of both iterations), not ones below its eps"""
    g = torch.Generator().manual_seed(spec["seed"] + 1000 * attempt)
    n, h, w, c = spec["n"], spec["h"], spec["w"], spec["n_class"]
    cw = torch.rand(c, generator=g) + 0.5
    cw[-1] = 0.0
    per_sample = torch.tensor([1.0, -2.0]).view(n, 1, 1, 1)
    src = (torch.randn(n, spec["cin"], h, w, generator=g) + 0.5) * per_sample * spec["gain"]
    tgt = (torch.randn(n, spec["cin"], h, w, generator=g) * 1.5 - 0.3) * per_sample.flip(0) * spec["gain"]
    return {"src": src.numpy(), "tgt": tgt.numpy(),
            "lbl": torch.randint(0, c, (n, 8 * h, 8 * w), generator=g).numpy().astype(np.uint8), "cw": cw.numpy()}


def step_modules(dfcn, spec):
    torch.manual_seed(spec["seed"])
    g = nn.Conv2d(spec["cin"], spec["n_class"], 1)
    f = dfcn.DRNSegPixelClassifier(n_class=spec["n_class"])
    d = dfcn.DRNSegDomainClassifier(spec["n_class"])
    d.fc1 = nn.Linear((spec["h"] // 4) * (spec["w"] // 4), 10)
    with torch.no_grad():  # (a wide fc1: what BatchNorm1d normalises has a spread of order 10, far above sqrt(eps))
        d.fc1.weight.mul_(spec["fc1_gain"])
    return {"g": g, "f": f, "d": d}


def run_step(ref_mu, init, spec, inp, dtype, iterations, zero_d_before_update2=False):
    mods = {k: copy.deepcopy(m).to(dtype).train() for k, m in init.items()}
    opts = {k: ref_mu.get_optimizer(m.parameters(), "sgd", spec["lr"], spec["momentum"], spec["weight_decay"]) for k, m in mods.items()}
    cw = _t(inp["cw"], dtype)
    src, tgt, lbl = _t(inp["src"], dtype), _t(inp["tgt"], dtype), torch.as_tensor(inp["lbl"]).long()
    out, c_loss, d_loss, variances = {}, [], [], []
    mods["d"].fc1.register_forward_hook(lambda mod, i, o: variances.append(float(o.detach().var(0, unbiased=False).min())))
    for it in range(iterations):
        def snap(update, it=it):
            for name in (("g", "f") if update == 1 else ("d",)):
                for k, v in mods[name].state_dict().items():
                    out["i%du%d/%s.%s" % (it, update, name, k)] = v.detach().numpy().copy()
        c, dl = R.step(mods["g"], mods["f"], mods["d"], opts["g"], opts["f"], opts["d"], lambda p, t: F.cross_entropy(p, t, weight=cw),
                       src, lbl, tgt, after_update=snap, zero_d_before_update2=zero_d_before_update2)
        c_loss.append(c), d_loss.append(dl)
    out["c_loss"], out["d_loss"], out["min_variance"] = np.array(c_loss), np.array(d_loss), np.float64(min(variances))
    return out


def main(path=os.path.join(HERE, "dann_small.npz")):
    warnings.simplefilter("ignore")
    _, _, dfcn, _, ref_mu = load_reference()
    out = {"keys": np.array(json.dumps([[k, list(v.shape)] for k, v in dfcn.DRNSegDomainClassifier(5).state_dict().items()]))}

    def case(name, d, r32, r64, mine):
        for k, v in r64.items():
            scale = mine["db1_scale"] if (k == "db1" and int(d.get("training", 0))) else None  # (a sum that cancels: dann_ref.rel_to_max)
            err = R.rel_to_max(mine[k], v, scale)
            assert err < 1e-12, (name, k, err)
            print("%-14s %-12s dann_ref vs reference fp64: %.1e   (fp32 reference: %.2e)" % (name, k, err, R.rel_to_max(r32[k], v, scale)))
        if "db1_scale" in mine:
            out[name + "/db1_scale"] = np.float64(mine["db1_scale"])
        for k, v in d.items():
            v = np.asarray(v)
            out["%s/%s" % (name, k)] = v.astype(np.float32) if v.dtype.kind == "f" else v
        for tag, res in (("f32", r32), ("f64", r64)):
            for k, v in res.items():
                out["%s/%s/%s" % (name, tag, k)] = v

    for name, spec in DOWN.items():
        d = R.make_inputs(**spec)
        R.conditions(d)
        case("down/" + name, d, run_down(dfcn, d, torch.float32), run_down(dfcn, d, torch.float64), R.down_case(d))
    for name, spec in TAIL.items():
        d = R.make_inputs(**spec)
        R.conditions(d)
        case("tail/" + name, d, run_tail(dfcn, ref_mu, d, torch.float32), run_tail(dfcn, ref_mu, d, torch.float64),
             R.tail_case(d, training=bool(int(d["training"]))))

    init = step_modules(dfcn, STEP)
    for attempt in range(50):  # (the first draw whose trajectory keeps every BatchNorm1d batch variance of D above 1e-2: dann_ref.conditions' rule)
        inp = step_inputs(STEP, attempt)
        low = run_step(ref_mu, init, STEP, inp, torch.float64, 2)["min_variance"]
        print("step: draw %d, the smallest batch variance BatchNorm1d sees in two iterations: %.3e" % (attempt, low))
        if low > 1e-2:
            break
    else:
        raise RuntimeError("no draw of the step case meets the variance condition")
    for k, v in inp.items():
        out["step/" + k] = v
    for name, m in init.items():
        for k, v in m.state_dict().items():
            out["step/init/%s.%s" % (name, k)] = v.numpy().copy()
    out["step/hyper"] = np.array([STEP["lr"], STEP["momentum"], STEP["weight_decay"]])
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        for k, v in run_step(ref_mu, init, STEP, inp, dtype, 2).items():
            out["step/%s/%s" % (tag, k)] = v
        assert out["step/%s/min_variance" % tag] > 1e-2
        alone = run_step(ref_mu, init, STEP, inp, dtype, 1, zero_d_before_update2=True)
        for k, v in alone.items():
            if k.startswith("i0u2/"):
                out["step/%s/d_alone/%s" % (tag, k[5:])] = v
    # the carried-over gradient is visible: D's first step is not the step on update 2's gradient alone
    gap = max(R.rel_to_max(out["step/f64/i0u2/" + k[len("step/f64/d_alone/"):]], v) for k, v in out.items()
              if k.startswith("step/f64/d_alone/") and k.endswith("weight"))
    print("step: D after iteration 0 vs the step on update 2's gradient alone: %.2e relative to max" % gap)
    assert gap > 1e-4
    np.savez_compressed(path, **out)
    return path


if __name__ == "__main__":
    print(main(), os.path.getsize(os.path.join(HERE, "dann_small.npz")), "bytes")
