"""The domain classifier of the DANN baseline restated in numpy / fp64 -- what csrc/dann.hip computes, written out as formulas, and the
two-update iteration of dann_trainer.py over given modules.  tests/golden/make_dann_golden.py asserts all of it against the real
reference in fp64 (1e-12 relative to max); the tests compare the HIP kernels with the golden data and use this module to recompute it.

  down_fwd / down_bwd     DownConv: conv3x3+bias, ReLU, conv3x3+bias, ReLU, MaxPool2d(2,2); the pooling's gradient goes to the FIRST
                          maximum of a window in row-major order (np.argmax's rule and torch's), and nowhere when that is a ReLU zero
  tail_fwd / tail_bwd     Linear(F,10), BatchNorm1d(10) with statistics per group, ReLU, Linear(10,2), mean cross-entropy per group
  step                    one iteration = the two updates (with D's gradient of update 1 left in place), over torch modules
  make_inputs, conditions the test data and what makes a comparison on it meaningful
"""
import numpy as np
import torch

HID = 10
DOWN = ("down/a", "down/b", "down/c", "down/wide", "down/ties", "down/ties_odd")  # the kernel cases of tests/golden/dann_small.npz
TAIL = ("tail/a", "tail/b", "tail/eval")


def case(fx, name):
    """the inputs of one golden case (everything stored under "<name>/" but the reference's results)"""
    skip = ("f32/", "f64/")
    return {k[len(name) + 1:]: fx[k] for k in fx.files if k.startswith(name + "/") and not k[len(name) + 1:].startswith(skip)}


def rel_to_max(x, truth, scale=None):
    """distance of ``x`` to ``truth`` relative to the truth's largest magnitude (the project's per-tensor error measure), or to ``scale``
    where the truth is a sum whose terms cancel (fc1's bias gradient behind a training-mode BatchNorm1d is zero in exact arithmetic:
    its scale is the largest sum of the terms' magnitudes, ``db1_scale``)"""
    truth = np.asarray(truth, np.float64)
    den = float(np.abs(truth).max()) if scale is None else float(scale)
    return float(np.abs(np.asarray(x, np.float64) - truth).max()) / (den if den > 0 else 1.0)


def _f64(*xs):
    return [np.asarray(x, np.float64) for x in xs]


# ------------------------------------------------------------------------------------------------ DownConv
def conv3x3(x, w, b):
    n, c, h, wd = x.shape
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    z = np.zeros((n, w.shape[0], h, wd)) + b[None, :, None, None]
    for a in range(3):
        for d in range(3):
            z += np.einsum("nchw,oc->nohw", xp[:, :, a:a + h, d:d + wd], w[:, :, a, d])
    return z


def conv3x3_bwd(x, w, dz):
    n, c, h, wd = x.shape
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    dzp = np.pad(dz, ((0, 0), (0, 0), (1, 1), (1, 1)))
    dx, dw = np.zeros_like(x), np.zeros_like(w)
    for a in range(3):
        for d in range(3):
            dx += np.einsum("nohw,oc->nchw", dzp[:, :, 2 - a:2 - a + h, 2 - d:2 - d + wd], w[:, :, a, d])
            dw[:, :, a, d] = np.einsum("nohw,nchw->oc", dz, xp[:, :, a:a + h, d:d + wd])
    return dx, dw, dz.sum((0, 2, 3))


def _windows(a):
    """[N,C,H,W] -> [N,C,H//2,W//2,4], a window's elements in row-major order; the last row / column of an odd map is left out"""
    n, c, h, w = a.shape
    hp, wp = h // 2, w // 2
    return a[:, :, :2 * hp, :2 * wp].reshape(n, c, hp, 2, wp, 2).transpose(0, 1, 2, 4, 3, 5).reshape(n, c, hp, wp, 4)


def down_fwd(x, w1, b1, w2, b2):
    x, w1, b1, w2, b2 = _f64(x, w1, b1, w2, b2)
    z1 = conv3x3(x, w1, b1)
    a1 = np.maximum(z1, 0)
    z2 = conv3x3(a1, w2, b2)
    a2 = np.maximum(z2, 0)
    win = _windows(a2)
    arg = win.argmax(-1)  # the first maximum
    return {"x": x, "w1": w1, "w2": w2, "z1": z1, "a1": a1, "z2": z2, "a2": a2, "arg": arg, "y": win.max(-1)}


def pool_bwd(arg, dy, shape):
    n, c, h, w = shape
    hp, wp = h // 2, w // 2
    g = np.zeros((n, c, hp, wp, 4))
    np.put_along_axis(g, arg[..., None], np.asarray(dy, np.float64)[..., None], -1)
    out = np.zeros(shape)
    out[:, :, :2 * hp, :2 * wp] = g.reshape(n, c, hp, wp, 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(n, c, 2 * hp, 2 * wp)
    return out


def down_bwd(f, dy):
    da2 = pool_bwd(f["arg"], dy, f["a2"].shape)
    dz2 = da2 * (f["z2"] > 0)
    da1, dw2, db2 = conv3x3_bwd(f["a1"], f["w2"], dz2)
    dz1 = da1 * (f["z1"] > 0)
    dx, dw1, db1 = conv3x3_bwd(f["x"], f["w1"], dz1)
    return {"dx": dx, "dw1": dw1, "db1": db1, "dw2": dw2, "db2": db2, "da2": da2}


# ------------------------------------------------------------------------------------------------ the tail
def tail_fwd(h, labels, w1, b1, gamma, beta, rm, rv, w2, b2, groups, momentum=0.1, eps=1e-5, training=True):
    h, w1, b1, gamma, beta, rm, rv, w2, b2 = _f64(h, w1, b1, gamma, beta, rm, rv, w2, b2)
    rows = h.shape[0]
    n = rows // groups
    z = h @ w1.T + b1
    zg = z.reshape(groups, n, HID)
    rm, rv = rm.copy(), rv.copy()
    if training:
        mean, var = zg.mean(1), zg.var(1)  # biased variance normalises
        for g in range(groups):            # the groups in order, as one module call per domain
            rm = (1 - momentum) * rm + momentum * mean[g]
            rv = (1 - momentum) * rv + momentum * var[g] * n / (n - 1)
    else:
        mean, var = np.tile(rm, (groups, 1)), np.tile(rv, (groups, 1))
    rstd = 1.0 / np.sqrt(var + eps)
    xhat = (zg - mean[:, None]) * rstd[:, None]
    bn = xhat * gamma + beta
    a = np.maximum(bn, 0)
    logits = a.reshape(rows, HID) @ w2.T + b2
    lg = logits.reshape(groups, n, 2)
    m = lg.max(-1, keepdims=True)
    lse = m[..., 0] + np.log(np.exp(lg - m).sum(-1))
    lab = np.asarray(labels).astype(np.int64)
    picked = np.take_along_axis(lg, np.broadcast_to(lab[:, None, None], (groups, n, 1)), -1)[..., 0]
    loss = (lse - picked).mean(1)
    return {"h": h, "w1": w1, "w2": w2, "gamma": gamma, "z": z, "xhat": xhat, "bn": bn, "a": a, "rstd": rstd, "logits": logits, "loss": loss,
            "running_mean": rm, "running_var": rv, "labels": lab, "groups": groups, "n": n, "training": training}


def tail_bwd(f, upstream):
    groups, n = f["groups"], f["n"]
    lg = f["logits"].reshape(groups, n, 2)
    p = np.exp(lg - lg.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    onehot = np.eye(2)[f["labels"]][:, None, :]
    dl = (p - onehot) * (np.asarray(upstream, np.float64)[:, None, None] / n)
    a = f["a"].reshape(groups * n, HID)
    dl2 = dl.reshape(groups * n, 2)
    dw2, db2 = dl2.T @ a, dl2.sum(0)
    dbn = (dl2 @ f["w2"]).reshape(groups, n, HID) * (f["bn"] > 0)
    dgamma, dbeta = (dbn * f["xhat"]).sum((0, 1)), dbn.sum((0, 1))
    if f["training"]:
        dz = f["gamma"] * f["rstd"][:, None] * (dbn - dbn.mean(1, keepdims=True) - f["xhat"] * (dbn * f["xhat"]).mean(1, keepdims=True))
    else:
        dz = f["gamma"] * f["rstd"][:, None] * dbn
    dz = dz.reshape(groups * n, HID)
    return {"db1_scale": np.abs(dz).sum(0).max(), "dh": dz @ f["w1"], "dw1": dz.T @ f["h"], "db1": dz.sum(0), "dgamma": dgamma, "dbeta": dbeta, "dw2": dw2, "db2": db2}


TAIL_PARAMS = ("w1", "b1", "gamma", "beta", "rm", "rv", "w2", "b2")


def tail_case(d, training=True):
    f = tail_fwd(d["h"], d["labels"], *[d[k] for k in TAIL_PARAMS], groups=int(d["groups"]), training=training)
    out = {k: f[k] for k in ("loss", "logits", "running_mean", "running_var")}
    out.update(tail_bwd(f, d["up"]))
    return out


def down_case(d):
    f = down_fwd(d["x"], d["w1"], d["b1"], d["w2"], d["b2"])
    out = {"y": f["y"]}
    out.update({k: v for k, v in down_bwd(f, d["dy"]).items() if k != "da2"})
    return out


# ------------------------------------------------------------------------------------------------ one iteration of the trainer
def step(model_g, model_f, model_d, opt_g, opt_f, opt_d, criterion, src, lbl, tgt, num_k=1, after_update=None, zero_d_before_update2=False):
    """dann_trainer.py:273-326 over the given modules: update 1 descends CE(F(G(src))) - CE(D(G(src)),1) - CE(D(G(tgt)),0) in G and F --
    D receives that (negative) gradient too and keeps it --; update 2 adds the gradient of +CE +CE on the new G and steps D, which is
    zeroed only then.  Returns (c_loss, d_loss).  ``zero_d_before_update2`` is NOT the reference: it is the step D would take on update
    2's gradient alone, which the golden data stores to show that the two differ."""
    ce = torch.nn.functional.cross_entropy
    ones = torch.ones(src.shape[0], dtype=torch.long, device=src.device)
    opt_g.zero_grad()
    opt_f.zero_grad()
    src_fet, tgt_fet = model_g(src), model_g(tgt)
    loss_d = -ce(model_d(src_fet), ones)
    loss_d = loss_d - ce(model_d(tgt_fet), 0 * ones)
    loss = criterion(model_f(src_fet), lbl)
    c_loss = float(loss.detach())
    (loss + loss_d).backward()
    opt_g.step()
    opt_f.step()
    if after_update is not None:
        after_update(1)
    opt_g.zero_grad()
    opt_f.zero_grad()
    if zero_d_before_update2:
        opt_d.zero_grad()
    src_fet, tgt_fet = model_g(src), model_g(tgt)
    loss_d = ce(model_d(src_fet), ones) + ce(model_d(tgt_fet), 0 * ones)
    loss_d.backward()
    opt_d.step()
    opt_d.zero_grad()
    if after_update is not None:
        after_update(2)
    return c_loss, float(loss_d.detach()) / num_k


class TorchDomainClassifier(torch.nn.Module):
    """the classifier composed from torch modules with the reference's attribute names (a test double for the CPU tests: the product's
    module runs on HIP kernels only)"""

    class _Down(torch.nn.Module):
        def __init__(self, cin, cout):
            super().__init__()
            self.conv1 = torch.nn.Conv2d(cin, cout, 3, padding=1)
            self.conv2 = torch.nn.Conv2d(cout, cout, 3, padding=1)

        def forward(self, x):
            return torch.nn.functional.max_pool2d(torch.relu(self.conv2(torch.relu(self.conv1(x)))), 2, 2)

    def __init__(self, n_class, fc_in):
        super().__init__()
        self.conv1, self.conv2 = self._Down(n_class, HID), self._Down(HID, 1)
        self.fc1, self.bn1, self.fc2 = torch.nn.Linear(fc_in, HID), torch.nn.BatchNorm1d(HID), torch.nn.Linear(HID, 2)

    def forward(self, x):
        h = self.conv2(self.conv1(x))
        return self.fc2(torch.relu(self.bn1(self.fc1(h.view(h.size(0), -1)))))


# ------------------------------------------------------------------------------------------------ test data
def _down_inputs(rng, n, cin, cout, h, w):
    """weights scaled so that the pre-activations have a spread of tens: a value within 1e-3 of the ReLU kink is then rare enough that a
    few draws find data without one"""
    x = rng.standard_normal((n, cin, h, w))
    w1 = rng.standard_normal((cout, cin, 3, 3)) * (10.0 / np.sqrt(9 * cin))
    b1 = rng.standard_normal(cout)
    w2 = rng.standard_normal((cout, cout, 3, 3)) * (3.0 / np.sqrt(9 * cout))
    b2 = rng.standard_normal(cout)
    dy = rng.standard_normal((n, cout, h // 2, w // 2))
    return {"x": x, "w1": w1, "b1": b1, "w2": w2, "b2": b2, "dy": dy}


def _ties_inputs(h, w):
    """Cin = Cout = 1, identity kernels (centre tap 1, no bias): a2 = relu(x), so the windows are the input's and dx is the routed dy
    itself.  The 4 x 4 map holds a window with two equal positive maxima (first at index 1), one with four, one all zero (negative
    inputs) and one ordinary; the 5 x 5 map adds a dropped last row and column, whose dx must be exactly 0."""
    x = np.array([[1.0, 3.0, 2.0, 2.0],
                  [3.0, 0.5, 2.0, 2.0],
                  [-1.0, -2.0, 0.25, 4.0],
                  [-3.0, -0.5, 1.0, 0.5]])
    if (h, w) == (5, 5):
        x = np.pad(x, ((0, 1), (0, 1)), constant_values=7.0)
    ident = np.zeros((1, 1, 3, 3))
    ident[0, 0, 1, 1] = 1.0
    dy = np.array([[0.5, -1.5], [2.0, 0.75]])
    return {"x": x[None, None], "w1": ident, "b1": np.zeros(1), "w2": ident.copy(), "b2": np.zeros(1), "dy": dy[None, None], "ties": np.int64(1)}


def _tail_inputs(rng, groups, n, f, labels):
    rows = groups * n
    return {"h": np.abs(rng.standard_normal((rows, f))), "labels": np.array(labels, np.int32), "groups": np.int64(groups),
            "w1": rng.standard_normal((HID, f)) / np.sqrt(f), "b1": rng.standard_normal(HID) * 0.1, "gamma": rng.random(HID) + 0.5,
            "beta": rng.standard_normal(HID) * 0.5, "rm": rng.standard_normal(HID) * 0.3, "rv": rng.random(HID) + 0.5,
            "w2": rng.standard_normal((2, HID)) * 0.5, "b2": rng.standard_normal(2) * 0.1, "up": np.array([-1.0, 1.0, 0.7][:groups])}


def make_inputs(seed, kind, **shape):
    """kind "down": n, cin, cout, h, w; "ties": h, w; "tail": groups, n, f, labels, training.  Draws until ``conditions`` holds (the draw
    that does is a function of the seed alone), and rounds everything to fp32 values first: the kernels and fp64 see the same numbers."""
    if kind == "ties":
        d = _ties_inputs(shape["h"], shape["w"])
        conditions(d)
        return d
    for attempt in range(400):
        rng = np.random.default_rng([seed, attempt])
        if kind == "down":
            d = _down_inputs(rng, shape["n"], shape["cin"], shape["cout"], shape["h"], shape["w"])
        else:
            d = _tail_inputs(rng, shape["groups"], shape["n"], shape["f"], shape["labels"])
            d["training"] = np.int64(shape.get("training", 1))
        d = {k: (np.asarray(v, np.float32).astype(np.float64) if np.asarray(v).dtype.kind == "f" else v) for k, v in d.items()}
        try:
            conditions(d)
        except AssertionError:
            continue
        return d
    raise RuntimeError("no draw of seed %d meets the conditions" % seed)


def conditions(d):
    """What makes fp32-against-fp64 meaningful on this data.  DownConv: no pre-activation within 1e-3 of the ReLU kink and, in every
    pooling window with a positive maximum, the two largest values more than 1e-3 apart -- except in a "ties" case, whose zeros and
    equal maxima are exact in every precision.  Tail: every BatchNorm1d feature has a batch variance above 1e-2 in each group (training
    mode), and no BatchNorm output lies within 1e-3 of the kink."""
    if "x" in d:
        f = down_fwd(d["x"], d["w1"], d["b1"], d["w2"], d["b2"])
        if "ties" in d:
            assert np.array_equal(f["a2"], np.maximum(d["x"], 0))
            return
        for z in (f["z1"], f["z2"]):
            assert float(np.abs(z).min()) >= 1e-3, float(np.abs(z).min())
        top = np.sort(_windows(f["a2"]), -1)
        live = top[..., 3] > 0
        assert live.any() and float((top[..., 3] - top[..., 2])[live].min()) > 1e-3
        return
    training = bool(d.get("training", 1))
    f = tail_fwd(d["h"], d["labels"], *[d[k] for k in TAIL_PARAMS], groups=int(d["groups"]), training=training)
    if training:
        assert float(f["z"].reshape(f["groups"], f["n"], HID).var(1).min()) > 1e-2
    assert float(np.abs(f["bn"]).min()) >= 1e-3
    assert (f["bn"] > 0).any() and (f["bn"] < 0).any()
