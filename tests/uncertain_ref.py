"""Restatement of the Monte-Carlo dropout loss of the uncertain model (include/mcdseg.h: mcdseg_up8_uncertain_loss_fwd / _bwd) in torch
on the CPU, in whatever dtype it is asked for.  A test helper, like refine_ref.py; nothing here is used by the package.

  one_pass(...)   the formulas the kernel implements: U = up(s) and V = up_std(s) formed ONCE, the T draws applied per pixel, the
                  closed forms of GU = dL/dU and GV = dL/dV, and torch's transposed convolution for d/ds and the weight gradients
  literal(...)    the reference's loop (models/dilated_fcn.py:176-204): T passes m_t s -> up, relu(up_std) -> cross entropy and
                  exp(y_hat[g] - log(sum(exp(y_hat)))) summed over the draws, gradients by autograd.  In fp32 it is the yardstick the
                  GPU tests measure the kernel's error in; in fp64 it is the truth where no golden value exists
  std_sum(...)    relu(up_std(s))[:, :n_used].sum(1)
  extra_case(C, T, variant)   the inputs of tests/test_uncertain_gpu.py beyond the golden cases
  conditions(...)             what every input set of these tests satisfies (asserted by the fixture generator and the tests)

Both return {"B", "U", "W", "ds", "dw_up", "dw_std"} (numpy, the dtype asked for); gb / gu are the upstream gradients of B and U_n.
Pixels whose label is ignore_index or outside [0, C) contribute to nothing; HW stays the full pixel count.
"""
import numpy as np
import torch
import torch.nn.functional as F

IGNORE = -100


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a)).to(dtype)


def up(s, w):
    return F.conv_transpose2d(s, w, stride=8, padding=4, groups=s.shape[1])


def _prep(s, w_up, w_std, labels, cw, keep, r, dtype, keep_scale, ignore_index):
    s, w_up, w_std = (_t(a, dtype).clone().requires_grad_(True) for a in (s, w_up, w_std))
    labels = torch.as_tensor(np.asarray(labels)).long()
    c = w_up.shape[0]  # (not s.shape[1]: with a trunk, s is the network's input)
    cw = torch.ones(c, dtype=dtype) if cw is None else _t(cw, dtype)
    m = _t(keep, dtype) * torch.tensor(keep_scale, dtype=dtype)   # [T,N,C]
    r = _t(r, dtype)
    valid = (labels != ignore_index) & (labels >= 0) & (labels < c)
    g = torch.where(valid, labels, torch.zeros_like(labels))
    wy = torch.where(valid, cw[g], torch.zeros((), dtype=dtype))
    return s, w_up, w_std, m, r, valid, g, wy


def _pack(B, Un, W, grads, dtype):
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    out = {"B": np.asarray(B.detach().numpy(), np_dt), "U": np.asarray(Un.detach().numpy(), np_dt), "W": np.asarray(W.detach().numpy(), np_dt)}
    for k, v in zip(("ds", "dw_up", "dw_std"), grads):
        out[k] = np.asarray(v.detach().numpy(), np_dt)
    return out


def literal(s, w_up, w_std, labels, cw, keep, r, lam=0.1, gb=1.0, gu=None, wsum=None, keep_scale=1.25, ignore_index=IGNORE,
            dtype=torch.float64, trunk=None):
    """``trunk`` (a module already in ``dtype``): ``s`` is then the network's INPUT and every draw runs ``trunk(s)`` anew, as the
    reference's loop does; the result also holds "trunk": {parameter name: gradient} and "ds" is left out."""
    s, w_up, w_std, m, r, valid, g, wy = _prep(s, w_up, w_std, labels, cw, keep, r, dtype, keep_scale, ignore_index)
    x = s.detach() if trunk is not None else None
    n, c = s.shape[0], w_up.shape[0]
    t_n = m.shape[0]
    hw = valid[0].numel()
    W = wy.sum() if wsum is None else _t(wsum, dtype).reshape(())
    B, psum = 0, 0
    for t in range(t_n):
        st = (s if trunk is None else trunk(x)) * m[t][:, :, None, None]
        pred_mean, pred_std = up(st, w_up), torch.relu(up(st, w_std))
        nll = -torch.gather(F.log_softmax(pred_mean, 1), 1, g[:, None])[:, 0]
        B = B + (wy * nll).sum() / W
        y_hat = pred_mean + pred_std * r[t]
        psum = psum + torch.exp(torch.gather(y_hat, 1, g[:, None])[:, 0] - torch.log(torch.exp(y_hat).sum(1)))
    B = B / t_n
    Un = torch.where(valid, torch.log(psum / t_n), torch.zeros((), dtype=dtype)).sum((1, 2)) / hw * lam
    gu = torch.ones(n, dtype=dtype) if gu is None else _t(gu, dtype)
    if trunk is None:
        return _pack(B, Un, W, torch.autograd.grad(B * gb + (Un * gu).sum(), (s, w_up, w_std)), dtype)
    named = list(trunk.named_parameters())
    grads = torch.autograd.grad(B * gb + (Un * gu).sum(), [w_up, w_std] + [p for _, p in named])
    out = _pack(B, Un, W, (grads[0], grads[0], grads[1]), dtype)
    del out["ds"]  # (no single score map exists in this form)
    out["trunk"] = {k: v.detach().numpy() for (k, _), v in zip(named, grads[2:])}
    return out


def one_pass(s, w_up, w_std, labels, cw, keep, r, lam=0.1, gb=1.0, gu=None, wsum=None, keep_scale=1.25, ignore_index=IGNORE,
             dtype=torch.float64):
    s, w_up, w_std, m, r, valid, g, wy = _prep(s, w_up, w_std, labels, cw, keep, r, dtype, keep_scale, ignore_index)
    n, c = s.shape[:2]
    t_n = m.shape[0]
    hw = valid[0].numel()
    W = wy.sum() if wsum is None else _t(wsum, dtype).reshape(())
    gu = torch.ones(n, dtype=dtype) if gu is None else _t(gu, dtype)
    U, V = up(s, w_up), up(s, w_std)
    Ud, R = U.detach(), torch.relu(V.detach())
    onehot = F.one_hot(g, c).permute(0, 3, 1, 2).to(dtype)
    vf = valid.to(dtype)
    ce, S, drawn = 0, 0, []
    for t in range(t_n):
        mt = m[t][:, :, None, None]
        y = mt * Ud
        y_hat = y + (mt * R) * r[t]
        lse = torch.logsumexp(y, 1)
        ce = ce + (wy * (lse - torch.gather(y, 1, g[:, None])[:, 0])).sum()
        sm_hat = torch.softmax(y_hat, 1)
        p = torch.gather(sm_hat, 1, g[:, None])[:, 0]
        S = S + p
        drawn.append((mt, torch.softmax(y, 1), sm_hat, p, r[t]))
    B = ce / (t_n * W)
    Un = (vf * torch.log(torch.where(valid, S, torch.ones((), dtype=dtype)) / t_n)).sum((1, 2)) * (lam / hw)
    GU, GV = torch.zeros_like(Ud), torch.zeros_like(Ud)
    for mt, sm, sm_hat, p, rt in drawn:
        a = (gb * wy / (t_n * W))[:, None] * (sm - onehot)
        b = (gu[:, None, None] * (lam / hw) * vf * p / torch.where(valid, S, torch.ones((), dtype=dtype)))[:, None] * (onehot - sm_hat)
        GU += mt * (a + b)
        GV += mt * (V.detach() > 0).to(dtype) * rt * b
    grads = torch.autograd.grad((U, V), (s, w_up, w_std), (GU, GV))
    return _pack(B, Un, W, grads, dtype)


def std_sum(s, w_std, n_used, dtype=torch.float64):
    return torch.relu(up(_t(s, dtype), _t(w_std, dtype)))[:, :n_used].sum(1).numpy()


def make_inputs(seed, n, c, hi, wi, t):
    """scores, the two up-sampling kernels, labels, class weights (zero for the last class), keep bits and r.  The scores are positive
    and the sign of a ``w_std`` tap depends on the class and on the tap's phase (ky % 8, kx % 8) only -- the four taps a pixel uses share
    their phase -- so V = up_std(s) changes sign inside every channel and |V| >= 0.5 * 0.05 everywhere: no pixel sits on relu's kink."""
    g = torch.Generator().manual_seed(seed)
    s = torch.rand(n, c, hi, wi, generator=g) + 0.5
    w_up = torch.randn(c, 1, 16, 16, generator=g) * 0.5
    sign = (torch.rand(c, 1, 8, 8, generator=g) < 0.5).float() * 2 - 1
    w_std = (torch.rand(c, 1, 16, 16, generator=g) * 0.1 + 0.05) * sign.repeat(1, 1, 2, 2)
    labels = torch.randint(0, c, (n, 8 * hi, 8 * wi), generator=g)
    cw = torch.rand(c, generator=g) + 0.5
    cw[-1] = 0.0
    keep = (torch.rand(t, n, c, generator=g) >= 0.2).to(torch.uint8)
    r = torch.rand(t, generator=g)
    return {"s": s.numpy(), "w_up": w_up.numpy(), "w_std": w_std.numpy(), "labels": labels.numpy(), "cw": cw.numpy(),
            "keep": keep.numpy(), "r": r.numpy()}


VARIANTS = ("plain", "wsum", "gb0", "gu0")


def extra_case(c, t, variant):
    """N = 2, 3 x 9 scores (24 x 72 pixels: a row crosses the 64-column segment).  Draw 0 drops the channel of sample 0's first label,
    the last draw drops every channel of sample 1, 3 % of the labels are ignore_index and 3 % equal C."""
    assert variant in VARIANTS
    n, hi, wi = 2, 3, 9
    d = make_inputs(1000 + 10 * c + t, n, c, hi, wi, t)
    g = torch.Generator().manual_seed(c + t)
    labels = torch.from_numpy(d["labels"]).clone()
    u = torch.rand(labels.shape, generator=g)
    labels[u < 0.03] = IGNORE
    labels[(u >= 0.03) & (u < 0.06)] = c
    labels[0, 0, 0] = 1  # (a valid label whose channel draw 0 drops)
    d["labels"] = labels.numpy()
    d["keep"][0, 0, 1] = 0
    d["keep"][t - 1, 1, :] = 0
    d["lam"] = 0.1
    d["gb"], d["gu"] = (0.0 if variant == "gb0" else 0.7), np.array([0.0, 0.0] if variant == "gu0" else [1.3, -0.4], np.float32)
    d["wsum"] = np.array([777.0], np.float32) if variant == "wsum" else None
    return d


def conditions(d):
    """no |V| < 1e-4 (relu's kink), every S_i > 1e-20, at most 10 % of the pixels ignored"""
    s, w_std = _t(d["s"], torch.float64), _t(d["w_std"], torch.float64)
    V = up(s, w_std)
    assert float(V.abs().min()) >= 1e-4, float(V.abs().min())
    labels = torch.as_tensor(d["labels"]).long()
    c = s.shape[1]
    valid = (labels != IGNORE) & (labels >= 0) & (labels < c)
    assert float((~valid).float().mean()) <= 0.10
    U = up(s, _t(d["w_up"], torch.float64))
    m = _t(d["keep"], torch.float64) * 1.25
    g = torch.where(valid, labels, torch.zeros_like(labels))
    S = 0
    for t in range(m.shape[0]):
        mt = m[t][:, :, None, None]
        S = S + torch.gather(torch.softmax(mt * U + mt * torch.relu(V) * float(d["r"][t]), 1), 1, g[:, None])[:, 0]
    assert float(S[valid].min()) > 1e-20, float(S[valid].min())
    return True


def rel_to_max(x, truth):
    """distance of ``x`` to ``truth`` relative to the truth's largest magnitude (the project's per-tensor error measure)"""
    truth = np.asarray(truth, np.float64)
    den = float(np.abs(truth).max())
    return float(np.abs(np.asarray(x, np.float64) - truth).max()) / (den if den > 0 else 1.0)
