"""BatchNorm2d as include/mcdseg.h states it, in plain torch-CPU float64: the statement the HIP kernels of csrc/bn.hip are held to
(tests/test_bn_contract_gpu.py) after tests/test_bn_ref_host.py has shown it equal to ``F.batch_norm`` and its autograd in float64.

Every function takes tensors of any float dtype and works in float64; per-channel vectors are [C], activations [N, C, H, W]."""
import math

import numpy as np
import torch

EPS = float(np.float32(1e-5))   # the ``float eps`` the C ABI receives
MOMENTUM = float(np.float32(0.1))


def _d(t):
    return None if t is None else t.detach().to(torch.float64)


def _c(v):
    return v.view(1, -1, 1, 1)


def running_update(running, stat, momentum=MOMENTUM, updates=1):
    """running = (1 - momentum) running + momentum stat, ``updates`` times, each rounded to fp32 as a separate pass would"""
    r = _d(running)
    for _ in range(int(updates)):
        r = ((1.0 - momentum) * r + momentum * _d(stat)).to(torch.float32).to(torch.float64)
    return r


def merge_rows(count, mean, m2, eps=EPS, running_mean=None, running_var=None, momentum=MOMENTUM, running_updates=1):
    """Merge partial rows (count, mean, M2) [rows, C] with Chan's formula: n = sum n_r, mean = sum n_r mean_r / n,
    M2 = sum M2_r + sum n_r (mean_r - mean)^2 (the centred form: no cancellation).  Returns a dict of [C] float64 vectors:
    n, mean, var (biased), rstd = 1/sqrt(var + eps), unbiased (M2 / (n - 1); the biased one when n <= 1), and -- when running
    statistics are given -- running_mean / running_var after ``running_updates`` updates."""
    cnt, mu, m2 = _d(count), _d(mean), _d(m2)
    n = cnt.sum(0)
    safe = n.clamp_min(1.0)
    m = (cnt * mu).sum(0) / safe
    M2 = m2.sum(0) + (cnt * (mu - m) ** 2).sum(0)
    var = M2 / safe
    unbiased = torch.where(n > 1, M2 / (n - 1.0).clamp_min(1.0), var)
    out = {"n": n, "mean": m, "var": var, "rstd": 1.0 / torch.sqrt(var + eps), "unbiased": unbiased}
    if running_mean is not None:
        out["running_mean"] = running_update(running_mean, m, momentum, running_updates)
        out["running_var"] = running_update(running_var, unbiased, momentum, running_updates)
    return out


def batch_stats(z, eps=EPS):
    """the train-mode statistics of z itself: one row per channel"""
    z = _d(z)
    n = z.numel() // z.shape[1]
    mean = z.mean((0, 2, 3))
    m2 = ((z - _c(mean)) ** 2).sum((0, 2, 3))
    return merge_rows(torch.full((1, z.shape[1]), float(n), dtype=torch.float64), mean[None], m2[None], eps)


def eval_stats(running_mean, running_var, eps=EPS):
    """eval mode: mean = running_mean, rstd = 1/sqrt(running_var + eps)"""
    return _d(running_mean), 1.0 / torch.sqrt(_d(running_var) + eps)


def eval_affine(gamma, beta, running_mean, running_var, conv_bias=None, eps=EPS):
    """eval-mode BatchNorm as an affine map: scale = gamma / sqrt(running_var + eps), shift = beta + (conv_bias - running_mean) scale"""
    scale = _d(gamma) / torch.sqrt(_d(running_var) + eps)
    bias = _d(conv_bias) if conv_bias is not None else 0.0
    return scale, _d(beta) + (bias - _d(running_mean)) * scale


def forward(z, mean, rstd, gamma, beta, residual=None, relu=False):
    """y = act(gamma (z - mean) rstd + beta (+ residual)), act = ReLU if relu"""
    y = _c(_d(gamma)) * ((_d(z) - _c(_d(mean))) * _c(_d(rstd))) + _c(_d(beta))
    if residual is not None:
        y = y + _d(residual)
    return y.clamp_min(0.0) if relu else y


def backward_reduce(dy, z, mean, rstd, mask=None):
    """dy_m = dy where ``mask`` (bool, y > 0 of the forward pass; None: no ReLU); dbeta = sum dy_m, dgamma = sum dy_m xhat
    (dgamma is None when z is None: the conv-bias form).  Returns (dgamma, dbeta, dy_m)."""
    g = _d(dy)
    if mask is not None:
        g = torch.where(mask, g, torch.zeros_like(g))
    dbeta = g.sum((0, 2, 3))
    if z is None:
        return None, dbeta, g
    xhat = (_d(z) - _c(_d(mean))) * _c(_d(rstd))
    return (g * xhat).sum((0, 2, 3)), dbeta, g


def backward_apply(dy, z, mean, rstd, gamma, dgamma, dbeta, mask=None, train=True):
    """dz = gamma rstd (dy_m - dbeta/n - xhat dgamma/n) (train) or gamma rstd dy_m (eval); dres = dy_m.  Returns (dz, dres)."""
    g = _d(dy)
    if mask is not None:
        g = torch.where(mask, g, torch.zeros_like(g))
    a = _c(_d(gamma) * _d(rstd))
    if not train:
        return a * g, g
    n = float(g.numel() // g.shape[1])
    xhat = (_d(z) - _c(_d(mean))) * _c(_d(rstd))
    return a * (g - _c(_d(dbeta)) / n - xhat * _c(_d(dgamma)) / n), g


def backward(dy, z, mean, rstd, gamma, mask=None, train=True):
    """reduce + apply: (dgamma, dbeta, dz, dres)"""
    dgamma, dbeta, _ = backward_reduce(dy, z, mean, rstd, mask)
    dz, dres = backward_apply(dy, z, mean, rstd, gamma, dgamma, dbeta, mask, train)
    return dgamma, dbeta, dz, dres


def y_bound(gamma, beta, n, res_bound=0.0):
    """max_c(|gamma_c| sqrt(n - 1) + |beta_c|) + res_bound (Samuelson: |xhat| <= sqrt(n - 1); train mode only)"""
    s = math.sqrt(n - 1.0) if n > 1 else 1.0
    return float((_d(gamma).abs() * s + _d(beta).abs()).max()) + float(res_bound)


def dz_bound(gamma, rstd, dy_m, dgamma, dbeta, train=True):
    """max_c |gamma_c rstd_c| (max|dy_m|_c + |dbeta_c|/n + sqrt(n - 1) |dgamma_c|/n) (train); max_c |gamma_c rstd_c| max|dy_m|_c (eval)"""
    g = _d(dy_m)
    n = float(g.numel() // g.shape[1])
    ar = (_d(gamma) * _d(rstd)).abs()
    mg = g.abs().amax((0, 2, 3))
    if not train:
        return float((ar * mg).max())
    s = math.sqrt(n - 1.0) if n > 1 else 1.0
    return float((ar * (mg + _d(dbeta).abs() / n + s * _d(dgamma).abs() / n)).max())
