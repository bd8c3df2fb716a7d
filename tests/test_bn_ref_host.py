"""Host: tests/bn_ref.py -- the float64 statement of include/mcdseg.h's BatchNorm that tests/test_bn_contract_gpu.py holds the HIP
kernels to -- against ``F.batch_norm`` and its autograd in float64, at benign statistics and at |mean|/std = 1e3, with and without
residual and ReLU, in train and eval mode.  The reference is shown right here before any kernel is judged by it."""
import math

import pytest
import torch
import torch.nn.functional as F

import bn_ref

N, C, H, W = 3, 6, 10, 20   # n = 600 values per channel


def _data(adverse, seed=5):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    z = z * 1e-2 + 10.0 if adverse else z + 0.3          # |mean|/std = 1e3 or 0.3
    gamma = torch.randn(C, generator=g, dtype=torch.float64) + 1.0
    beta = torch.randn(C, generator=g, dtype=torch.float64) * 0.3
    res = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    dy = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    if adverse:  # running statistics of the same kind as the data's
        rm = 10.0 + 1e-3 * torch.randn(C, generator=g, dtype=torch.float64)
        rv = 1e-4 * (1.0 + 0.1 * torch.rand(C, generator=g, dtype=torch.float64))
    else:
        rm = 0.3 + 0.05 * torch.randn(C, generator=g, dtype=torch.float64)
        rv = 1.0 + 0.1 * torch.rand(C, generator=g, dtype=torch.float64)
    return z, gamma, beta, res, dy, rm, rv


def _close(got, want, what, rtol=1e-11):
    # float64 on both sides: what differs is the order of the operations -- a few 1e-16 of the terms that cancel, which at
    # |mean|/std = 1e3 are 1e3 times the result
    err = float((got - want).abs().max())
    scale = float(want.abs().max()) + 1e-300
    assert err <= rtol * scale, "%s: %.3e of %.3e" % (what, err, scale)


@pytest.mark.parametrize("adverse", [False, True], ids=["benign", "mean_over_std_1e3"])
@pytest.mark.parametrize("use_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_forward_and_backward_are_batch_norm_and_its_autograd(adverse, use_res, relu, train):
    z, gamma, beta, res, dy, rm, rv = _data(adverse)
    zz, gg, bb, rr = (t.clone().requires_grad_() for t in (z, gamma, beta, res))
    run_m, run_v = rm.clone(), rv.clone()
    o = F.batch_norm(zz, run_m, run_v, gg, bb, training=train, momentum=0.1, eps=bn_ref.EPS)
    if use_res:
        o = o + rr
    if relu:
        o = F.relu(o)
    grads = torch.autograd.grad(o, [zz, gg, bb] + ([rr] if use_res else []), dy)

    if train:
        st = bn_ref.merge_rows(torch.full((1, C), float(N * H * W)), z.mean((0, 2, 3))[None],
                               ((z - z.mean((0, 2, 3), keepdim=True)) ** 2).sum((0, 2, 3))[None],
                               running_mean=rm, running_var=rv, momentum=0.1)
        mean, rstd = st["mean"], st["rstd"]
        # (the running statistics are rounded to fp32 per update by definition: compare at that resolution)
        _close(st["running_mean"], run_m, "running_mean", 1e-7)
        _close(st["running_var"], run_v, "running_var", 1e-7)
        _close(st["var"], z.var((0, 2, 3), unbiased=False), "biased variance", 1e-9)
        _close(st["unbiased"], z.var((0, 2, 3), unbiased=True), "unbiased variance", 1e-9)
        bs = bn_ref.batch_stats(z)
        assert torch.equal(bs["mean"], mean) and torch.equal(bs["rstd"], rstd)
    else:
        mean, rstd = bn_ref.eval_stats(rm, rv)
    y = bn_ref.forward(z, mean, rstd, gamma, beta, res if use_res else None, relu)
    _close(y, o.detach(), "y")
    mask = (o.detach() > 0) if relu else None
    dgamma, dbeta, dz, dres = bn_ref.backward(dy, z, mean, rstd, gamma, mask, train)
    _close(dz, grads[0], "dz", 1e-9)
    _close(dgamma, grads[1], "dgamma", 1e-9)
    _close(dbeta, grads[2], "dbeta")
    if use_res:
        assert torch.equal(dres, grads[3]), "dres is dy under the mask: exact"


@pytest.mark.parametrize("rows", [1, 7, 333])
@pytest.mark.parametrize("adverse", [False, True], ids=["benign", "mean_over_std_1e3"])
def test_merge_of_partial_rows_is_the_statistics_of_the_whole(rows, adverse):
    z = _data(adverse)[0]
    flat = z.permute(1, 0, 2, 3).reshape(C, -1)
    n = flat.shape[1]
    edges = [(n * r) // rows for r in range(rows + 1)]
    cnt, mu, m2 = torch.zeros(rows, C, dtype=torch.float64), torch.zeros(rows, C, dtype=torch.float64), torch.zeros(rows, C, dtype=torch.float64)
    for r in range(rows):
        s = flat[:, edges[r]:edges[r + 1]]
        if s.shape[1]:
            cnt[r], mu[r] = s.shape[1], s.mean(1)
            m2[r] = ((s - mu[r][:, None]) ** 2).sum(1)
    st = bn_ref.merge_rows(cnt, mu, m2)
    assert float(st["n"][0]) == n
    _close(st["mean"], flat.mean(1), "mean", 1e-13)
    _close(st["var"], flat.var(1, unbiased=False), "var", 1e-9)
    _close(st["rstd"], 1.0 / torch.sqrt(flat.var(1, unbiased=False) + bn_ref.EPS), "rstd", 1e-9)
    _close(st["unbiased"], flat.var(1, unbiased=True), "unbiased", 1e-9)


def test_running_update_rounds_every_update_to_fp32():
    rm = torch.tensor([0.25, -3.0], dtype=torch.float32)
    stat = torch.tensor([1.0 / 3.0, 1000.123456789], dtype=torch.float64)
    want = rm.clone()
    for _ in range(3):
        want = (0.9 * want.double() + 0.1 * stat).float()
    got = bn_ref.running_update(rm, stat, 0.1, 3)
    assert torch.equal(got, want.double())
    once = bn_ref.running_update(rm, stat, 0.1, 1)
    assert torch.equal(once, (0.9 * rm.double() + 0.1 * stat).float().double())


def test_bound_formulas():
    gamma = torch.tensor([0.5, -2.0, 0.0])
    beta = torch.tensor([3.0, -0.25, 0.0])
    assert bn_ref.y_bound(gamma, beta, 101) == 2.0 * 10.0 + 0.25
    assert bn_ref.y_bound(gamma, beta, 101, 1.5) == 2.0 * 10.0 + 0.25 + 1.5
    # a channel that attains Samuelson's bound: zeros and one outlier, gamma and beta of the same sign
    n = 600
    z = torch.zeros(1, 1, 1, n, dtype=torch.float64)
    z[0, 0, 0, 17] = 1000.0
    st = bn_ref.batch_stats(z)
    g1, b1 = torch.tensor([2.5]), torch.tensor([9.0])
    y = bn_ref.forward(z, st["mean"], st["rstd"], g1, b1)
    top = float(y.abs().max())
    assert 0.99999 * bn_ref.y_bound(g1, b1, n) < top <= bn_ref.y_bound(g1, b1, n)
    # dz: the bound dominates the tensor it is stated for, in train and eval mode
    g = torch.Generator().manual_seed(3)
    z = torch.randn(2, 3, 4, 5, generator=g, dtype=torch.float64) * 1e-2 + 10
    dy = torch.randn(2, 3, 4, 5, generator=g, dtype=torch.float64)
    st = bn_ref.batch_stats(z)
    mask = torch.rand(2, 3, 4, 5, generator=g) > 0.4
    for train in (True, False):
        dgamma, dbeta, dz, dres = bn_ref.backward(dy, z, st["mean"], st["rstd"], gamma, mask, train)
        b = bn_ref.dz_bound(gamma, st["rstd"], dres, dgamma, dbeta, train)
        assert float(dz.abs().max()) <= b
        if not train:
            assert math.isclose(b, float(dz.abs().max()), rel_tol=1e-12)
