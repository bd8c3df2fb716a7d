"""GPU: the U-Net generator and classifiers (``--net unet``) and the kernels of csrc/unet.hip.

* ``mcdseg_maxpool2_fwd`` / ``_bwd`` bit for bit against torch's CPU ``F.max_pool2d(return_indices=True)`` and its autograd -- ties, +-0,
  NaN and +-inf included --, the companion and the bound bit for bit what ``mcdseg_split_cb(y, bound)`` writes, for every arithmetic.
* ``mcdseg_relu_fwd`` / ``_bwd`` bit for bit (in place too), the companion likewise.
* ``mcdseg_deconv2x2_*`` against the fp64 CPU result within the derived bound (K + 2) * 2^-24 * S per element -- K the number of products
  summed, S the fp64 sum of |bias| and of the products' magnitudes: it holds for any summation order, with or without FMA --, through a
  channel slice of a poisoned buffer, two runs bitwise equal, one-hot inputs exact.
* MCDSEG_FUSED_UNET=0 against the kernels inside ``UNetBase`` + ``UNetClassifier``: pool and ReLU bit for bit through the whole network,
  every join within the bound above of its composed form, and of the fp64 truth.
* ``models.unet`` against what the REAL reference produced (tests/golden/unet_small.npz): features, logits, running statistics and every
  stored gradient held to the fp64 truth in units of the reference's own fp32 distance from it, by the rule and constants of
  tests/test_fusenet_gpu.py (a factor 2 on that unit, a floor of 2e-5 of the tensor's largest magnitude).  The fixture's inputs were
  chosen so that the fp32 reference takes the same side of every ReLU and 2x2 maximum as fp64 (make_unet_golden.py): the case is benign
  by construction, and a kernel that took the other side of a near-tie would not be met here.  What pins the decisions themselves are
  the bit-for-bit pool and ReLU tests above, ties included.
* the memory contract of the three ops (tests/guards.py); one ``MCDSolver.step`` against one ``adapt_trainer.dropin_step``; the trainer, a
  resumed epoch and the tester end to end.
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import unet_ref as R

pytestmark = pytest.mark.gpu

FACTOR, FLOOR = 2.0, 2e-5
U = 2.0 ** -24
MATHS = ("f16x3", "f16x1", "bf16x6")
MATH_ID = {"f16x3": 3, "f16x1": 1, "bf16x6": 6}
PIECES = {"f16x3": 2, "f16x1": 2, "bf16x6": 3}
COMMON = ["--net", "unet", "--input_ch", "6", "-b", "2", "--train_img_shape", "96", "64", "--synthetic", "--synthetic_len", "4", "--no_tflog",
          "--epochs", "1", "--max_iter", "10"]
# (H, W): one window, one row / one column of windows, a width off the 16-byte path (W % 4 != 0), widths on it, several blocks
POOL_PLANES = ((2, 2), (2, 6), (6, 2), (4, 10), (4, 8), (16, 48))


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("MCDSEG_PRETRAINED", "0")
    monkeypatch.setenv("MCDSEG_FUSED_UNET", "1")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _raw_split(ops, y, bound, math):
    """what mcdseg_split_cb writes for ``y`` under ``bound`` (a device scalar, or None for bf16x6)"""
    n, c, h, w = y.shape
    cb = torch.full((PIECES[math] * y.numel(),), 0x7e00, dtype=torch.int16, device=y.device)
    ops.check(ops.lib().mcdseg_split_cb(ops._p(y), ops._p(cb), ops._p(bound), MATH_ID[math], n, c, h * w, None), "split_cb")
    return cb


# ------------------------------------------------------------------------------------------------ the pool
def _pool_input(kind, shape, gen):
    x = torch.randn(shape, generator=gen)
    if kind == "post_relu":      # half zeros: ties at 0 all the time
        x = torch.relu(x)
    elif kind == "constant":     # every window a four-way tie
        x = torch.full(shape, 0.75)
    elif kind == "signed_zeros":  # +0 and -0 mixed (neither is greater), a few other values
        x = torch.where(torch.rand(shape, generator=gen) < 0.5, 0.0, -0.0) * torch.where(x.abs() < 1.5, 1.0, x)
        x = torch.where(torch.rand(shape, generator=gen) < 0.1, torch.randn(shape, generator=gen), x)
    elif kind == "nan":          # NaN: alone in a window, two in a window, behind and in front of larger values
        x = torch.where(torch.rand(shape, generator=gen) < 0.2, float("nan"), x)
    elif kind == "inf":          # +-inf, and whole windows of -inf
        r = torch.rand(shape, generator=gen)
        x = torch.where(r < 0.15, float("inf"), torch.where(r < 0.6, -float("inf"), x))
    return x


def _raw_pool(ops, x, bound=None, math=None):
    n, c, h, w = x.shape
    y = torch.full((n, c, h // 2, w // 2), float("nan"), device=x.device)
    cb = torch.full((PIECES[math] * y.numel(),), 0x7e00, dtype=torch.int16, device=x.device) if math else None
    yb = torch.full((1,), float("nan"), device=x.device) if bound is not None else None
    ops.check(ops.lib().mcdseg_maxpool2_fwd(ops._p(x), ops._p(bound), ops._p(y), ops._p(cb), ops._p(yb), MATH_ID.get(math, 0), n, c, h, w,
                                            None), "maxpool2_fwd")
    return y, cb, yb


def _raw_pool_bwd(ops, x, dy):
    n, c, h, w = x.shape
    dx = torch.full_like(x, float("nan"))
    ops.check(ops.lib().mcdseg_maxpool2_bwd(ops._p(x), ops._p(dy), ops._p(dx), n, c, h, w, None), "maxpool2_bwd")
    return dx


@pytest.mark.parametrize("kind", ["random", "post_relu", "constant", "signed_zeros", "nan", "inf"])
def test_pool_is_torch_cpu_bit_for_bit(kind):
    dev = _dev()
    from mcdseg import ops
    gen = torch.Generator().manual_seed(11)
    seen = 0
    for n in (1, 3):
        for c in (1, 8, 24):
            for h, w in POOL_PLANES:
                x = _pool_input(kind, (n, c, h, w), gen)
                dy = torch.randn(n, c, h // 2, w // 2, generator=gen)
                xr = x.clone().requires_grad_(True)
                want_y, idx = F.max_pool2d(xr, 2, return_indices=True)
                want_y.backward(dy)
                xd, dyd = x.to(dev), dy.to(dev)
                torch.cuda.synchronize()  # (the kernels run on the null stream)
                y, _, _ = _raw_pool(ops, xd)
                dx = _raw_pool_bwd(ops, xd, dyd)
                torch.cuda.synchronize()
                what = (kind, n, c, h, w)
                assert _same_bits(y.cpu(), want_y.detach()), what
                assert _same_bits(dx.cpu(), xr.grad), what
                # the arg-max itself: dx is dy at idx and zero elsewhere
                flat = torch.zeros(n, c, h * w).scatter_(2, idx.view(n, c, -1), dy.view(n, c, -1)).view(n, c, h, w)
                assert _same_bits(dx.cpu(), flat), what
                seen += 1
    assert seen == 36


def test_pool_off_the_16_byte_grid():
    """W % 4 == 0 but the tensors 4 bytes off the 16-byte grid: the scalar form, the same bits"""
    dev = _dev()
    from mcdseg import ops
    gen = torch.Generator().manual_seed(12)
    x = torch.relu(torch.randn(2, 8, 8, 16, generator=gen)).to(dev)
    dy = torch.randn(2, 8, 4, 8, generator=gen).to(dev)
    ox = torch.empty(x.numel() + 1, device=dev)[1:].view(x.shape)
    ody = torch.empty(dy.numel() + 1, device=dev)[1:].view(dy.shape)
    ox.copy_(x), ody.copy_(dy)
    assert ox.data_ptr() % 16 == 4
    bound = x.abs().max().reshape(1)
    torch.cuda.synchronize()
    y, cb, yb = _raw_pool(ops, x, bound, "f16x3")
    y2, cb2, yb2 = _raw_pool(ops, ox, bound, "f16x3")
    dx, dx2 = _raw_pool_bwd(ops, x, dy), _raw_pool_bwd(ops, ox, ody)
    torch.cuda.synchronize()
    assert _same_bits(y, y2) and _same_bits(cb, cb2) and _same_bits(yb, yb2) and _same_bits(dx, dx2)
    assert _same_bits(y.cpu(), F.max_pool2d(x.cpu(), 2))


@pytest.mark.parametrize("math", MATHS)
def test_pool_companion_is_the_split_of_y(math):
    dev = _dev()
    from mcdseg import ops
    scaled = math != "bf16x6"
    gen = torch.Generator().manual_seed(13)
    seen = 0
    for kind in ("random", "post_relu", "signed_zeros", "nan"):
        for n in (1, 3):
            for c in (8, 24):
                for h, w in POOL_PLANES:
                    x = _pool_input(kind, (n, c, h, w), gen)
                    finite = torch.where(torch.isfinite(x), x, torch.zeros(())).abs().max()
                    bound = (finite * 1.7 + 0.1).reshape(1).to(dev) if scaled else None  # an upper bound, as a producer supplies it
                    xd = x.to(dev)
                    torch.cuda.synchronize()
                    y0, _, _ = _raw_pool(ops, xd)
                    y, cb, yb = _raw_pool(ops, xd, bound, math)
                    y2, cb2, _ = _raw_pool(ops, xd, bound, math)
                    want_cb = _raw_split(ops, y, yb, math)
                    torch.cuda.synchronize()
                    what = (math, kind, n, c, h, w)
                    assert _same_bits(y, y0) and _same_bits(y, y2) and _same_bits(cb, cb2), what
                    assert _same_bits(cb, want_cb), what
                    if scaled:
                        assert _same_bits(yb, bound), what  # the bound of x, handed on: nothing is measured
                    seen += 1
    assert seen == 96


# ------------------------------------------------------------------------------------------------ the ReLU
def _relu_input(shape, gen):
    x = torch.randn(shape, generator=gen)
    f = x.view(-1)
    special = [0.0, -0.0, float("nan"), float("inf"), -float("inf"), 1e-41, -1e-41]
    for k, v in enumerate(special[:f.numel()]):
        f[(k * 5) % f.numel()] = v
    return x


def _raw_relu(ops, x, bound=None, math=None, inplace=False):
    n, c, h, w = x.shape
    y = x if inplace else torch.full_like(x, float("nan"))
    cb = torch.full((PIECES[math] * x.numel(),), 0x7e00, dtype=torch.int16, device=x.device) if math else None
    yb = torch.full((1,), float("nan"), device=x.device) if bound is not None else None
    ops.check(ops.lib().mcdseg_relu_fwd(ops._p(x), ops._p(bound), ops._p(y), ops._p(cb), ops._p(yb), MATH_ID.get(math, 0), n, c, h * w, None),
              "relu_fwd")
    return y, cb, yb


@pytest.mark.parametrize("count", [1, 63, 256, 257, 1028])
def test_relu_forward_backward_and_companion(count):
    dev = _dev()
    from mcdseg import ops
    gen = torch.Generator().manual_seed(14)
    for n, c in ((1, 1), (2, 3), (1, 8), (3, 16)):
        x = _relu_input((n, c, 1, count), gen)
        dy = torch.randn(x.shape, generator=gen)
        want = torch.relu(x)  # torch's CPU clamp: a negative value becomes +0; -0 and NaN pass
        finite = torch.where(torch.isfinite(x), x, torch.zeros(()))
        xr = finite.clone().requires_grad_(True)
        torch.relu(xr).backward(dy)
        xd, dyd = x.to(dev), dy.to(dev)
        torch.cuda.synchronize()
        y, _, _ = _raw_relu(ops, xd)
        dx = torch.full_like(xd, float("nan"))
        ops.check(ops.lib().mcdseg_relu_bwd(ops._p(y), ops._p(dyd), ops._p(dx), y.numel(), None), "relu_bwd")
        yi, _, _ = _raw_relu(ops, xd.clone(), inplace=True)
        # off the 16-byte grid: the scalar form
        ox = torch.empty(x.numel() + 1, device=dev)[1:].view(x.shape)
        ox.copy_(xd)
        yo, _, _ = _raw_relu(ops, ox)
        torch.cuda.synchronize()
        what = (count, n, c)
        assert _same_bits(y.cpu(), want) and _same_bits(yi, y) and _same_bits(yo, y), what
        assert _same_bits(dx.cpu(), torch.where(want > 0, dy, torch.zeros(()))), what  # dx = y > 0 ? dy : 0
        fin = torch.isfinite(x)
        assert torch.equal(dx.cpu()[fin], xr.grad[fin]), what  # ... which is torch's autograd wherever x is finite
        if c % 8:
            continue
        for math in MATHS:
            scaled = math != "bf16x6"
            bound = (finite.abs().max() * 1.3 + 0.1).reshape(1).to(dev) if scaled else None
            yc, cb, yb = _raw_relu(ops, xd, bound, math)
            xc = xd.clone()
            _, cbi, _ = _raw_relu(ops, xc, bound, math, inplace=True)
            want_cb = _raw_split(ops, yc, yb, math)
            torch.cuda.synchronize()
            assert _same_bits(yc, y) and _same_bits(xc, y), (what, math)
            assert _same_bits(cb, want_cb) and _same_bits(cbi, want_cb), (what, math)
            if scaled:
                assert _same_bits(yb, bound), (what, math)


# ------------------------------------------------------------------------------------------------ the up-convolution
UP_CASES = [(n, cin, cout, h, w) for (cin, cout) in ((5, 3), (16, 8), (32, 16)) for (h, w) in ((1, 1), (2, 3), (7, 5)) for n in (1, 3)] + \
           [(1, 256, 128, 2, 3)]


ABOVE = 2  # channels of the buffer above the slice: [0, Cs) below it, [Cs, Cs + Cout) the slice, then these


def _up_fwd(ops, x, w, b, cs, poison=float("nan"), above=0):
    n, cin, h, wd = x.shape
    cout = w.shape[1]
    ct = cs + cout + above
    buf = torch.full((n, ct, 2 * h, 2 * wd), poison, device=x.device)
    ops.check(ops.lib().mcdseg_deconv2x2_fwd(ops._p(x), ops._p(w), ops._p(b), ops._p(buf), ct * 4 * h * wd, ct, cs, n, cin, cout, h, wd, None),
              "deconv2x2_fwd")
    return buf


def _up_bwd(ops, x, w, dbuf, cs):
    n, cin, h, wd = x.shape
    cout = w.shape[1]
    ct = dbuf.shape[1]
    L = ops.lib()
    dx = torch.full_like(x, float("nan"))
    ops.check(L.mcdseg_deconv2x2_bwd_data(ops._p(dbuf), ct * 4 * h * wd, ct, cs, ops._p(w), ops._p(dx), n, cin, cout, h, wd, None),
              "deconv2x2_bwd_data")
    dw, db = torch.full_like(w, float("nan")), torch.full((cout,), float("nan"), device=x.device)
    nbytes = L.mcdseg_deconv2x2_bwd_weight_workspace_bytes(n, cin, cout, h, wd)
    ws = torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device=x.device)
    ops.check(L.mcdseg_deconv2x2_bwd_weight(ops._p(x), ops._p(dbuf), ct * 4 * h * wd, ct, cs, ops._p(dw), ops._p(db), n, cin, cout, h, wd,
                                            ops._p(ws), nbytes, None), "deconv2x2_bwd_weight")
    return dx, dw, db


def _up_truth(x, w, b, dy):
    """fp64 results and the sums of magnitudes S of each, with the number of products K"""
    x, w, b, dy = x.double(), w.double(), b.double(), dy.double()
    n, cin, h, wd = x.shape
    cout = w.shape[1]
    t = {"y": (F.conv_transpose2d(x, w, b, stride=2), F.conv_transpose2d(x.abs(), w.abs(), b.abs(), stride=2), cin),
         "dx": (F.conv2d(dy, w, stride=2), F.conv2d(dy.abs(), w.abs(), stride=2), 4 * cout)}
    d6 = dy.view(n, cout, h, 2, wd, 2)
    t["dw"] = (torch.einsum("ncij,noiajb->coab", x, d6), torch.einsum("ncij,noiajb->coab", x.abs(), d6.abs()), n * h * wd)
    t["db"] = (dy.sum(dim=(0, 2, 3)), dy.abs().sum(dim=(0, 2, 3)), n * 4 * h * wd)
    return t


def _within(got, truth, s, k, what, factor=1.0):
    err = (got.double().cpu() - truth).abs()
    bound = factor * (k + 2) * U * s
    worst = float((err / bound.clamp_min(1e-300)).max())
    print("%-44s K %6d  worst error / bound %.3f" % (what, k, worst))
    assert bool((err <= bound).all()), (what, worst)


@pytest.mark.parametrize("case", UP_CASES, ids=lambda c: "x".join(map(str, c)))
def test_up_convolution_against_fp64(case):
    dev = _dev()
    from mcdseg import ops
    n, cin, cout, h, wd = case
    gen = torch.Generator().manual_seed(15)
    x = torch.randn(n, cin, h, wd, generator=gen) * 1.5 + 0.3
    w = torch.randn(cin, cout, 2, 2, generator=gen) * 0.4
    b = torch.randn(cout, generator=gen)
    dy = torch.randn(n, cout, 2 * h, 2 * wd, generator=gen)
    truth = _up_truth(x, w, b, dy)
    xd, wdv, bd = x.to(dev), w.to(dev), b.to(dev)
    for cs in (0, cout):
        poison = torch.tensor(float("nan")).view(torch.int32).item()
        torch.cuda.synchronize()
        buf = _up_fwd(ops, xd, wdv, bd, cs, above=ABOVE)
        buf2 = _up_fwd(ops, xd, wdv, bd, cs, above=ABOVE)
        dbuf = torch.full((n, cs + cout + ABOVE, 2 * h, 2 * wd), float("nan"), device=dev)  # NaN below and above the slice: never read
        dbuf[:, cs:cs + cout] = dy.to(dev)
        torch.cuda.synchronize()
        dx, dw, db = _up_bwd(ops, xd, wdv, dbuf, cs)
        dx2, dw2, db2 = _up_bwd(ops, xd, wdv, dbuf, cs)
        torch.cuda.synchronize()
        what = "%s Cs=%d " % ("x".join(map(str, case)), cs)
        assert _same_bits(buf, buf2) and _same_bits(dx, dx2) and _same_bits(dw, dw2) and _same_bits(db, db2), what  # two runs, one result
        for outside in (buf[:, :cs], buf[:, cs + cout:]):  # below and above the slice: the poison, untouched
            assert bool((outside.contiguous().view(torch.int32) == poison).all()), what
        got = {"y": buf[:, cs:cs + cout], "dx": dx, "dw": dw, "db": db}
        for k, (t, s, terms) in truth.items():
            _within(got[k], t, s, terms, what + k)
    # without a bias: the same sums from 0
    buf = _up_fwd(ops, xd, wdv, None, 0)
    torch.cuda.synchronize()
    _within(buf, F.conv_transpose2d(x.double(), w.double(), None, stride=2),
            F.conv_transpose2d(x.double().abs(), w.double().abs(), None, stride=2), cin, "no bias")


def test_up_convolution_one_hot_is_exact():
    """one non-zero term has no rounding: pins which tap (a, b) meets which output pixel"""
    dev = _dev()
    from mcdseg import ops
    gen = torch.Generator().manual_seed(16)
    n, cin, cout, h, wd = 2, 5, 3, 3, 4
    w = torch.randn(cin, cout, 2, 2, generator=gen)
    zero_b = torch.zeros(cout)
    for (k, ci, i, j) in ((0, 0, 0, 0), (1, 4, 2, 3), (1, 2, 1, 2)):
        x = torch.zeros(n, cin, h, wd)
        x[k, ci, i, j] = 2.0
        want = torch.zeros(n, cout, 2 * h, 2 * wd)
        want[k, :, 2 * i:2 * i + 2, 2 * j:2 * j + 2] = 2.0 * w[ci]
        buf = _up_fwd(ops, x.to(dev), w.to(dev), zero_b.to(dev), 0)
        torch.cuda.synchronize()
        assert torch.equal(buf.cpu(), want), (k, ci, i, j)
    x = torch.randn(n, cin, h, wd, generator=gen)
    for (k, co, r, s) in ((0, 0, 0, 0), (1, 2, 5, 7), (0, 1, 2, 5), (1, 1, 3, 2)):
        dy = torch.zeros(n, cout, 2 * h, 2 * wd)
        dy[k, co, r, s] = 0.5
        i, a, j, b = r // 2, r % 2, s // 2, s % 2
        want_dx = torch.zeros(n, cin, h, wd)
        want_dx[k, :, i, j] = 0.5 * w[:, co, a, b]
        want_dw = torch.zeros(cin, cout, 2, 2)
        want_dw[:, co, a, b] = 0.5 * x[k, :, i, j]
        want_db = torch.zeros(cout)
        want_db[co] = 0.5
        dx, dw, db = _up_bwd(ops, x.to(dev), w.to(dev), dy.to(dev), 0)
        torch.cuda.synchronize()
        assert torch.equal(dx.cpu(), want_dx) and torch.equal(dw.cpu(), want_dw) and torch.equal(db.cpu(), want_db), (k, co, r, s)


# ------------------------------------------------------------------------------------------------ the ops
@pytest.mark.parametrize("math", ["f16x3", "bf16x6", "f32"])
def test_ops_attach_companions_by_the_stage_join_rules(math, monkeypatch):
    dev = _dev()
    from mcdseg import ops
    monkeypatch.setattr(ops, "CONV_MATH", math)
    gen = torch.Generator().manual_seed(17)
    for c, expect_cb in ((24, math != "f32"), (8, False), (20, False)):
        out = {}
        for fused in ("1", "0"):
            monkeypatch.setenv("MCDSEG_FUSED_UNET", fused)
            g = torch.Generator().manual_seed(18)
            x0 = torch.randn(2, c, 6, 8, generator=g).to(dev)
            supplied = (x0.abs().max() * 2.5).reshape(1)
            res = []
            for fn in (ops.max_pool2, ops.relu):
                x = x0.clone().requires_grad_(True)
                u = x * 1.0
                u._mcd_cb = (None, supplied, u._version, u.data_ptr())  # a producer's bound
                y = fn(u)
                cb, bound = ops._cb_of(y)
                assert (cb is not None) == expect_cb, (math, c, fn.__name__)
                assert (bound is not None) == (math == "f16x3" and c >= 16), (math, c, fn.__name__)
                if bound is not None:
                    assert _same_bits(bound, supplied)
                dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(19)).to(dev)
                y.backward(dy)
                res += [y.detach(), cb, bound, x.grad]
            out[fused] = res
        for a, b in zip(out["1"], out["0"]):  # the composed form: the same bits
            assert (a is None) == (b is None)
            assert a is None or _same_bits(a, b), (math, c)
    # the join: shortcut copied, up-convolution in the upper slice, a measured bound and the companion of the whole buffer
    monkeypatch.setenv("MCDSEG_FUSED_UNET", "1")
    s = torch.randn(2, 8, 6, 10, generator=gen).to(dev).requires_grad_(True)
    h = torch.randn(2, 16, 3, 5, generator=gen).to(dev).requires_grad_(True)
    w = (torch.randn(16, 8, 2, 2, generator=gen) * 0.3).to(dev).requires_grad_(True)
    b = torch.randn(8, generator=gen).to(dev).requires_grad_(True)
    y = ops.up_join(s * 1.0, h * 1.0, w, b)
    cb, bound = ops._cb_of(y)
    assert y.shape == (2, 16, 6, 10) and _same_bits(y[:, :8].contiguous(), s)
    assert (cb is not None) == (math != "f32") and (bound is not None) == (math == "f16x3")
    if bound is not None:
        assert _same_bits(bound, y.detach().abs().max().reshape(1))
    if cb is not None:
        assert _same_bits(cb, _raw_split(ops, y.detach(), bound, math))
    dy = torch.randn(y.shape, generator=gen).to(dev)
    y.backward(dy)
    assert _same_bits(s.grad, dy[:, :8].contiguous())
    t = _up_truth(h.detach().cpu(), w.detach().cpu(), b.detach().cpu(), dy[:, 8:].cpu())
    for k, got in (("dx", h.grad), ("dw", w.grad), ("db", b.grad)):
        _within(got, t[k][0], t[k][1], t[k][2], "ops.up_join " + k)
    with torch.no_grad():  # bare inputs without grad mode: y only
        y = ops.up_join(s.detach(), h.detach(), w.detach(), b.detach())
        assert ops._cb_of(y) == (None, None)
        assert ops._cb_of(ops.max_pool2(s.detach())) == (None, None) and ops._cb_of(ops.relu(s.detach())) == (None, None)


# ------------------------------------------------------------------------------------------------ composed against fused, in the network
def _models(dev, feature_scale, n_class, seed=R.SPEC["fill_seed"]):
    from models.unet import UNetBase, UNetClassifier
    ms = [UNetBase(feature_scale=feature_scale, input_ch=6), UNetClassifier(feature_scale=feature_scale, n_classes=n_class),
          UNetClassifier(feature_scale=feature_scale, n_classes=n_class)]
    return [m.to(dev) for m in R.fill_models(ms, seed)]


def _network_pass(ms, x, labels):
    g, f1, f2 = ms
    for m in ms:
        m.train()
        m.zero_grad()
    xx = x.clone().requires_grad_(True)
    feats = g(xx)
    o1, o2 = f1(feats), f2(feats)
    vals = R.losses(o1, o2, labels)
    (vals["ce"] + 10.0 * vals["diff"]).backward()
    torch.cuda.synchronize()
    out = {"o1": o1.detach().clone(), "o2": o2.detach().clone(), "dx": xx.grad.clone()}
    out.update(("feat/" + k, v.detach().clone()) for k, v in feats.items())
    for tag, m in zip(("g", "f1", "f2"), ms):
        out.update(("grad/%s.%s" % (tag, k), p.grad.detach().clone()) for k, p in m.named_parameters())
        out.update(("state/%s.%s" % (tag, k), v.detach().clone()) for k, v in m.state_dict().items() if "running_" in k)
    return out


def _composed(fn, monkeypatch):
    def call(*args, **kw):
        monkeypatch.setenv("MCDSEG_FUSED_UNET", "0")
        try:
            return fn(*args, **kw)
        finally:
            monkeypatch.setenv("MCDSEG_FUSED_UNET", "1")
    return call


def test_composed_pool_and_relu_are_bitwise_and_joins_within_the_bound(monkeypatch):
    """feature_scale=4 (16 .. 256 channels: every tensor carries a companion).  First MCDSEG_FUSED_UNET=0 for the pool and the ReLU
    alone: the whole network, every gradient included, bit for bit.  Then every join of the network, both ways on the same inputs: the
    fused one within (K + 2) 2^-24 S of the composed one, and of the fp64 result."""
    dev = _dev()
    from mcdseg import ops
    ms = _models(dev, 4, 5)
    state = [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in ms]
    g = torch.Generator().manual_seed(21)
    x = torch.randn(2, 6, 32, 48, generator=g).to(dev)
    labels = torch.randint(0, 5, (2, 32, 48), generator=g).to(dev)
    fused = _network_pass(ms, x, labels)
    assert all(torch.isfinite(v).all() for v in fused.values())
    for m, s in zip(ms, state):
        m.load_state_dict(s)
    pool, relu, join = ops.max_pool2, ops.relu, ops.up_join
    calls = {"pool": 0, "relu": 0}

    def counted(name, fn):
        def call(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return call
    monkeypatch.setattr(ops, "max_pool2", counted("pool", _composed(pool, monkeypatch)))
    monkeypatch.setattr(ops, "relu", counted("relu", _composed(relu, monkeypatch)))
    composed = _network_pass(ms, x, labels)
    assert calls == {"pool": 4, "relu": 16}
    assert fused.keys() == composed.keys()
    differ = [k for k in fused if not _same_bits(fused[k], composed[k])]
    assert not differ, differ[:8]
    monkeypatch.setattr(ops, "max_pool2", pool)
    monkeypatch.setattr(ops, "relu", relu)

    seen = []

    def both(shortcut, h, w, b, companion=True):
        """the fused join (returned) and the composed one, on detached copies, forward and backward, against fp64 on the device"""
        res = {}
        dy = torch.randn((h.shape[0], shortcut.shape[1] + w.shape[1], 2 * h.shape[2], 2 * h.shape[3]),
                         generator=torch.Generator().manual_seed(22)).to(dev)
        for name, fn in (("fused", join), ("composed", _composed(join, monkeypatch))):
            leaves = [t.detach().clone().requires_grad_(True) for t in (shortcut, h, w, b)]
            y = fn(*leaves)
            y.backward(dy)
            res[name] = [y.detach()] + [t.grad for t in leaves]
        cs, cin, cout = shortcut.shape[1], w.shape[0], w.shape[1]
        n, hh, wh = h.shape[0], h.shape[2], h.shape[3]
        hd, wd_, bd, dyd = (t.detach().double().cpu() for t in (h, w, b, dy[:, cs:]))  # (the sums of magnitudes: fp64 on the host)
        d6 = dyd.reshape(n, cout, hh, 2, wh, 2)
        truth = {"y": F.conv_transpose2d(hd, wd_, bd, stride=2), "dh": F.conv2d(dyd, wd_, stride=2),
                 "dw": torch.einsum("ncij,noiajb->coab", hd, d6), "db": dyd.sum(dim=(0, 2, 3))}
        sums = [(F.conv_transpose2d(hd.abs(), wd_.abs(), bd.abs(), stride=2), cin), None,
                (F.conv2d(dyd.abs(), wd_.abs(), stride=2), 4 * cout), (torch.einsum("ncij,noiajb->coab", hd.abs(), d6.abs()), n * hh * wh),
                (dyd.abs().sum(dim=(0, 2, 3)), n * 4 * hh * wh)]
        (yf, dsf, dhf, dwf, dbf), (yc, dsc, dhc, dwc, dbc) = res["fused"], res["composed"]
        assert _same_bits(yf[:, :cs].contiguous(), yc[:, :cs].contiguous()) and _same_bits(dsf.contiguous(), dsc.contiguous())  # copies
        for what, a, c, sk in (("y", yf[:, cs:], yc[:, cs:], sums[0]), ("dh", dhf, dhc, sums[2]), ("dw", dwf, dwc, sums[3]), ("db", dbf, dbc, sums[4])):
            s, k = sk
            bound = (k + 2) * U * s
            for other, ref in (("composed", c.double().cpu()), ("fp64", truth[what])):
                err = (a.double().cpu() - ref).abs()
                worst = float((err / bound.clamp_min(1e-300)).max())
                print("join %3d -> %3d at %2d x %2d  %-2s fused against %-8s: worst difference / bound %.3f" % (cin, cout, hh, wh, what, other, worst))
                assert bool((err <= bound).all()), (cin, cout, what, other, worst)
        seen.append((cin, cout))
        return join(shortcut, h, w, b, companion=companion)
    monkeypatch.setattr(ops, "up_join", both)
    for m, s in zip(ms, state):
        m.load_state_dict(s)
    again = _network_pass(ms, x, labels)
    assert seen == [(256, 128), (128, 64), (64, 32), (32, 16)] * 2
    assert not [k for k in fused if not _same_bits(fused[k], again[k])]  # (and the network is reproducible run to run)


# ------------------------------------------------------------------------------------------------ the model against the reference
def test_model_against_the_reference():
    dev = _dev()
    fx, units = R.load_golden()
    spec = json.loads(str(fx["spec"]))
    ms = _models(dev, spec["feature_scale"], spec["n_class"], spec["fill_seed"])
    x, labels = R.inputs(spec)
    got = R.run(*ms, x, labels)
    torch.cuda.synchronize()
    assert sorted(got) == sorted(units)
    counters = [k for k in got if k.endswith("num_batches_tracked")]
    assert len(counters) == 10 and all(int(got[k]) == int(fx["f64/" + k]) == 1 for k in counters)
    worst = []
    for k in sorted(got):
        if k in counters:
            continue
        truth, unit = fx["f64/" + k], float(units[k])
        scale = float(fx["scale/" + k]) if ("scale/" + k) in fx.files else None
        assert got[k].shape == truth.shape, k
        err = R.rel_to_max(got[k], truth, scale)
        print("%-44s kernel %.3e  the reference's fp32 (the unit) %.3e  ratio %.2f  of the bound max(2 units, %.0e) %.2f"
              % (k, err, unit, err / unit if unit > 0 else float(err > 0), FLOOR, err / max(FACTOR * unit, FLOOR)))
        if err > max(FACTOR * unit, FLOOR):
            worst.append((k, err, unit))
    assert not worst, worst


# ------------------------------------------------------------------------------------------------ the memory contract
def test_memory_contract_of_the_three_ops(device, monkeypatch):
    """stock / 0xFF / 0x00 (tests/guards_hold.hold): guards intact, results bitwise equal"""
    from mcdseg import ops
    from guards_hold import hold
    monkeypatch.setattr(ops, "CONV_MATH", "f16x3")

    def tagged(y, out, name):
        cb, bound = ops._cb_of(y)
        out[name] = y
        if cb is not None:
            out[name + "_unsplit"] = ops.materialize(y, cb, bound)
        if bound is not None:
            out[name + "_bound"] = bound

    for shape in ((2, 24, 6, 10), (2, 16, 4, 8), (1, 5, 2, 6)):
        def pool_relu(put):
            g = torch.Generator().manual_seed(31)
            x = put(torch.randn(*shape, generator=g), requires_grad=True)
            x2 = put(torch.randn(*shape, generator=g), requires_grad=True)
            out = {}
            y = ops.max_pool2(x)
            tagged(y, out, "pool")
            y.backward(put(torch.randn(y.shape, generator=g)))
            r = ops.relu(x2)
            tagged(r, out, "relu")
            r.backward(put(torch.randn(r.shape, generator=g)))
            out.update(pool_dx=x.grad, relu_dx=x2.grad)
            return out
        hold(device, pool_relu, family="unet pool / relu %s" % (shape,))

    for n, cs, cin, cout, h, w in ((2, 8, 16, 8, 3, 5), (1, 3, 5, 3, 2, 3)):
        def join(put):
            g = torch.Generator().manual_seed(32)
            s = put(torch.randn(n, cs, 2 * h, 2 * w, generator=g), requires_grad=True)
            x = put(torch.randn(n, cin, h, w, generator=g), requires_grad=True)
            wt = put(torch.randn(cin, cout, 2, 2, generator=g), requires_grad=True)
            b = put(torch.randn(cout, generator=g), requires_grad=True)
            out = {}
            y = ops.up_join(s, x, wt, b)
            tagged(y, out, "join")
            y.backward(put(torch.randn(y.shape, generator=g)))
            out.update(ds=s.grad, dh=x.grad, dw=wt.grad, db=b.grad)
            return out
        hold(device, join, workspace=True, family="unet up_join %d+%d" % (cs, cout))


# ------------------------------------------------------------------------------------------------ one MCD step
def _checksums(mod):
    return {k: (float(v.double().sum()), float(v.double().norm())) for k, v in mod.state_dict().items()}


def _same_state(mod, ref, rtol):
    """the comparison of tests/test_fusenet_gpu.py: every state tensor's sum and norm"""
    got, want = _checksums(mod), _checksums(ref)
    assert got.keys() == want.keys()
    numel = {k: v.numel() for k, v in mod.state_dict().items()}
    bad = [(k, got[k][1], l2) for k, (s, l2) in want.items() if abs(got[k][1] - l2) > rtol * max(abs(l2), 1e-6)]
    assert not bad, bad[:5]
    bad = [(k, got[k][0], s) for k, (s, l2) in want.items() if abs(got[k][0] - s) > rtol * max(abs(l2), 1e-6) * max(numel[k], 1) ** 0.5]
    assert not bad, bad[:5]


def test_solver_step_against_the_drop_in_loop():
    dev = _dev()
    import adapt_trainer
    from loss import CrossEntropyLoss2d, get_prob_distance_criterion
    from models.model_util import get_optimizer
    from recipe import make_batch
    from solvers.solver import MCDSolver
    nc, num_k = 5, 2
    s, l, t = (v.to(dev) for v in make_batch(31, 2, 6, 32, 48, nc))
    cw = torch.ones(nc)
    cw[nc - 1] = 0
    ce = CrossEntropyLoss2d(cw.to(dev))

    def models():
        g, f1, f2 = _models(dev, 4, nc)
        for m in (g, f1, f2):
            m.train()
        og = get_optimizer(g.parameters(), "sgd", 1e-3, 0.9, 2e-5)
        of = get_optimizer(list(f1.parameters()) + list(f2.parameters()), "sgd", 1e-3, 0.9, 2e-5)
        return g, f1, f2, og, of
    g, f1, f2, og, of = models()
    rg, rf1, rf2, rog, rof = models()
    solver = MCDSolver(g, f1, f2, og, of, ce, get_prob_distance_criterion("diff"), num_k=num_k)
    assert not solver.reuse_tgt and not solver.fork_ok and not solver.fused_up  # the literal schedule on full-resolution logits
    c_loss, d_loss = solver.step(s, l, t)
    rc, rd = adapt_trainer.dropin_step(rg, rf1, rf2, rog, rof, ce, get_prob_distance_criterion("diff"), s, l, t, num_k, 1)
    torch.cuda.synchronize()
    c_loss, d_loss, rc, rd = float(c_loss), float(d_loss), float(rc), float(rd)
    print("c_loss %.7f vs %.7f, d_loss %.6e vs %.6e" % (c_loss, rc, d_loss, rd))
    for m in (g, rg):
        counters = {k: int(v) for k, v in m.state_dict().items() if k.endswith("num_batches_tracked")}
        assert len(counters) == 10 and all(v == 3 + num_k for v in counters.values()), counters
    assert np.isfinite(c_loss) and np.isfinite(d_loss) and d_loss > 0
    assert abs(c_loss - rc) <= 1e-4 * abs(rc)
    assert abs(d_loss - rd) <= 2e-3 * abs(rd)
    _same_state(g, rg, 3e-4), _same_state(f1, rf1, 3e-4), _same_state(f2, rf2, 3e-4)


# ------------------------------------------------------------------------------------------------ trainer, resume, tester
def test_trainer_resume_and_tester(tmp_path):
    _dev()
    import adapt_tester
    import adapt_trainer
    import util
    from PIL import Image
    out = str(tmp_path / "out")
    assert adapt_trainer.main(["suncg", "nyu", "--base_outdir", out] + COMMON) == 0
    d = os.path.join(out, "suncg-train2nyu-train_6ch")
    ck_fn = os.path.join(d, "pth", "MCD-normal-unet-1.pth.tar")
    ck = util.load_checkpoint(ck_fn)
    assert sorted(ck.keys()) == ["args", "epoch", "f1_state_dict", "f2_state_dict", "g_state_dict", "optimizer_f", "optimizer_g"]
    assert ck["args"].net == "unet" and ck["epoch"] == 1
    gsd, fsd = ck["g_state_dict"], ck["f1_state_dict"]
    keys = R.load_keys()
    assert [[k, list(v.shape)] for k, v in gsd.items()] == keys["base/4"]
    assert [k for k, _ in keys["classifier/4"]] == list(fsd.keys()) and tuple(fsd["up_concat4.up.weight"].shape) == (256, 128, 2, 2)
    assert int(gsd["conv1.conv1.1.num_batches_tracked"]) == 14  # 2 iterations x 7 generator forwards
    assert all(torch.isfinite(v).all() for sd in (gsd, fsd, ck["f2_state_dict"]) for v in sd.values() if v.dtype.is_floating_point)
    ck["args"].epochs = 2
    util.save_checkpoint(ck, False, ck_fn)
    assert adapt_trainer.main(["suncg", "nyu", "--resume", ck_fn] + COMMON) == 0
    ck2 = util.load_checkpoint(os.path.join(d, "pth", "MCD-normal-unet-2.pth.tar"))
    assert ck2["epoch"] == 2 and int(ck2["g_state_dict"]["conv1.conv1.1.num_batches_tracked"]) == 28
    assert not torch.equal(ck2["f1_state_dict"]["up_concat1.up.weight"], fsd["up_concat1.up.weight"])
    res = adapt_tester.main(["nyu", ck_fn, "--synthetic", "--synthetic_len", "2", "--outdir", str(tmp_path / "test"),
                             "--test_img_shape", "80", "64"])
    label_dir, ave_ent = res[:2]
    names = sorted(os.listdir(label_dir))
    assert len(names) == 2 and all(Image.open(os.path.join(label_dir, nm)).size == (80, 64) for nm in names)
    assert np.isfinite(ave_ent) and os.path.exists(os.path.join(os.path.dirname(label_dir), "eval_result.json"))
