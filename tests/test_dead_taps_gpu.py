"""Option SKIP_DEAD_TAPS of the ping-pong convolution kernels (csrc/conv_gemm_split_pp.hip, csrc/conv_wgrad_split_pp.hip): a pixel
tile's loader steps over the taps that lie in the zero padding for every pixel of the tile, the weight gradient's over the output rows
whose shifted input row lies outside the image.  The skipped K-steps added ``w * 0``, so every result must be BIT FOR BIT that of the
full loop (SKIP_DEAD_TAPS=0): forward output, BatchNorm partial rows, data gradient (with and without addend) and weight gradient.

Every case runs with ``PP_CUS=16, PP_MIN_ROUNDS=1`` like the other ping-pong tests, and with ``PINGPONG=4`` (the 320-pixel tile
wherever the kernel applies): the cases here have 3 to 5 pixel tiles, which no CU count plans on that tile by itself.  The weight
gradient is planned for as many "CUs" (``WGRAD_PP_CUS``) as give these small batches the slab plan, and once as stream-K."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TILE = 320  # pixels of the wide ping-pong tile


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _live_taps(n, h, w, k, dil, pad, ho, wo, tile, dgrad=False):
    """number of taps of pixel tile ``tile`` that some pixel of it uses (stride 1): what the kernel's live mask must come to"""
    hd, wd, hs, ws = (h, w, ho, wo) if dgrad else (ho, wo, h, w)
    live = set()
    for pix in range(tile * TILE, min((tile + 1) * TILE, n * hd * wd)):
        py, px = (pix % (hd * wd)) // wd, pix % wd
        for ky in range(k):
            for kx in range(k):
                sy = py + pad - ky * dil if dgrad else py + ky * dil - pad
                sx = px + pad - kx * dil if dgrad else px + kx * dil - pad
                if 0 <= sy < hs and 0 <= sx < ws:
                    live.add((ky, kx))
    return len(live)


class _Names:
    def __init__(self):
        self.names = []

    def wants(self, name):
        self.names.append(name)
        return False


def _inputs(cin, cout, k, dil, n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (k * k * cout)) ** 0.5
    return x, wt, dil * (k // 2)


def _run_both(libopt, fn):
    """fn() with the dead steps skipped (the default) and with every step run"""
    out = {}
    for skip in (1, 0):
        libopt(SKIP_DEAD_TAPS=skip)
        out[skip] = fn()
    libopt(SKIP_DEAD_TAPS=1)
    return out[1], out[0]


def _same(a, b, what):
    assert a.shape == b.shape and torch.equal(a, b), "%s differs from the full loop's (max %.3e)" % (what, float((a.double() - b.double()).abs().max()))


# (name, Cin, Cout, k, dil, N, H, W, math, live taps of the first and of the last forward tile, weight-gradient plans)
# weight-gradient plans: (WGRAD_PP, WGRAD_PP_CUS) -- 2 = the slab plan, 1 = stream-K (pieces that begin in the middle of a row)
CASES = [
    # BASELINE config 2's layer6 geometry, small: tiles of 320 = 4 rows of 80, so the first tile of an image has the three taps ky = 0
    # dead and the last the three taps ky = 2; two slabs of one image each, and stream-K pieces of 45 K-steps
    ("cfg2", 256, 256, 3, 4, 2, 8, 80, "f16x3", (6, 6), ((2, 18), (2, 9), (1, 16))),
    # H <= dilation: both outer kernel rows are dead in every tile, only the centre row lives
    ("low", 256, 256, 3, 4, 2, 4, 80, "f16x3", (3, 3), ((2, 9),)),
    # tiles that straddle two images (240 pixels per image): the live mask is the OR over both -- tile 1 holds rows 2-5 of image 1
    # (ky = 0 live) and rows 0-3 of image 2 (ky = 2 live); the last tile is rows 4-5 of image 2 and 240 masked pixels: ky = 2 dead
    ("straddle", 256, 256, 3, 2, 3, 6, 40, "f16x3", (9, 6), ((2, 9),)),
    # ragged last tile: 1440 pixels = 4.5 tiles; the last holds rows 7-8 of image 1 and 160 masked pixels
    ("ragged", 256, 256, 3, 4, 2, 9, 80, "f16x3", (6, 6), ((2, 9), (1, 16))),
    # no dead taps: 1 x 1, and dilation 1 (a tile of four rows reaches every tap) -- the same results from the same number of steps
    ("1x1", 256, 256, 1, 1, 2, 8, 80, "f16x3", (1, 1), ()),
    ("dil1", 256, 256, 3, 1, 2, 8, 80, "f16x3", (9, 9), ((2, 9),)),
    # the one-term arithmetic with two K-steps per barrier interval (PP_DEEP = 1): 6 live taps x 16 channel chunks = an even step count
    ("deep-even", 256, 256, 3, 4, 2, 8, 80, "f16x1", (6, 6), ((2, 9),)),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_dead_taps_bitwise(case, monkeypatch, libopt):
    """forward (+ BatchNorm partial rows), data gradient, data gradient + addend (staged through LDS) and weight gradient with the dead
    K-steps skipped against the full loop: torch.equal; ``cfg2`` also against fp64 within the ping-pong tests' 2e-5"""
    dev = _dev()
    from mcdseg import ops
    name, cin, cout, k, dil, n, h, w, math, want_live, wgrad_plans = case
    monkeypatch.setattr(ops, "CONV_MATH", math)
    libopt(PP_CUS=16, PP_MIN_ROUNDS=1, PINGPONG=4, PP_DEEP=1)
    x, wt, pad = _inputs(cin, cout, k, dil, n, h, w, 51)
    desc = ops.conv_desc(x.shape, wt.shape, 1, pad, dil)
    tiles = -(-n * desc.Ho * desc.Wo // TILE)
    assert (_live_taps(n, h, w, k, dil, pad, desc.Ho, desc.Wo, 0), _live_taps(n, h, w, k, dil, pad, desc.Ho, desc.Wo, tiles - 1)) == want_live
    if name == "straddle":
        assert _live_taps(n, h, w, k, dil, pad, desc.Ho, desc.Wo, 1) == 9
    pk = ops.PackedWeights()
    wf, wd, mpf = pk.get(wt.to(dev), desc)
    xg = x.to(dev)
    gy = torch.randn(n, cout, desc.Ho, desc.Wo, generator=torch.Generator().manual_seed(52))
    gyg = gy.to(dev)
    addend = torch.randn(x.shape, generator=torch.Generator().manual_seed(53)).to(dev)
    x_cb, x_bound = ops.split_companion(xg)
    gy_cb, gy_bound = ops.split_companion(gyg)
    L, mid = ops.lib(), ops.MATH_ID[math]
    assert L.mcdseg_conv_split_wide_pingpong(ctypes.byref(desc), mid, 1, 0) == 1 and L.mcdseg_conv_split_wide_pingpong(ctypes.byref(desc), mid, 1, 1) == 1
    deep = math == "f16x1"
    assert bool(L.mcdseg_conv_split_pp_deep(ctypes.byref(desc), mid, 0)) == deep

    def fwd_bwd():
        rec = _Names()
        prev, ops.LAUNCH_TIMER = ops.LAUNCH_TIMER, rec
        try:
            y, part, rows = ops._conv_fprop(desc, xg, wf, None, True, mpf, x_cb, x_bound, pk.w_bound)
            dx = ops._conv_dgrad(desc, None, wd, gy_cb, gy_bound, pk.w_bound)
            dx_add = ops._conv_dgrad(desc, None, wd, gy_cb, gy_bound, pk.w_bound, addend=addend)
        finally:
            ops.LAUNCH_TIMER = prev
        assert rec.names == [ops.pingpong_kernel_name(False, wide=1, deep=deep)] + [ops.pingpong_kernel_name(True, wide=1, deep=deep)] * 2, rec.names
        return y, part, rows, dx, dx_add

    (y, part, rows, dx, dx_add), (y0, part0, rows0, dx0, dx_add0) = _run_both(libopt, fwd_bwd)
    _same(y, y0, "forward")
    assert rows == rows0
    _same(part, part0, "BatchNorm partial rows")
    _same(dx, dx0, "data gradient")
    _same(dx_add, dx_add0, "data gradient + addend")
    assert torch.equal(dx_add, dx + addend)
    if name == "cfg2":  # the skipped taps were zero contributions, not merely the same in both forms
        ref = F.conv2d(x.double(), wt.double(), None, 1, pad, dil)
        err, scale = float((y.double().cpu() - ref).abs().max()), float(ref.abs().max())
        assert err <= 2e-5 * scale, "forward against fp64: max err %.3e vs scale %.3e" % (err, scale)

    for mode, cus in wgrad_plans:
        libopt(WGRAD_PP=mode, WGRAD_PP_CUS=cus)
        assert L.mcdseg_conv_wgrad_variant(ctypes.byref(desc), mid, 1) == 17, (mode, cus)

        def wgrad():
            rec = _Names()
            prev, ops.LAUNCH_TIMER = ops.LAUNCH_TIMER, rec
            try:
                dw = ops._conv_wgrad(desc, xg, gyg, x_cb, gy_cb, x_bound, gy_bound)
            finally:
                ops.LAUNCH_TIMER = prev
            assert rec.names == ["conv_wgrad_split_pp_kernel<%s>" % ("SplitF16x1D" if deep else ops.POLICY[math])], rec.names
            return dw

        dw, dw0 = _run_both(libopt, wgrad)
        _same(dw, dw0, "weight gradient (WGRAD_PP=%d, %d CUs)" % (mode, cus))
        if name == "cfg2" and mode == 2 and cus == 18:
            w64 = wt.double().requires_grad_()
            (gw_ref,) = torch.autograd.grad(F.conv2d(x.double(), w64, None, 1, pad, dil), [w64], gy.double())
            err, scale = float((dw.double().cpu() - gw_ref).abs().max()), float(gw_ref.abs().max())
            assert err <= 2e-5 * scale, "weight gradient against fp64: max err %.3e vs scale %.3e" % (err, scale)


def test_dead_taps_odd_live_steps_fall_back(monkeypatch, libopt):
    """``f16x1`` with PP_DEEP=1 pairs K-steps, so a tile whose live step count is odd must run the full loop.  2 x 2 kernel, dilation 4,
    48 -> 256 channels (3 channel chunks: 12 K-steps, six intervals), 57 x 17 -> 61 x 21 = 1281 pixels: the fifth tile holds ONE pixel, the
    bottom-right corner, which only tap (0, 0) reaches -- 3 live steps.  Forward and partial rows against the full loop and fp64."""
    dev = _dev()
    from mcdseg import ops
    monkeypatch.setattr(ops, "CONV_MATH", "f16x1")
    libopt(PP_CUS=16, PP_MIN_ROUNDS=1, PINGPONG=4, PP_DEEP=1)
    cin, cout, k, dil, n, h, w = 48, 256, 2, 4, 1, 57, 17
    x, wt, pad = _inputs(cin, cout, k, dil, n, h, w, 54)
    desc = ops.conv_desc(x.shape, wt.shape, 1, pad, dil)
    assert (desc.Ho, desc.Wo) == (61, 21)
    assert [_live_taps(n, h, w, k, dil, pad, 61, 21, t) for t in (0, 4)] == [4, 1]
    L, mid = ops.lib(), ops.MATH_ID["f16x1"]
    assert L.mcdseg_conv_split_pp_deep(ctypes.byref(desc), mid, 0) == 1
    pk = ops.PackedWeights()
    wf, _, mpf = pk.get(wt.to(dev), desc)
    xg = x.to(dev)
    x_cb, x_bound = ops.split_companion(xg)

    def fwd():
        rec = _Names()
        prev, ops.LAUNCH_TIMER = ops.LAUNCH_TIMER, rec
        try:
            out = ops._conv_fprop(desc, xg, wf, None, True, mpf, x_cb, x_bound, pk.w_bound)
        finally:
            ops.LAUNCH_TIMER = prev
        assert rec.names == [ops.pingpong_kernel_name(False, wide=1, deep=True)], rec.names
        return out

    (y, part, rows), (y0, part0, rows0) = _run_both(libopt, fwd)
    _same(y, y0, "forward")
    assert rows == rows0
    _same(part, part0, "BatchNorm partial rows")
    # the one-term arithmetic rounds both operands to fp16 (2^-11 each, so 2^-10 per product) and adds in fp32: per output
    # |error| <= 2^-10 sum |x| |w|, plus the fp32 sums' and the below-normal operands' share, far under 1e-5 of the scale
    ref = F.conv2d(x.double(), wt.double(), None, 1, pad, dil)
    bound = 2.0 ** -10 * F.conv2d(x.double().abs(), wt.double().abs(), None, 1, pad, dil) + 1e-5 * float(ref.abs().max())
    assert bool(((y.double().cpu() - ref).abs() <= bound).all()), float(((y.double().cpu() - ref).abs() / bound).max())


def test_dead_rows_row_of_taps_weight_gradient(monkeypatch, libopt):
    """``conv_wgrad_split_pp3_kernel`` (a tile is one kernel ROW of three taps): 128 -> 128, 8 x 80, dilation 4 -- rows 0-3 of every image
    are dead for ky = 0, rows 4-7 for ky = 2 -- as one slab and as two slabs of one image each, against the full loop and fp64"""
    dev = _dev()
    from mcdseg import ops
    monkeypatch.setattr(ops, "CONV_MATH", "f16x3")
    libopt(PP_CUS=16, PP_MIN_ROUNDS=1)
    x, wt, pad = _inputs(128, 128, 3, 4, 2, 8, 80, 55)
    desc = ops.conv_desc(x.shape, wt.shape, 1, pad, 4)
    gy = torch.randn(2, 128, 8, 80, generator=torch.Generator().manual_seed(56))
    xg, gyg = x.to(dev), gy.to(dev)
    x_cb, x_bound = ops.split_companion(xg)
    gy_cb, gy_bound = ops.split_companion(gyg)
    L, mid = ops.lib(), ops.MATH_ID["f16x3"]
    w64 = wt.double().requires_grad_()
    (gw_ref,) = torch.autograd.grad(F.conv2d(x.double(), w64, None, 1, pad, 4), [w64], gy.double())
    for cus in (3, 6):
        libopt(WGRAD_PP_CUS=cus)
        assert L.mcdseg_conv_wgrad_variant(ctypes.byref(desc), mid, 1) == 18, cus

        def wgrad():
            rec = _Names()
            prev, ops.LAUNCH_TIMER = ops.LAUNCH_TIMER, rec
            try:
                dw = ops._conv_wgrad(desc, xg, gyg, x_cb, gy_cb, x_bound, gy_bound)
            finally:
                ops.LAUNCH_TIMER = prev
            assert rec.names == ["conv_wgrad_split_pp3_kernel<SplitF16x3>"], rec.names
            return dw

        dw, dw0 = _run_both(libopt, wgrad)
        _same(dw, dw0, "weight gradient (row of taps, %d CUs)" % cus)
        err, scale = float((dw.double().cpu() - gw_ref).abs().max()), float(gw_ref.abs().max())
        assert err <= 2e-5 * scale, "weight gradient against fp64: max err %.3e vs scale %.3e" % (err, scale)
