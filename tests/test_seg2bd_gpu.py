"""GPU: the two boundary losses of the triple multitask decoder (csrc/seg2bd.hip, csrc/boundary.hip) --

  ops.seg2bd_bce                bce2d(sigmoid(conv5x5(bilinear8(z)) + b), t) for two heads, from the 1/8-resolution logits
  ops.boundary_head_bce_target  bce2d(boundary_head(s1, s2, s3), t) against a given target

-- against the statement in plain torch on the CPU, in fp64 (the truth) and fp32 (the yardstick):

  t_bce2d(sigmoid(F.conv2d(F.interpolate(z, scale_factor=8, mode="bilinear", align_corners=False), w, b, padding=2)), t)

Tolerance: the rule of tests/test_segbd_gpu.py, whose helper is used as it stands -- |HIP - fp64| <= 2.0 * |torch fp32 - fp64| + 2e-6 * scale,
per tensor (loss1, loss2, beta, dz1, dz2, dw, db); the ratio is printed per tensor.  The kernel sums over the channels at LOW
resolution (the up-sampler and the convolution are linear), i.e. in another order than torch; the margin of 2 and the 2e-6 of the scale
are for exactly that and for the device's expf / logf.  Inputs: z = 2 randn, w = 0.5 randn / sqrt(25 C), and max |v| < 8 is asserted
in fp64, so the rule compares arithmetic, not sigmoid saturation (which has a test of its own).  Where a check is bitwise or exactly
zero it is written as such.

Shapes (N, C, H, W): (1,1,8,8) -- the 1/8 map is one pixel, every bilinear tap clamps and the 5x5 window overhangs all four borders;
(2,5,16,24); (3,41,40,72) -- odd C, a 5 x 9 low-resolution map, several blocks; (1,3,72,40) -- taller than wide."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from test_segbd_gpu import SHAPES as HEAD_SHAPES
from test_segbd_gpu import _Truth, _labels, _maps, t_bce2d, t_boundary

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 8, 8), (2, 5, 16, 24), (3, 41, 40, 72), (1, 3, 72, 40)]
TARGETS = ["u8", "f32", "soft"]
UP = (0.7, 1.3)  # the two losses' incoming gradients
_ids = lambda s: "x".join(map(str, s))  # noqa: E731


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def t_seg2bd(z, w, b, t):
    u = F.interpolate(z, scale_factor=8, mode="bilinear", align_corners=False)
    return t_bce2d(torch.sigmoid(F.conv2d(u, w, b, padding=2)), t)


def _target(shape, kind):
    n, _, h, w = shape
    if kind == "soft":
        return torch.rand(n, 1, h, w, generator=torch.Generator().manual_seed(h + 3 * w)) ** 3
    hard = t_boundary(_labels((n, h, w), "random", h))[:, None]
    return hard.to(torch.uint8) if kind == "u8" else hard.float()


@functools.lru_cache(maxsize=None)
def _case(shape, kind):
    """inputs and the fp64 / fp32 CPU results of one shape and target kind, computed once and shared (read-only)"""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(1000 * c + 7 * h + w)
    z = [2 * torch.randn(n, c, h // 8, w // 8, generator=g) for _ in range(2)]
    wt = torch.randn(1, c, 5, 5, generator=g) * 0.5 / math.sqrt(25 * c)
    b = 0.1 * torch.randn(1, generator=g)
    t = _target(shape, kind)
    out = {"z": z, "w": wt, "b": b, "t": t}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        zx = [a.to(dt).requires_grad_() for a in z]
        wx, bx = wt.to(dt).requires_grad_(), b.to(dt).requires_grad_()
        losses = [t_seg2bd(a, wx, bx, t) for a in zx]
        out["loss" + tag] = [v.detach() for v in losses]
        out["grad" + tag] = torch.autograd.grad(UP[0] * losses[0] + UP[1] * losses[1], zx + [wx, bx])
        if tag == "64":
            with torch.no_grad():
                v = F.conv2d(F.interpolate(zx[0], scale_factor=8, mode="bilinear", align_corners=False), wx, bx, padding=2)
            assert float(v.abs().max()) < 8, float(v.abs().max())
    out["beta64"] = 1 - t.double().mean()
    out["beta32"] = 1 - t.float().mean()
    return out


def _run(ops, dev, c, target=None, two=True, up=UP):
    zx = [a.to(dev).requires_grad_() for a in c["z"]]
    wx, bx = c["w"].to(dev).requires_grad_(), c["b"].to(dev).requires_grad_()
    t = c["t"].to(dev) if target is None else target
    l1, l2, beta = ops.seg2bd_bce(zx[0], zx[1] if two else None, wx, bx, t, return_beta=True)
    total = up[0] * l1 + (up[1] * l2 if two else 0)
    grads = torch.autograd.grad(total, (zx if two else zx[:1]) + [wx, bx])
    return l1, l2, beta, grads


# ------------------------------------------------------------------------------------------------------------------ seg2bd_bce
@pytest.mark.parametrize("kind", TARGETS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_seg2bd_bce_fwd_bwd(shape, kind):
    dev = _dev()
    from mcdseg import ops
    c = _case(shape, kind)
    l1, l2, beta, grads = _run(ops, dev, c)
    t = _Truth("seg2bd_bce %s %s" % (kind, _ids(shape)))
    t.check(l1, c["loss64"][0], c["loss32"][0], "loss1")
    t.check(l2, c["loss64"][1], c["loss32"][1], "loss2")
    t.check(beta, c["beta64"], c["beta32"], "beta")
    for k, name in enumerate(("dz1", "dz2", "dw", "db")):
        assert grads[k].shape == c["grad64"][k].shape
        t.check(grads[k], c["grad64"][k], c["grad32"][k], name)
    t.report()


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_channel_slice_target_is_read_in_place_bitwise(shape):
    """the trainer's target is channel 6 of its 7-channel source batch: the view is handed to the kernel with its batch stride"""
    dev = _dev()
    from mcdseg import ops
    n, _, h, w = shape
    for kind in ("f32", "u8"):
        c = _case(shape, kind)
        wide = torch.zeros(n, 7, h, w, dtype=c["t"].dtype)
        wide[:, :6] = 3  # (anything the kernel must not read)
        wide[:, 6:] = c["t"]
        wide = wide.to(dev)
        view = wide[:, 6:, :, :]
        assert not view.is_contiguous() or n == 1
        a = _run(ops, dev, c, target=view)
        b = _run(ops, dev, c, target=view.contiguous())
        for x, y in zip(a[:3] + tuple(a[3]), b[:3] + tuple(b[3])):
            assert torch.equal(x, y)
        flat = _run(ops, dev, c, target=wide[:, 6])  # [N,H,W]
        assert torch.equal(flat[0], a[0]) and torch.equal(flat[3][0], a[3][0])


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_one_head_is_head_one_of_the_two_head_call(shape):
    dev = _dev()
    from mcdseg import ops
    c = _case(shape, "soft")
    l1, l2, beta, grads = _run(ops, dev, c, two=False)
    assert l2 is None
    m1, _, mbeta, mgrads = _run(ops, dev, c, two=True, up=(UP[0], 0.0))
    assert torch.equal(l1, m1) and torch.equal(beta, mbeta)
    assert torch.equal(grads[0], mgrads[0])  # dz1
    assert float(mgrads[1].abs().max()) == 0.0  # head 2 received a zero upstream gradient
    # dw and db are fp64 sums over heads and pixels, rounded once: the silent head adds exact zeros, only the grouping of the partial
    # rows may differ
    for a, b in ((grads[1], mgrads[2]), (grads[2], mgrads[3])):
        assert float((a - b).abs().max()) <= 2.0 ** -22 * float(b.abs().max())


def test_two_launches_are_bitwise_equal():
    dev = _dev()
    from mcdseg import ops
    c = _case(SHAPES[2], "soft")
    runs = []
    for _ in range(2):
        l1, l2, beta, grads = _run(ops, dev, c)
        runs.append([l1, l2, beta] + list(grads))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("value", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_degenerate_targets_give_exact_zeros(shape, value):
    """an all-zero target has beta = 1 and an all-one target beta = 0: the weight 1 - beta + (2 beta - 1) t of every pixel is exactly 0"""
    dev = _dev()
    from mcdseg import ops
    n, cc, h, w = shape
    c = dict(_case(shape, "f32"))
    for dtype in (torch.uint8, torch.float32):
        for amp in (1.0, 20.0):
            c["z"] = [a * amp for a in _case(shape, "f32")["z"]]
            l1, l2, beta, grads = _run(ops, dev, c, target=torch.full((n, 1, h, w), value, dtype=dtype, device=dev))
            assert float(l1) == 0.0 and float(l2) == 0.0 and float(beta) == 1.0 - value
            for gr in grads:
                assert bool(torch.isfinite(gr).all()) and float(gr.abs().max()) == 0.0


@pytest.mark.parametrize("sign", ["plus", "minus", "mixed"])
@pytest.mark.parametrize("shape", SHAPES[1:3], ids=_ids)
def test_saturated_logits_follow_torch_clamp_and_eps(shape, sign):
    """|v| > 40 everywhere, in the form of the segbd test of this name: constant logits of +-1 under a constant weight, the power of two
    with 9 C w > 40 -- a corner pixel, whose window holds 9 of the 25 taps, reaches 45 (C = 5) or 46.125 (C = 41), an interior one 125 or
    128.125.  Every product and partial sum is then exact in fp32, whatever the order, so v is the same number on the device, in torch's
    fp32 and in fp64, and what is compared is the clamp and eps arithmetic behind it: sigmoid is 1 or (nearly) 0, the logs are clamped at
    -100 and the backward denominator at 1e-12.  (Logits with rounding errors would not do: where q = exp(-|v|), half an ulp of v = 45 is
    a RELATIVE error of 2e-6 in every gradient, whichever order the sum was taken in -- the size of the rule's whole allowance.)  Finite
    everywhere and within the rule of torch's own results."""
    dev = _dev()
    from mcdseg import ops
    n, cc, h, w = shape
    z = [torch.ones(n, cc, h // 8, w // 8) for _ in range(2)]
    if sign == "minus":
        z = [-a for a in z]
    if sign == "mixed":  # per image, so that no window mixes signs
        flip = torch.tensor([1.0 if k % 2 == 0 else -1.0 for k in range(n)]).reshape(n, 1, 1, 1)
        z = [a * flip for a in z]
    wt = torch.full((1, cc, 5, 5), 2.0 ** math.ceil(math.log2(40.0 / (9 * cc))))
    b = torch.zeros(1)
    tt = _target(shape, "f32")
    res = {}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        zx = [a.to(dt).requires_grad_() for a in z]
        wx, bx = wt.to(dt).requires_grad_(), b.to(dt).requires_grad_()
        losses = [t_seg2bd(a, wx, bx, tt) for a in zx]
        res[tag] = ([v.detach() for v in losses], torch.autograd.grad(losses[0] + losses[1], zx + [wx, bx]))
        if tag == "64":
            with torch.no_grad():
                v = F.conv2d(F.interpolate(zx[0], scale_factor=8, mode="bilinear", align_corners=False), wx, bx, padding=2)
            assert float(v.abs().min()) > 40
    c = {"z": z, "w": wt, "b": b, "t": tt}
    l1, l2, _, grads = _run(ops, dev, c, up=(1.0, 1.0))
    t = _Truth("seg2bd saturated %s %s" % (sign, _ids(shape)))
    t.check(l1, res["64"][0][0], res["32"][0][0], "loss1")
    t.check(l2, res["64"][0][1], res["32"][0][1], "loss2")
    for k, name in enumerate(("dz1", "dz2", "dw", "db")):
        t.check(grads[k], res["64"][1][k], res["32"][1][k], name)
    t.report()


def test_seg2bd_statement_and_kernel_match_the_reference_fixture(golden):
    """ties the torch statement above to what the REAL reference's get_boundary_loss_by_extra_conv returned
    (tests/golden/make_triple_golden.py), then the kernel to the reference's fp64 numbers under the tolerance of
    test_decoder_boundary_forward_matches_the_reference_fixture: max(2 |ref32 - ref64|, 2e-5 of the scale)"""
    dev = _dev()
    from mcdseg import ops
    fx = golden.npz("triple_small.npz")
    w64, b64 = (torch.from_numpy(fx["seg2bd_conv." + k]).double() for k in ("weight", "bias"))
    gt = torch.from_numpy(fx["gt_bd"])
    soft = torch.from_numpy(fx["f64/boundary_forward"])
    for name, t in (("extra_gt", gt), ("extra_none", soft)):
        for k in (1, 2):
            got = float(t_seg2bd(torch.from_numpy(fx["f64/z%d" % k]), w64, b64, t.double()))
            want = float(fx["f64/" + name][k - 1])
            assert abs(got - want) <= 1e-12 * abs(want), (name, k, got, want)
    zx = [torch.from_numpy(fx["f64/z%d" % k]).float().to(dev).requires_grad_() for k in (1, 2)]
    wx, bx = w64.float().to(dev).requires_grad_(), b64.float().to(dev).requires_grad_()
    l1, l2 = ops.seg2bd_bce(zx[0], zx[1], wx, bx, gt.to(dev))
    dw, db = torch.autograd.grad(l1 + l2, [wx, bx])
    n1, n2 = ops.seg2bd_bce(zx[0], zx[1], wx, bx, soft.float().to(dev))
    cases = (("extra_gt", torch.stack([l1, l2])), ("extra_none", torch.stack([n1, n2])), ("d_seg2bd_w", dw), ("d_seg2bd_b", db))
    for name, got in cases:
        r64, r32 = torch.from_numpy(fx["f64/" + name]).double(), torch.from_numpy(fx["f32/" + name]).double()
        e, e32 = float((got.detach().double().cpu() - r64).abs().max()), float((r32 - r64).abs().max())
        print("seg2bd fixture %s: |HIP - ref64| %.3e, |ref32 - ref64| %.3e" % (name, e, e32))
        assert e <= max(2.0 * e32, 2e-5 * float(r64.abs().max())), name


# ------------------------------------------------------------------------------------------------------------------ boundary_head_bce_target
@pytest.mark.parametrize("kind", ["f32", "u8", "view"])
@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=_ids)
def test_boundary_head_bce_target_is_the_composition(shape, kind):
    """the gradients are those of ops.boundary_head -> ops.bce2d on the same target bit for bit (the same device functions, fp contraction
    off); the loss agrees up to the order of its partial sums"""
    dev = _dev()
    from mcdseg import ops
    n, h, w = shape
    s = _maps(shape, 5 * h + w)
    hard = t_boundary(_labels(shape, "random", w))[:, None]
    tgt = (hard.to(torch.uint8) if kind == "u8" else hard.float()).to(dev)
    given = tgt
    if kind == "view":
        wide = torch.full((n, 7, h, w), 3.0, device=dev)
        wide[:, 6:] = tgt
        given = wide[:, 6:]
    gout = torch.tensor(0.6, device=dev)
    sx = [t.to(dev).requires_grad_() for t in s]
    loss = ops.boundary_head_bce_target(*sx, given)
    ds = torch.autograd.grad(loss, sx, gout)
    sy = [t.to(dev).requires_grad_() for t in s]
    loss_c = ops.bce2d(ops.boundary_head(*sy), tgt)
    ds_c = torch.autograd.grad(loss_c, sy, gout)
    print("boundary_head_bce_target %s %s: loss %.9g, composition %.9g" % (kind, _ids(shape), float(loss), float(loss_c)))
    assert abs(float(loss) - float(loss_c)) <= 2e-6 * abs(float(loss_c))
    for a, b in zip(ds, ds_c):
        assert torch.equal(a, b)
    # ... and both against the torch statement, under the rule
    res = {}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        st = [t.to(dt).requires_grad_() for t in s]
        from test_segbd_gpu import t_head
        lt = t_bce2d(t_head(*st), hard)
        res[tag] = (lt.detach(), torch.autograd.grad(lt, st))
    t = _Truth("boundary_head_bce_target %s %s" % (kind, _ids(shape)))
    t.check(loss, res["64"][0], res["32"][0], "loss")
    for k in range(3):
        t.check(ds[k], 0.6 * res["64"][1][k], 0.6 * res["32"][1][k], "ds%d" % (k + 1))
    t.report()


def test_ops_check_their_arguments():
    dev = _dev()
    from mcdseg import ops
    z = torch.zeros(1, 3, 2, 2, device=dev)
    w, b = torch.zeros(1, 3, 5, 5, device=dev), torch.zeros(1, device=dev)
    with pytest.raises(ValueError, match="does not match"):
        ops.seg2bd_bce(z, z, w, b, torch.zeros(1, 1, 8, 8, device=dev))
    with pytest.raises(ValueError, match="nn.Conv2d"):
        ops.seg2bd_bce(z, z, torch.zeros(1, 3, 3, 3, device=dev), b, torch.zeros(1, 1, 16, 16, device=dev))
    with pytest.raises(TypeError, match="uint8 or torch.float32"):
        ops.seg2bd_bce(z, z, w, b, torch.zeros(1, 1, 16, 16, device=dev, dtype=torch.int64))
    with pytest.raises(ValueError, match="target"):
        ops.seg2bd_bce(z, z, w, b, torch.zeros(1, 1, 16, 16, device=dev, requires_grad=True))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.seg2bd_bce(z.cpu(), None, w.cpu(), b.cpu(), torch.zeros(1, 1, 16, 16))
