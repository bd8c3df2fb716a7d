"""GPU: the small streaming kernels -- gate_mix, softmax_ch, prob_nll (csrc/fusion.hip) and sgd_momentum_flat (csrc/sgd.hip) --
against a plain fp64 PyTorch-CPU statement of the same operation, at the edges of their launch geometry: both sides of every
template and grid boundary, partial last blocks, image offsets, the float4 body / scalar tail / all-scalar forms, saturated
exponentials, ignored and out-of-range labels.

Tolerance: the rule of tests/test_model_gpu.py (TRUTH_OUTPUT) per tensor -- a HIP result may be at most 2.0 times as far from
fp64 as fp32 torch on the CPU is, plus 2e-6 of the tensor's scale.  Each test prints the ratio err_hip / err_torch32 it measured
(docs/MEASURED_HISTORY.md records them).  Where a check is bitwise or exactly zero it is written as such."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TRUTH_OUTPUT = 2.0  # tests/test_model_gpu.py: max |HIP - fp64| in units of fp32 torch's own distance from fp64 (+ 2e-6 of the scale)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class _Truth:
    """collects err_hip / err_torch32 of every tensor a test checks and prints the worst"""

    def __init__(self, kernel):
        self.kernel, self.worst, self.where = kernel, 0.0, "-"

    def check(self, got, ref64, ref32, what, scale=None):
        got = got.detach().double().cpu()
        ref64 = ref64.detach().double()
        assert got.shape == ref64.shape, "%s %s: shape %s vs %s" % (self.kernel, what, tuple(got.shape), tuple(ref64.shape))
        assert bool(torch.isfinite(got).all()), "%s %s: not finite" % (self.kernel, what)
        e = float((got - ref64).abs().max())
        e32 = float((ref32.detach().double() - ref64).abs().max())
        sc = float(ref64.abs().max()) if scale is None else float(scale)
        ratio = e / e32 if e32 > 0 else (0.0 if e == 0 else float("inf"))
        if e32 > 0 and ratio > self.worst:
            self.worst, self.where = ratio, what
        print("%s %s: |HIP - fp64| %.3e, |torch32 - fp64| %.3e (ratio %.2f), scale %.3e" % (self.kernel, what, e, e32, ratio, sc))
        assert e <= TRUTH_OUTPUT * e32 + 2e-6 * sc, "%s %s: max |HIP - fp64| %.3e, fp32 torch's %.3e (scale %.3e)" % (self.kernel, what, e, e32, sc)

    def report(self):
        print("%s: worst err_hip / err_torch32 = %.2f (%s)" % (self.kernel, self.worst, self.where))


def _offset(t, dev):
    """the values of 1-D ``t`` on the GPU as ``base[1:1+n]``: contiguous, 4 bytes past a 16-byte boundary"""
    base = torch.zeros(t.numel() + 8, dtype=t.dtype, device=dev)
    v = base[1:1 + t.numel()]
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


# ------------------------------------------------------------------------------------------------------------------ softmax_ch
SOFTMAX_CASES = [(1, 1, 1, 1),
                 (2, 24, 3, 5), (2, 25, 3, 5), (1, 48, 1, 7), (1, 49, 2, 3), (1, 64, 1, 3),  # both sides of <24> | <48> | <64>
                 (2, 41, 1, 255), (2, 41, 1, 256), (3, 41, 1, 257), (2, 19, 17, 31)]        # HW around one block; 527 = 3 blocks


def _softmax_inputs(shape, kind, g):
    if kind == "equal":
        return torch.full(shape, float(torch.randn(1, generator=g)) * 3)
    x = torch.randn(shape, generator=g) * 3
    if kind == "saturated":  # most probabilities underflow to exact 0, one per pixel is about 1
        x = x + (torch.rand(shape, generator=g) * 180 - 90)
    return x


@pytest.mark.parametrize("kind", ["randn", "saturated", "equal"])
@pytest.mark.parametrize("shape", SOFTMAX_CASES, ids=lambda s: "x".join(map(str, s)))
def test_softmax_channels_fwd_bwd(shape, kind):
    dev = _dev()
    from mcdseg import ops
    n, c, h, w = shape
    g = torch.Generator().manual_seed(1000 * c + h * w)
    x = _softmax_inputs(shape, kind, g)
    dy = torch.randn(shape, generator=g)
    x64, x32 = x.double().requires_grad_(), x.clone().requires_grad_()
    y64, y32 = F.softmax(x64, 1), F.softmax(x32, 1)
    (dx64,) = torch.autograd.grad(y64, x64, dy.double())
    (dx32,) = torch.autograd.grad(y32, x32, dy)
    xd = x.to(dev).requires_grad_()
    y = ops.softmax_channels(xd)
    (dx,) = torch.autograd.grad(y, xd, dy.to(dev))
    t = _Truth("softmax_ch %s %s" % (kind, "x".join(map(str, shape))))
    t.check(y, y64, y32, "y")
    t.check(dx, dx64, dx32, "dx")
    yc, dxc = y.detach().double().cpu(), dx.detach().double().cpu()
    assert bool(torch.isfinite(yc).all()) and bool(torch.isfinite(dxc).all())
    assert float(yc.min()) >= 0.0 and float(yc.max()) <= 1.0
    assert float((yc.sum(1) - 1.0).abs().max()) <= c * 2.0 ** -23
    if kind == "equal":
        assert float((yc - 1.0 / c).abs().max()) <= 2.0 ** -24  # y = v * (1 / s) with v = expf(0) = 1 and s = C exactly: one rounding
    # sum_c dx = 0 in exact arithmetic: held to the rule above with 0 as the truth and dx's own scale
    t.check(dx.detach().double().cpu().sum(1), torch.zeros(n, h, w, dtype=torch.float64), dx32.double().sum(1), "sum_c dx",
            scale=dx64.abs().max())
    t.report()


def test_softmax_channels_refuses_more_than_64_channels():
    dev = _dev()
    from mcdseg import ops
    with pytest.raises(RuntimeError, match="C <= 64"):
        ops.softmax_channels(torch.zeros(1, 65, 2, 3, device=dev))


# -------------------------------------------------------------------------------------------------------------------- gate_mix
GATE_BODY = 4 * (3 * 1024 + 17)  # 3089 float4s on 4 blocks x 256 threads: three full grid-stride iterations and a ragged fourth
GATE_CASES = [(1,), (3,), (4,), (5,), (615,), (1, 41, 3, 5), (GATE_BODY,), (GATE_BODY + 3,)]
GATE_EDGES = [0.0, 20.0, -20.0, 88.0, -88.0, 104.0, -104.0, 1e4, -1e4]  # expf(-g) overflows to inf above 88.7, underflows to 0 below -103.3


def _gate_inputs(shape, gates, seed):
    g = torch.Generator().manual_seed(seed)
    x1, x2, dy = (torch.randn(shape, generator=g) for _ in range(3))
    gl = torch.randn(shape, generator=g) * 2
    if gates == "edges":
        flat = gl.reshape(-1)
        k = torch.arange(0, flat.numel(), 2)  # every other element, so that both neighbours of a float4 differ
        flat[k] = torch.tensor(GATE_EDGES)[(k // 2) % len(GATE_EDGES)]
    return x1, x2, gl, dy


def _gate_reference(x1, x2, gl, dy):
    s = torch.sigmoid(gl)
    return x1 * s + x2 * (1 - s), dy * s, dy * (1 - s), dy * (x1 - x2) * s * (1 - s)


def _gate_hip(ops, x1, x2, gl, dy):
    x1, x2, gl = (v.detach().requires_grad_() for v in (x1, x2, gl))  # (detach keeps the storage offset of a slice)
    out = ops.gate_mix(x1, x2, gl)
    return (out,) + torch.autograd.grad(out, [x1, x2, gl], dy)


@pytest.mark.parametrize("gates", ["randn", "edges"])
@pytest.mark.parametrize("shape", GATE_CASES, ids=lambda s: "x".join(map(str, s)))
def test_gate_mix_fwd_bwd(shape, gates):
    dev = _dev()
    from mcdseg import ops
    cpu = _gate_inputs(shape, gates, 7 + len(shape) + shape[-1])
    ref64 = _gate_reference(*(v.double() for v in cpu))
    ref32 = _gate_reference(*cpu)
    got = _gate_hip(ops, *(v.to(dev) for v in cpu))
    t = _Truth("gate_mix %s %s" % (gates, "x".join(map(str, shape))))
    for name, a, r64, r32 in zip(("out", "dx1", "dx2", "dg"), got, ref64, ref32):
        t.check(a, r64, r32, name)
    t.report()


@pytest.mark.parametrize("which", ["all", "g"])
@pytest.mark.parametrize("gates", ["randn", "edges"])
@pytest.mark.parametrize("n", [615, GATE_BODY + 3])
def test_gate_mix_offset_pointers_give_the_aligned_bits(n, gates, which):
    """operands as base[1:1+n] (4 bytes past the 16-byte grid) run the all-scalar form; it evaluates the expression of the
    float4 body, so the results are those of aligned copies bit for bit -- and within the fp64 bound"""
    dev = _dev()
    from mcdseg import ops
    cpu = _gate_inputs((n,), gates, 31 + n)
    aligned = [v.to(dev) for v in cpu]
    assert all(v.data_ptr() % 16 == 0 for v in aligned)
    x1, x2, gl, dy = aligned
    moved = [_offset(x1, dev), _offset(x2, dev), _offset(gl, dev), _offset(dy, dev)] if which == "all" else [x1, x2, _offset(gl, dev), dy]
    want = _gate_hip(ops, *aligned)
    got = _gate_hip(ops, *moved)
    for name, a, b in zip(("out", "dx1", "dx2", "dg"), got, want):
        assert torch.equal(a, b), "gate_mix %s: the offset call differs from the aligned one in %d elements" % (name, int((a != b).sum()))
    ref64 = _gate_reference(*(v.double() for v in cpu))
    ref32 = _gate_reference(*cpu)
    t = _Truth("gate_mix offset(%s) %s n=%d" % (which, gates, n))
    for name, a, r64, r32 in zip(("out", "dx1", "dx2", "dg"), got, ref64, ref32):
        t.check(a, r64, r32, name)
    t.report()


@pytest.mark.parametrize("score", [False, True], ids=["GateFusion", "ScoreGateFusion"])
def test_gate_fusion_module_on_an_odd_element_count(score):
    """GateFusion(41) on one 3x5 score map: 615 elements, not a multiple of 4.  Forward and backward against the module's
    formula in fp64, the 1x1 gate convolution from F.conv2d in fp64."""
    dev = _dev()
    from models.fusion import get_fusion_model
    g = torch.Generator().manual_seed(41 + int(score))
    m = get_fusion_model("MFNet-ScoreGateFusion" if score else "MFNet-GateFusion", 41)
    with torch.no_grad():
        m.conv.weight.copy_(torch.randn(m.conv.weight.shape, generator=g) * 0.2)
        m.conv.bias.copy_(torch.randn(41, generator=g))
    x1, x2, gy = (torch.randn(1, 41, 3, 5, generator=g) * (3 if score else 1) for _ in range(3))

    def formula(dtype):
        a, b = x1.clone().to(dtype).requires_grad_(), x2.clone().to(dtype).requires_grad_()
        wt, bs = m.conv.weight.detach().to(dtype).requires_grad_(), m.conv.bias.detach().to(dtype).requires_grad_()
        p1, p2 = (F.softmax(a, 1), F.softmax(b, 1)) if score else (a, b)
        s = torch.sigmoid(F.conv2d(torch.cat([p1, p2], 1), wt, bs))
        y = p1 * s + p2 * (1 - s)
        return (y,) + torch.autograd.grad(y, [a, b, wt, bs], gy.to(dtype))

    ref64, ref32 = formula(torch.float64), formula(torch.float32)
    m = m.to(dev)
    a, b = x1.to(dev).requires_grad_(), x2.to(dev).requires_grad_()
    y = m(a, b)
    got = (y,) + torch.autograd.grad(y, [a, b, m.conv.weight, m.conv.bias], gy.to(dev))
    t = _Truth("ScoreGateFusion(41)" if score else "GateFusion(41)")
    for name, v, r64, r32 in zip(("y", "dx1", "dx2", "dweight", "dbias"), got, ref64, ref32):
        t.check(v, r64, r32, name)
    t.report()


# -------------------------------------------------------------------------------------------------------------------- prob_nll
PROB_CASES = [(2, 41, 16, 32), (3, 5, 7, 9), (2, 2, 1, 1), (2, 3, 40, 52)]  # the last: 4160 pixels = five partial blocks, HW % 256 != 0


def _prob_inputs(shape, ignore_index, seed):
    n, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    p = F.softmax(torch.randn(shape, generator=g) * 3, 1)
    assert float(p.min()) > 0
    labels = torch.randint(0, c, (n, h, w), generator=g)
    u = torch.rand(n, h, w, generator=g)
    for k, bad in enumerate((ignore_index, -1, c, c + 7)):  # about 5 % each
        labels[(u >= 0.05 * k) & (u < 0.05 * (k + 1))] = bad
    labels[0, 0, 0], labels[1, 0, 0] = 0, c - 1  # live in both images, another channel in image 1: a wrong image offset shows
    weight = torch.rand(c, generator=g) + 0.5
    return p, labels, weight


def _prob_reference(p, labels, weight, ignore_index, size_average, dtype):
    """F.nll_loss(log p) and 3 x its gradient.  torch raises for a label outside [0, C); the kernel treats such a pixel as
    ignored, so those labels are mapped to ignore_index first."""
    c = p.shape[1]
    mapped = torch.where((labels < 0) | (labels >= c), torch.full_like(labels, ignore_index), labels)
    pp = p.detach().clone().to(dtype).requires_grad_()
    loss = F.nll_loss(torch.log(pp), mapped, None if weight is None else weight.to(dtype), ignore_index=ignore_index,
                      reduction="mean" if size_average else "sum")
    (grad,) = torch.autograd.grad(3.0 * loss, pp)
    return loss.detach(), grad


def _live_mask(shape, labels, ignore_index):
    n, c, h, w = shape
    live = (labels != ignore_index) & (labels >= 0) & (labels < c)
    mask = torch.zeros(shape, dtype=torch.bool)
    mask.scatter_(1, labels.clamp(0, c - 1).unsqueeze(1), live.unsqueeze(1))
    return live, mask


def _prob_case(shape, weighted, size_average, ignore_index):
    dev = _dev()
    from mcdseg import ops
    n, c, h, w = shape
    p, labels, weight = _prob_inputs(shape, ignore_index, 5 * c + h)
    if not weighted:
        weight = None
    live, mask = _live_mask(shape, labels, ignore_index)
    assert bool(live[0, 0, 0]) and bool(live[1, 0, 0]) and int(labels[0, 0, 0]) != int(labels[1, 0, 0])
    loss64, grad64 = _prob_reference(p, labels, weight, ignore_index, size_average, torch.float64)
    loss32, grad32 = _prob_reference(p, labels, weight, ignore_index, size_average, torch.float32)
    wd = None if weight is None else weight.to(dev)
    pd = p.clone().to(dev).requires_grad_()
    loss = ops.prob_cross_entropy2d(pd, labels.to(dev), wd, ignore_index, size_average)
    (grad,) = torch.autograd.grad(3.0 * loss, pd)
    t = _Truth("prob_nll %s %s %s ignore=%d" % ("x".join(map(str, shape)), "weight" if weighted else "noweight",
                                                 "mean" if size_average else "sum", ignore_index))
    t.check(loss.reshape(1), loss64.reshape(1), loss32.reshape(1), "loss")
    t.check(grad, grad64, grad32, "grad")
    gc = grad.cpu()
    assert torch.equal(gc[~mask], torch.zeros(int((~mask).sum()))), "gradient off the label channel or at an ignored pixel is not 0.0"
    assert bool((gc[mask] < 0).all())
    loss_only = ops.prob_cross_entropy2d(p.to(dev), labels.to(dev), wd, ignore_index, size_average)  # no gradient buffer: the same bits
    assert not loss_only.requires_grad and torch.equal(loss_only, loss.detach())
    t.report()


@pytest.mark.parametrize("ignore_index", [-100, 255])
@pytest.mark.parametrize("size_average", [True, False], ids=["mean", "sum"])
@pytest.mark.parametrize("weighted", [True, False], ids=["weight", "noweight"])
@pytest.mark.parametrize("shape", PROB_CASES, ids=lambda s: "x".join(map(str, s)))
def test_prob_cross_entropy2d(shape, weighted, size_average, ignore_index):
    _prob_case(shape, weighted, size_average, ignore_index)


@pytest.mark.parametrize("size_average", [True, False], ids=["mean", "sum"])
@pytest.mark.parametrize("weighted", [True, False], ids=["weight", "noweight"])
@pytest.mark.parametrize("shape", [(3, 5, 7, 9), (2, 3, 40, 52)], ids=lambda s: "x".join(map(str, s)))
def test_prob_cross_entropy2d_ignores_a_class_index(shape, weighted, size_average):
    """ignore_index = 1 lies inside [0, C): -100 and 255 are also out of range for these C, so only here does a pixel count as
    ignored through the ``y == ignore_index`` comparison alone -- about a third of the labels"""
    _prob_case(shape, weighted, size_average, 1)


@pytest.mark.parametrize("weighted", [True, False], ids=["weight", "noweight"])
def test_prob_cross_entropy2d_with_every_label_ignored(weighted):
    dev = _dev()
    from mcdseg import ops
    shape = (2, 5, 7, 9)
    p, labels, weight = _prob_inputs(shape, 255, 77)
    labels = torch.tensor([255, -1, 5, 12])[torch.randint(0, 4, labels.shape, generator=torch.Generator().manual_seed(1))]
    labels[0, 0, 0] = 255
    if not weighted:
        weight = None
    wd = None if weight is None else weight.to(dev)
    for size_average in (False, True):
        loss64, _ = _prob_reference(p, labels, weight, 255, size_average, torch.float64)
        pd = p.to(dev).requires_grad_()
        loss = ops.prob_cross_entropy2d(pd, labels.to(dev), wd, 255, size_average)
        (grad,) = torch.autograd.grad(3.0 * loss, pd)
        if not size_average:
            assert float(loss) == 0.0 and float(loss64) == 0.0
        assert torch.allclose(loss.detach().double().cpu(), loss64, rtol=0, atol=0, equal_nan=True), (float(loss), float(loss64))
        assert torch.equal(grad.cpu(), torch.zeros(shape))


# ----------------------------------------------------------------------------------------------------------- sgd_momentum_flat
@pytest.mark.parametrize("n", [7, 1027])
def test_sgd_momentum_flat_on_offset_slices(n):
    """two steps on base[1:1+n] slices (the all-scalar form: FlatSGD itself only ever passes the start of its buffers) against
    the fp64 recurrence v = mu*v + wd*p + gs*g; p -= lr*v, and bit for bit against the same call on aligned copies, which runs
    the float4 body (and its tail) with the same fmaf expressions"""
    dev = _dev()
    from mcdseg import ops
    lr, mu, wd, gs = 1e-2, 0.9, 2e-3, 0.5
    gen = torch.Generator().manual_seed(n)
    p0, v0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) for _ in range(2)]

    def recurrence(dtype):
        p, v = p0.to(dtype), v0.to(dtype)
        for gr in grads:
            v = mu * v + wd * p + gs * gr.to(dtype)
            p = p - lr * v
        return p, v

    (p64, v64), (p32, v32) = recurrence(torch.float64), recurrence(torch.float32)
    pa, va = p0.to(dev), v0.to(dev)
    po, vo = _offset(p0, dev), _offset(v0, dev)
    for gr in grads:
        ga = gr.to(dev)
        assert pa.data_ptr() % 16 == 0 and ga.data_ptr() % 16 == 0 and va.data_ptr() % 16 == 0
        ops.sgd_momentum_flat_(pa, ga, va, lr, mu, wd, gs, params=())
        ops.sgd_momentum_flat_(po, _offset(gr, dev), vo, lr, mu, wd, gs, params=())
    assert torch.equal(po, pa) and torch.equal(vo, va)
    t = _Truth("sgd_momentum_flat n=%d" % n)
    t.check(po, p64, p32, "p")
    t.check(vo, v64, v32, "v")
    t.report()
