"""GPU: the boundary branch of the segmentation + boundary multitask variant -- label_boundary, boundary_head, bce2d and the fused
boundary_head_bce (csrc/boundary.hip) -- against a plain fp64 PyTorch-CPU statement of the same operation, then the decoder and the
solver step built on them against torch modules restated here, on the CPU in fp64.

The reference itself cannot run its boundary loss on today's torch (tests/golden/make_segbd_golden.py says what it could capture), so
for the kernels the fp64 torch restatement below is the yardstick; tests/test_segbd.py ties that restatement to what the reference's
own functions return on the golden case.

Tolerance: the rule of tests/test_model_gpu.py (TRUTH_OUTPUT), as tests/test_fusion_kernels_gpu.py applies it per tensor -- a HIP
result may be at most 2.0 times as far from fp64 as fp32 torch on the CPU is, plus 2e-6 of the tensor's scale.  The margin of 2 is for
what legitimately differs from torch's fp32: the order of the sums (per-thread fp32, then fp64 partials, against torch's vectorised
pairwise sums; the gather order of the up-samplers' backward) and the device's expf / logf / log1pf (1-2 ulp) against the host's
vector maths.  The bound never comes from the HIP output.  Each test prints the ratio it measured (docs/MEASURED_HISTORY.md).
Where a check is bitwise or exactly zero it is written as such.

Shapes (full resolution): 8x8 N=1 (the 1/8 map is one pixel: every tap clamps), 16x24 N=2 (interior and edge taps at all scales),
40x72 N=3 (8640 pixels: not a multiple of a block's work, several blocks in the gather kernels)."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TRUTH_OUTPUT = 2.0
SHAPES = [(1, 8, 8), (2, 16, 24), (3, 40, 72)]
_ids = lambda s: "x".join(map(str, s))  # noqa: E731


@pytest.fixture(autouse=True)
def _no_pretrained(monkeypatch):
    monkeypatch.setenv("MCDSEG_PRETRAINED", "0")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class _Truth:
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


# ---------------------------------------------------------------------------------------------- the torch statement (CPU, any dtype)
def t_boundary(labels):
    v = labels.float()[:, None]
    dilation = F.max_pool2d(v, kernel_size=3, stride=1, padding=1)
    erosion = -F.max_pool2d(-v, kernel_size=3, stride=1, padding=1)
    return (dilation != erosion)[:, 0]


def t_head(s1, s2, s3):
    up = lambda x, k: F.interpolate(x, scale_factor=k, mode="bilinear", align_corners=False)  # noqa: E731
    return (torch.sigmoid(up(s1, 2)) + torch.sigmoid(up(s2, 4)) + torch.sigmoid(up(s3, 8))) / 3


def t_bce2d(p, t):
    t = t.reshape(p.shape).to(p.dtype)
    beta = 1 - torch.mean(t)
    w = 1 - beta + (2 * beta - 1) * t
    return F.binary_cross_entropy(p, t, w, reduction="mean")


def _maps(shape, seed, amp=2.0):
    n, h, w = shape
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, 1, h // k, w // k, generator=g) * amp for k in (2, 4, 8)]


def _labels(shape, kind, seed=0):
    n, h, w = shape
    if kind == "constant":
        return torch.zeros(n, h, w, dtype=torch.int64)
    if kind == "checkerboard":
        yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        return ((yy + xx) % 2).expand(n, h, w).contiguous()
    if kind == "corners":
        lab = torch.full((n, h, w), 7, dtype=torch.int64)
        lab[:, 0, 0], lab[:, 0, -1], lab[:, -1, 0], lab[:, -1, -1] = 1, 2, 3, 4
        return lab
    g = torch.Generator().manual_seed(100 + seed)
    # blobs: a coarse random map blown up, so that boundaries are a minority class as in real label maps
    coarse = torch.randint(0, 5, (n, 1, (h + 3) // 4, (w + 3) // 4), generator=g).float()
    return F.interpolate(coarse, size=(h, w), mode="nearest")[:, 0].long().contiguous()


@functools.lru_cache(maxsize=None)
def _head_case(shape, amp=2.0):
    """inputs and the fp64 / fp32 CPU results of one shape, computed once and shared (read-only)"""
    n, h, w = shape
    s = _maps(shape, 7 * h + w, amp)
    g = torch.Generator().manual_seed(h * w)
    dp = torch.randn(n, 1, h, w, generator=g)
    lab = _labels(shape, "random", h)
    out = {"s": s, "dp": dp, "labels": lab}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        sx = [t.to(dt).requires_grad_() for t in s]
        p = t_head(*sx)
        out["p" + tag] = p.detach()
        out["ds" + tag] = torch.autograd.grad(p, sx, dp.to(dt), retain_graph=True)
        loss = t_bce2d(p, t_boundary(lab))
        out["loss" + tag] = loss.detach()
        out["dloss" + tag] = torch.autograd.grad(loss, sx)
    return out


# ------------------------------------------------------------------------------------------------------------------ label_boundary
@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8], ids=["int64", "uint8"])
@pytest.mark.parametrize("kind", ["random", "constant", "checkerboard", "corners"])
@pytest.mark.parametrize("shape", SHAPES + [(2, 5, 13), (1, 1, 1)], ids=_ids)  # (W % 8 != 0: the one-pixel-per-thread kernel)
def test_label_boundary_is_the_max_pool_expression_bitwise(shape, kind, dtype):
    dev = _dev()
    from mcdseg import ops
    lab = _labels(shape, kind, shape[1]).to(dtype)
    want = t_boundary(lab).to(torch.uint8)
    got = ops.label_boundary(lab.to(dev))
    assert got.dtype == torch.uint8 and tuple(got.shape) == shape
    assert torch.equal(got.cpu(), want)
    if kind == "constant":
        assert int(got.sum()) == 0
    if kind == "checkerboard" and shape[1] * shape[2] > 1:
        assert int(got.sum()) == got.numel()
    if kind == "corners" and min(shape[1:]) >= 5:
        assert int(got.sum()) == 4 * 4 * shape[0]  # each island marks its 2x2 corner window


def test_label_boundary_treats_every_integer_as_a_value():
    dev = _dev()
    from mcdseg import ops
    lab = torch.zeros(1, 8, 16, dtype=torch.int64)
    lab[0, 3, 4], lab[0, 6, 12] = -100, 255  # an "ignore" value and the background: values like any other
    assert torch.equal(ops.label_boundary(lab.to(dev)).cpu(), t_boundary(lab).to(torch.uint8))
    big = torch.full((1, 8, 8), 2 ** 40, dtype=torch.int64)
    big[0, 4, 4] = 2 ** 40 + 1  # (float32 could not tell these two apart; the kernel compares integers)
    assert int(ops.label_boundary(big.to(dev)).sum()) == 9


# ------------------------------------------------------------------------------------------------------------------ boundary_head
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_boundary_head_fwd_bwd(shape):
    dev = _dev()
    from mcdseg import ops
    c = _head_case(shape)
    sx = [t.to(dev).requires_grad_() for t in c["s"]]
    p = ops.boundary_head(*sx)
    ds = torch.autograd.grad(p, sx, c["dp"].to(dev))
    t = _Truth("boundary_head " + _ids(shape))
    t.check(p, c["p64"], c["p32"], "p")
    for k in range(3):
        t.check(ds[k], c["ds64"][k], c["ds32"][k], "ds%d" % (k + 1))
    t.report()
    pc = p.detach().cpu()
    assert float(pc.min()) >= 0.0 and float(pc.max()) <= 1.0


# ------------------------------------------------------------------------------------------------------------------ bce2d
@pytest.mark.parametrize("target", ["uint8", "soft"])
@pytest.mark.parametrize("shape", SHAPES + [(1, 3, 7)], ids=_ids)  # (21 elements: the one-by-one tail alone)
def test_bce2d_fwd_bwd(shape, target):
    dev = _dev()
    from mcdseg import ops
    n, h, w = shape
    g = torch.Generator().manual_seed(31 * h + w)
    p = torch.rand(n, 1, h, w, generator=g) * 0.98 + 0.01
    tt = t_boundary(_labels(shape, "random", 3)).to(torch.uint8) if target == "uint8" else torch.rand(n, h, w, generator=g) ** 3
    gout = torch.tensor(1.7)
    res = {}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        px = p.to(dt).requires_grad_()
        loss = t_bce2d(px, tt)
        res[tag] = (loss.detach(), torch.autograd.grad(loss, px, gout.to(dt))[0])
    pd = p.to(dev).requires_grad_()
    loss, beta = ops.bce2d(pd, tt.to(dev), return_beta=True)
    (dp,) = torch.autograd.grad(loss, pd, gout.to(dev))
    t = _Truth("bce2d %s %s" % (target, _ids(shape)))
    t.check(loss, res["64"][0], res["32"][0], "loss")
    t.check(dp, res["64"][1], res["32"][1], "dp")
    t.report()
    assert abs(float(beta) - (1 - float(tt.double().mean()))) <= 2.0 ** -23


def test_bce2d_binary_prediction_has_the_closed_form():
    """the gradient-free extra losses feed bce2d an arg-max boundary: p exactly 0 or 1.  Both logs clamp at -100, so a wrong pixel
    costs 100 w: loss = 100 (beta #(t=1, p=0) + (1 - beta) #(t=0, p=1)) / n"""
    dev = _dev()
    from mcdseg import ops
    g = torch.Generator().manual_seed(5)
    for shape in SHAPES:
        n = shape[0] * shape[1] * shape[2]
        p = (torch.rand(shape, generator=g) < 0.3).to(torch.uint8)
        t = (torch.rand(shape, generator=g) < 0.2).to(torch.uint8)
        beta = 1.0 - float(t.sum()) / n
        closed = 100.0 * (beta * int(((t == 1) & (p == 0)).sum()) + (1 - beta) * int(((t == 0) & (p == 1)).sum())) / n
        loss = float(ops.bce2d(p.float().to(dev), t.to(dev)))
        lossf = float(ops.bce2d(p.float().to(dev), t.float().to(dev)))
        print("bce2d binary %s: HIP %.9g closed form %.9g" % (_ids(shape), loss, closed))
        assert abs(loss - closed) <= 2.0 ** -23 * closed and lossf == loss
        ref32 = float(t_bce2d(p.float(), t))
        assert abs(ref32 - closed) <= 1e-5 * closed  # (torch's own fp32 result: the same clamp)


# ------------------------------------------------------------------------------------------------------------------ fused pair
def _composition(ops, sx, labels):
    p = ops.boundary_head(*sx)
    return ops.bce2d(p, ops.label_boundary(labels))


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_fused_boundary_loss_fwd_bwd_and_composition(shape):
    dev = _dev()
    from mcdseg import ops
    c = _head_case(shape)
    lab = c["labels"].to(dev)
    gout = torch.tensor(0.6, device=dev)
    sx = [t.to(dev).requires_grad_() for t in c["s"]]
    loss = ops.boundary_head_bce(*sx, lab)
    ds = torch.autograd.grad(loss, sx, gout)
    t = _Truth("boundary_head_bce " + _ids(shape))
    t.check(loss, c["loss64"], c["loss32"], "loss")
    for k in range(3):
        t.check(ds[k], 0.6 * c["dloss64"][k], 0.6 * c["dloss32"][k], "ds%d" % (k + 1))
    t.report()
    # against the composition of the three unfused entry points: the same fp32 expressions, only the order of the partial sums may
    # differ (a thread sums at most 16 values in fp32: 16 * 2^-24 < 2e-6 relative)
    sy = [t.to(dev).requires_grad_() for t in c["s"]]
    loss_c = _composition(ops, sy, lab)
    ds_c = torch.autograd.grad(loss_c, sy, gout)
    assert abs(float(loss) - float(loss_c)) <= 2e-6 * abs(float(loss_c)), (float(loss), float(loss_c))
    for k in range(3):
        sc = float(ds_c[k].abs().max())
        err = float((ds[k] - ds_c[k]).abs().max())
        print("fused vs composition %s ds%d: max |diff| %.3e of scale %.3e%s" % (_ids(shape), k + 1, err, sc, " (bitwise)" if err == 0 else ""))
        assert err <= 2e-6 * sc


@pytest.mark.parametrize("kind,beta", [("constant", 1.0), ("checkerboard", 0.0)])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_degenerate_label_maps_give_exact_zeros(shape, kind, beta):
    """a constant label map has no boundary (beta = 1, weight of every pixel 0), a checkerboard is all boundary (beta = 0, likewise)"""
    dev = _dev()
    from mcdseg import ops
    lab = _labels(shape, kind).to(dev)
    for amp in (2.0, 40.0):
        for fused in (True, False):
            sx = [t.to(dev).requires_grad_() for t in _maps(shape, 3, amp)]
            loss = ops.boundary_head_bce(*sx, lab) if fused else _composition(ops, sx, lab)
            ds = torch.autograd.grad(loss, sx)
            assert float(loss) == 0.0, (kind, amp, fused, float(loss))
            for d in ds:
                assert bool(torch.isfinite(d).all()) and float(d.abs().max()) == 0.0
    tt = ops.label_boundary(lab)
    _, b = ops.bce2d(torch.full((shape[0], 1) + shape[1:], 0.25, device=dev), tt, return_beta=True)
    assert float(b) == beta


@pytest.mark.parametrize("sign", ["plus", "minus", "mixed"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_saturated_logits_follow_torch_clamp_and_eps(shape, sign):
    """logits of +-40 on all three scales: sigmoid is 1 (or 4e-18) in fp32 and in fp64 alike, log1p(-p) is clamped at -100 and the
    backward denominator at 1e-12; finite everywhere and within the rule of torch's own results"""
    dev = _dev()
    from mcdseg import ops
    n, h, w = shape
    s = [torch.full((n, 1, h // k, w // k), 40.0 if sign == "plus" else -40.0) for k in (2, 4, 8)]
    if sign == "mixed":  # per image: planes never mix, so every pixel of an image is saturated the same way
        flip = torch.tensor([1.0 if k % 2 == 0 else -1.0 for k in range(n)]).reshape(n, 1, 1, 1)
        s = [t * flip for t in s]
    lab = _labels(shape, "random", 9)
    res = {}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        sx = [t.to(dt).requires_grad_() for t in s]
        loss = t_bce2d(t_head(*sx), t_boundary(lab))
        res[tag] = (loss.detach(), torch.autograd.grad(loss, sx))
    for fused in (True, False):
        sx = [t.to(dev).requires_grad_() for t in s]
        loss = ops.boundary_head_bce(*sx, lab.to(dev)) if fused else _composition(ops, sx, lab.to(dev))
        ds = torch.autograd.grad(loss, sx)
        t = _Truth("saturated %s %s %s" % (sign, "fused" if fused else "composed", _ids(shape)))
        t.check(loss, res["64"][0], res["32"][0], "loss")
        gscale = max(float(d.abs().max()) for d in res["64"][1])
        for k in range(3):
            t.check(ds[k], res["64"][1][k], res["32"][1][k], "ds%d" % (k + 1), scale=gscale)
        t.report()
    if sign == "plus":
        assert float(ops.boundary_head(*[t.to(dev) for t in s]).min()) == 1.0


def test_two_launches_are_bitwise_equal():
    dev = _dev()
    from mcdseg import ops
    shape = SHAPES[-1]
    c = _head_case(shape)
    lab = c["labels"].to(dev)
    runs = []
    for _ in range(2):
        sx = [t.to(dev).requires_grad_() for t in c["s"]]
        loss = ops.boundary_head_bce(*sx, lab)
        ds = torch.autograd.grad(loss, sx)
        sy = [t.to(dev).requires_grad_() for t in c["s"]]
        p = ops.boundary_head(*sy)
        loss2 = ops.bce2d(p, ops.label_boundary(lab))
        ds2 = torch.autograd.grad(loss2, sy)
        runs.append([loss, loss2, p.detach()] + list(ds) + list(ds2))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------ decoder and step
# The same model in plain torch, restated here (the DRN stages and the three-layer decoders are the CPU oracle's: the segbd classes
# are the reference's models/dilated_fcn.py:569-629, 743-787, 1027-1217 and adapt_segbd_multitask_trainer.py:193-257).
NC = 41
NET = "drn_d_22"


def _torch_models():
    import torch.nn as nn
    from oracle import ref_loss, ref_models, ref_multitask

    class Enc(nn.Module):
        def __init__(self):
            super().__init__()
            trunk, _ = ref_models.drn_trunk(NET, 3)
            for k in range(9):
                setattr(self, "main_layer%d" % k, trunk[k])

        def forward(self, x):
            out = {}
            for k in range(9):
                x = getattr(self, "main_layer%d" % k)(x)
                out["h%d" % k] = x
            return out

    def boundary_loss(pred, gt, pred_type="semseg", gt_type="semseg"):
        gt_b = t_boundary(gt) if gt_type == "semseg" else gt.detach()
        pred_b = t_boundary(pred) if pred_type == "semseg" else pred
        return t_bce2d(pred_b.to(gt_b.dtype if gt_b.dtype.is_floating_point else torch.float64), gt_b)

    class Dec(nn.Module):
        def __init__(self):
            super().__init__()
            self.s_semsegcls, self.s_boundary = nn.Parameter(torch.ones(1)), nn.Parameter(torch.ones(1))
            self.semsegcls_dec1, self.semsegcls_dec2 = ref_multitask.ThreeLayerDecoder(NC), ref_multitask.ThreeLayerDecoder(NC)
            self.conv1, self.conv2, self.conv3 = nn.Conv2d(32, 1, 1), nn.Conv2d(64, 1, 1), nn.Conv2d(512, 1, 1)

        def semseg_forward(self, x):
            up = lambda t: F.interpolate(t, scale_factor=8, mode="bilinear", align_corners=False)  # noqa: E731
            return up(self.semsegcls_dec1(x["h8"])), up(self.semsegcls_dec2(x["h8"]))

        def boundary_forward(self, x):
            return t_head(self.conv1(x["h2"]), self.conv2(x["h3"]), self.conv3(x["h8"]))

        def get_cls_descrepancy(self, x):
            return self.discrepancy_criterion(*self.semseg_forward(x))

        def get_loss(self, x, gt):
            a, b = self.semseg_forward(x)
            l1 = self.semseg_criterion(a, gt) + boundary_loss(a.max(1)[1], gt)
            l2 = self.semseg_criterion(b, gt) + boundary_loss(b.max(1)[1], gt)
            s = self.s_semsegcls
            semseg = ((torch.exp(-s) * l1 + s) + (torch.exp(-s) * l2 + s)) / 2
            bd = torch.exp(-self.s_boundary) * boundary_loss(self.boundary_forward(x), gt, pred_type="boundary") + self.s_boundary
            return semseg, bd, (a.detach(), b.detach())

    return Enc(), Dec(), ref_loss


def _torch_step(enc, dec, oe, od, src, gt, tgt, num_k):
    oe.zero_grad(), od.zero_grad()
    src_fet = enc(src)
    enc(tgt)
    semseg, bd, logits = dec.get_loss(src_fet, gt)
    loss = semseg + bd
    loss.backward()
    first = (float(loss.detach()), float(semseg.detach()), float(bd.detach()), logits)
    oe.step(), od.step()
    oe.zero_grad(), od.zero_grad()
    semseg, _, _ = dec.get_loss(enc(src), gt)
    loss = semseg - dec.get_cls_descrepancy(enc(tgt))
    loss.backward()
    od.step()
    for _ in range(num_k):
        oe.zero_grad()
        loss = dec.get_cls_descrepancy(enc(tgt))
        loss.backward()
        oe.step()
    return first, float(loss.detach()) / num_k


def _segbd_batch():
    g = torch.Generator().manual_seed(77)
    n, h, w = 2, 32, 48
    src, tgt = torch.randn(n, 3, h, w, generator=g), torch.randn(n, 3, h, w, generator=g)
    coarse = torch.randint(0, NC, (n, 1, h // 8, w // 8), generator=g).float()
    gt = F.interpolate(coarse, size=(h, w), mode="nearest")[:, 0].long().contiguous()
    return src, gt, tgt


NAMED = ["enc/main_layer0.0.weight"] + ["dec/" + k for k in ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight",
                                                               "conv3.bias", "s_boundary", "s_semsegcls")]
STEP_FIXTURE = "segbd_step.npz"


def _class_weights():
    cw = torch.ones(NC)
    cw[NC - 1] = 0
    return cw


def torch_step_reference():
    """the fp64 CPU side of test_segbd_step_vs_torch_fp64 (40 s of fp64 convolutions on the host, so its results are kept as a fixture:
    ``python tests/test_segbd_gpu.py`` writes tests/golden/segbd_step.npz from the torch modules restated above)"""
    from recipe import fill_state_
    src, gt, tgt = _segbd_batch()
    tenc, tdec, ref_loss = _torch_models()
    fill_state_(tenc, 91), fill_state_(tdec, 92)
    tdec.semseg_criterion, tdec.discrepancy_criterion = ref_loss.CrossEntropyLoss2d(_class_weights().double()), ref_loss.Diff2d()
    tenc.double().train(), tdec.double().train()
    state = lambda: {tag + "/" + k: v.detach().clone() for tag, m in (("enc", tenc), ("dec", tdec)) for k, v in m.state_dict().items()}  # noqa: E731
    before = state()
    toe = torch.optim.SGD(tenc.parameters(), lr=1e-3, momentum=0.9, weight_decay=2e-5)
    tod = torch.optim.SGD(tdec.parameters(), lr=1e-3, momentum=0.9, weight_decay=2e-5)
    (rc, rseg, rbd, logits), rd = _torch_step(tenc, tdec, toe, tod, src.double(), gt, tgt.double(), 2)
    # the reference's own precondition: the arg-max behind the extra losses is well defined -- no top-2 gap that fp32 noise on the logits
    # (4e-5 of their scale: tests/test_model_gpu.py, _assert_fp32_noise) could flip
    gap = min(float((z.topk(2, dim=1)[0][:, 0] - z.topk(2, dim=1)[0][:, 1]).min()) / float(z.abs().max()) for z in logits)
    assert gap > 4e-5, gap
    after = state()
    out = {"losses": torch.tensor([rc, rseg, rbd, rd], dtype=torch.float64).numpy(), "gap": torch.tensor(gap, dtype=torch.float64).numpy(),
           "keys": list(after.keys())}
    out["norm"] = torch.tensor([float(v.double().norm()) for v in after.values()], dtype=torch.float64).numpy()
    out["sum"] = torch.tensor([float(v.double().sum()) for v in after.values()], dtype=torch.float64).numpy()
    for k in NAMED:
        out["before/" + k], out["after/" + k] = before[k].numpy(), after[k].numpy()
    return out


def test_segbd_step_vs_torch_fp64(golden):
    """one SegBDMultiTaskMCDSolver.step at 2 x 3 x 32 x 48 (drn_d_22) against the same step of the torch modules above holding the same
    weights, on the CPU in fp64 (``torch_step_reference``, kept in tests/golden/segbd_step.npz).  Tolerances: the form of
    tests/test_model_gpu.py::test_multitask_cfg4_vs_reference -- step A's losses to 1e-4, the discrepancy after the updates to 5e-3, the
    state's norms and sums to 1e-2 (encoder) / 5e-3 (decoder) -- and, for the tensors of NAMED, the UPDATE itself to 15 % (smoke()'s
    per-tensor bound on updates through train-mode BatchNorms)."""
    dev = _dev()
    from loss import CrossEntropyLoss2d, Diff2d
    from models.model_util import get_optimizer, get_segbd_multitask_models
    from recipe import fill_state_
    from solvers.solver import SegBDMultiTaskMCDSolver
    fx = golden.npz(STEP_FIXTURE)
    rc, rseg, rbd, rd = (float(v) for v in fx["losses"])
    src, gt, tgt = _segbd_batch()
    enc, dec = get_segbd_multitask_models(NET, 3, NC)
    fill_state_(enc, 91), fill_state_(dec, 92)
    dec.semseg_criterion, dec.discrepancy_criterion = CrossEntropyLoss2d(_class_weights()), Diff2d()
    enc.to(dev).train(), dec.to(dev).train()
    oe = get_optimizer(enc.parameters(), "sgd", 1e-3, 0.9, 2e-5)
    od = get_optimizer(dec.parameters(), "sgd", 1e-3, 0.9, 2e-5)
    c, d, parts = SegBDMultiTaskMCDSolver(enc, dec, oe, od, num_k=2).step(src.to(dev), gt.to(dev), tgt.to(dev))
    torch.cuda.synchronize()
    print("segbd step: c_loss %.7f (torch fp64 %.7f) semseg %.7f (%.7f) boundary %.7f (%.7f) d_loss %.3e (%.3e)"
          % (float(c), rc, float(parts[0]), rseg, float(parts[1]), rbd, float(d), rd))
    assert abs(float(c) - rc) <= 1e-4 * abs(rc)
    assert abs(float(parts[0]) - rseg) <= 1e-4 * abs(rseg) and abs(float(parts[1]) - rbd) <= 1e-4 * abs(rbd) and parts[2] == 0
    assert abs(float(d) - rd) <= 5e-3 * abs(rd)
    got = {tag + "/" + k: v for tag, m in (("enc", enc), ("dec", dec)) for k, v in m.state_dict().items()}
    assert list(got.keys()) == [str(k) for k in fx["keys"]]
    for i, (k, v) in enumerate(got.items()):
        rn, rs = float(fx["norm"][i]), float(fx["sum"][i])
        if not v.dtype.is_floating_point:
            assert int(v) == int(rs), k
            continue
        rtol = 1e-2 if k.startswith("enc/") else 5e-3
        a = v.detach().double().cpu()
        assert abs(float(a.norm()) - rn) <= rtol * max(rn, 1e-6), k
        assert abs(float(a.sum()) - rs) <= rtol * max(rn, 1e-6) * max(a.numel(), 1) ** 0.5, k
    for k in NAMED:
        b = torch.from_numpy(fx["before/" + k])
        u_ref = torch.from_numpy(fx["after/" + k]) - b
        u_hip = got[k].detach().double().cpu() - b
        rel = float((u_hip - u_ref).norm() / u_ref.norm())
        print("segbd step update %-26s rel L2 %.3e (|update| %.3e)" % (k, rel, float(u_ref.norm())))
        assert float(u_ref.norm()) > 0 and rel <= 0.15, (k, rel)


def test_segbd_encoder_refuses_compact_storage_on_the_gpu(monkeypatch):
    dev = _dev()
    from mcdseg import ops
    from models.model_util import get_segbd_multitask_models
    enc, _ = get_segbd_multitask_models(NET, 3, NC)
    enc.to(dev)
    monkeypatch.setattr(ops, "ACT_STORAGE", "compact")
    with pytest.raises(NotImplementedError, match="MCDSEG_ACT_STORAGE=compact"):
        enc(torch.zeros(1, 3, 32, 48, device=dev))


def test_decoder_boundary_forward_matches_the_reference_fixture(golden):
    """MCDSegBDMultiTaskDecoder.boundary_forward on the golden case: the REAL reference's fp64 output is the truth, its fp32 output the
    yardstick (tests/golden/make_segbd_golden.py)"""
    dev = _dev()
    from models.dilated_fcn import MCDSegBDMultiTaskDecoder
    fx = golden.npz("segbd_small.npz")
    dec = MCDSegBDMultiTaskDecoder(5, 3)
    with torch.no_grad():
        for name in ("conv1", "conv2", "conv3"):
            getattr(dec, name).weight.copy_(torch.from_numpy(fx[name + ".weight"]))
            getattr(dec, name).bias.copy_(torch.from_numpy(fx[name + ".bias"]))
    dec.to(dev).eval()
    with torch.no_grad():
        p = dec.boundary_forward({k: torch.from_numpy(fx[k]).to(dev) for k in ("h2", "h3", "h8")})
    t = _Truth("decoder boundary_forward")
    # (the 1x1 projections run on the split-fp16 matrix path, whose own bound is 2e-5 of the scale: tests/truth.py, summary)
    got, r64, r32 = p.double().cpu(), torch.from_numpy(fx["f64/boundary_forward"]), torch.from_numpy(fx["f32/boundary_forward"])
    e, e32 = float((got - r64).abs().max()), float((r32.double() - r64).abs().max())
    print("decoder boundary_forward: |HIP - ref64| %.3e, |ref32 - ref64| %.3e" % (e, e32))
    assert e <= max(TRUTH_OUTPUT * e32, 2e-5 * float(r64.abs().max()))
    t.report()


# ------------------------------------------------------------------------------------------------------------------ command lines
CLI = ["-b", "2", "--train_img_shape", "96", "64", "--synthetic", "--synthetic_len", "4", "--no_pretrained", "--no_tflog",
       "--max_iter", "0", "--net", NET]


@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_segbd_trainer_resume_and_tester(tmp_path, opt):
    _dev()
    import json
    import os

    from PIL import Image

    import adapt_segbd_multitask_tester
    import adapt_segbd_multitask_trainer
    import util
    out = str(tmp_path / "out")
    extra = ["--add_pred_seg_boundary_loss", "--boundary_loss_converging_epoch", "-1", "--opt", opt]
    assert adapt_segbd_multitask_trainer.main(["suncg", "nyu", "--base_outdir", out, "--epochs", "1"] + extra + CLI) == 0  # 2 iterations
    pth = os.path.join(out, "suncg-train2nyu-train_3ch_MCD_segbd_multitask", "pth")
    ck_fn = os.path.join(pth, "MCD-normal-%s-1.pth.tar" % NET)
    ck = util.load_checkpoint(ck_fn)
    assert sorted(ck.keys()) == ["args", "dec_state_dict", "enc_state_dict", "epoch", "optimizer_dec", "optimizer_enc"]
    assert "s_pred_seg_boundary" in ck["dec_state_dict"] and list(ck["dec_state_dict"]["conv2.weight"].shape) == [1, 64, 1, 1]
    assert "main_layer8.0.weight" in ck["enc_state_dict"] and ck["args"].add_pred_seg_boundary_loss
    assert all(bool(torch.isfinite(v).all()) for v in ck["dec_state_dict"].values() if v.dtype.is_floating_point)
    # resume: one more epoch from the checkpoint, under the checkpoint's arguments
    assert adapt_segbd_multitask_trainer.main(["suncg", "nyu", "--resume", ck_fn, "--epochs", "2"] + CLI) == 0
    ck2 = util.load_checkpoint(os.path.join(pth, "MCD-normal-%s-2.pth.tar" % NET))
    assert ck2["epoch"] == 2 and not torch.equal(ck2["dec_state_dict"]["conv1.weight"], ck["dec_state_dict"]["conv1.weight"])
    if opt != "sgd":
        return
    label_dir, boundary_dir, ent = adapt_segbd_multitask_tester.main(["nyu", ck_fn, "--outdir", str(tmp_path / "test"), "--synthetic",
                                                                      "--synthetic_len", "3", "-b", "2", "--test_img_shape", "80", "56"])
    base = os.path.dirname(label_dir)
    names = sorted(os.listdir(boundary_dir))
    assert len(names) == 3 and names == sorted(os.listdir(label_dir))
    im = Image.open(os.path.join(boundary_dir, names[0]))
    assert im.size == (80, 56) and im.mode == "L" and Image.open(os.path.join(label_dir, names[0])).size == (80, 56)
    assert len([f for f in os.listdir(base) if f.startswith("ave_ent_")]) == 1 and ent == ent
    with open(os.path.join(base, "eval_result.json")) as f:
        assert "mIoU" in json.load(f)


if __name__ == "__main__":  # python tests/test_segbd_gpu.py: (re)write the fp64 CPU fixture of the step test
    import os
    import sys

    import numpy as np
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    for path in (os.path.join(here, "golden"), root, os.path.join(root, "multichannel-semseg-with-uda_amd")):
        sys.path.insert(0, path)
    os.environ.setdefault("MCDSEG_PRETRAINED", "0")
    ref = torch_step_reference()
    np.savez_compressed(os.path.join(here, "golden", STEP_FIXTURE), **ref)
    print("wrote %s: losses %s, relative top-2 gap %.2e" % (STEP_FIXTURE, ref["losses"], float(ref["gap"])))
