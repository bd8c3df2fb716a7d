"""GPU: the argmax / entropy inference tails -- ``predict_kernel<16|24|48>`` (csrc/loss.hip) and ``predict_up8_kernel<16|24|41|48,
learned|bilinear>`` (csrc/infer.hip) -- against the float64 statement of ``infer_tail_ref.predict_truth`` (torch-CPU, nothing of
``mcdseg``; checked by test_infer_tail_ref_host.py), at every instantiation boundary, at exact ties, with the maximum in an excluded
channel, with saturated logits, around one workgroup's 256 pixels, with more partial sums than the finalize stride, at Hi = 1 and
Wi = 1, and at dynamic-LDS sizes up to the 160 KB the entry accepts.

Labels: equal to the truth on EVERY pixel wherever the fp32 logits are exact (one head; two heads, see ``_plain_inputs``; the
up-samplers on ``exact`` inputs); on general up-sampled inputs wherever the truth's margin exceeds the up-sampler's own 1e-5 bar.

Entropy: ``|got - truth| <= 2e-6 |truth| + 6e-8``.  2e-6 is the bar loss values are held to (VAL_RTOL of
test_prob_distance_gpu.py); 6e-8 = 2^-24 is half an fp32 ulp of 1, the rounding of ``p + 1e-6`` at p near 1, which the reference's
own fp32 arithmetic has at most once per pixel.  Where the reference's literal fp32 expression on the CPU misses that bar on the
same inputs (it rounds (z1 + z2)/2 and a - max to fp32 at logits of order 1e2), the bar is 4 x that CPU-fp32 error -- computed
here from the inputs, never from the kernel.  Every measured error is printed (``pytest -s``); docs/MEASURED_HISTORY.md has the table."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from infer_tail_ref import bilinear8_truth, predict_truth, up8_truth

pytestmark = pytest.mark.gpu

ENT_RTOL, ENT_ATOL = 2e-6, 6e-8
MARGIN_RTOL = 1e-5  # the relative bar test_up8_fwd_bwd holds the up-sampler's forward to


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _ids(c):
    return "x".join(map(str, c))


def _entropy_fp32_cpu(o):
    """util.py:44-48 as written, fp32 on the CPU"""
    p = F.softmax(o, dim=1)
    return float(-torch.mean(p * torch.log(p + 1e-6)))


def _entropy_bar(truth, cpu32):
    """(bar, whether it is the widened one): the docstring's rule"""
    bar = ENT_RTOL * abs(truth) + ENT_ATOL
    e32 = abs(cpu32 - truth)
    return (4 * e32, True) if e32 > bar else (bar, False)


def _check_entropy(tag, got, truth, cpu32):
    bar, widened = _entropy_bar(truth, cpu32)
    err = abs(got - truth)
    print("ENT %s got %.9e truth %.9e err %.3e rel %.3e bar %.3e%s cpu_fp32_err %.3e" %
          (tag, got, truth, err, err / abs(truth) if truth else float("nan"), bar, " (4 x CPU fp32)" if widened else "", abs(cpu32 - truth)))
    # 4 x the CPU-fp32 error of the same inputs where that expression itself misses 2e-6 |truth| + 6e-8, else that bar
    assert err <= bar, (tag, got, truth, err, bar)


def _first_max(o):
    """first index of the maximum over dim 1, without argmax"""
    k = o.shape[1]
    idx = torch.arange(k).view(1, k, 1, 1).expand_as(o)
    return torch.where(o == o.max(1, keepdim=True)[0], idx, torch.full_like(idx, k)).min(1)[0].to(torch.uint8)


# ---------------------------------------------------------------------------------------------------------------------------------
# the plain kernel: N, C, H, W, n_used
PLAIN = [
    (1, 1, 1, 1, 1),        # single class, single pixel
    (2, 2, 3, 5, 1),        # n_used = 1
    (2, 16, 9, 13, 16),     # top of the <16> instantiation
    (1, 17, 16, 16, 16),    # bottom of <24>; P = 256
    (3, 24, 5, 17, 23),     # top of <24>; P = 255
    (1, 25, 257, 1, 25),    # bottom of <48>; P = 257, HW odd
    (2, 41, 7, 9, 40),      # the datasets' own class count
    (2, 41, 7, 9, 41),      # background class trained
    (1, 48, 19, 23, 47),    # largest C
    (1, 48, 4, 4, 1),       # largest C, n_used = 1
    (2, 41, 200, 170, 40),  # 266 partial sums: more than the finalize kernel's 256-thread stride
]
KINDS = ["randn", "saturated", "tied", "excluded-max", "constant"]
PLAIN_PARAMS = [pytest.param(case, kind, id="%s-%s" % (_ids(case), kind)) for case in PLAIN for kind in KINDS
                if not (kind == "excluded-max" and case[1] < 2)]


def _plain_inputs(case, kind, two):
    """(z1, z2 or None, n_used).  With two heads the kernel's fp32 (a + b)/2 is exact for ``tied`` and ``constant`` and rounded once
    for the others; rounding is monotone, so the fp32 first-index argmax can differ from the fp64 one only where it makes two
    different averages equal -- the test asserts from the inputs that this happens on no pixel."""
    n, c, h, w, used = case
    g = torch.Generator().manual_seed(1000 * c + 10 * h + used + (500 if two else 0) + KINDS.index(kind))
    shape = (n, c, h, w)

    def draw():
        if kind == "tied":
            return torch.randint(-2, 3, shape, generator=g).float()
        if kind == "constant":
            return torch.full(shape, -1.75)
        z = torch.randn(shape, generator=g) * (80 if kind == "saturated" else 2)
        if kind == "excluded-max":
            z[:, c - 1] += 50
        return z
    z1 = draw()
    z2 = draw() if two else None
    if kind == "constant" and two:
        z2 = z2 + 4.0  # the average, 0.25, is still one constant
    return z1, z2, (c - 1 if kind == "excluded-max" else used)


@pytest.mark.parametrize("two", [False, True], ids=["one-head", "two-heads"])
@pytest.mark.parametrize("case,kind", PLAIN_PARAMS)
def test_predict_labels_against_fp64_truth(case, kind, two):
    dev = _dev()
    from mcdseg import ops
    n, c, h, w, _ = case
    z1, z2, used = _plain_inputs(case, kind, two)
    lab_t, ent_t, margin = predict_truth(z1, z2, used)
    o32 = z1 if z2 is None else (z1 + z2) / 2  # the reference's own fp32 average
    # the claim of _plain_inputs, from the inputs alone: the fp32 first-index argmax is the fp64 one on every pixel
    assert torch.equal(_first_max(o32[:, :used]), lab_t)
    if kind == "tied" and c >= 16 and used > 1:
        assert float((margin == 0).double().mean()) >= 0.1
    if kind == "excluded-max":
        assert bool((o32.argmax(1) == c - 1).all())  # the maximum over ALL classes sits in the excluded channel, everywhere
    if kind == "constant":
        assert not lab_t.any() and abs(ent_t + np.log(1.0 / c + 1e-6) / c) <= 1e-14
    with torch.no_grad():
        lab, ent = ops.predict_labels(z1.to(dev), None if z2 is None else z2.to(dev), used)
    torch.cuda.synchronize()
    assert lab.dtype == torch.uint8 and tuple(lab.shape) == (n, h, w) and ent.dim() == 0
    lab = lab.cpu()
    wrong = int((lab != lab_t).sum())
    assert wrong == 0, "%d of %d labels differ from the fp64 truth (first at %s)" % (wrong, lab.numel(), (lab != lab_t).nonzero()[0].tolist())
    _check_entropy("plain %s %s %s" % (_ids(case), kind, "two" if two else "one"), float(ent), ent_t, _entropy_fp32_cpu(o32))


# ---------------------------------------------------------------------------------------------------------------------------------
# the fused kernels: N, C, Hi, Wi, n_used
FUSED = [
    (1, 1, 1, 1, 1),      # single class, single input pixel
    (2, 2, 1, 3, 2),      # Hi = 1: both bands read the one input row
    (1, 16, 2, 1, 16),    # Wi = 1; top of <16>
    (2, 17, 3, 5, 16),    # bottom of <24>
    (1, 24, 5, 7, 23),    # top of <24>
    (1, 25, 3, 9, 25),    # bottom of <48>
    (2, 41, 5, 7, 40),    # <41>
    (1, 42, 3, 5, 42),    # <48>, next to the 41 special
    (3, 19, 7, 9, 19),
    (1, 41, 2, 160, 40),  # 94.5 KB of LDS learned: config 5's width
    (1, 48, 2, 200, 47),  # 126 KB learned, 76.8 KB bilinear
]
WIDEST = (1, 48, 1, 400, 47)  # bilinear: 153.6 KB, the largest the entry accepts; learned: 202752 bytes, refused
FUSED_PARAMS = ([pytest.param(case, learned, id="%s-%s" % (_ids(case), "up8" if learned else "bilinear8")) for case in FUSED
                 for learned in (True, False)] + [pytest.param(WIDEST, False, id="%s-bilinear8" % _ids(WIDEST))])
# (case, learned, exact) -> added to the seed where the drawn inputs missed a condition asserted from the truth
SEED_BUMP = {((1, 24, 5, 7, 23), False, True): 1}  # 9.6% of pixels tied at the first seed, 10% asked


def _fused_inputs(case, learned, exact):
    """``exact``: integer scores in [-2, 2] and weights in {-1, -.5, 0, .5, 1} -- every interpolated logit (a multiple of 1/256 for
    the bilinear form, of 1/2 for the learned one, below 16 in size) is exact in fp32 whatever the order of operations
    (test_infer_tail_ref_host.py::test_up_samplers_in_fp64 shows fp32 and fp64 torch agreeing bit for bit on such inputs)."""
    n, c, hi, wi, _ = case
    g = torch.Generator().manual_seed(100 * hi + wi + 7 * c + SEED_BUMP.get((case, learned, exact), 0))
    if exact:
        s = torch.randint(-2, 3, (n, c, hi, wi), generator=g).float()
        w = torch.randint(-2, 3, (c, 1, 16, 16), generator=g).float() / 2
    else:
        s = torch.randn(n, c, hi, wi, generator=g) * 3
        w = torch.randn(c, 1, 16, 16, generator=g) * 0.1
    return s, (w if learned else None)


def _fused_truth(case, learned, exact):
    s, w = _fused_inputs(case, learned, exact)
    z = up8_truth(s, w) if learned else bilinear8_truth(s)
    return (s, w, z) + predict_truth(z, None, case[4])


def _fused(ops, dev, s, w, used):
    with torch.no_grad():
        lab, ent = ops.predict_labels_up8(s.to(dev), w.to(dev), used) if w is not None else ops.predict_labels_bilinear8(s.to(dev), used)
    torch.cuda.synchronize()
    return lab.cpu(), float(ent)


def _fp32_cpu_logits(s, w):
    return F.conv_transpose2d(s, w, stride=8, padding=4, groups=s.shape[1]) if w is not None else \
        F.interpolate(s, scale_factor=8, mode="bilinear", align_corners=False)


@pytest.mark.parametrize("case,learned", FUSED_PARAMS)
def test_fused_labels_on_exact_inputs_ties_included(case, learned):
    """does not go through the library's own predict_labels: the fp32 logits are the fp64 ones, so the labels are the truth's on
    every pixel, the first maximal index at every tie"""
    dev = _dev()
    from mcdseg import ops
    n, c, hi, wi, used = case
    s, w, z, lab_t, ent_t, margin = _fused_truth(case, learned, True)
    z32 = _fp32_cpu_logits(s, w)
    assert torch.equal(z32.double(), z)  # exactness of these inputs, from the inputs
    if c >= 16:
        assert float((margin == 0).double().mean()) >= 0.1, float((margin == 0).double().mean())
    lab, ent = _fused(ops, dev, s, w, used)
    assert lab.dtype == torch.uint8 and tuple(lab.shape) == (n, 8 * hi, 8 * wi)
    wrong = int((lab != lab_t).sum())
    assert wrong == 0, "%d of %d labels differ from the fp64 truth (first at %s)" % (wrong, lab.numel(), (lab != lab_t).nonzero()[0].tolist())
    _check_entropy("fused %s %s exact" % (_ids(case), "up8" if learned else "bilinear8"), ent, ent_t, _entropy_fp32_cpu(z32))


@pytest.mark.parametrize("case,learned", FUSED_PARAMS)
def test_fused_labels_and_entropy_on_general_inputs(case, learned):
    dev = _dev()
    from mcdseg import ops
    n, c, hi, wi, used = case
    s, w, z, lab_t, ent_t, margin = _fused_truth(case, learned, False)
    decided = margin > MARGIN_RTOL * float(z.abs().max())
    left_out = 1.0 - float(decided.double().mean())
    assert left_out <= 1e-3, left_out  # from the truth alone
    lab, ent = _fused(ops, dev, s, w, used)
    assert lab.dtype == torch.uint8 and tuple(lab.shape) == (n, 8 * hi, 8 * wi)
    assert int(lab.max()) < used
    bad = (lab != lab_t) & decided
    wrong = int(bad.sum())
    print("LAB fused %s %s general: %d of %d pixels below the margin, %d of those differ" %
          (_ids(case), "up8" if learned else "bilinear8", int((~decided).sum()), decided.numel(), int(((lab != lab_t) & ~decided).sum())))
    assert wrong == 0, "%d of %d decided labels differ from the fp64 truth (first at %s)" % (wrong, lab.numel(), bad.nonzero()[0].tolist())
    _check_entropy("fused %s %s general" % (_ids(case), "up8" if learned else "bilinear8"), ent, ent_t, _entropy_fp32_cpu(_fp32_cpu_logits(s, w)))


def test_fused_learned_form_refuses_what_the_lds_cannot_hold():
    """two rows of 48 x 400 scores and 48 16x16 kernels are 202752 bytes: above the 160 KB of a CU, so the entry refuses before
    any launch and says what it would need"""
    dev = _dev()
    from mcdseg import ops
    n, c, hi, wi, used = WIDEST
    s = torch.zeros(n, c, hi, wi, device=dev)
    w = torch.zeros(c, 1, 16, 16, device=dev)
    need = (2 * c * wi + c * 256) * 4
    assert need == 202752 and need > 160 * 1024 >= 2 * c * wi * 4
    with pytest.raises(RuntimeError, match=r"%d bytes of LDS" % need):
        ops.predict_labels_up8(s, w, used)
    torch.cuda.synchronize()
    lab, _ = ops.predict_labels_bilinear8(s, used)  # the bilinear form of the same scores fits, and the library still works
    assert not lab.any()


# ---------------------------------------------------------------------------------------------------------------------------------
def test_tail_to_metrics_end_to_end():
    """scores -> predict_labels_bilinear8 -> ConfusionMeter.update (uint8 labels, a label map carrying 255s) -> summary, against the
    numpy bincount formulas of eval.py:21-47 and :123-144 applied to the TRUTH's labels"""
    dev = _dev()
    from mcdseg import ops
    import eval as mc_eval
    case = (2, 41, 6, 8, 40)
    n, c, hi, wi, used = case
    s, _, z, lab_t, _, _ = _fused_truth(case, False, True)
    g = torch.Generator().manual_seed(5)
    gt = torch.randint(0, 40, (n, 8 * hi, 8 * wi), generator=g)
    agree = torch.rand(gt.shape, generator=g) < 0.6
    gt = torch.where(agree, lab_t.long(), gt)  # a plausible accuracy, so that no metric is degenerate
    gt[torch.rand(gt.shape, generator=g) < 0.1] = 255
    gt[:, :3, :5] = 255
    gt[gt == 7] = 255  # a class absent from the ground truth: the summary leaves it out (eval.py:143-144)
    meter = mc_eval.ConfusionMeter(c, background_id=255, device=dev)
    with torch.no_grad():
        lab, _ = ops.predict_labels_bilinear8(s.to(dev), used)
    assert lab.dtype == torch.uint8
    for i in range(n):
        meter.update(lab[i], gt[i].to(torch.uint8))
    got = meter.summary()
    a, b = gt.numpy().reshape(-1), lab_t.numpy().astype(np.int64).reshape(-1)
    k = (a >= 0) & (a < c)
    assert 0.05 < 1 - k.mean() < 0.3
    hist = np.bincount(c * a[k] + b[k], minlength=c * c).reshape(c, c).astype(np.float64)
    assert np.array_equal(meter.hist.cpu().numpy(), hist.astype(np.int64))
    ids = np.where(hist.sum(1) != 0)[0]
    assert 7 not in ids and len(ids) == 39
    sub = hist[ids][:, ids]
    iu = np.diag(sub) / (sub.sum(1) + sub.sum(0) - np.diag(sub))
    assert got["used_class_ids"] == ids.tolist()
    assert np.array_equal(np.array(got["IoU"]), iu * 100)
    assert got["mIoU"] == 100 * float(iu.mean()) and 20 < got["mIoU"] < 90
    assert got["pixAcc"] == 100 * (np.diag(sub).sum() / sub.sum(1).sum())
    assert got["mAcc"] == 100 * np.nanmean(np.diag(sub) / sub.sum(1))
    assert got["fwIoU"] == 100 * (np.nansum(sub.sum(1) * np.diag(sub) / (sub.sum(0) + sub.sum(1) - np.diag(sub))) / sub.sum(1).sum())
    # the two distributions come from the whole matrix (eval.py:141-159): predictions of the absent class 7 still count in a row's total
    assert got["pred_distribution"] == hist.sum(0)[ids].tolist() and got["gt_distribution"] == hist.sum(1)[ids].tolist()
    assert hist[:, 7].sum() > 0
