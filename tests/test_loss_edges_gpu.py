"""GPU: the fused cross-entropy + L1-discrepancy kernels (csrc/loss.hip, csrc/loss_front.h) -- the plain form, the register-staged fused
x8 up-sampler form and the LDS-DMA form -- against the fp64 numpy oracle of tests/loss_ref.py, at the class counts on both sides of every
instantiation switch and of the counted wait's switch, at saturated, offset, uniform and tied logits, and at labels outside [0, C).

Bars (loss_ref.held): VAL_RTOL, GRAD_RTOL = 2e-6, 5e-6 of tests/test_prob_distance_gpu.py -- a value relative to the fp64 value, a
gradient relative to the fp64 gradient's largest entry; at adverse inputs (spread 30, offsets of +-100) max(bar, FACTOR * unit), FACTOR = 2
as in tests/test_dense_crf_gpu.py, unit = the distance of the SAME oracle run in fp32 from its fp64 run on that very case, computed here.
Gradients that hold an L1 term are compared on the pixels loss_ref.sure() keeps (sign(p1 - p2) is not determined where the heads agree to
rounding); tests/test_loss_ref_host.py asserts that this leaves out at most 2 % of the pixels of every case built by tests/loss_cases.py.
Every comparison prints kernel error, unit and bound.

Cases that need FACTOR * unit above the bar (MI355X, as printed; all of them in docs/MEASURED_HISTORY.md, "Loss kernels against fp64"): only
one saturated pixel alone -- 1 x C x 1 x 1 at spread 30 (C = 16 ... 48) and 1 x 2 x 1 x 1 at spreads 4 and 8 (to two classes what spread 30 is
to sixteen: tests/loss_cases.py, spreads).  Its gradients are 1e-3 ... 1e-30 and are formed as p - 1 or s - sum s p with p = 1 - e, which keeps
2^-24 / e of relative precision in any fp32 evaluation, and nothing larger stands beside them; the kernel's error equals the fp32 oracle's to
the printed digits: g1 5.92e-5 of max|g| 1.04e-3 (unit 5.92e-5, bound 1.18e-4) at C = 2, spread 8, CE single head; g2 4.63e-5 of 7.36e-5
(unit 4.63e-5) at C = 2, spread 4, Diff only; CE2 1.93e-4 of 6.49e-3 (unit 1.93e-4) at C = 31, spread 30.  27 figures of 3 800; the kernel
is at most 0.51 of any such bound.  On every shape with more than one pixel, spread 30 and the +-100 offsets stay under the bars themselves
(worst gradient 3.0e-6 against the truth without the offset, fused C = 41).  Worst figures whose bound is the bar: plain 2.4e-7 / 3.6e-6
(value / gradient; the gradient on a one-pixel shape, 2.1e-6 beyond those), register-staged and LDS-DMA 1.1e-7 / 1.2e-6.
C = 2 at spread 8: the margin rule would leave out 4.0 % of the pixels, over the cap, so there the gradients with an L1 term are not
compared (values and the CE-only gradient are); spread 4 (0.17 %) is added, where everything is."""
import numpy as np
import pytest
import torch

import loss_cases as LC
import loss_ref as R
from guards import guarded

pytestmark = pytest.mark.gpu


def _tag(family):
    return lambda s: print("[%s] %s" % (family, s))


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def run(case, device, want_grad=True, g=None, labels_t=None):
    """the kernel on ``case``: ((losses[4], g1, g2) as numpy, the same as tensors).  ``g``: a guards.guarded context -- inputs are guarded
    copies, outputs and workspaces come poisoned.  ``labels_t``: the label tensor to use instead of a fresh copy of ``case.labels``."""
    from mcdseg import ops

    def to(a):
        if a is None:
            return None
        t = torch.from_numpy(np.ascontiguousarray(a))
        return g.put(t) if g is not None else t.to(device)
    labels = labels_t if labels_t is not None else to(case.labels)
    wsum = None if case.wsum is None else torch.tensor([case.wsum], dtype=torch.float32, device=device)
    kw = dict(ignore_index=case.ignore_index, ce_coef=case.ce_coef, diff_coef=case.diff_coef, want_grad=want_grad, wsum=wsum)
    if case.fused:
        s1 = to(case.s1)
        s2 = s1 if case.s2 is case.s1 else to(case.s2)  # the shared-scores mode hands the kernel one tensor twice
        raw = ops.up8_mcd_losses(s1, to(case.w1), s2, to(case.w2), labels, to(case.cw), **kw)
    else:
        raw = ops.mcd_losses(to(case.z1), to(case.z2), labels, to(case.cw), **kw)
    torch.cuda.synchronize()
    assert raw[0].dtype == torch.float32 and tuple(raw[0].shape) == (4,)
    return tuple(_np(t) for t in raw), raw


def _same(a, b, what):
    """two results of the kernels, bit for bit"""
    for k, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), (what, k)
        if x is not None:
            assert torch.equal(x, y), "%s: output %d differs" % (what, k)


def expected_kernel(c, two, dma):
    """the instantiation csrc/loss.hip is meant to launch, as rocprofv3 names it"""
    two = "true" if two else "false"
    if dma:
        nc = 16 if c <= 16 else (24 if c <= 24 else (41 if c == 41 else 48))
        return "up8_softmax_ce_l1_dma_kernel<%d, %s, %s>" % (nc, two, "true" if c == nc else "false")
    return "up8_softmax_ce_l1_kernel<%d, %s>" % (16 if c <= 16 else (24 if c <= 24 else 48), two)


def _named(case, dma, labelled=None):
    from mcdseg import ops
    n, c, hi, wi = case.s1.shape
    name = ops.up8_loss_kernel_name(n, c, hi, wi, case.two, (case.labels is not None) if labelled is None else labelled)
    assert name == expected_kernel(c, case.two, dma), (case.what, name)


# ---------------------------------------------------------------------------------------------------- a. the plain kernel
@pytest.mark.parametrize("c", LC.PLAIN_C)
def test_plain_kernel_against_fp64(c, device):
    """NCMAX 16 / 24 / 48 on both sides of each switch, C = 1 and 2; 234 pixels (a block that straddles the image boundary and ends
    ragged), one pixel, 768 pixels (exactly three blocks); spread 2 and 30 (C <= 2: 2, 4, 8); CE single head, CE - Diff, CE + 0.7 Diff,
    Diff only; zero class weights on used classes; three ignored pixels"""
    for case in LC.plain_cases(c):
        got, _ = run(case, device)
        R.held(got, case, out=_tag("plain"))


# ---------------------------------------------------------------------------------------------------- b. adverse logits
def _adverse(cases, device, family, pixels=None):
    out = _tag(family)
    for name in ("offset", "offset-diff"):
        # +-100 on every logit of a pixel of head 1: the probabilities, hence every value and gradient, are those of the problem without it
        case, base = cases[name]
        got, _ = run(case, device)
        R.held(got, case, out=out)
        # (fused: the border pixels, whose taps do not sum to 1, do change -- and the values with them: gradients of the interior only)
        R.held(got, case.but(case.what + " vs the truth without the offset"), truth=base, pixels=pixels, values=pixels is None, out=out)
    for name in ("uniform-pixels", "constant-head"):
        got, _ = run(cases[name], device)
        R.held(got, cases[name], out=out)
    # pixels whose logits are the same bits in both heads, among pixels that differ: d = 0 in every precision
    case = cases["identical-pixels"]
    z1, z2 = case.logits()
    same = torch.from_numpy((z1 == z2).all(axis=1))
    assert 3 <= int(same.sum()) <= R.LEFT_OUT * same.numel()
    got, raw = run(case, device)
    R.held(got, case, out=out)
    _, ce_only = run(case.but(None, diff_coef=0.0), device)
    _, diff_only = run(case.but(None, ce_coef=0.0, labels=None, cw=None), device)
    for k in (1, 2):
        at = same[:, None].expand_as(raw[k]).to(raw[k].device)
        assert float(diff_only[k][at].abs().max()) == 0.0, "an L1 gradient where the heads are identical"
        assert torch.equal(raw[k][at], ce_only[k][at]), "the L1 term moved the CE gradient of a pixel whose heads are identical"
        assert float(diff_only[k].abs().max()) > 0.0
    # identical heads: no discrepancy and no gradient of it, exactly
    case = cases["identical-heads"]
    got, raw = run(case, device)
    R.held(got, case, grads=False, out=out)
    _, ce_only = run(case.but(None, diff_coef=0.0), device)
    _, diff_only = run(case.but(None, ce_coef=0.0, labels=None, cw=None), device)
    assert float(raw[0][2]) == 0.0 and float(diff_only[0][2]) == 0.0
    assert float(diff_only[1].abs().max()) == 0.0 and float(diff_only[2].abs().max()) == 0.0
    assert torch.equal(raw[1], ce_only[1]) and torch.equal(raw[2], ce_only[2])
    ce_case = case.but(case.what + " CE only", diff_coef=0.0)
    R.held(_np_all(ce_only), ce_case, out=out)


def _np_all(raw):
    return tuple(_np(t) for t in raw)


@pytest.mark.parametrize("c", LC.ADVERSE_PLAIN_C)
def test_plain_kernel_at_adverse_logits(c, device):
    _adverse(LC.adverse_plain(c), device, "plain")


@pytest.mark.parametrize("dma", [1, 0], ids=["dma", "reg"])
@pytest.mark.parametrize("c", LC.ADVERSE_FUSED_C)
def test_fused_kernels_at_adverse_logits(c, dma, device, libopt):
    """(the offset reaches the logits through the scores: taps whose four per pixel sum to exactly 1 turn a constant on an image's scores
    into that constant on every logit of a pixel with all four inputs present -- the comparison with the truth without the offset is made
    there; the border pixels are held to the truth of the offset problem itself)"""
    libopt(UP8_LOSS_DMA=dma)
    cases = LC.adverse_fused(c)
    _named(cases["constant-head"], dma)
    _adverse(cases, device, "dma" if dma else "register", pixels=LC.interior((2, 3, 20)))


# ---------------------------------------------------------------------------------------------------- c. labels
@pytest.mark.parametrize("front", ["plain", "register", "dma"])
def test_labels_outside_the_classes_are_ignored(front, device, libopt):
    """0, C - 1, C, C + 1, 255, -1, -7, +-2^40 and values that differ from a valid class in the high 32 bits only, with ignore_index -100,
    255 (>= C) and 3 (a valid class); the wsum override.  ``ops`` passes label VALUES through unchecked (shape and dtype only), so
    there is no rejection to assert: the kernels' rule is what is held."""
    if front != "plain":
        libopt(UP8_LOSS_DMA=int(front == "dma"))
    out = _tag(front)
    kind = "plain" if front == "plain" else "fused"
    c = LC.LABEL_C
    for ii in (-100, 255, 3):
        case = LC.label_case(kind, ii)
        if kind == "fused":
            _named(case, front == "dma")
        y = torch.from_numpy(case.labels)
        out_of = torch.from_numpy(~R.counted(case.labels, c, ii))
        assert int(((y >= c) | ((y < 0) & (y != ii))).sum()) >= 80 and int((y == 0).sum()) and int((y == c - 1).sum())
        got, raw = run(case, device)
        R.held(got, case, out=out)  # (W = losses[3] among the values)
        _, rep = run(LC.oob_replaced(case), device)
        _same(raw, rep, "labels outside [0, C) against the same labels set to ignore_index")
        _, ce_only = run(case.but(None, diff_coef=0.0), device)
        for k in (1, 2):
            at = out_of[:, None].expand_as(ce_only[k]).to(device)
            assert float(ce_only[k][at].abs().max()) == 0.0, "a CE gradient at a pixel that is not counted"
            assert float(ce_only[k].abs().max()) > 0.0
        if ii == 3:
            assert int((y == 3).sum()) > 0 and bool(out_of[y == 3].all())
    # the normaliser handed in: 2.5 W scales CE values and CE gradients by 1 / 2.5 and is what losses[3] reports
    case = LC.label_case(kind, -100).but(None, diff_coef=0.0)
    w = float(np.float32(2.5 * float(case.truth()[3])))
    over = case.but(case.what + " wsum", wsum=w)
    got, raw = run(over, device)
    R.held(got, over, out=out)
    ref, _ = run(case, device)
    assert float(got[0][3]) == w
    assert abs(got[0][0] * 2.5 - ref[0][0]) <= R.VAL_RTOL * ref[0][0] and abs(got[0][1] * 2.5 - ref[0][1]) <= R.VAL_RTOL * ref[0][1]
    for k in (1, 2):
        assert np.abs(got[k].astype(np.float64) * 2.5 - ref[k]).max() <= R.GRAD_RTOL * np.abs(ref[k]).max()


# ---------------------------------------------------------------------------------------------------- d. the fused kernels
@pytest.mark.parametrize("dma", [1, 0], ids=["dma", "reg"])
@pytest.mark.parametrize("c", LC.FUSED_C)
def test_fused_kernels_against_fp64(c, dma, device, libopt):
    """every instantiation (<16 | 24 | 41 | 48, EXACT> of the LDS-DMA form, 16 / 24 / 48 of the register-staged form) at one ragged 8-pixel
    segment, exactly one full segment, a second segment 8 pixels wide and 2 x 3 x 20 scores; the truth up-samples with loss_ref.up8"""
    libopt(UP8_LOSS_DMA=dma)
    out = _tag("dma" if dma else "register")
    for case in LC.fused_cases(c):
        _named(case, dma)
        got, raw = run(case, device)
        R.held(got, case, out=out)
        vals, raw_v = run(case, device, want_grad=False)
        assert raw_v[1] is None and raw_v[2] is None and torch.equal(raw_v[0], raw[0]), "the values depend on whether gradients are asked for"


# ---------------------------------------------------------------------------------------------------- e. buffer reuse, the counted wait
@pytest.mark.parametrize("c,heads", LC.WAIT_CASES)
def test_buffer_reuse_and_the_counted_wait_against_fp64(c, heads, device, libopt):
    """768 items on 256 workgroups: every workgroup goes through LDS buffer 0, 1 and 0 again, with an item's 2 C gradient stores of each
    wave in flight behind the next item's DMAs -- vmcnt(0) at 62 stores (C = 31) and at 48 (C = 48, one head), vmcnt(63) at 64 (C = 32).
    A wait that lets an item start before its inputs have landed, or a buffer refilled while it is read, shows against the truth."""
    case = LC.wait_case(c, heads)
    n, _, hi, wi = case.s1.shape
    assert n * (hi + 1) * -(-8 * wi // 64) == 3 * 256 and (8 * wi) % 64 == 8
    libopt(UP8_LOSS_DMA=1)
    _named(case, 1)
    got, raw = run(case, device)
    R.held(got, case, out=_tag("dma"))
    libopt(UP8_LOSS_DMA=0)
    _named(case, 0)
    _, reg = run(case, device)
    _same(raw, reg, "the LDS-DMA form against the register-staged form")
    libopt(UP8_LOSS_DMA=1)
    with guarded(device, interior=0xFF) as g:  # outputs arrive as NaN: an element no store reached stays one
        _, again = run(case, device, g=g)
        assert g.check() == []
        _same(again, raw, "the run on poisoned outputs")
    assert bool(torch.isfinite(raw[1]).all()) and (heads == 1 or bool(torch.isfinite(raw[2]).all()))


# ---------------------------------------------------------------------------------------------------- f. label base alignment
@pytest.mark.parametrize("c", [16, 41])
def test_labels_at_an_8_byte_aligned_base_run_the_register_kernel(c, device, libopt):
    """The LDS-DMA kernel fetches labels as 16-byte units from base + a multiple of 16; that such a fetch from an address that is only
    8-byte aligned is legal is not established, so the library sends a contiguous label view that starts at an odd element of a larger
    tensor to the register-staged kernel: the name says so, and the result is the truth's and, bit for bit, that of aligned labels."""
    case = LC.in_mode(LC.fused_problem(c, (2, 3, 20)), "ce+diff", LC.FUSED_MODES)
    n, _, hi, wi = case.s1.shape
    p = n * 64 * hi * wi
    flat = torch.full((p + 2,), -100, dtype=torch.int64, device=device)
    base = 0 if flat.data_ptr() % 16 == 0 else 1
    odd = flat[base + 1:base + 1 + p].view(n, 8 * hi, 8 * wi)
    odd.copy_(torch.from_numpy(case.labels))
    assert odd.is_contiguous() and odd.data_ptr() % 16 == 8
    libopt(UP8_LOSS_DMA=1)
    _named(case, 1)
    _named(case, 0, labelled=odd)
    got, raw = run(case, device, labels_t=odd)
    R.held(got, case, out=_tag("register"))
    _, aligned = run(case, device)
    _same(raw, aligned, "labels at an odd element against aligned labels")
