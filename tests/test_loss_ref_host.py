"""CPU: the fp64 oracle of the loss kernels (tests/loss_ref.py) against torch's fp64 autograd and the golden vectors, its edge behaviour,
the margin rule's left-out share on every input of tests/test_loss_edges_gpu.py, and the comparison helper on deliberately wrong
"kernel results", each of which it must reject."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_cases as LC
import loss_ref as R


def _torch_truth(z1, z2, y, cw, ignore_index, ce_coef, diff_coef):
    a = torch.from_numpy(z1).double().requires_grad_()
    b = torch.from_numpy(z2).double().requires_grad_() if z2 is not None else None
    w = torch.from_numpy(cw).double() if cw is not None else None
    t = torch.from_numpy(y)
    ce1 = F.cross_entropy(a, t, weight=w, ignore_index=ignore_index)
    total = ce_coef * ce1
    ce2 = diff = torch.zeros((), dtype=torch.float64)
    if b is not None:
        ce2 = F.cross_entropy(b, t, weight=w, ignore_index=ignore_index)
        diff = (F.softmax(a, dim=1) - F.softmax(b, dim=1)).abs().mean()
        total = total + ce_coef * ce2 + diff_coef * diff
    total.backward()
    return float(ce1.detach()), float(ce2.detach()), float(diff.detach()), a.grad.numpy(), (b.grad.numpy() if b is not None else None)


@pytest.mark.parametrize("c,shape,ignore_index", [(7, (2, 5, 6), -100), (41, (1, 4, 9), -100), (19, (2, 3, 4), 255), (5, (2, 6, 6), 3), (1, (1, 2, 2), -100)])
def test_oracle_against_torch_autograd(c, shape, ignore_index):
    rs = np.random.RandomState(c)
    n, h, w = shape
    z1, z2 = (3 * rs.standard_normal((2, n, c, h, w))).astype(np.float32)
    y = rs.randint(0, c, size=(n, h, w)).astype(np.int64)
    y[0, 0, :2] = ignore_index
    cw = rs.uniform(0.5, 1.5, c).astype(np.float32)
    cw[c // 2] = 0.0 if c > 1 else cw[0]
    for two, (ce, df) in [(True, (1.0, -1.0)), (True, (0.3, 0.7)), (False, (1.0, 0.0))]:
        got = R.losses(z1, z2 if two else None, y, cw, ignore_index, ce, df)
        t = _torch_truth(z1, z2 if two else None, y, cw, ignore_index, ce, df)
        for k in range(3):
            assert abs(float(got[k]) - t[k]) <= 1e-13 * max(abs(t[k]), 1.0), (k, got[k], t[k])
        assert float(got[3]) == pytest.approx(float(cw.astype(np.float64)[y[R.counted(y, c, ignore_index)]].sum()), rel=1e-14)
        assert np.abs(got[4] - t[3]).max() <= 1e-13 * max(np.abs(t[3]).max(), 1e-300)
        if two:
            assert np.abs(got[5] - t[4]).max() <= 1e-13 * max(np.abs(t[4]).max(), 1e-300)
        else:
            assert got[5] is None
    f32 = R.losses(z1, z2, y, cw, ignore_index, 1.0, -1.0, dtype=np.float32)
    assert all(np.asarray(v).dtype == np.float32 for v in f32), [np.asarray(v).dtype for v in f32]


@pytest.mark.parametrize("shape", [(2, 5, 1, 1), (1, 3, 2, 9), (2, 4, 3, 5)])
def test_up8_oracle_against_conv_transpose2d(shape):
    n, c, hi, wi = shape
    rs = np.random.RandomState(hi)
    s = rs.standard_normal(shape).astype(np.float32)
    w = rs.standard_normal((c, 1, 16, 16)).astype(np.float32)
    ref = F.conv_transpose2d(torch.from_numpy(s).double(), torch.from_numpy(w).double(), stride=8, padding=4, groups=c).numpy()
    got = R.up8(s, w)
    assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-14 * np.abs(ref).max()
    got32 = R.up8(s, w, np.float32)
    assert got32.dtype == np.float32 and np.abs(got32 - ref).max() <= 1e-6 * np.abs(ref).max()


def test_oracle_against_the_golden_vectors(golden):
    from oracle import ref_loss
    fx = golden.npz("loss_small.npz")
    ce1, ce2, diff, W, g1, g2 = R.losses(fx["z1"], fx["z2"], fx["y"], fx["w"], -100, 1.0, -1.0)
    assert abs(ce1 - float(fx["ce"])) <= 1e-6 * float(fx["ce"])  # (the vectors are the reference's own fp32 results)
    assert abs(diff - float(fx["diff"])) <= 1e-6 * float(fx["diff"])
    l2, gce2 = ref_loss.ce_and_grad(fx["z2"], fx["y"], fx["w"])
    d, gd1, gd2 = ref_loss.diff_and_grad(fx["z1"], fx["z2"])
    assert abs(ce2 - l2) <= 1e-14 * l2 and abs(diff - d) <= 1e-14 * d
    assert np.abs(g1 - (fx["g_ce"].astype(np.float64) - fx["g_d1"])).max() <= 1e-6 * np.abs(g1).max()
    assert np.abs(g2 - (gce2 - gd2)).max() <= 1e-14 * np.abs(g2).max()
    assert abs(W - float(fx["w"].astype(np.float64)[fx["y"]].sum())) <= 1e-12 * W


def test_oracle_edge_behaviour():
    for ii in (-100, 255, 3):
        case = LC.label_case("plain", ii)
        rep = LC.oob_replaced(case)
        y = case.labels
        assert {0, 18, 19, 20, 255, -1, -7, 2 ** 40, -2 ** 40} <= set(y.reshape(-1).tolist())
        a, b = case.truth(), rep.truth()
        assert all(np.array_equal(u, v) for u, v in zip(a, b)), "labels outside [0, C) are not the same as ignored ones"
        gce = case.but("ce only", diff_coef=0.0).truth()[4]
        out = ~R.counted(y, LC.LABEL_C, ii)
        assert out.sum() >= 80 and np.all(np.moveaxis(gce, 1, -1)[out] == 0.0)
        if ii == 3:
            assert (y == 3).sum() > 0 and np.all(np.moveaxis(gce, 1, -1)[y == 3] == 0.0)
    case = LC.label_case("plain", -100)
    ce1, ce2, diff, W, g1, g2 = case.truth()
    ce_only = case.but("ce", diff_coef=0.0)
    o1, o2, od, oW, og1, og2 = ce_only.but("wsum", wsum=2.5 * W).truth()
    assert oW == 2.5 * W and od == diff
    assert abs(o1 - ce1 / 2.5) <= 1e-15 * ce1 and abs(o2 - ce2 / 2.5) <= 1e-15 * ce2
    assert np.abs(og1 - ce_only.truth()[4] / 2.5).max() <= 1e-15 * np.abs(og1).max()
    # W = 0 (every used class has weight 0): NaN values, NaN gradients at the counted pixels, zeros at the others
    z = np.random.RandomState(0).standard_normal((1, 3, 2, 2)).astype(np.float32)
    y = np.array([[[0, 1], [-100, 7]]], np.int64)
    with np.errstate(all="ignore"):
        ce1, ce2, diff, W, g1, g2 = R.losses(z, None, y, np.array([0, 0, 1], np.float32), -100, 1.0, 0.0)
    assert W == 0 and np.isnan(ce1) and np.isnan(ce2) and np.isnan(g1[0, :, 0, :]).all() and np.all(g1[0, :, 1, :] == 0.0)


def test_the_margin_rule_leaves_out_at_most_two_percent_of_every_gpu_input():
    worst, cases = 0.0, 0
    for case in LC.every_margin_case():
        share = case.left_out()
        assert share <= R.LEFT_OUT, "%s: the margin rule leaves out %.4f of the pixels" % (case.what, share)
        worst, cases = max(worst, share), cases + 1
    print("%d cases, worst left-out share %.4f" % (cases, worst))
    assert cases > 300
    # the reason C <= 2 stops at spread 8: at spread 30 two saturated heads that agree on the class leave the sign to rounding too often
    assert LC.plain_problem(2, (2, 24, 40), 30.0).but("", diff_coef=1.0).left_out() > R.LEFT_OUT
    # ... and two classes at spread 8 still do (4.0 %), which is why the L1 gradients of that one family are not compared, and spread 4 is
    assert LC.plain_problem(2, (2, 60, 100), 8.0).but("", diff_coef=1.0).left_out() > R.LEFT_OUT
    assert LC.plain_problem(2, (2, 60, 100), 4.0).but("", diff_coef=1.0).left_out() < 0.1 * R.LEFT_OUT
    skipped = [case.what for c in LC.PLAIN_C for case in LC.plain_cases(c) if not case.grads]
    assert len(skipped) == 9 and all(w.startswith("plain C=2 ") and "spread 8 " in w for w in skipped), skipped
    # an identical-pixels case leaves out exactly the identical pixels (d = 0 in every class) and nothing else of note
    ident = LC.adverse_plain(19)["identical-pixels"]
    z1, z2 = ident.logits()
    same = (z1 == z2).all(axis=1)
    assert same.sum() == 3 and not ident.sure()[same].any()


def _as_kernel(t):
    """the truth as a kernel would hand it over: fp32"""
    ls = np.array([t[0], t[1], t[2], t[3]], np.float32)
    return ls, t[4].astype(np.float32), (t[5].astype(np.float32) if t[5] is not None else None)


def _rejected(got, case, word):
    with pytest.raises(AssertionError, match=word):
        R.held(got, case, out=lambda s: None)


def test_the_comparison_rejects_wrong_kernel_results():
    c = 19
    case = LC.label_case("plain", 255)
    t = case.truth()
    R.held(_as_kernel(t), case, out=lambda s: None)  # the truth itself, rounded to fp32, passes
    z1, z2 = case.logits()
    p1, p2 = R.softmax(z1)[0], R.softmax(z2)[0]

    # 1. one class's sign term flipped at a sure pixel
    n, h, w = [int(v[0]) for v in np.nonzero(case.sure())]
    k = int(np.argmax(p1[n, :, h, w] * (1 - p1[n, :, h, w])))
    s = np.sign(p1[n, :, h, w] - p2[n, :, h, w])
    s[k] = -s[k]
    kd = case.diff_coef / p1.size
    plain_s = np.sign(p1[n, :, h, w] - p2[n, :, h, w])
    ls, g1, g2 = _as_kernel(t)
    g1 = g1.astype(np.float64)
    g1[n, :, h, w] += kd * p1[n, :, h, w] * ((s - (s * p1[n, :, h, w]).sum()) - (plain_s - (plain_s * p1[n, :, h, w]).sum()))
    _rejected((ls, g1.astype(np.float32), g2), case, "g1: error")

    # 2. a cross-entropy that clamps y into [0, C) instead of ignoring it
    y = case.labels
    clamped = np.where(y == case.ignore_index, y, np.clip(y, 0, c - 1))
    assert case.cw[c - 1] > 0 and case.cw[0] == 0
    _rejected(_as_kernel(case.but("clamped", labels=clamped).truth()), case, "CE1: error")
    wrong = case.but("clamped", labels=clamped).truth()
    _rejected((_as_kernel(t)[0], wrong[4].astype(np.float32), wrong[5].astype(np.float32)), case, "g1: error")

    # 3. W that counts labels outside [0, C)
    ls = _as_kernel(t)[0].copy()
    ls[3] += float(((y >= c) & (y != case.ignore_index)).sum() + (y < 0).sum())
    _rejected((ls,) + _as_kernel(t)[1:], case, "W: error")

    # 4. the logits of class C - 1 dropped: the padding error of an instantiation edge
    for mode in ("ce-diff", "diff", "ce-single"):
        cm = LC.in_mode(case, mode)
        a, b = z1.copy(), z2.copy()
        a[:, c - 1], b[:, c - 1] = -1e4, -1e4
        with np.errstate(all="ignore"):
            wrong = cm.but("dropped", z1=a, z2=b if cm.two else None, labels=None if cm.labels is None else np.where(y == c - 1, -100, y)).truth()
        _rejected(_as_kernel(wrong), cm, "error")
        _rejected((_as_kernel(cm.truth())[0],) + _as_kernel(wrong)[1:], cm, "g1: error")

    # the same through a fused case: a truth that up-samples with one tap of one class wrong
    fc = LC.in_mode(LC.fused_problem(16, (2, 1, 8)), "ce+diff", LC.FUSED_MODES)
    R.held(_as_kernel(fc.truth()), fc, out=lambda s: None)
    w1 = fc.w1.copy()
    w1[15, 0, 11, 12] += 0.01  # (the tap of output row 7 on input row 0, of columns 8 k on input column k - 1)
    _rejected(_as_kernel(fc.but("tap", w1=w1).truth()), fc, "g1: error")


def test_labels_that_are_not_16_byte_aligned_name_the_register_kernel(libopt):
    from mcdseg import ops
    libopt(UP8_LOSS_DMA=1)
    flat = torch.zeros(2 * 8 * 8 + 2, dtype=torch.int64)
    base = 0 if flat.data_ptr() % 16 == 0 else 1
    aligned, odd = flat[base:base + 128].view(2, 8, 8), flat[base + 1:base + 129].view(2, 8, 8)
    assert odd.is_contiguous() and odd.data_ptr() % 16 == 8
    assert ops.up8_loss_kernel_name(2, 41, 1, 1, True, aligned) == "up8_softmax_ce_l1_dma_kernel<41, true, true>"
    assert ops.up8_loss_kernel_name(2, 41, 1, 1, True, True) == "up8_softmax_ce_l1_dma_kernel<41, true, true>"
    assert ops.up8_loss_kernel_name(2, 41, 1, 1, True, odd) == "up8_softmax_ce_l1_kernel<48, true>"
    assert ops.up8_loss_kernel_name(2, 41, 1, 1, True, odd, dist="jsd") == "up8_softmax_ce_dist_kernel<48, 3>"
    assert ops.up8_loss_kernel_name(2, 41, 1, 1, True, None) == "up8_softmax_ce_l1_dma_kernel<41, true, true>"
