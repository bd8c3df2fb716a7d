"""Host: the float64 statement of the argmax / entropy tail (``infer_tail_ref.predict_truth``) and of the two x8 up-samplers,
checked against the reference's literal fp32 torch expression (util.py:44-48, adapt_tester.py:104-124), numpy's argmax and the
closed forms for constant logits.  No GPU, nothing of ``mcdseg``."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from infer_tail_ref import bilinear8_truth, predict_truth, up8_truth


def _literal_fp32(z1, z2, n_used):
    """adapt_tester.py:104-124 as written, one image at a time for the labels"""
    outputs = z1.clone()
    if z2 is not None:
        outputs = outputs + z2
        outputs /= 2
    prob = F.softmax(outputs, dim=1)
    ent = float(-torch.mean(prob * torch.log(prob + 1e-6)))
    pred = torch.stack([outputs[i, :n_used].max(0)[1] for i in range(outputs.shape[0])])
    return np.uint8(pred.numpy()), ent


CASES = [(1, 1, 1, 1, 1), (2, 2, 3, 5, 1), (2, 16, 9, 13, 16), (3, 24, 5, 17, 23), (2, 41, 7, 9, 40), (2, 41, 7, 9, 41), (1, 48, 19, 23, 47)]


@pytest.mark.parametrize("two", [False, True], ids=["one-head", "two-heads"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_truth_matches_the_literal_fp32_expression_on_easy_inputs(case, two):
    n, c, h, w, used = case
    g = torch.Generator().manual_seed(c * 10 + used)
    z1 = torch.randn(n, c, h, w, generator=g) * 2
    z2 = torch.randn(n, c, h, w, generator=g) * 2 if two else None
    lab, ent, margin = predict_truth(z1, z2, used)
    ref_lab, ref_ent = _literal_fp32(z1, z2, used)
    assert lab.dtype == torch.uint8 and tuple(lab.shape) == (n, h, w) and isinstance(ent, float)
    assert margin.dtype == torch.float64 and tuple(margin.shape) == (n, h, w)
    # the fp32 expression may differ only where the fp64 gap is within its rounding of (a + b)/2: none such on these inputs
    clear = margin.numpy() > 1e-5
    assert clear.mean() > 0.999
    assert np.array_equal(lab.numpy()[clear], ref_lab[clear])
    assert abs(ent - ref_ent) <= 2e-6 * abs(ent) + 6e-8  # fp32 against fp64 at spread 2: 1e-7 relative is typical
    if used == 1:
        assert bool(torch.isinf(margin).all()) and not lab.any()
    else:
        assert bool((margin >= 0).all()) and bool(torch.isfinite(margin).all())


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_labels_are_numpy_argmax_ties_included(case):
    """np.argmax documents the first occurrence; integer logits in [-2, 2] tie at the maximum on most pixels"""
    n, c, h, w, used = case
    g = torch.Generator().manual_seed(c + 7)
    z1 = torch.randint(-2, 3, (n, c, h, w), generator=g).float()
    z2 = torch.randint(-2, 3, (n, c, h, w), generator=g).float()
    for a, b in ((z1, None), (z1, z2)):
        lab, _, margin = predict_truth(a, b, used)
        o = a.double().numpy() if b is None else (a.double().numpy() + b.double().numpy()) / 2
        assert np.array_equal(lab.numpy(), np.argmax(o[:, :used], axis=1).astype(np.uint8))
        if used > 1:
            srt = np.sort(o[:, :used], axis=1)
            assert np.array_equal(margin.numpy(), srt[:, -1] - srt[:, -2])
            tied = margin.numpy() == 0
            if c >= 16 and tied.size >= 100:
                assert tied.mean() > 0.1
            # at a tie the label is the smallest maximal index: no earlier class reaches the maximum
            top = o[:, :used].max(1)
            for i in zip(*np.nonzero(tied)):
                k = int(lab.numpy()[i])
                assert o[i[0], k, i[1], i[2]] == top[i] and not (o[i[0], :k, i[1], i[2]] == top[i]).any()


@pytest.mark.parametrize("c", [1, 2, 16, 17, 41, 48])
@pytest.mark.parametrize("value", [0.0, -3.25, 80.0])
def test_constant_logits_closed_form(c, value):
    z = torch.full((2, c, 3, 5), value)
    for used in sorted({1, c}):
        for z2 in (None, z):
            lab, ent, margin = predict_truth(z, z2, used)
            assert not lab.any()
            assert math.isclose(ent, -(1.0 / c) * math.log(1.0 / c + 1e-6), rel_tol=1e-14, abs_tol=0.0)
            assert bool((margin == (float("inf") if used == 1 else 0.0)).all())


def test_excluded_channel_never_wins_but_counts_in_the_entropy():
    g = torch.Generator().manual_seed(3)
    z = torch.randn(2, 5, 4, 6, generator=g)
    z[:, 4] += 50
    lab, ent, _ = predict_truth(z, None, 4)
    assert int(lab.max()) <= 3 and np.array_equal(lab.numpy(), np.argmax(z[:, :4].numpy(), 1))
    lab_all, ent_all, _ = predict_truth(z, None, 5)
    assert bool((lab_all == 4).all()) and ent == ent_all
    assert ent < 1e-12  # p = 1 on the excluded channel: -(1/5) (log(1 + 1e-6) + ...) is about -2e-7, not the 4-class entropy


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 2, 1, 3), (1, 16, 2, 1), (2, 17, 3, 5), (1, 41, 2, 9)], ids=lambda s: "x".join(map(str, s)))
def test_up_samplers_in_fp64(shape):
    """the fp64 up-samplers against their definitions written out per output pixel, and the claim the GPU test's exact inputs rest
    on: integer scores in [-2, 2] and weights in {-1, -.5, 0, .5, 1} make every interpolated logit exact in fp32"""
    n, c, hi, wi = shape
    g = torch.Generator().manual_seed(hi * 10 + wi)
    s = torch.randint(-2, 3, shape, generator=g).float()
    w = torch.randint(-2, 3, (c, 1, 16, 16), generator=g).float() / 2
    zb, zu = bilinear8_truth(s), up8_truth(s, w)
    assert zb.dtype == torch.float64 and tuple(zb.shape) == (n, c, 8 * hi, 8 * wi) == tuple(zu.shape)
    assert torch.equal(F.interpolate(s, scale_factor=8, mode="bilinear", align_corners=False).double(), zb)
    assert torch.equal(F.conv_transpose2d(s, w, stride=8, padding=4, groups=c).double(), zu)
    sd, wd = s.double().numpy(), w.double().numpy()
    eb, eu = np.zeros(zb.shape), np.zeros(zu.shape)
    for oy in range(8 * hi):
        fy = max((oy + 0.5) / 8 - 0.5, 0.0)
        y0 = int(fy)
        y1, ly = min(y0 + 1, hi - 1), fy - y0
        for ox in range(8 * wi):
            fx = max((ox + 0.5) / 8 - 0.5, 0.0)
            x0 = int(fx)
            x1, lx = min(x0 + 1, wi - 1), fx - x0
            eb[:, :, oy, ox] = (1 - ly) * ((1 - lx) * sd[:, :, y0, x0] + lx * sd[:, :, y0, x1]) + ly * ((1 - lx) * sd[:, :, y1, x0] + lx * sd[:, :, y1, x1])
            for iy in range(hi):  # out[oy] += in[iy] * w[oy + 4 - 8 iy] where that tap exists
                ky = oy + 4 - 8 * iy
                if not 0 <= ky < 16:
                    continue
                for ix in range(wi):
                    kx = ox + 4 - 8 * ix
                    if 0 <= kx < 16:
                        eu[:, :, oy, ox] += sd[:, :, iy, ix] * wd[None, :, 0, ky, kx]
    assert np.array_equal(zb.numpy(), eb) and np.array_equal(zu.numpy(), eu)
