"""Every input of tests/test_loss_edges_gpu.py, as ``loss_ref.Case`` s built from seeded numpy draws: the GPU test runs them, and
tests/test_loss_ref_host.py checks -- on the reference alone -- that the margin rule leaves out at most LEFT_OUT of each one's pixels.

Class counts: both sides of every instantiation switch of csrc/loss.hip (plain kernel NCMAX 16 / 24 / 48; LDS-DMA kernel
<16 | 24 | 41 | 48, EXACT = (C == NCMAX)>), both sides of the counted wait's switch (two heads: 62 stores at C = 31, 64 at C = 32), and
the smallest counts."""
import numpy as np

from loss_ref import Case

PLAIN_C = (1, 2, 16, 17, 24, 25, 31, 32, 41, 47, 48)
# 234 pixels: not a multiple of the 256-thread block, and the block straddles the image boundary; one pixel; 768 = exactly three blocks
PLAIN_SHAPES = ((2, 9, 13), (1, 1, 1), (3, 16, 16))
# name: (ce_coef, diff_coef, heads, labelled)
MODES = {"ce-single": (1.0, 0.0, 1, True), "ce-diff": (1.0, -1.0, 2, True), "ce+0.7diff": (1.0, 0.7, 2, True), "diff": (0.0, 1.0, 2, False)}

FUSED_C = (1, 16, 17, 24, 25, 31, 32, 41, 47, 48)
# one ragged 8-pixel segment with both image borders in one patch; exactly one full segment; a second segment 8 pixels wide; several rows
FUSED_SHAPES = ((1, 1, 1), (2, 1, 8), (1, 2, 9), (2, 3, 20))
# name: (ce_coef, diff_coef, heads, labelled, shared scores) -- the modes of test_up8_loss_fused_equals_two_pass
FUSED_MODES = {"ce+diff": (1.0, 0.7, 2, True, False), "diff": (0.0, 0.7, 2, False, False), "ce-single": (1.0, 0.0, 1, True, False),
               "shared-scores": (1.0, 0.7, 2, True, True)}

ADVERSE_PLAIN_C = (2, 19, 41)
ADVERSE_FUSED_C = (16, 41)
WAIT_CASES = ((31, 2), (32, 2), (48, 1))  # (C, heads): 62 and 64 stores per item and wave around the vmcnt(63) switch; 48: the vmcnt(0) branch
WAIT_SHAPE = (4, 23, 57)                  # N, Hi, Wi: 4 * 24 * 8 = 768 items on 256 workgroups, three each; the last segment is 8 wide
LABEL_C, LABEL_SHAPE = 19, (2, 3, 9)      # N, Hi, Wi -> 24 x 72 pixels an image: one full 64-label segment and a ragged one of 8


def spreads(c):
    """(spread, adverse).  Two classes at spread 30 leave 6 % of the pixels to the margin rule (both heads saturate on the same class),
    so C <= 2 stops at spread 8.  At C = 2 spread 8 still leaves out 4.0 % (measured on 2 x 2 x 240 x 400 logits: 1.6 % at spread 6,
    0.17 % at spread 4 -- tests/test_loss_ref_host.py asserts it): there the values and the CE-only gradient are held, the gradients with
    an L1 term are not compared, and spread 4 is added, where everything is.
    Spreads 4 and 8 are to one and two classes what spread 30 is to sixteen and more -- the saturated end, hence adverse: the two logits
    of a pixel differ by 5.7 and 11 standard deviations, p is 1 - e with e down to 1e-7, and p - 1 (the CE gradient of the labelled
    class, the L1 gradient's s - sum s p) keeps 2^-24 / e of relative precision in ANY fp32 evaluation; on the one-pixel shape nothing
    larger stands beside it (the fp32 oracle's own error there: 5.9e-5 of max|g| at spread 8, 4.6e-5 at spread 4)."""
    if c == 1:
        return ((2.0, False), (8.0, True))
    return ((2.0, False), (4.0, True), (8.0, True)) if c == 2 else ((2.0, False), (30.0, True))


def over_the_cap(c, spread, mode):
    """the one family whose L1 gradient the margin rule cannot hold within LEFT_OUT"""
    return c == 2 and spread == 8.0 and MODES[mode][2] == 2


def zero_weight_classes(c):
    """classes whose weight is zero although labels use them: two where that leaves a positive weight, never class C - 1"""
    return (0, c // 2) if c >= 3 else ((0,) if c == 2 else ())


def _labels_and_weights(rs, c, n, h, w):
    """labels that use every zero-weight class, three ignored pixels (where there are that many to spare), weights in [0.5, 1.5)"""
    y = rs.randint(0, c, size=(n, h, w)).astype(np.int64)
    cw = rs.uniform(0.5, 1.5, c).astype(np.float32)
    flat = y.reshape(-1)
    if flat.size == 1:
        flat[0] = c - 1
    else:
        for k, cls in enumerate(zero_weight_classes(c)):
            flat[1 + k] = cls
        flat[[0, flat.size // 2, flat.size - 1]] = -100
    for cls in zero_weight_classes(c):
        cw[cls] = 0.0
    return y, cw


def plain_problem(c, shape, spread, adverse=False, seed=0):
    n, h, w = shape
    rs = np.random.RandomState(1000 * c + 10 * h + int(spread) + seed)
    z1 = (spread * rs.standard_normal((n, c, h, w))).astype(np.float32)
    z2 = (spread * rs.standard_normal((n, c, h, w))).astype(np.float32)
    y, cw = _labels_and_weights(rs, c, n, h, w)
    return Case("plain C=%d %s spread %g" % (c, "x".join(map(str, shape)), spread), z1=z1, z2=z2, labels=y, cw=cw, adverse=adverse)


def in_mode(case, mode, modes=MODES):
    """``case`` (which holds both heads, labels and weights) as one of the kernel's modes"""
    ce, diff, heads, labelled = modes[mode][:4]
    ch = dict(ce_coef=ce, diff_coef=diff)
    if heads == 1:
        ch.update(z2=None, s2=None, w2=None)
    if not labelled:
        ch.update(labels=None, cw=None)
    if len(modes[mode]) > 4 and modes[mode][4]:
        ch.update(s2=case.s1)
    return case.but("%s %s" % (case.what, mode), **ch)


def plain_cases(c):
    return [in_mode(plain_problem(c, shape, spread, adverse), mode).but(None, grads=not over_the_cap(c, spread, mode))
            for shape in PLAIN_SHAPES for spread, adverse in spreads(c) for mode in MODES]


def fused_problem(c, shape, seed=11, unit_taps=False, **kw):
    """scores 2 randn, taps 0.2 randn, five ignored labels, weights in [0.5, 1.5): the problem of the existing fused tests.
    ``unit_taps``: taps that are multiples of 2^-10 and whose four taps of every pixel phase sum to exactly 1 (as a bilinear kernel's do),
    so that a constant added to every score of an image adds that constant to every logit of a pixel with all four inputs present"""
    n, hi, wi = shape
    rs = np.random.RandomState(100 * c + 10 * hi + wi + seed)
    s1 = (2 * rs.standard_normal((n, c, hi, wi))).astype(np.float32)
    s2 = (2 * rs.standard_normal((n, c, hi, wi))).astype(np.float32)
    w1 = (0.2 * rs.standard_normal((c, 1, 16, 16))).astype(np.float32)
    w2 = (0.2 * rs.standard_normal((c, 1, 16, 16))).astype(np.float32)
    if unit_taps:
        for w in (w1, w2):
            w[:] = np.round(w * 1024) / 1024
            w[:, :, 8:, 8:] = 1 - (w[:, :, :8, :8] + w[:, :, :8, 8:] + w[:, :, 8:, :8])
    y = rs.randint(0, c, size=(n, 8 * hi, 8 * wi)).astype(np.int64)
    y[0, 0, :5] = -100
    cw = (0.5 + rs.uniform(size=c)).astype(np.float32)
    return Case("fused C=%d %s" % (c, "x".join(map(str, shape))), s1=s1, w1=w1, s2=s2, w2=w2, labels=y, cw=cw, **kw)


def fused_cases(c):
    return [in_mode(fused_problem(c, shape), mode, FUSED_MODES) for shape in FUSED_SHAPES for mode in FUSED_MODES]


def wait_case(c, heads):
    n, hi, wi = WAIT_SHAPE
    case = fused_problem(c, WAIT_SHAPE, seed=5, unit=False)
    if heads == 1:
        return case.but("wait C=%d single head" % c, s2=None, w2=None, ce_coef=1.0)
    return case.but("wait C=%d" % c, ce_coef=1.0, diff_coef=-1.0)


# ---------------------------------------------------------------------------------------------------- adverse logits
def adverse_plain(c):
    """{name: Case or (Case, truth Case)} on 2 x C x 9 x 13 logits at spread 2, CE - Diff"""
    base = in_mode(plain_problem(c, (2, 9, 13), 2.0, seed=3), "ce-diff")
    rs = np.random.RandomState(77 + c)
    out = {}
    off = np.where(rs.uniform(size=(2, 1, 9, 13)) < 0.5, -100.0, 100.0).astype(np.float32)
    shifted = base.but("plain C=%d offset" % c, z1=base.z1 + off, adverse=True)
    out["offset"] = (shifted, base)
    out["offset-diff"] = (in_mode(shifted, "diff"), in_mode(base, "diff"))
    z1 = base.z1.copy()
    z1.reshape(2, c, -1)[:, :, [3, 50, 116]] = 0.25
    out["uniform-pixels"] = base.but("plain C=%d uniform pixels" % c, z1=z1)
    out["constant-head"] = base.but("plain C=%d constant head" % c, z2=np.full_like(base.z2, 0.5))
    z2 = base.z2.copy()
    z2.reshape(2, c, -1)[0][:, [7, 64, 110]] = base.z1.reshape(2, c, -1)[0][:, [7, 64, 110]]
    out["identical-pixels"] = base.but("plain C=%d identical pixels" % c, z2=z2)
    out["identical-heads"] = base.but("plain C=%d identical heads" % c, z2=base.z1.copy())
    return out


def adverse_fused(c):
    """the same on 2 x C x 3 x 20 scores (24 x 160 pixels an image), CE - Diff"""
    shape = (2, 3, 20)
    base = fused_problem(c, shape, seed=3, unit_taps=True).but("fused C=%d unit taps" % c, ce_coef=1.0, diff_coef=-1.0)
    out = {}
    off = np.array([100.0, -100.0], np.float32)[:, None, None, None]
    shifted = base.but("fused C=%d offset" % c, s1=base.s1 + off, adverse=True)
    out["offset"] = (shifted, base)
    out["offset-diff"] = (in_mode(shifted, "diff", FUSED_MODES), in_mode(base, "diff", FUSED_MODES))
    plain = fused_problem(c, shape, seed=4).but("fused C=%d" % c, ce_coef=1.0, diff_coef=-1.0)
    s1 = plain.s1.copy()
    s1[:, :, 1:3, 5:8] = 0.0  # every logit of the 8 x 16 pixels between these inputs is 0
    out["uniform-pixels"] = plain.but("fused C=%d uniform pixels" % c, s1=s1)
    out["constant-head"] = plain.but("fused C=%d constant head" % c, s2=np.zeros_like(plain.s2))
    s2 = plain.s2.copy()
    s2[0, :, 1:3, 10:12] = plain.s1[0, :, 1:3, 10:12]  # with equal taps: the 8 x 8 pixels between these inputs
    out["identical-pixels"] = plain.but("fused C=%d identical pixels" % c, s2=s2, w2=plain.w1.copy())
    out["identical-heads"] = plain.but("fused C=%d identical heads" % c, s2=plain.s1.copy(), w2=plain.w1.copy())
    return out


def interior(shape):
    """[N,H,W]: the output pixels of the fused kernels with all four inputs present (where unit taps sum to 1)"""
    n, hi, wi = shape
    m = np.zeros((n, 8 * hi, 8 * wi), bool)
    m[:, 4:-4, 4:-4] = True
    return m


# ---------------------------------------------------------------------------------------------------- labels
def special_labels(c, n, h, w, seed=9):
    """a label map that holds 0, C - 1 and -- several times each, across segment and row ends -- labels outside [0, C)"""
    rs = np.random.RandomState(seed)
    y = rs.randint(0, c, size=(n, h, w)).astype(np.int64)
    flat = y.reshape(-1)
    special = [0, c - 1, c, c + 1, 255, -1, -7, 2 ** 40, -2 ** 40, 2 ** 32, 2 ** 32 + 1, -2 ** 32 + 1]
    at = rs.choice(flat.size, size=8 * len(special), replace=False)
    for k, v in enumerate(special):
        flat[at[k::len(special)]] = v
    flat[:len(special)] = special  # ... and side by side at the start of the first row
    return y


def label_case(front, ignore_index, seed=0):
    """``front``: "plain" (logits) or "fused" (scores and taps), C = 19, 2 x 24 x 72 pixels, CE - Diff"""
    n, hi, wi = LABEL_SHAPE
    y = special_labels(LABEL_C, n, 8 * hi, 8 * wi)
    if front == "plain":
        case = plain_problem(LABEL_C, (n, 8 * hi, 8 * wi), 2.0, seed=21 + seed)
    else:
        case = fused_problem(LABEL_C, LABEL_SHAPE, seed=21 + seed)
    return case.but("%s labels ignore_index=%d" % (front, ignore_index), labels=y, ignore_index=ignore_index, ce_coef=1.0, diff_coef=-1.0)


def oob_replaced(case):
    """the same case with every label outside [0, C) set to ``ignore_index``"""
    y = case.labels.copy()
    y[(y < 0) | (y >= LABEL_C)] = case.ignore_index
    return case.but(case.what + " replaced", labels=y)


def every_margin_case():
    """every Case whose gradients the GPU test compares under the margin rule (the identical-heads cases are held to exact zeros instead)"""
    for c in PLAIN_C:
        yield from (case for case in plain_cases(c) if case.grads)
    for c in FUSED_C:
        yield from fused_cases(c)
    for c in ADVERSE_PLAIN_C:
        for name, v in adverse_plain(c).items():
            if name != "identical-heads":
                yield v[0] if isinstance(v, tuple) else v
    for c in ADVERSE_FUSED_C:
        for name, v in adverse_fused(c).items():
            if name != "identical-heads":
                yield v[0] if isinstance(v, tuple) else v
    for front in ("plain", "fused"):
        for ii in (-100, 255, 3):
            yield label_case(front, ii)
    for c, heads in WAIT_CASES:
        yield wait_case(c, heads)
