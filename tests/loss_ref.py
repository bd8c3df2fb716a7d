"""The fp64 truth of the fused cross-entropy + L1-discrepancy kernels (csrc/loss.hip, csrc/loss_front.h): numpy only.

``losses``   the semantics of ``ops.mcd_losses`` (d_loss "diff"), every statement in ``dtype``: np.float64 is the truth, np.float32 the
             "unit" -- what a plain fp32 evaluation of the same statements loses on the same inputs
``up8``      the x8 up-sampler (depthwise transposed convolution, stride 8, padding 4, 16x16 kernel) as four-tap sums
``sure``     the pixels at which sign(p1 - p2), hence the L1 gradient, is determined (the margin rule)
``Case``     one problem (logits, or scores + taps of the fused kernels) with its truth in both precisions, computed once
``held``     the comparison of a kernel's result with a Case: prints every figure, then asserts

Bars: VAL_RTOL / GRAD_RTOL of tests/test_prob_distance_gpu.py (a value relative to the fp64 value, a gradient relative to the fp64
gradient's largest entry); at adverse inputs max(bar, FACTOR * unit) with the FACTOR of tests/test_dense_crf_gpu.py."""
import numpy as np

VAL_RTOL, GRAD_RTOL = 2e-6, 5e-6
FACTOR = 2.0
LEFT_OUT = 0.02
CLOSE, LIVE = 1e-5, 1e-7  # the margin rule's two constants


def softmax(z, dtype=np.float64):
    """(p [N,C,H,W], log sum exp [N,H,W]) over axis 1, stable"""
    z = np.asarray(z, dtype=dtype)
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(axis=1, keepdims=True)
    return e / s, (m + np.log(s))[:, 0]


def counted(labels, n_class, ignore_index=-100):
    """the pixels whose label takes part: inside [0, C) and not ``ignore_index`` (which may itself be a valid class)"""
    y = np.asarray(labels, dtype=np.int64)
    return (y >= 0) & (y < n_class) & (y != ignore_index)


def sure(p1, p2):
    """[N,H,W] bool.  A pixel is NOT sure when some class has |p1_c - p2_c| < 1e-5 max(p1_c, p2_c) -- the heads agree to rounding, the
    sign is anybody's -- while max(p1_c (1 - p1_c), p2_c (1 - p2_c)) > 1e-7: a saturated class cannot move the gradient whichever way
    its sign falls, so it leaves the pixel sure."""
    p1, p2 = np.asarray(p1, np.float64), np.asarray(p2, np.float64)
    close = np.abs(p1 - p2) < CLOSE * np.maximum(p1, p2)
    live = np.maximum(p1 * (1 - p1), p2 * (1 - p2)) > LIVE
    return ~(close & live).any(axis=1)


def losses(z1, z2, labels, cw, ignore_index=-100, ce_coef=0.0, diff_coef=0.0, wsum=None, dtype=np.float64):
    """(ce1, ce2, diff, W, g1, g2) as ``ops.mcd_losses`` defines them:
      ce_k = sum_i w[y_i] (lse_i - z_k,i[y_i]) / W over the counted pixels, W = sum_i w[y_i] or ``wsum`` when given (0 without labels);
      diff = mean |softmax(z1) - softmax(z2)| over N C H W;   g_k = ce_coef dce_k/dz_k + diff_coef ddiff/dz_k.
    ``z2 = None`` is the single-head form (ce2 = 0 / W, no diff, g2 None).  W = 0 with labels is the reference's 0/0: NaN values, and
    NaN gradients at the counted pixels (their weights are all zero), as the kernel documents."""
    dt = np.dtype(dtype).type
    z1 = np.asarray(z1, dtype=dt)
    n, c, h, w = z1.shape
    two = z2 is not None
    p1, lse1 = softmax(z1, dt)
    p2, lse2 = softmax(z2, dt) if two else (None, None)
    m = dt(p1.size)
    with np.errstate(invalid="ignore", divide="ignore"):
        kce = None
        if labels is None:
            ce1 = ce2 = dt(0)
            W = dt(0) if wsum is None else dt(wsum)
        else:
            cnt = counted(labels, c, ignore_index)
            ys = np.where(cnt, np.asarray(labels, dtype=np.int64), 0)
            wy = (np.ones(c, dt) if cw is None else np.asarray(cw, dtype=dt))[ys] * cnt.astype(dt)
            W = wy.sum() if wsum is None else dt(wsum)
            ce1 = (wy * (lse1 - np.take_along_axis(z1, ys[:, None], axis=1)[:, 0])).sum() / W
            ce2 = (wy * (lse2 - np.take_along_axis(np.asarray(z2, dtype=dt), ys[:, None], axis=1)[:, 0])).sum() / W if two else dt(0) / W
            if ce_coef != 0.0:
                kce = np.where(cnt, dt(ce_coef) * wy / W, dt(0))

        def ce_grad(p):
            if kce is None:
                return np.zeros_like(p)
            g = p.copy()
            np.put_along_axis(g, ys[:, None], np.take_along_axis(g, ys[:, None], axis=1) - dt(1), axis=1)
            return kce[:, None] * g  # (p - onehot at pixels that are not counted is multiplied by an exact 0)

        g1 = ce_grad(p1)
        g2 = ce_grad(p2) if two else None
        diff = dt(0)
        if two:
            d = p1 - p2
            diff = np.abs(d).sum() / m
            s = np.sign(d)
            kd = dt(diff_coef) / m
            g1 = g1 + kd * (p1 * (s - (s * p1).sum(axis=1, keepdims=True)))
            g2 = g2 - kd * (p2 * (s - (s * p2).sum(axis=1, keepdims=True)))
    return ce1, ce2, diff, W, g1, g2


def up8(s, w, dtype=np.float64):
    """out[n,c,oy,ox] = sum over (iy,ky,ix,kx) with oy = 8 iy - 4 + ky, ox = 8 ix - 4 + kx of s[n,c,iy,ix] w[c,0,ky,kx]: per axis the two
    inputs (oy + 4) // 8 - a with kernel index (oy + 4) % 8 + 8 a, a = 0, 1 -- four taps a pixel, absent inputs count as zeros"""
    dt = np.dtype(dtype).type
    s, w = np.asarray(s, dtype=dt), np.asarray(w, dtype=dt)
    n, c, hi, wi = s.shape
    assert w.shape == (c, 1, 16, 16), w.shape
    sp = np.zeros((n, c, hi + 2, wi + 2), dt)
    sp[:, :, 1:-1, 1:-1] = s
    oy, ox = np.arange(8 * hi), np.arange(8 * wi)
    out = np.zeros((n, c, 8 * hi, 8 * wi), dt)
    for a in (0, 1):
        for b in (0, 1):
            rows, cols = (oy + 4) // 8 - a + 1, (ox + 4) // 8 - b + 1  # (in the padded map)
            ky, kx = (oy + 4) % 8 + 8 * a, (ox + 4) % 8 + 8 * b
            out += sp[:, :, rows[:, None], cols[None, :]] * w[:, 0][:, ky[:, None], kx[None, :]][None]
    return out


class Case:
    """One problem of the loss kernels and its truth.  Either logits ``z1`` / ``z2`` [N,C,H,W] (the plain kernel) or scores and taps
    ``s1, w1, s2, w2`` (the fused kernels: the truth up-samples with ``up8`` in the truth's own precision).  ``adverse``: the bound is
    max(bar, FACTOR * unit).  ``unit = False`` (large cases that are not adverse): the fp32 evaluation is not made, its figures print as nan.
    ``grads = False``: only the values are held (a case whose L1 gradient the margin rule would leave out of at more pixels than the cap).
    ``what``: the case's name in the printed figures."""

    def __init__(self, what, z1=None, z2=None, s1=None, w1=None, s2=None, w2=None, labels=None, cw=None, ignore_index=-100, ce_coef=0.0,
                 diff_coef=0.0, wsum=None, adverse=False, unit=True, grads=True):
        self.what, self.adverse, self.unit, self.grads = what, adverse, unit or adverse, grads
        self.z1, self.z2, self.s1, self.w1, self.s2, self.w2 = z1, z2, s1, w1, s2, w2
        self.labels, self.cw, self.wsum = labels, cw, wsum
        self.ignore_index, self.ce_coef, self.diff_coef = ignore_index, ce_coef, diff_coef
        self.fused = s1 is not None
        self.two = (s2 if self.fused else z2) is not None
        self._truth, self._sure = {}, None

    def but(self, what, **changes):
        """the same problem with some fields changed"""
        kw = dict(z1=self.z1, z2=self.z2, s1=self.s1, w1=self.w1, s2=self.s2, w2=self.w2, labels=self.labels, cw=self.cw, wsum=self.wsum,
                  ignore_index=self.ignore_index, ce_coef=self.ce_coef, diff_coef=self.diff_coef, adverse=self.adverse, unit=self.unit, grads=self.grads)
        kw.update(changes)
        return Case(what if what is not None else self.what, **kw)

    def logits(self, dtype=np.float64):
        if not self.fused:
            return self.z1, self.z2
        z1 = up8(self.s1, self.w1, dtype)
        return z1, (up8(self.s2, self.w2, dtype) if self.two else None)

    def truth(self, dtype=np.float64):
        """``losses`` of this case in ``dtype``: computed once, then left unchanged"""
        key = np.dtype(dtype).name
        if key not in self._truth:
            z1, z2 = self.logits(dtype)
            self._truth[key] = losses(z1, z2, self.labels, self.cw, self.ignore_index, self.ce_coef, self.diff_coef, self.wsum, dtype)
        return self._truth[key]

    def sure(self):
        """[N,H,W]: the pixels whose gradient is compared (all of them unless the L1 term takes part)"""
        if self._sure is None:
            z1, z2 = self.logits(np.float64)
            if self.two and self.diff_coef != 0.0:
                self._sure = sure(softmax(z1)[0], softmax(z2)[0])
            else:
                self._sure = np.ones((z1.shape[0],) + z1.shape[2:], bool)
        return self._sure

    def left_out(self):
        return 1.0 - float(self.sure().mean())


def _rel(a, ref):
    """|a - ref| relative to |ref|; where the truth is exactly 0 (one class, identical heads, no labels) the absolute distance"""
    a, ref = float(a), float(ref)
    return abs(a - ref) / abs(ref) if ref != 0.0 else abs(a)


def held(got, case, truth=None, pixels=None, grads=True, values=True, out=print):
    """Hold a kernel's result ``got = (losses[4], g1, g2)`` (numpy; a gradient that was not asked for is None) to the fp64 truth of
    ``case``.  Values: CE1, CE2, Diff and W relative to the truth's.  Gradients: on the sure pixels (and inside ``pixels`` [N,H,W] when
    given), relative to the truth's largest entry there.  ``truth``: another Case whose fp64 result is the truth instead (the same
    problem before an offset that changes no probability); the unit is then the distance of THIS case's fp32 evaluation from THAT truth.
    ``values = False``: the values are not compared (a truth whose border pixels differ from the case's).
    Prints kernel error, unit and bound of every figure, then asserts; returns {"value": worst error, "grad": worst error}."""
    t64 = (truth if truth is not None else case).truth(np.float64)
    t32 = case.truth(np.float32) if case.unit else (np.nan,) * 4 + (None, None)
    ls = np.asarray(got[0], dtype=np.float64)
    bad, worst = [], {"value": 0.0, "grad": 0.0}
    for k, name in enumerate(("CE1", "CE2", "Diff", "W") if values else ()):
        ref = float(t64[k])
        if np.isnan(ref):
            if not np.isnan(ls[k]):
                bad.append("%s: %r where the truth is NaN" % (name, ls[k]))
            continue
        err, unit = _rel(ls[k], ref), _rel(t32[k], ref)
        bound = max(VAL_RTOL, FACTOR * unit) if case.adverse else (VAL_RTOL if ref != 0.0 else 0.0)
        out("%s %s: kernel %.9e truth %.9e error %.2e, the fp32 oracle's %.2e, bound %.2e" % (case.what, name, ls[k], ref, err, unit, bound))
        worst["value"] = max(worst["value"], err)
        if not err <= bound:
            bad.append("%s: error %.3e > bound %.3e (unit %.3e)" % (name, err, bound, unit))
    if grads and case.grads:
        mask = (truth if truth is not None else case).sure()
        if truth is not None:
            mask = mask & case.sure()
        if pixels is not None:
            mask = mask & pixels
        out("%s: %d of %d pixels left out by the margin rule" % (case.what, int((~case.sure()).sum()), mask.size))
        idx = np.broadcast_to(mask[:, None], t64[4].shape)
        for k in (4, 5):
            if t64[k] is None:
                if got[k - 3] is not None:
                    bad.append("g%d exists without a second head" % (k - 3))
                continue
            g = np.asarray(got[k - 3], dtype=np.float64)
            r64 = t64[k][idx]
            r32 = np.asarray(t32[k], dtype=np.float64)[idx] if case.unit else np.full_like(r64, np.nan)
            if np.isnan(r64).any():  # W = 0: NaN exactly where the truth has them
                if not np.array_equal(np.isnan(g[idx]), np.isnan(r64)):
                    bad.append("g%d: NaN pattern differs from the truth's" % (k - 3))
                continue
            if not np.isfinite(g).all():
                bad.append("g%d is not finite" % (k - 3))
                continue
            scale = float(np.abs(r64).max()) if r64.size else 0.0
            div = scale if scale != 0.0 else 1.0
            err = float(np.abs(g[idx] - r64).max()) / div if r64.size else 0.0
            unit = float(np.abs(r32 - r64).max()) / div if r64.size else 0.0
            bound = max(GRAD_RTOL, FACTOR * unit) if case.adverse else (GRAD_RTOL if scale != 0.0 else 0.0)
            out("%s g%d: error %.2e of max|g| %.3e, the fp32 oracle's %.2e, bound %.2e" % (case.what, k - 3, err, scale, unit, bound))
            worst["grad"] = max(worst["grad"], err)
            if not err <= bound:
                bad.append("g%d: error %.3e > bound %.3e (unit %.3e)" % (k - 3, err, bound, unit))
    assert not bad, "%s: %s" % (case.what, "; ".join(bad))
    return worst
