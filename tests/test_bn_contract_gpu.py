"""GPU: every BatchNorm entry point of the fp32 family (csrc/bn.hip) and ``mcdseg_bn_bwd_reduce_half``, called through the C ABI one at a
time, against tests/bn_ref.py -- the float64 statement of include/mcdseg.h that tests/test_bn_ref_host.py has shown equal to
``F.batch_norm`` -- on ADVERSE data, and the contract of the two bound scalars (``y_bound``, ``dz_bound``) the fp16 split scales come from.

Tolerances.  No constant is taken from the kernels.  For each compared tensor the budget is the error, against the same fp64 truth, of
a plain fp32 statement of the header's formulas (torch-CPU float32 tensors and ``.sum()``, below: ``_plain_*``), times 4 (fp32
summation orders differ by a small factor), plus 4 ulp of the tensor's scale (for cases where the plain statement happens to be
exact).  The truth of a train-mode case is the fp64 chain from the fp32 data (fp64 statistics included); the kernels are handed those
statistics rounded to fp32, the plain statement forms its own in fp32.  Every figure is printed before it is asserted
(``pytest -s``): docs/MEASURED_HISTORY.md holds the table.

Data (``_case``), built once per shape on the CPU, seeded; channel c takes recipe (c + off) % 8 of
  benign       randn + 0.3
  off1e2       randn + 1e2                        |mean|/std = 1e2
  off1e3       randn * 1e-2 + 10                  |mean|/std = 1e3; rstd = 100: the channel that decides dz_bound
  const        3.25 everywhere                    rstd = 1/sqrt(eps)
  tight        zeros and one 1000 (the LAST pixel of the last image), gamma = 2.5, beta = 9: attains Samuelson's bound, and --
               the largest |gamma| and |beta| of all channels -- decides y_bound
  zero         gamma = beta = 0
  neg          gamma = -1.25
  dead         beta = -8: ReLU kills the whole channel
In every channel the pixel with the lowest pre-activation carries dy = 8 (twice any other |dy|) and a non-positive residual: a
gradient ReLU kills must not enter dz_bound."""
import ctypes
import functools
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_ref

pytestmark = pytest.mark.gpu

EPS, MOM = bn_ref.EPS, bn_ref.MOMENTUM
F16X3, BF16X6 = 3, 6
RECIPES = ("benign", "off1e2", "off1e3", "const", "tight", "zero", "neg", "dead")

# (N, C, H, W): the smallest shapes at which each code path of csrc/bn.hip exists
SHAPES = [
    (2, 5, 3, 7),       # HW = 21: the scalar loops (HW % 4 != 0) of apply / reduce / backward apply; C no multiple of 4 (one ragged block of
                        # the one-wave-per-channel finalize kernels) or 8 (no companion, no bit-plane); recipes off1e3 .. neg (off = 2)
    (1, 8, 1, 4),       # HW = 4: one float4 per plane, n = 4 values per channel; one lane of one wave of the four-pixel kernels
    (2, 8, 12, 21),     # HW = 252: 63 float4 -- one ragged wave in a single 256-pixel block of the bit-plane / the companion's LDS image
    (3, 16, 13, 20),    # HW = 260: a second 256-pixel block holding one float4 (one lane of the second wave); two channel groups
    (1, 8, 41, 100),    # HW = 4100: bwd_plan gives cpp = 2 chunks of 2304 pixels per plane, the second ragged (1796); 17 bit-plane blocks
    (2, 1024, 41, 100), # bwd_plan: want = 2048 / C = 2 splits <= N, so cpp = 1 and the chunk is the whole plane, 4100 > 4096 elements: the
                        # four-step float4 loop of bn_bwd_reduce_kernel takes a second trip that holds ONE float4.  The smallest such
                        # tensor: cpp = 1 needs N * C >= 2048, the second trip HW > 4096 with HW % 4 == 0 (33.6 MB per tensor)
]
CB_SHAPES = [s for s in SHAPES if s[1] % 8 == 0 and (s[2] * s[3]) % 4 == 0]   # the _cb / mask variants: C % 8 == 0 and HW % 4 == 0
_ids = lambda s: "x".join(map(str, s))


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _api():
    from mcdseg import ops
    return ops.lib(), ops._p, ops._stream(), ops.check


def _cv(v):
    return v.view(1, -1, 1, 1)


@functools.lru_cache(maxsize=2)
def _case(shape):
    """the adverse data of one shape (CPU fp32) with its fp64 train-mode statistics; shared by the tests, never modified"""
    n_, c_, h, w = shape
    g = torch.Generator().manual_seed(4000 + 131 * c_ + h * w)
    kinds = [RECIPES[(c + (2 if c_ < 8 else 0)) % 8] for c in range(c_)]
    z = torch.randn(shape, generator=g)
    gamma = 0.75 + 0.5 * torch.rand(c_, generator=g)
    beta = 0.2 * torch.randn(c_, generator=g)
    for c, k in enumerate(kinds):
        if k == "off1e2":
            z[:, c] += 1e2
        elif k == "off1e3":
            z[:, c] = z[:, c] * 1e-2 + 10.0
            gamma[c] = 1.5
        elif k == "const":
            z[:, c] = 3.25
            gamma[c] = 0.25
        elif k == "tight":
            z[:, c] = 0.0
            z[-1, c, -1, -1] = 1000.0
            gamma[c], beta[c] = 2.5, 9.0
        else:
            z[:, c] += 0.3
            if k == "zero":
                gamma[c], beta[c] = 0.0, 0.0
            elif k == "neg":
                gamma[c] = -1.25
            elif k == "dead":
                gamma[c], beta[c] = 1.0, -8.0
    st = bn_ref.batch_stats(z)
    pre = bn_ref.forward(z, st["mean"], st["rstd"], gamma, beta)
    low = pre.permute(1, 0, 2, 3).reshape(c_, -1).argmin(1)          # per channel: the pixel with the lowest pre-activation
    dy = torch.randn(shape, generator=g).clamp_(-4.0, 4.0)
    res = 0.5 * torch.randn(shape, generator=g)
    hw = h * w
    for c in range(c_):
        i, pix = int(low[c]) // hw, int(low[c]) % hw
        dy[i, c].view(-1)[pix] = 8.0
        res[i, c].view(-1)[pix] = -abs(float(res[i, c].view(-1)[pix]))
    # eval mode: running statistics of the same adverse kind as the data's (the constant channel: running_var = 0)
    rm = (st["mean"] + 0.1 * torch.sqrt(st["var"])).float()
    rv = (1.1 * st["var"]).float()
    return types.SimpleNamespace(shape=shape, n=n_ * hw, hw=hw, kinds=kinds, z=z, gamma=gamma, beta=beta, dy=dy, res=res, stats=st,
                                 mean=st["mean"].float(), rstd=st["rstd"].float(), rm=rm, rv=rv)


# ---- the plain fp32 statement of the header's formulas (torch-CPU float32, .sum()): the yardstick of every budget
def _plain_stats(z):
    n = float(z.numel() // z.shape[1])
    mean = z.sum((0, 2, 3)) / n
    var = ((z - _cv(mean)) ** 2).sum((0, 2, 3)) / n
    return mean, 1.0 / torch.sqrt(var + EPS), var


def _plain_merge(cnt, mu, m2, rm, rv, updates):
    n = cnt.sum(0)
    safe = n.clamp_min(1.0)
    mean = (cnt * mu).sum(0) / safe
    M2 = m2.sum(0) + (cnt * (mu - mean) ** 2).sum(0)
    var = M2 / safe
    unb = torch.where(n > 1, M2 / (n - 1.0).clamp_min(1.0), var)
    rm, rv = rm.clone(), rv.clone()
    for _ in range(updates):
        rm = (1.0 - MOM) * rm + MOM * mean
        rv = (1.0 - MOM) * rv + MOM * unb
    return mean, 1.0 / torch.sqrt(var + EPS), rm, rv


def _plain_forward(z, mean, rstd, gamma, beta, res, relu):
    y = _cv(gamma) * ((z - _cv(mean)) * _cv(rstd)) + _cv(beta)
    if res is not None:
        y = y + res
    return y.clamp_min(0.0) if relu else y


def _plain_backward(dy, z, mean, rstd, gamma, mask, train):
    g = torch.where(mask, dy, torch.zeros_like(dy)) if mask is not None else dy
    n = float(g.numel() // g.shape[1])
    xhat = (z - _cv(mean)) * _cv(rstd)
    dbeta = g.sum((0, 2, 3))
    dgamma = (g * xhat).sum((0, 2, 3))
    a = _cv(gamma * rstd)
    dz = a * (g - _cv(dbeta) / n - xhat * _cv(dgamma) / n) if train else a * g
    return dgamma, dbeta, dz


def _judge(what, got, plain, truth, per_channel=False):
    """kernel error <= 4 x (error of the plain fp32 statement) + 4 ulp of the tensor's scale; the figures are printed first.
    ``per_channel`` (the statistics, [C] vectors whose channels differ by orders of magnitude -- rstd 316 beside 1e-3): the same rule
    for every channel by itself; what is printed is the channel that comes closest to its budget."""
    truth = truth.double()
    errs = (got.detach().double().cpu() - truth).abs()
    perrs = (plain.double() - truth).abs()
    ulp = float(np.finfo(np.float32).eps)
    if per_channel:
        budgets = 4.0 * perrs + 4.0 * ulp * truth.abs()
        c = int((errs - budgets).argmax())
        err, perr, scale, budget = float(errs[c]), float(perrs[c]), float(truth[c].abs()), float(budgets[c])
        assert bool((errs <= budgets).all()) == (err <= budget)
    else:
        err, perr, scale = float(errs.max()), float(perrs.max()), float(truth.abs().max())
        budget = 4.0 * perr + 4.0 * ulp * scale
    print("BNFIG %-58s err %.3e  plain %.3e  scale %.3e  budget %.3e  %s" % (what, err, perr, scale, budget, "ok" if err <= budget else "OVER"))
    assert err <= budget, "%s: kernel error %.3e over the budget %.3e (plain fp32 %.3e, scale %.3e)" % (what, err, budget, perr, scale)


# ---- the entry points, one call each
def _k_stats(part, rows, c, mp, dev, gamma=None, beta=None, res_bound=None, want_bound=False, running=None, updates=1, bound_init=0.0):
    L, p, st, check = _api()
    mean, rstd = torch.empty(c, device=dev), torch.empty(c, device=dev)
    rm, rv, nbt = (running[0].clone(), running[1].clone(), running[2].clone()) if running is not None else (None, None, None)
    yb = torch.full((1,), bound_init, device=dev) if want_bound else None
    nbytes = L.mcdseg_bn_stats_workspace_bytes(rows, c)
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=dev)
    check(L.mcdseg_bn_stats_finalize(p(part), rows, c, mp, p(mean), p(rstd), p(rm), p(rv), p(nbt), MOM, EPS, p(gamma), p(beta), p(res_bound), p(yb),
                                     updates, p(ws), ctypes.c_size_t(ws.numel() * 8), st), "bn_stats_finalize")
    torch.cuda.synchronize()
    return mean, rstd, rm, rv, nbt, yb


def _k_apply(z, mean, rstd, gamma, beta, res, relu):
    L, p, st, check = _api()
    n, c, h, w = z.shape
    y = torch.empty_like(z)
    check(L.mcdseg_bn_apply(p(z), p(mean), p(rstd), p(gamma), p(beta), p(res), p(y), n, c, h * w, int(relu), st), "bn_apply")
    return y


def _bwd_ws(shape, dev):
    L = _api()[0]
    n, c, h, w = shape
    return torch.empty(L.mcdseg_bn_bwd_workspace_bytes(n, c, h * w) // 4 + 1, device=dev)


def _k_reduce(dy, y, z, mean, rstd, gamma, relu, train, want_bound=False, y_cb=None, math_id=F16X3, want_dgamma=True):
    L, p, st, check = _api()
    n, c, h, w = dy.shape
    dev = dy.device
    dgamma = torch.empty(c, device=dev) if want_dgamma else None
    dbeta, db = torch.empty(c, device=dev), (torch.full((1,), 1e30, device=dev) if want_bound else None)
    ws = _bwd_ws(dy.shape, dev)
    check(L.mcdseg_bn_bwd_reduce(p(dy), p(y), p(y_cb), math_id, p(z), p(mean), p(rstd), p(dgamma), p(dbeta), p(gamma), p(db), int(train), n, c, h * w,
                                 int(relu), p(ws), ctypes.c_size_t(ws.numel() * 4), st), "bn_bwd_reduce")
    return dgamma, dbeta, db


def _k_reduce_zmask(dy, z, mean, rstd, gamma, beta, train, want_bound=True):
    L, p, st, check = _api()
    n, c, h, w = dy.shape
    dev = dy.device
    dgamma, dbeta, db = torch.empty(c, device=dev), torch.empty(c, device=dev), (torch.full((1,), 1e30, device=dev) if want_bound else None)
    ws = _bwd_ws(dy.shape, dev)
    check(L.mcdseg_bn_bwd_reduce_zmask(p(dy), p(z), p(mean), p(rstd), p(gamma), p(beta), p(dgamma), p(dbeta), p(db), int(train), n, c, h * w, p(ws),
                                       ctypes.c_size_t(ws.numel() * 4), st), "bn_bwd_reduce_zmask")
    return dgamma, dbeta, db


def _k_reduce_mask(dy, rmask, z, mean, rstd, gamma, train, want_bound=True):
    L, p, st, check = _api()
    n, c, h, w = dy.shape
    dev = dy.device
    dgamma, dbeta, db = torch.empty(c, device=dev), torch.empty(c, device=dev), (torch.full((1,), 1e30, device=dev) if want_bound else None)
    ws = _bwd_ws(dy.shape, dev)
    check(L.mcdseg_bn_bwd_reduce_mask(p(dy), p(rmask), p(z), p(mean), p(rstd), p(gamma), p(dgamma), p(dbeta), p(db), int(train), n, c, h * w, p(ws),
                                      ctypes.c_size_t(ws.numel() * 4), st), "bn_bwd_reduce_mask")
    return dgamma, dbeta, db


def _k_bwd_apply(dy, y, z, mean, rstd, gamma, dgamma, dbeta, relu, train, want_dres):
    L, p, st, check = _api()
    n, c, h, w = dy.shape
    dz = torch.empty_like(dy)
    dres = torch.empty_like(dy) if want_dres else None
    check(L.mcdseg_bn_bwd_apply(p(dy), p(y), p(z), p(mean), p(rstd), p(gamma), p(dgamma), p(dbeta), p(dz), p(dres), n, c, h * w, int(relu), int(train),
                                st), "bn_bwd_apply")
    return dz, dres


def _pieces(math_id):
    return 2 if math_id == F16X3 else 3


def _new_cb(t, math_id):
    return torch.empty(_pieces(math_id) * t.numel(), dtype=torch.int16, device=t.device)


def _k_apply_cb(z, mean, rstd, gamma, beta, res, relu, bound, math_id, want_y=True):
    L, p, st, check = _api()
    n, c, h, w = z.shape
    y = torch.empty_like(z) if want_y else None
    cb = _new_cb(z, math_id)
    check(L.mcdseg_bn_apply_cb(p(z), p(mean), p(rstd), p(gamma), p(beta), p(res), None, None, p(y), p(cb), p(bound) if math_id == F16X3 else None,
                               math_id, n, c, h * w, int(relu), st), "bn_apply_cb")
    return y, cb


def _k_apply_cb_mask(z, mean, rstd, gamma, beta, res, bound, math_id):
    L, p, st, check = _api()
    n, c, h, w = z.shape
    y, cb = torch.empty_like(z), _new_cb(z, math_id)
    nbytes = L.mcdseg_bn_relu_mask_bytes(n, c, h * w)
    assert nbytes == n * c * ((h * w + 255) // 256) * 32
    rmask = torch.full((nbytes // 8,), -1, dtype=torch.int64, device=z.device)
    check(L.mcdseg_bn_apply_cb_mask(p(z), p(mean), p(rstd), p(gamma), p(beta), p(res), p(y), p(cb), p(bound) if math_id == F16X3 else None, p(rmask),
                                    math_id, n, c, h * w, st), "bn_apply_cb_mask")
    return y, cb, rmask


def _k_bwd_apply_cb(dy, y, y_cb, z, mean, rstd, gamma, dgamma, dbeta, bound, math_id, relu, train, want_dz=True, want_dres=True):
    L, p, st, check = _api()
    n, c, h, w = dy.shape
    dz = torch.empty_like(dy) if want_dz else None
    dres = torch.empty_like(dy) if want_dres else None
    cb = _new_cb(dy, math_id)
    check(L.mcdseg_bn_bwd_apply_cb(p(dy), p(y), p(y_cb), p(z), p(mean), p(rstd), p(gamma), p(dgamma), p(dbeta), p(dz), p(dres), p(cb),
                                   p(bound) if math_id == F16X3 else None, math_id, n, c, h * w, int(relu), int(train), st), "bn_bwd_apply_cb")
    return dz, dres, cb


def _k_bwd_apply_cb_zmask(dy, z, mean, rstd, gamma, beta, dgamma, dbeta, bound, math_id, train):
    L, p, st, check = _api()
    n, c, h, w = dy.shape
    dz, cb = torch.empty_like(dy), _new_cb(dy, math_id)
    check(L.mcdseg_bn_bwd_apply_cb_zmask(p(dy), p(z), p(mean), p(rstd), p(gamma), p(beta), p(dgamma), p(dbeta), p(dz), p(cb),
                                         p(bound) if math_id == F16X3 else None, math_id, n, c, h * w, int(train), st), "bn_bwd_apply_cb_zmask")
    return dz, cb


def _k_bwd_apply_cb_mask(dy, rmask, z, mean, rstd, gamma, dgamma, dbeta, bound, math_id, train):
    L, p, st, check = _api()
    n, c, h, w = dy.shape
    dz, dres, cb = torch.empty_like(dy), torch.empty_like(dy), _new_cb(dy, math_id)
    check(L.mcdseg_bn_bwd_apply_cb_mask(p(dy), p(rmask), p(z), p(mean), p(rstd), p(gamma), p(dgamma), p(dbeta), p(dz), p(dres), p(cb),
                                        p(bound) if math_id == F16X3 else None, math_id, n, c, h * w, int(train), st), "bn_bwd_apply_cb_mask")
    return dz, dres, cb


def _k_unsplit(cb, bound, math_id, like):
    L, p, st, check = _api()
    n, c, h, w = like.shape
    x = torch.empty_like(like)
    check(L.mcdseg_unsplit_cb(p(cb), p(bound) if math_id == F16X3 else None, math_id, n, c, h * w, p(x), st), "unsplit_cb")
    return x


def _rows_of(case, rows, mp):
    """the fp64 data of a shape cut into ``rows`` partial rows (count, mean, M2) per channel, rounded to fp32: [rows, 3, Mp].  Rows
    beyond the data (rows > n) are empty: count 0."""
    c_ = case.shape[1]
    flat = case.z.double().permute(1, 0, 2, 3).reshape(c_, -1)
    n = flat.shape[1]
    part = torch.zeros(rows, 3, mp, dtype=torch.float64)
    for r in range(rows):
        a, b = (n * r) // rows, (n * (r + 1)) // rows
        if b > a:
            s = flat[:, a:b]
            mu = s.mean(1)
            part[r, 0, :c_], part[r, 1, :c_], part[r, 2, :c_] = b - a, mu, ((s - mu[:, None]) ** 2).sum(1)
    return part.float()


# ------------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("rows", [1, 7, 333])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_statistics_from_partial_rows(shape, rows, libopt):
    """``mcdseg_bn_stats_finalize`` through both kernel paths (``bn_stats_one_kernel``: BN_STATS_ONE at its default;
    ``bn_stats_partial_kernel`` + ``bn_stats_finalize_kernel``: BN_STATS_ONE = 0) on rows cut from the adverse data, Mp > C: mean, rstd
    and the running statistics after 1 and 3 updates against the fp64 merge of the same fp32 rows; num_batches_tracked exact; the two
    paths bit for bit."""
    dev = _dev()
    case = _case(shape)
    c_ = shape[1]
    mp = c_ + 5
    part = _rows_of(case, rows, mp)
    cnt, mu, m2 = part[:, 0, :c_], part[:, 1, :c_], part[:, 2, :c_]
    g = torch.Generator().manual_seed(77)
    rm0, rv0 = case.rm + 0.01 * torch.randn(c_, generator=g), case.rv * 0.9 + 0.05
    part_d, gam, bet = part.to(dev), case.gamma.to(dev), case.beta.to(dev)
    from mcdseg._lib import option_default
    default_one = option_default("BN_STATS_ONE")
    assert rows <= default_one, "the one-launch path would not be taken"
    for updates in (1, 3):
        ref = bn_ref.merge_rows(cnt, mu, m2, EPS, rm0, rv0, MOM, updates)
        assert float(ref["n"][0]) == case.n
        plain = _plain_merge(cnt, mu, m2, rm0, rv0, updates)
        out = {}
        for one in (0, None):
            libopt(BN_STATS_ONE=0 if one == 0 else default_one)
            out[one] = _k_stats(part_d, rows, c_, mp, dev, gam, bet, None, True, (rm0.to(dev), rv0.to(dev), torch.full((1,), 5, dtype=torch.int64, device=dev)),
                                updates, bound_init=0.0 if one == 0 else 1e30)
        names = ("mean", "rstd", "running_mean", "running_var", "num_batches_tracked", "y_bound")
        for a, b, what in zip(out[0], out[None], names):
            assert torch.equal(a, b), "%s differs between the one-launch and the two-stage statistics" % what
        for path, o in (("two-stage", out[0]), ("one-launch", out[None])):
            tag = "%s rows=%d upd=%d %s " % (_ids(shape), rows, updates, path)
            _judge(tag + "mean", o[0], plain[0], ref["mean"], per_channel=True)
            _judge(tag + "rstd", o[1], plain[1], ref["rstd"], per_channel=True)
            _judge(tag + "running_mean", o[2], plain[2], ref["running_mean"], per_channel=True)
            _judge(tag + "running_var", o[3], plain[3], ref["running_var"], per_channel=True)
            assert int(o[4]) == 5 + updates


@pytest.mark.parametrize("cin,cout", [(16, 16), (64, 128)])
def test_statistics_from_the_convolution_epilogue(cin, cout):
    """A 1x1 convolution without padding on x = randn + 1000 (N = 2, 9 x 12: z has a large mean and no border effect): its
    ``stat_partials`` through ``mcdseg_bn_stats_finalize`` against the fp64 statistics of the fp64 convolution -- the check that the
    per-wave shifted sums of the epilogue really are centred.  Budget: the fp32 convolution followed by the plain fp32 statistics.
    (The convolution is launched the way tests/test_kernels_gpu.py launches it, through ``ops.PackedWeights`` and ``ops._conv_fprop`` --
    helpers of mcdseg/ops.py, not the C ABI, so a refactor there has to carry this test along; ``pk.w_bound`` is the scalar the weight pack
    measured, None outside the f16 arithmetics.)"""
    dev = _dev()
    from mcdseg import ops
    g = torch.Generator().manual_seed(90 + cin)
    x = torch.randn(2, cin, 9, 12, generator=g) + 1000.0
    wt = torch.randn(cout, cin, 1, 1, generator=g) * (2.0 / cout) ** 0.5
    desc = ops.conv_desc(x.shape, wt.shape, 1, 0, 1)
    pk = ops.PackedWeights()
    wf, _, mpf = pk.get(wt.to(dev), desc, need_dgrad=False)
    z, part, rows = ops._conv_fprop(desc, x.to(dev), wf, None, True, mpf, None, None, pk.w_bound)
    mean, rstd = _k_stats(part, rows, cout, mpf, dev)[:2]
    st = bn_ref.batch_stats(F.conv2d(x.double(), wt.double()))
    pm, pr, _ = _plain_stats(F.conv2d(x, wt))
    # (what the statistics kernels add to the convolution's own arithmetic: against the fp64 statistics of the z the kernel wrote)
    own = bn_ref.batch_stats(z.cpu())
    print("BNFIG conv %dto%d vs the fp64 statistics of the kernel's own z: mean %.3e rstd %.3e (rel)" % (
        cin, cout, float((mean.cpu().double() - own["mean"]).abs().max()), float(((rstd.cpu().double() - own["rstd"]) / own["rstd"]).abs().max())))
    _judge("conv %dto%d epilogue mean" % (cin, cout), mean, pm, st["mean"])
    _judge("conv %dto%d epilogue rstd" % (cin, cout), rstd, pr, st["rstd"])


def test_eval_statistics_and_affine_map():
    """``mcdseg_bn_eval_stats`` / ``mcdseg_bn_eval_affine`` at adverse running statistics (|mean|/std to 1e3, running_var = 0)"""
    dev = _dev()
    L, p, st, check = _api()
    case = _case(SHAPES[3])
    c_ = case.shape[1]
    g = torch.Generator().manual_seed(8)
    bias = torch.randn(c_, generator=g)
    rm, rv, gam, bet = case.rm, case.rv, case.gamma, case.beta
    mean, rstd, scale, shift = (torch.empty(c_, device=dev) for _ in range(4))
    rmd, rvd, gd, bd, biasd = (t.to(dev) for t in (rm, rv, gam, bet, bias))   # (held: a kernel argument must outlive the call)
    check(L.mcdseg_bn_eval_stats(p(rmd), p(rvd), c_, EPS, p(mean), p(rstd), st), "bn_eval_stats")
    assert torch.equal(mean.cpu(), rm)
    _judge("eval_stats rstd", rstd, 1.0 / torch.sqrt(rv + EPS), bn_ref.eval_stats(rm, rv)[1], per_channel=True)
    for cb in (None, bias):
        check(L.mcdseg_bn_eval_affine(p(gd), p(bd), p(rmd), p(rvd), p(biasd) if cb is not None else None, c_, EPS, p(scale), p(shift), st),
              "bn_eval_affine")
        ref = bn_ref.eval_affine(gam, bet, rm, rv, cb)
        ps = gam / torch.sqrt(rv + EPS)
        _judge("eval_affine scale", scale, ps, ref[0])
        _judge("eval_affine shift", shift, bet + ((cb if cb is not None else 0.0) - rm) * ps, ref[1])


# ------------------------------------------------------------------------------------------------ forward / backward against fp64
# train / eval x ReLU x residual, all eight at every shape -- the 33.6 MB one included: its second trip of the reduce loop exists in every
# MASK instantiation, and relu = 0 is the only way to MASK == 0
COMBOS = [(t, r, u) for t in (True, False) for r in (False, True) for u in (False, True)]


@pytest.mark.parametrize("shape,train,relu,use_res", [(s,) + cmb for s in SHAPES for cmb in COMBOS],
                         ids=lambda v: _ids(v) if isinstance(v, tuple) else str(int(v)))
def test_apply_reduce_and_backward_apply_against_fp64(shape, train, relu, use_res):
    """``mcdseg_bn_apply``, ``mcdseg_bn_bwd_reduce`` (also with z == NULL: dbeta alone) and ``mcdseg_bn_bwd_apply``: y, dgamma, dbeta,
    dz and dres against tests/bn_ref.py.  The ReLU mask handed to the reference is the kernel's own ``y > 0``; it is asserted
    separately: with a residual that is minus the kernel's own no-residual output on every 7th pixel (y must be exactly +0 there, the
    mask false, dres 0), and -0.0 on the gamma = beta = 0 channels.

    The eval-mode cases are the ones that decide the forward map: there the statistics are exact inputs, and fma(z, a, beta - mean a)
    alone was 2.0e-05 .. 8.4e-05 off at the four small shapes for budgets of 7.2e-06 .. 4.2e-05 (csrc/bn.hip, bn_forward_map;
    docs/MEASURED_HISTORY.md)."""
    dev = _dev()
    case = _case(shape)
    tag = "%s %s relu=%d res=%d " % (_ids(shape), "train" if train else "eval", relu, use_res)
    z, gam, bet, dy = case.z, case.gamma, case.beta, case.dy
    if train:
        mean64, rstd64 = case.stats["mean"], case.stats["rstd"]
        mean32, rstd32 = case.mean, case.rstd
        pmean, prstd, _ = _plain_stats(z)
    else:
        mean64, rstd64 = bn_ref.eval_stats(case.rm, case.rv)
        mean32, rstd32 = case.rm, rstd64.float()
        pmean, prstd = case.rm, 1.0 / torch.sqrt(case.rv + EPS)
    zd, gd, bd, dyd, md, rd = (t.to(dev) for t in (z, gam, bet, dy, mean32, rstd32))
    res, zero_set = None, None
    if use_res:
        y0 = _k_apply(zd, md, rd, gd, bd, None, False).cpu()
        res = case.res.clone()
        zero_set = (torch.arange(z.numel()).view(z.shape) % 7) == 3
        res[zero_set] = -y0[zero_set]
        for c, k in enumerate(case.kinds):
            if k == "zero":
                res[:, c] = -0.0
                zero_set[:, c] = True
    resd = res.to(dev) if use_res else None
    y = _k_apply(zd, md, rd, gd, bd, resd, relu)
    yc = y.cpu()
    if use_res:
        assert bool((yc[zero_set] == 0).all()), "y is exactly zero where the residual cancels the kernel's own BatchNorm output"
    _judge(tag + "y", y, _plain_forward(z, pmean, prstd, gam, bet, res, relu), bn_ref.forward(z, mean64, rstd64, gam, bet, res, relu))
    mask = (yc > 0) if relu else None
    if relu and use_res:
        assert not bool(mask[zero_set].any())
    if relu and not use_res:
        for c, k in enumerate(case.kinds):
            if k in ("dead", "zero"):
                assert not bool(mask[:, c].any()), "ReLU kills the whole %s channel" % k
    dgamma, dbeta, _ = _k_reduce(dyd, y if relu else None, zd, md, rd, gd, relu, train)
    rg, rb, dz64, dres64 = bn_ref.backward(dy, z, mean64, rstd64, gam, mask, train)
    pg, pb, pdz = _plain_backward(dy, z, pmean, prstd, gam, mask, train)
    _judge(tag + "dgamma", dgamma, pg, rg)
    _judge(tag + "dbeta", dbeta, pb, rb)
    _, dbeta_only, _ = _k_reduce(dyd, y if relu else None, None, None, None, None, relu, train, want_dgamma=False)
    _judge(tag + "dbeta (z == NULL)", dbeta_only, pb, rb)
    dz, dres = _k_bwd_apply(dyd, y if relu else None, zd, md, rd, gd, dgamma, dbeta, relu, train, use_res)
    _judge(tag + "dz", dz, pdz, dz64)
    if use_res:
        assert torch.equal(dres.cpu().double(), dres64), "dres is dy under the mask y > 0: exact"
        if relu:
            assert bool((dres.cpu()[zero_set] == 0).all())


SWITCH_RATIOS = (0.0, 7.9, 8.0, 8.1, -7.9, -8.1, 7.999, 16.0)   # mean rstd per channel, around BN_CENTRE_RATIO = 8 of csrc/bn.hip


def _switch_case():
    """statistics handed over as exact inputs (as in eval mode), rstd = 1: channel c has mean rstd = SWITCH_RATIOS[c]"""
    g = torch.Generator().manual_seed(808)
    shape = (2, 8, 12, 21)
    mean = torch.tensor(SWITCH_RATIOS)
    rstd = torch.ones(8)
    z = torch.randn(shape, generator=g) + _cv(mean)
    gamma = (0.75 + 0.5 * torch.rand(8, generator=g)) * torch.tensor([1.0, 1.0, -1.0, 1.0, -1.0, 1.0, 1.0, -1.0])
    beta = 0.2 * torch.randn(8, generator=g)
    dy = torch.randn(shape, generator=g)
    return z, mean, rstd, gamma, beta, dy


def test_forward_map_on_both_sides_of_its_ratio_threshold():
    """``bn_forward_map`` (csrc/bn.hip) subtracts the mean first in a channel whose |mean| rstd exceeds 8: channels just below, at and
    just above that ratio, of both signs, against fp64 -- and the kernels that recompute ``y > 0`` from z still agree with the stored y
    bit for bit on both sides."""
    dev = _dev()
    z, mean, rstd, gam, bet, dy = _switch_case()
    zd, md, rd, gd, bd, dyd = (t.to(dev) for t in (z, mean, rstd, gam, bet, dy))
    for relu in (False, True):
        y = _k_apply(zd, md, rd, gd, bd, None, relu)
        _judge("ratio threshold relu=%d y" % relu, y, _plain_forward(z, mean, rstd, gam, bet, None, relu), bn_ref.forward(z, mean, rstd, gam, bet, None, relu))
    yb = torch.tensor([float(y.abs().max()) * 1.5], device=dev)
    for math_id in (F16X3, BF16X6):
        y_cb, _ = _k_apply_cb(zd, md, rd, gd, bd, None, True, yb, math_id)
        assert torch.equal(y_cb, y)
    dgamma, dbeta, db = _k_reduce(dyd, y, zd, md, rd, gd, True, True, want_bound=True)
    zg, zb_, zdb = _k_reduce_zmask(dyd, zd, md, rd, gd, bd, True)
    assert torch.equal(zg, dgamma) and torch.equal(zb_, dbeta) and torch.equal(zdb, db), "reduce_zmask"
    dz, _ = _k_bwd_apply(dyd, y, zd, md, rd, gd, dgamma, dbeta, True, True, False)
    dz1, _ = _k_bwd_apply_cb_zmask(dyd, zd, md, rd, gd, bd, dgamma, dbeta, db, F16X3, True)
    assert torch.equal(dz1, dz), "bwd_apply_cb_zmask"


# ------------------------------------------------------------------------------------------------ variants, bit for bit
def _bit_plane(y):
    """the header's layout: per (image, channel) and block of 256 pixels four 64-bit words, bit l of word j = (y > 0) of pixel
    256 blk + 4 l + j; pixels past the end of the plane: 0"""
    n, c, h, w = y.shape
    hw = h * w
    nblk = (hw + 255) // 256
    bits = np.zeros((n, c, nblk * 256), dtype=np.uint64)
    bits[:, :, :hw] = (y.reshape(n, c, hw) > 0).cpu().numpy()
    bits = bits.reshape(n, c, nblk, 64, 4)                                                   # [.., l, j]
    words = (bits << np.arange(64, dtype=np.uint64)[None, None, None, :, None]).sum(axis=3, dtype=np.uint64)   # [n, c, nblk, j]
    return torch.from_numpy(words.view(np.int64).reshape(-1))


@pytest.mark.parametrize("shape,math_id", [(s, m) for s in CB_SHAPES for m in (F16X3, BF16X6)],
                         ids=lambda v: _ids(v) if isinstance(v, tuple) else {F16X3: "f16x3", BF16X6: "bf16x6"}[v])
def test_variants_are_bitwise_the_base_entry_points(shape, math_id, libopt):
    """``mcdseg_bn_apply_cb`` (also y == NULL; four-pixel and one-pixel kernels), ``mcdseg_bn_apply_cb_mask``, the ``_zmask`` and
    ``_mask`` reduce / apply pairs, ``mcdseg_bn_bwd_apply_cb`` (fp32 y; y == NULL with y_cb) on the adverse data, in both arithmetics:
    their fp32 outputs are bit for bit those of ``mcdseg_bn_apply`` / ``mcdseg_bn_bwd_reduce`` / ``mcdseg_bn_bwd_apply``, and the
    bit-plane is ``y > 0`` of the stored y, word for word, the ragged last block included."""
    dev = _dev()
    case = _case(shape)
    zd, gd, bd, dyd, md, rd = (t.to(dev) for t in (case.z, case.gamma, case.beta, case.dy, case.mean, case.rstd))
    resd = case.res.to(dev)
    n = case.n
    yb = torch.tensor([bn_ref.y_bound(case.gamma, case.beta, n, float(case.res.abs().max())) * 1.0001], device=dev)
    # a group WITHOUT residual: base, _cb (y and y == NULL, both kernels), mask from z
    y = _k_apply(zd, md, rd, gd, bd, None, True)
    for v4 in (1, 0):
        libopt(BN_V4=v4)
        y_cb, cb = _k_apply_cb(zd, md, rd, gd, bd, None, True, yb, math_id)
        _, cb2 = _k_apply_cb(zd, md, rd, gd, bd, None, True, yb, math_id, want_y=False)
        assert torch.equal(y_cb, y) and torch.equal(cb, cb2), "apply_cb (BN_V4=%d)" % v4
    dgamma, dbeta, db = _k_reduce(dyd, y, zd, md, rd, gd, True, True, want_bound=True)
    zg, zb_, zdb = _k_reduce_zmask(dyd, zd, md, rd, gd, bd, True)
    assert torch.equal(zg, dgamma) and torch.equal(zb_, dbeta) and torch.equal(zdb, db), "reduce_zmask"
    dz, _ = _k_bwd_apply(dyd, y, zd, md, rd, gd, dgamma, dbeta, True, True, False)
    for v4 in (1, 0):
        libopt(BN_V4=v4)
        dz1, cbz = _k_bwd_apply_cb_zmask(dyd, zd, md, rd, gd, bd, dgamma, dbeta, db, math_id, True)
        dz2, dres2, cby = _k_bwd_apply_cb(dyd, y, None, zd, md, rd, gd, dgamma, dbeta, db, math_id, True, True)
        dz3, dres3, cbc = _k_bwd_apply_cb(dyd, None, cb, zd, md, rd, gd, dgamma, dbeta, db, math_id, True, True)
        _, _, cbn = _k_bwd_apply_cb(dyd, y, None, zd, md, rd, gd, dgamma, dbeta, db, math_id, True, True, want_dz=False, want_dres=False)
        assert torch.equal(dz1, dz) and torch.equal(dz2, dz) and torch.equal(dz3, dz), "backward apply variants (BN_V4=%d)" % v4
        assert torch.equal(dres2, torch.where(y > 0, dyd, torch.zeros_like(dyd))) and torch.equal(dres3, dres2)
        assert torch.equal(cbz, cby) and torch.equal(cbc, cby) and torch.equal(cbn, cby), "dz companions (BN_V4=%d)" % v4
    libopt(BN_V4=1)
    # the reduce that reads the mask from the companion sums in another order: against fp64
    cg, cbeta, cdb = _k_reduce(dyd, None, zd, md, rd, gd, True, True, want_bound=True, y_cb=cb, math_id=math_id)
    mask = (y > 0).cpu()
    rg, rb, _, _ = bn_ref.backward(case.dy, case.z, case.stats["mean"], case.stats["rstd"], case.gamma, mask, True)
    pg, pb, _ = _plain_backward(case.dy, case.z, *_plain_stats(case.z)[:2], case.gamma, mask, True)
    tag = "%s %s reduce(y_cb) " % (_ids(shape), "f16x3" if math_id == F16X3 else "bf16x6")
    _judge(tag + "dgamma", cg, pg, rg)
    _judge(tag + "dbeta", cbeta, pb, rb)
    # a group WITH residual: base, bit-plane forms
    yr = _k_apply(zd, md, rd, gd, bd, resd, True)
    ym, cbm, rmask = _k_apply_cb_mask(zd, md, rd, gd, bd, resd, yb, math_id)
    yr_cb, cbr = _k_apply_cb(zd, md, rd, gd, bd, resd, True, yb, math_id)
    assert torch.equal(ym, yr) and torch.equal(yr_cb, yr) and torch.equal(cbm, cbr), "apply_cb_mask"
    assert torch.equal(rmask.cpu(), _bit_plane(yr)), "the bit-plane is not y > 0 of the stored y in the header's layout"
    for train in (True, False):
        dgamma, dbeta, db = _k_reduce(dyd, yr, zd, md, rd, gd, True, train, want_bound=True)
        mg, mb, mdb = _k_reduce_mask(dyd, rmask, zd, md, rd, gd, train)
        assert torch.equal(mg, dgamma) and torch.equal(mb, dbeta) and torch.equal(mdb, db), "reduce_mask (train=%d)" % train
        dz, dres = _k_bwd_apply(dyd, yr, zd, md, rd, gd, dgamma, dbeta, True, train, True)
        dzm, dresm, cb_m = _k_bwd_apply_cb_mask(dyd, rmask, zd, md, rd, gd, dgamma, dbeta, db, math_id, train)
        dzy, dresy, cb_y = _k_bwd_apply_cb(dyd, yr, None, zd, md, rd, gd, dgamma, dbeta, db, math_id, True, train)
        assert torch.equal(dzm, dz) and torch.equal(dresm, dres) and torch.equal(dzy, dz) and torch.equal(dresy, dres), "apply_cb_mask (train=%d)" % train
        assert torch.equal(cb_m, cb_y)


# ------------------------------------------------------------------------------------------------ the bound contract
def _check_bound(tag, bound, formula, tensor, cb, like, margin=True):
    """(1) bound >= max|tensor| as the kernel wrote it; (2) formula <= bound <= formula (1 + 1e-3) -- the kernels carry a 1.0001 margin,
    test_conv_large_tile_kernels allows 1e-3; (3) the F16X3 companion written with the bound is finite and ``mcdseg_unsplit_cb`` of it
    returns the fp32 tensor to within 2^-22 bound (the header's 22 leading bits)"""
    b = float(bound)
    top = float(tensor.abs().max())
    print("BNFIG %-58s bound %.6e  formula %.6e  max|tensor| %.6e" % (tag, b, formula, top))
    assert math.isfinite(b) and b >= top, "%s: bound %.6e below max|tensor| %.6e" % (tag, b, top)
    if margin:
        assert formula <= b <= formula * (1.0 + 1e-3), "%s: bound %.6e outside [formula, formula (1 + 1e-3)], formula %.6e" % (tag, b, formula)
    if cb is not None:
        assert bool(torch.isfinite(cb.view(torch.float16)).all()), "%s: a companion piece is not finite" % tag
        back = _k_unsplit(cb, bound, F16X3, like)
        err = float((back.double() - tensor.double()).abs().max())
        print("BNFIG %-58s unsplit error %.3e  allowed %.3e" % (tag, err, 2.0 ** -22 * b))
        assert err <= 2.0 ** -22 * b, "%s: the companion loses more than 22 bits: %.3e > %.3e" % (tag, err, 2.0 ** -22 * b)


def _kernel_stats(case, dev, one, use_res, updates=1, rows=7):
    """mean, rstd and y_bound as ``mcdseg_bn_stats_finalize`` writes them from rows of the data"""
    c_ = case.shape[1]
    part = _rows_of(case, rows, c_ + 5).to(dev)
    resb = torch.tensor([float(case.res.abs().max())], device=dev) if use_res else None
    running = (case.rm.to(dev), case.rv.to(dev), torch.zeros(1, dtype=torch.int64, device=dev))
    mean, rstd, _, _, _, yb = _k_stats(part, rows, c_, c_ + 5, dev, case.gamma.to(dev), case.beta.to(dev), resb, True, running, updates,
                                       bound_init=0.0 if one == 0 else 1e30)
    return mean, rstd, yb


# (relu with residual + res_bound, running_updates, BN_STATS_ONE) at every shape.  (2, 5, 3, 7) has no companion (C % 8 != 0): there y comes
# from mcdseg_bn_apply and checks 1 and 2 run alone -- C = 5 leaves a ragged block in the one-wave-per-channel kernels that feed the maximum
Y_CASES = [(s, r, u, one) for s in SHAPES for (r, u) in ((False, 1), (True, 3)) for one in (0, 1024)]


@pytest.mark.parametrize("shape,relu,updates,one", Y_CASES, ids=lambda v: _ids(v) if isinstance(v, tuple) else str(int(v)))
def test_y_bound_contract(shape, relu, updates, one, libopt):
    """``y_bound`` of ``mcdseg_bn_stats_finalize`` (both kernel paths; with res_bound and running_updates = 3) against the y that
    ``mcdseg_bn_apply_cb`` (``mcdseg_bn_apply`` where the shape has no companion) then writes from the same statistics -- the
    Samuelson-tight channel decides the bound"""
    dev = _dev()
    use_res = relu
    libopt(BN_STATS_ONE=one)
    case = _case(shape)
    mean, rstd, yb = _kernel_stats(case, dev, one, use_res, updates)
    zd, gd, bd = case.z.to(dev), case.gamma.to(dev), case.beta.to(dev)
    resd = case.res.to(dev) if use_res else None
    if shape in CB_SHAPES:
        y, cb = _k_apply_cb(zd, mean, rstd, gd, bd, resd, relu, yb, F16X3)
    else:
        y, cb = _k_apply(zd, mean, rstd, gd, bd, resd, relu), None
    formula = bn_ref.y_bound(case.gamma, case.beta, case.n, float(case.res.abs().max()) if use_res else 0.0)
    tag = "%s y_bound %s relu=%d res=%d" % (_ids(shape), "two-stage" if one == 0 else "one-launch", relu, use_res)
    _check_bound(tag, yb, formula, y, cb, zd)
    if not use_res and not relu:  # the tight channel reaches the bound without its margin: the data does what the docstring says
        c = case.kinds.index("tight")
        assert float(y[:, c].abs().max()) >= 0.9999 * formula


DZ_ENTRIES = ["reduce", "reduce_cb", "reduce_zmask", "reduce_mask"]


@pytest.mark.parametrize("shape,entry,train", [(s, e, t) for s in CB_SHAPES for e in DZ_ENTRIES for t in (True, False)],
                         ids=lambda v: _ids(v) if isinstance(v, tuple) else (v if isinstance(v, str) else ("train" if v else "eval")))
def test_dz_bound_contract(shape, entry, train):
    """``dz_bound`` of the four fp32 entry points in front of ``bn_bwd_finalize_kernel`` against the dz the matching apply kernel then
    writes.  Eval mode has no margin: >= only."""
    dev = _dev()
    case = _case(shape)
    zd, gd, bd, dyd, md, rd = (t.to(dev) for t in (case.z, case.gamma, case.beta, case.dy, case.mean, case.rstd))
    yb = torch.tensor([bn_ref.y_bound(case.gamma, case.beta, case.n, float(case.res.abs().max())) * 1.0001], device=dev)
    if entry == "reduce_mask":
        y, y_cb, rmask = _k_apply_cb_mask(zd, md, rd, gd, bd, case.res.to(dev), yb, F16X3)
        dgamma, dbeta, db = _k_reduce_mask(dyd, rmask, zd, md, rd, gd, train)
        dz, _, cb = _k_bwd_apply_cb_mask(dyd, rmask, zd, md, rd, gd, dgamma, dbeta, db, F16X3, train)
    elif entry == "reduce_zmask":
        y = _k_apply(zd, md, rd, gd, bd, None, True)
        dgamma, dbeta, db = _k_reduce_zmask(dyd, zd, md, rd, gd, bd, train)
        dz, cb = _k_bwd_apply_cb_zmask(dyd, zd, md, rd, gd, bd, dgamma, dbeta, db, F16X3, train)
    elif entry == "reduce_cb":
        y, y_cb = _k_apply_cb(zd, md, rd, gd, bd, None, True, yb, F16X3)
        dgamma, dbeta, db = _k_reduce(dyd, None, zd, md, rd, gd, True, train, want_bound=True, y_cb=y_cb)
        dz, _, cb = _k_bwd_apply_cb(dyd, None, y_cb, zd, md, rd, gd, dgamma, dbeta, db, F16X3, True, train)
    else:
        y = _k_apply(zd, md, rd, gd, bd, None, True)
        dgamma, dbeta, db = _k_reduce(dyd, y, zd, md, rd, gd, True, train, want_bound=True)
        dz, _, cb = _k_bwd_apply_cb(dyd, y, None, zd, md, rd, gd, dgamma, dbeta, db, F16X3, True, train)
    mask = (y > 0).cpu()
    rg, rb, g_m = bn_ref.backward_reduce(case.dy, case.z, case.mean, case.rstd, mask)
    formula = bn_ref.dz_bound(case.gamma, case.rstd, g_m, rg, rb, train)
    _check_bound("%s dz_bound %s %s" % (_ids(shape), entry, "train" if train else "eval"), db, formula, dz, cb, zd, margin=train)


def _half_inputs(case, dev):
    """16-bit images of the adverse data as the 2-byte chain holds them (the helpers of tests/test_half_storage_gpu.py), what they
    decode to in fp64, and the fp64 statistics of that z rounded to fp32"""
    from test_half_storage_gpu import _nchw_to_units, _scale, _units_to_nchw
    n_, c_, h, w = case.shape
    z_bound = (case.z.abs().max() * 37.0).reshape(1)
    zs = _scale(z_bound)
    z16 = _nchw_to_units((case.z / zs).to(torch.float16))
    zq = _units_to_nchw(z16, n_, c_, h, w).double() * zs
    dy16 = _nchw_to_units(case.dy.to(torch.bfloat16))
    dyq = _units_to_nchw(dy16, n_, c_, h, w).double()
    stq = bn_ref.batch_stats(zq)
    mean, rstd = stq["mean"].float(), stq["rstd"].float()
    y_ref = bn_ref.forward(zq, mean, rstd, case.gamma, case.beta, case.res, True)
    ys = _scale(bn_ref.y_bound(case.gamma, case.beta, case.n, float(case.res.abs().max())))
    y16 = (y_ref / ys).to(torch.float16)
    d = types.SimpleNamespace(zq=zq, dyq=dyq, mean=mean, rstd=rstd, y16=y16)
    d.dev = [t.to(dev) for t in (dy16, _nchw_to_units(y16), z16, z_bound)]   # (held: a kernel argument must outlive the call)
    return d


def _k_reduce_half(h, shape, mean, rstd, gamma, beta, kind, train):
    L, p, st, check = _api()
    n_, c_, hh, w = shape
    dev = mean.device
    dy16d, y16d, z16d, zbd = h.dev
    dgamma, dbeta, db = torch.empty(c_, device=dev), torch.empty(c_, device=dev), torch.full((1,), 1e30, device=dev)
    ws = torch.empty(L.mcdseg_bn_bwd_half_workspace_bytes(n_, c_, hh * w) // 4 + 1, device=dev)
    check(L.mcdseg_bn_bwd_reduce_half(p(dy16d), p(y16d) if kind == 4 else None, p(z16d), p(zbd), p(mean), p(rstd), p(gamma), p(beta), p(dgamma), p(dbeta),
                                      p(db), kind, int(train), n_, c_, hh * w, p(ws), ctypes.c_size_t(ws.numel() * 4), st), "bn_bwd_reduce_half")
    return dgamma, dbeta, db


@pytest.mark.parametrize("kind", [0, 4], ids=["linear", "mask-from-y_cb"])
@pytest.mark.parametrize("shape", CB_SHAPES, ids=_ids)
def test_dz_bound_contract_of_the_half_reduce(shape, kind):
    """``mcdseg_bn_bwd_reduce_half`` on 16-bit images of the adverse data: its dz_bound against the dz the fp64 reference computes from
    the same 16-bit inputs, and against the header's formula.  Eval mode has no margin, and the bound is the fp32 product
    fl(fl(gamma rstd) max|dy_m|) the apply kernel's own dz = fl(fl(gamma rstd) dy_m) cannot exceed: there the reference product is rounded
    the same way, and the kernel's value is compared as it is."""
    dev = _dev()
    case = _case(shape)
    h = _half_inputs(case, dev)
    mean, rstd = h.mean, h.rstd
    mask = (h.y16 > 0) if kind == 4 else None
    md, rd, gd, bd = (t.to(dev) for t in (mean, rstd, case.gamma, case.beta))
    for train in (True, False):
        dgamma, dbeta, db = _k_reduce_half(h, shape, md, rd, gd, bd, kind, train)
        rg, rb, dz64, g_m = bn_ref.backward(h.dyq, h.zq, mean, rstd, case.gamma, mask, train)
        pg, pb, _ = _plain_backward(h.dyq.float(), h.zq.float(), mean, rstd, case.gamma, mask, train)
        tag = "%s half kind=%d %s " % (_ids(shape), kind, "train" if train else "eval")
        _judge(tag + "dgamma", dgamma, pg, rg)
        _judge(tag + "dbeta", dbeta, pb, rb)
        formula = bn_ref.dz_bound(case.gamma, rstd, g_m, rg, rb, train)
        dz = dz64 if train else _cv(case.gamma * rstd) * g_m.float()   # (dy_m is a bf16 value: exact in fp32)
        _check_bound(tag + "dz_bound", db, formula, dz, None, None, margin=train)


def test_nan_parameters_or_statistics_give_a_non_finite_bound(libopt):
    """every entry point that writes a bound: a NaN in gamma, beta or rstd must show in it"""
    dev = _dev()
    case = _case(SHAPES[3])
    c_ = case.shape[1]
    zd, gd, bd, dyd, md, rd = (t.to(dev) for t in (case.z, case.gamma, case.beta, case.dy, case.mean, case.rstd))
    part = _rows_of(case, 7, c_ + 5).to(dev)
    bad_gamma = gd.clone()
    bad_gamma[c_ - 3] = float("nan")
    for one in (0, 1024):
        libopt(BN_STATS_ONE=one)
        for gam, bet in ((bad_gamma, bd), (gd, bad_gamma)):
            yb = _k_stats(part, 7, c_, c_ + 5, dev, gam, bet, None, True)[5]
            assert not math.isfinite(float(yb)), "y_bound is finite with a NaN parameter (BN_STATS_ONE=%d)" % one
    y = _k_apply(zd, md, rd, gd, bd, None, True)
    yb = torch.tensor([bn_ref.y_bound(case.gamma, case.beta, case.n, float(case.res.abs().max())) * 1.0001], device=dev)
    _, y_cb = _k_apply_cb(zd, md, rd, gd, bd, None, True, yb, F16X3)
    _, _, rmask = _k_apply_cb_mask(zd, md, rd, gd, bd, case.res.to(dev), yb, F16X3)
    half = _half_inputs(case, dev)
    bad_rstd = rd.clone()
    bad_rstd[5] = float("nan")
    for gam, rs in ((bad_gamma, rd), (gd, bad_rstd)):
        for train in (True, False):
            assert not math.isfinite(float(_k_reduce(dyd, y, zd, md, rs, gam, True, train, want_bound=True)[2])), "reduce"
            assert not math.isfinite(float(_k_reduce_zmask(dyd, zd, md, rs, gam, bd, train)[2])), "reduce_zmask"
            assert not math.isfinite(float(_k_reduce(dyd, None, zd, md, rs, gam, True, train, want_bound=True, y_cb=y_cb)[2])), "reduce (y_cb)"
            assert not math.isfinite(float(_k_reduce_mask(dyd, rmask, zd, md, rs, gam, train)[2])), "reduce_mask"
            for kind in (0, 4):
                assert not math.isfinite(float(_k_reduce_half(half, case.shape, md, rs, gam, bd, kind, train)[2])), "reduce_half"
