"""GPU: the data-parallel loss contract on UNEQUAL shards, one process playing the ranks ("virtual ranks": ``wsum=`` is passed
explicitly, no process group) -- ``ops.label_weight_sum`` against exact arithmetic, every fused loss entry called once per shard with
``W_global / world`` against its own whole-batch call and against the fp64 statement of tests/dp_shard_ref.py, the shard that holds no
valid pixel, and ``grad_scale`` with the long loops of the two update kernels.  tests/test_dp_shard_ref_host.py proves on the statement
alone that a rank-local normaliser lies at least 100 bars away on every label layout used here."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import dp_shard_ref as ref
from test_adam_gpu import FACTOR
from test_adam_gpu import HYPER as ADAM
from test_fusion_kernels_gpu import _offset, _Truth
from test_prob_distance_gpu import GRAD_RTOL, VAL_RTOL

pytestmark = pytest.mark.gpu

L1_RTOL = 2e-6           # test_kernels_gpu.test_loss_kernel_edge_cases: the L1 / cross-entropy kernels' gradients
FLT_MIN = 2.0 ** -126


# ------------------------------------------------------------------------------------------------------------ a. label_weight_sum
def _junk_labels(p, c, ignore_index, g):
    """int64 [p]: valid classes and, for about a quarter of the pixels, -1, C, C + 1 and ``ignore_index``"""
    y = torch.randint(0, c, (p,), generator=g)
    junk = torch.tensor([-1, c, c + 1, ignore_index])
    bad = torch.rand(p, generator=g) < 0.25
    y = torch.where(bad, junk[torch.randint(0, 4, (p,), generator=g)], y)
    if p > 4:  # each of them at least once where there is room
        for k, v in enumerate(junk.tolist()):
            y[(k * 977) % p] = v
    return y


def _exact_sum(y, cw64, c, ignore_index):
    y = y.numpy()
    ok = (y != ignore_index) & (y >= 0) & (y < c)
    return float(ok.sum()) if cw64 is None else float(cw64[y[ok]].sum())


@pytest.mark.parametrize("p", [1, 255, 256, 257, 2048, 2049, 4097, 1024 * 2048 + 257])
def test_label_weight_sum_is_exact_on_dyadic_weights(device, p):
    """weights k/256, 0 <= k <= 512: every fp32 partial of ``label_wsum_kernel`` is exact (a thread adds at most 9 terms, a block's
    partial stays below 2304 * 2 < 2^14 at a resolution of 2^-8: 22 bits), the finalize kernel sums the partials in fp64, so the
    result is the correctly rounded exact sum.  1024 * 2048 + 257 is the first size past the 1024-block cap (threads take a 9th term)."""
    from mcdseg import ops
    for c in (1, 3, 41, 48):
        for ignore_index in (-100, 255):
            g = torch.Generator().manual_seed(p % 100003 + 11 * c + (ignore_index & 1))
            y = _junk_labels(p, c, ignore_index, g)
            k = torch.randint(0, 513, (c,), generator=g)
            cw64 = k.double().numpy() / 256.0
            yd = y.to(device)
            for cw in (torch.from_numpy(cw64).float(), None):
                want = np.float32(_exact_sum(y, None if cw is None else cw64, c, ignore_index))
                got = ops.label_weight_sum(yd, None if cw is None else cw.to(device), c, ignore_index)
                assert got.shape == (1,) and got.dtype == torch.float32
                assert np.float32(got.item()) == want, (p, c, ignore_index, cw is None, got.item(), float(want))


def test_label_weight_sum_on_arbitrary_weights(device):
    """P = 300 000, fp32 weights in [0.5, 1.5): 147 blocks of 256 threads, each thread adds ceil(300000 / 37632) = 8 terms, then 6
    butterfly steps of the wave sum and 2 additions of the four wave partials -- a value passes through at most 8 + 6 + 2 = 16 fp32
    additions (the first of them, onto 0, is exact, which pays for the one final rounding of the fp64 total to fp32).  All terms are
    non-negative, so the relative error of the sum is at most 16 * 2^-24."""
    from mcdseg import ops
    p, c = 300000, 41
    blocks = min(1024, -(-p // 2048))
    terms = -(-p // (blocks * 256))
    assert (blocks, terms) == (147, 8)
    bound = (terms + 6 + 2) * 2.0 ** -24
    g = torch.Generator().manual_seed(9)
    y = _junk_labels(p, c, 255, g)
    cw = 0.5 + torch.rand(c, generator=g)
    want = _exact_sum(y, cw.double().numpy(), c, 255)
    got = float(ops.label_weight_sum(y.to(device), cw.to(device), c, 255))
    print("label_weight_sum P=300000: %.9e vs %.9e, rel %.2e (bound %.2e)" % (got, want, abs(got - want) / want, bound))
    assert abs(got - want) <= bound * want
    # as [N, H, W] labels, the shape the callers pass
    got3 = ops.label_weight_sum(y.view(5, 200, 300).to(device), cw.to(device), c, 255)
    assert float(got3) == got


def test_label_weight_sum_of_nothing_and_bad_arguments(device):
    from mcdseg import ops
    from mcdseg._lib import check, lib
    for p in (1, 257, 4097):
        y = torch.tensor([-100, -1, 3, 4, 2])[torch.arange(p) % 5]     # ignored, negative, >= C, and a class of weight 0
        cw = torch.tensor([1.0, 0.5, 0.0])
        assert float(ops.label_weight_sum(y.to(device), cw.to(device), 3, -100)) == 0.0
    y = torch.zeros(300, dtype=torch.int64, device=device)
    cw = torch.ones(3, device=device)
    with pytest.raises(RuntimeError, match="label_weight_sum: bad arguments"):
        ops.label_weight_sum(y, cw, 0)
    with pytest.raises(RuntimeError, match="label_weight_sum: bad arguments"):
        ops.label_weight_sum(y[:0], cw, 3)
    L = lib()
    out = torch.full((1,), -7.0, device=device)
    need = L.mcdseg_label_weight_sum_workspace_bytes(4097)
    assert need == 3 * 4
    ws = torch.zeros(8, device=device)
    y = torch.zeros(4097, dtype=torch.int64, device=device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    with pytest.raises(RuntimeError, match="label_weight_sum: workspace too small"):
        check(L.mcdseg_label_weight_sum(p(y), p(cw), -100, 3, 4097, p(out), p(ws), ctypes.c_size_t(need - 1), st), "label_weight_sum")
    assert float(out) == -7.0   # refused before anything was launched
    check(L.mcdseg_label_weight_sum(p(y), p(cw), -100, 3, 4097, p(out), p(ws), ctypes.c_size_t(need), st), "label_weight_sum")
    assert float(out) == 4097.0


# ------------------------------------------------------------------------------------------------ b. sharded calls = the whole batch
FORMS = ("diff", "symkl", "mis_symkl", "jsd", "ce1")   # four two-head forms CE - discrepancy, and the one-head cross-entropy


def _dist_fn(form, c):
    if form in ("diff", "ce1"):
        return ref.diff_l1
    from loss import get_prob_distance_criterion
    return get_prob_distance_criterion(form, n_class=c)


@functools.lru_cache(maxsize=None)
def _labels(world, n, c, h, w, empty=None):
    ig = ref.ignore_of(c)
    return ref.make_labels(n, h, w, c, ig, world, empty=empty), ref.class_weights(c), ig


_TRUTH = {}


def _truth(key, form, z1, z2, y, cw, ig, c):
    """the fp64 statement for these logits, computed once per (case, form) and shared (the two forms of the up-sampling kernel see the
    same logits)"""
    if (key, form) not in _TRUTH:
        _TRUTH[(key, form)] = ref.global_objective(z1, None if form == "ce1" else z2, y, cw, ig, dist=_dist_fn(form, c))
    return _TRUTH[(key, form)]


def _check_sharded(entry, call, key, world, n, c, y, cw, ig, z1, z2, device):
    """``call(n0, n1, labels, form, wsum, want_grad)`` runs the entry on images n0:n1; the whole batch without ``wsum`` first, then one
    call per shard with W_global / world"""
    from mcdseg import ops
    yd, cwd = y.to(device), cw.to(device)
    w_global = ops.label_weight_sum(yd, cwd, c, ig)
    want_w = np.float32(float(ref.weight_sum(y, cw.double(), c, ig)))
    assert abs(float(w_global) - float(want_w)) <= 16 * 2.0 ** -24 * float(want_w)
    wsum = w_global / world
    cuts = ref.shards(n, world)
    for form in FORMS:
        two = form != "ce1"
        full_l, full_g1, full_g2 = call(0, n, yd, form, None, True)
        assert torch.equal(full_l[3], w_global[0])
        got = [call(n0, n1, yd[n0:n1], form, wsum, True) for n0, n1 in cuts]
        vals = [call(n0, n1, yd[n0:n1], form, wsum, False) for n0, n1 in cuts]
        t = _truth(key, form, z1, z2, y, cw, ig, c)
        what = "%s %s world %d C=%d %s" % (entry, form, world, c, "x".join(map(str, y.shape)))
        # ---- loss values: the mean over the ranks is the global loss; every call reports the normaliser it was given
        for name, res in (("grad", got), ("no grad", vals)):
            assert all(torch.equal(r[0][3], wsum[0]) for r in res), what
            if name == "no grad":
                assert all(r[1] is None and r[2] is None for r in res)
            for q, ref_val in ((0, t["ce1"]), (1, t["ce2"]), (2, t["dist"])):
                if q > 0 and not two:
                    continue
                mean = sum(float(r[0][q]) for r in res) / world
                err = abs(mean - float(ref_val)) / abs(float(ref_val))
                print("%s (%s): losses[%d] mean over shards %.9e vs fp64 %.9e (rel %.2e)" % (what, name, q, mean, float(ref_val), err))
                assert err <= VAL_RTOL, (what, name, q, err)
        # ---- gradients
        for k, full_g, ref_g in ((1, full_g1, t["g1"]), (2, full_g2, t["g2"])):
            if k == 2 and not two:
                assert full_g is None
                continue
            cat = torch.cat([r[k] for r in got])
            assert bool(torch.isfinite(cat).all()) and bool(torch.isfinite(full_g).all()), what
            if world in (2, 4):
                # a power of two through kce = ce_coef * wy / W and kd = diff_coef * inv_m scales every product and sum exactly,
                # as long as nothing is subnormal
                nz = full_g[full_g != 0].abs()
                assert nz.numel() > 0 and float(nz.min()) >= FLT_MIN, (what, float(nz.min()))
                same = torch.equal(cat / world, full_g)
                print("%s: g%d of the shards / %d bitwise the whole batch's: %s" % (what, k, world, same))
                assert same, (what, "g%d" % k, float((cat / world - full_g).abs().max()), float(full_g.abs().max()))
            else:
                bar = L1_RTOL if form in ("diff", "ce1") else GRAD_RTOL
                err = float((cat.double().cpu() / world - ref_g).abs().max() / ref_g.abs().max())
                print("%s: g%d of the shards / %d vs fp64: %.2e of the largest entry (bar %.0e)" % (what, k, world, err, bar))
                assert err <= bar, (what, k, err)


def _coefs(form):
    return dict(ce_coef=1.0, diff_coef=0.0 if form == "ce1" else -1.0, dist="diff" if form == "ce1" else form)


@pytest.mark.parametrize("hw", ref.PLAIN_HW, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("c", ref.CLASSES)
@pytest.mark.parametrize("world,n", ref.WORLDS)
def test_mcd_losses_on_shards_equal_the_whole_batch(device, world, n, c, hw):
    from mcdseg import ops
    h, w = hw
    y, cw, ig = _labels(world, n, c, h, w)
    g = torch.Generator().manual_seed(100 * c + h)
    z1, z2 = ((2 * torch.randn(n, c, h, w, generator=g)).to(device) for _ in range(2))
    cwd = cw.to(device)

    def call(n0, n1, labels, form, wsum, want_grad):
        return ops.mcd_losses(z1[n0:n1], None if form == "ce1" else z2[n0:n1], labels, cwd, ig, want_grad=want_grad, wsum=wsum, **_coefs(form))

    _check_sharded("mcd_losses", call, ("plain", world, c, h, w), world, n, c, y, cw, ig, z1, z2, device)


@pytest.mark.parametrize("dma", [1, 0])
@pytest.mark.parametrize("hiwi", ref.UP_HIWI, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("c", ref.CLASSES)
@pytest.mark.parametrize("world,n", ref.WORLDS)
def test_up8_mcd_losses_on_shards_equal_the_whole_batch(device, libopt, world, n, c, hiwi, dma):
    from mcdseg import ops
    libopt(UP8_LOSS_DMA=dma)
    hi, wi = hiwi
    y, cw, ig = _labels(world, n, c, 8 * hi, 8 * wi)
    g = torch.Generator().manual_seed(100 * c + hi)
    s1, s2 = ((2 * torch.randn(n, c, hi, wi, generator=g)).to(device) for _ in range(2))
    w1, w2 = ((torch.randn(c, 1, 16, 16, generator=g) * 0.2).to(device) for _ in range(2))
    z1, z2 = ops.up8(s1, w1), ops.up8(s2, w2)   # the logits the kernel forms on the fly: what the statement is evaluated on
    cwd = cw.to(device)

    def call(n0, n1, labels, form, wsum, want_grad):
        one = form == "ce1"
        return ops.up8_mcd_losses(s1[n0:n1], w1, None if one else s2[n0:n1], None if one else w2, labels, cwd, ig, want_grad=want_grad,
                                  wsum=wsum, **_coefs(form))

    _check_sharded("up8_mcd_losses dma=%d" % dma, call, ("up", world, c, hi, wi), world, n, c, y, cw, ig, z1, z2, device)


@pytest.mark.parametrize("empty", [0, 1])
def test_a_shard_without_a_valid_pixel(device, libopt, empty):
    """Data-parallel contract: a rank whose shard holds nothing but ignored pixels and weight-0 background contributes ZERO loss and a
    ZERO, finite gradient (W_local = 0, W_global > 0) -- the opposite of the single-process contract, 0/0 = NaN, which the same call
    keeps when the normaliser it is handed is itself 0."""
    from mcdseg import ops
    world, n, c, hi, wi = 2, 4, 20, 3, 5
    y, cw, ig = _labels(world, n, c, 8 * hi, 8 * wi, empty)
    n0, n1 = ref.shards(n, world)[empty]
    g = torch.Generator().manual_seed(5)
    s1, s2 = ((2 * torch.randn(n, c, hi, wi, generator=g)).to(device) for _ in range(2))
    w1, w2 = ((torch.randn(c, 1, 16, 16, generator=g) * 0.2).to(device) for _ in range(2))
    z1, z2 = ops.up8(s1, w1), ops.up8(s2, w2)
    yd, cwd = y.to(device), cw.to(device)
    assert float(ops.label_weight_sum(yd[n0:n1], cwd, c, ig)) == 0.0
    w_global = ops.label_weight_sum(yd, cwd, c, ig)
    assert float(w_global) > 0
    ys = yd[n0:n1]
    inrange = ((ys >= 0) & (ys < c) & (ys != ig))[:, None].expand(-1, c, -1, -1)
    assert bool(inrange.any()) and not bool(inrange.all())
    calls = [("mcd_losses %s" % d, lambda ws, d=d: ops.mcd_losses(z1[n0:n1], z2[n0:n1], ys, cwd, ig, ce_coef=1.0, wsum=ws, dist=d))
             for d in ("diff", "jsd")]
    calls.append(("mcd_losses one head", lambda ws: ops.mcd_losses(z1[n0:n1], None, ys, cwd, ig, ce_coef=1.0, wsum=ws)))
    for dma in (1, 0):
        for d in ("diff", "jsd"):
            calls.append(("up8_mcd_losses %s dma=%d" % (d, dma), lambda ws, d=d, dma=dma: (
                libopt(UP8_LOSS_DMA=dma), ops.up8_mcd_losses(s1[n0:n1], w1, s2[n0:n1], w2, ys, cwd, ig, ce_coef=1.0, wsum=ws, dist=d))[1]))
    for what, call in calls:
        losses, g1, g2 = call(w_global / world)
        assert float(losses[0]) == 0.0 and float(losses[1]) == 0.0, (what, losses.tolist())
        for gk in (g1, g2):
            if gk is not None:
                assert bool(torch.isfinite(gk).all()) and float(gk.abs().max()) == 0.0, what
        # the single-process contract: W = 0 handed in (or found) is 0/0
        for ws in (torch.zeros(1, device=device), None):
            losses, g1, g2 = call(ws)
            assert bool(torch.isnan(losses[0])) and float(losses[3]) == 0.0, (what, losses.tolist())
            assert bool(torch.isnan(g1[inrange]).all()), what            # weight-0 pixels: 0 / 0
            assert float(g1[~inrange].abs().max()) == 0.0, what          # ignored and out-of-range pixels: no term at all


def test_uncertain_loss_on_shards_equals_the_whole_batch(device):
    """``ops.up8_uncertain_loss`` (its ``wsum`` is held to tests/uncertain_ref.py elsewhere): world 2, the base loss and its gradient
    w.r.t. the score map.  The shard calls evaluate the whole-batch call's per-pixel expressions with W / 2 in the place of W, so they
    may differ from it by roundings of that scale only: the bars of the loss kernels' own tests (2e-6 on the value, 5e-6 of the
    largest gradient entry)."""
    from mcdseg import ops
    world, n, c, hi, wi, t = 2, 4, 12, 5, 7, 3
    y, cw, ig = _labels(world, n, c, 8 * hi, 8 * wi)
    g = torch.Generator().manual_seed(21)
    s = (2 * torch.randn(n, c, hi, wi, generator=g)).to(device)
    w_up, w_std = ((torch.randn(c, 1, 16, 16, generator=g) * 0.2).to(device) for _ in range(2))
    keep = (torch.rand(t, n, c, generator=g) < 0.8).to(torch.uint8).to(device)
    r = torch.rand(t, generator=g).to(device)
    yd, cwd = y.to(device), cw.to(device)

    def run(n0, n1, wsum):
        leaf = s[n0:n1].clone().requires_grad_()
        base, _ = ops.up8_uncertain_loss(leaf, w_up, w_std, yd[n0:n1], cwd, keep[:, n0:n1].contiguous(), r, ignore_index=ig, wsum=wsum)
        base.backward()
        return float(base.detach()), leaf.grad

    full, full_g = run(0, n, None)
    wsum = ops.label_weight_sum(yd, cwd, c, ig) / world
    parts = [run(n0, n1, wsum) for n0, n1 in ref.shards(n, world)]
    mean = sum(p[0] for p in parts) / world
    cat = torch.cat([p[1] for p in parts]) / world
    ev, eg = abs(mean - full) / abs(full), float((cat - full_g).abs().max() / full_g.abs().max())
    print("uncertain base loss: shards %.9e vs whole %.9e (rel %.2e); gradient %.2e of the largest entry, bitwise %s"
          % (mean, full, ev, eg, torch.equal(cat, full_g)))
    assert ev <= VAL_RTOL and eg <= GRAD_RTOL
    local = [float(ops.label_weight_sum(yd[n0:n1], cwd, c, ig)) for n0, n1 in ref.shards(n, world)]
    assert local[0] < 0.35 * local[1]      # (unequal shards: a local normaliser would be off by far more than the bar)


# ------------------------------------------------------------------------- c. grad_scale and the long loops of the update kernels
LONG = 2048 * 256 * 4 + 4 * 256 * 3 + 3    # past one trip of 2048 blocks x 256 threads x float4: a second trip for 768 threads, a scalar tail of 3
SCALES = [0.5, 1.0 / 3.0, 0.125]


def _update_inputs(n, gs):
    gen = torch.Generator().manual_seed(n % 1000 + int(1000 * gs))
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) for _ in range(2)]
    return gen, p0, grads


@pytest.mark.parametrize("gs", SCALES, ids=["half", "third", "eighth"])
@pytest.mark.parametrize("n", [1027, LONG])
def test_sgd_grad_scale_and_grid_stride_loop(device, n, gs):
    """two steps of ``ops.sgd_momentum_flat_`` as test_fusion_kernels_gpu.test_sgd_momentum_flat_on_offset_slices runs them, with the
    1/world of 2, 3 and 8 ranks and at a size that takes the grid-stride loop round again: aligned (float4 body + tail) and on
    base[1:1+n] slices (all scalar) bit for bit the same, both within fp32 torch's own distance (x 2) of the fp64 recurrence"""
    from mcdseg import ops
    lr, mu, wd = 1e-2, 0.9, 2e-3
    gen, p0, grads = _update_inputs(n, gs)
    v0 = torch.randn(n, generator=gen)

    def recurrence(dtype):
        p, v = p0.to(dtype), v0.to(dtype)
        for gr in grads:
            v = mu * v + wd * p + gs * gr.to(dtype)
            p = p - lr * v
        return p, v

    (p64, v64), (p32, v32) = recurrence(torch.float64), recurrence(torch.float32)
    pa, va = p0.to(device), v0.to(device)
    po, vo = _offset(p0, device), _offset(v0, device)
    for gr in grads:
        ga = gr.to(device)
        assert pa.data_ptr() % 16 == 0 and ga.data_ptr() % 16 == 0 and va.data_ptr() % 16 == 0
        ops.sgd_momentum_flat_(pa, ga, va, lr, mu, wd, gs, params=())
        ops.sgd_momentum_flat_(po, _offset(gr, device), vo, lr, mu, wd, gs, params=())
    assert torch.equal(po, pa) and torch.equal(vo, va)
    t = _Truth("sgd_momentum_flat n=%d gs=%g" % (n, gs))
    t.check(pa, p64, p32, "p")
    t.check(va, v64, v32, "v")
    t.report()


@pytest.mark.parametrize("gs", SCALES, ids=["half", "third", "eighth"])
@pytest.mark.parametrize("n", [1027, LONG])
def test_adam_grad_scale_and_pipelined_loop(device, n, gs):
    """two steps of ``ops.adam_flat_`` with grad_scale != 1, at a size whose float4 body takes the software-pipelined ``more`` branch
    (and a scalar tail), aligned and on base[1:1+n] slices bit for bit the same; against torch.optim.Adam in fp64 fed ``g * gs`` with
    test_adam_gpu's yardstick and margin: at most FACTOR = 2 times as far from it as torch's own fp32 Adam fed the fp32 ``g * gs``
    (why 2: test_adam_gpu.test_adam_kernel_against_fp64_truth)"""
    from mcdseg import ops
    gen, p0, grads = _update_inputs(n, gs)
    p64, p32 = torch.nn.Parameter(p0.double()), torch.nn.Parameter(p0.clone())
    truth, yard = torch.optim.Adam([p64], **ADAM), torch.optim.Adam([p32], foreach=False, **ADAM)
    pa, ma, va = p0.to(device), torch.zeros(n, device=device), torch.zeros(n, device=device)
    po, mo, vo = _offset(p0, device), _offset(torch.zeros(n), device), _offset(torch.zeros(n), device)
    bad = []
    for step, gr in enumerate(grads, 1):
        p64.grad, p32.grad = gr.double() * gs, gr * gs
        truth.step(), yard.step()
        ga = gr.to(device)
        assert all(x.data_ptr() % 16 == 0 for x in (pa, ga, ma, va))
        ops.adam_flat_(pa, ga, ma, va, ADAM["lr"], ADAM["betas"], ADAM["eps"], ADAM["weight_decay"], step, gs, params=())
        ops.adam_flat_(po, _offset(gr, device), mo, vo, ADAM["lr"], ADAM["betas"], ADAM["eps"], ADAM["weight_decay"], step, gs, params=())
        assert torch.equal(po, pa) and torch.equal(mo, ma) and torch.equal(vo, va)
        st64, st32 = truth.state[p64], yard.state[p32]
        for what, t64, t32, th in (("param", p64, p32, pa), ("exp_avg", st64["exp_avg"], st32["exp_avg"], ma),
                                   ("exp_avg_sq", st64["exp_avg_sq"], st32["exp_avg_sq"], va)):
            t64 = t64.detach()
            e32 = float((t32.detach().double() - t64).abs().max())
            e = float((th.double().cpu() - t64).abs().max())
            print("adam n=%d gs=%g step %d %-10s hip %.3e  fp32 torch %.3e  ratio %.3f" % (n, gs, step, what, e, e32, e / e32 if e32 else 0.0))
            assert bool(torch.isfinite(th).all())
            if not e <= FACTOR * e32:
                bad.append((step, what, e, e32))
    assert not bad, bad
