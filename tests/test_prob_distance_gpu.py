"""GPU: the distances of ``--d_loss`` besides L1 (jsd / symkl / mis_symkl and their aliases) on the fused loss kernels -- the
plain-logit kernel against the reference's own fp64 vectors and against the torch criteria in fp64, the fused x8 up-sampler
kernels against the two-pass result, kind 0 against the L1 entry points, the solvers against the drop-in statement loop, and the
trainers' command lines."""
import ctypes

import numpy as np
import pytest
import torch

from recipe import fill_state_, make_batch, state_checksums

pytestmark = pytest.mark.gpu

NAMES = ("jsd", "symkl", "nmlsymkl", "mysymkl", "spatial_jsd", "mis_symkl")
KINDS = ("symkl", "mis_symkl", "jsd")
# the bars test_loss_kernel_against_golden_and_closed_forms holds the L1 distance to: about 10x an fp32 evaluation of the criteria
VAL_RTOL, GRAD_RTOL = 2e-6, 5e-6


@pytest.fixture(autouse=True)
def _no_pretrained(monkeypatch):
    monkeypatch.setenv("MCDSEG_PRETRAINED", "0")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _held(what, got_val, ref_val, got_g, ref_g):
    """print every figure, then assert: value relative to the reference's, gradients relative to the reference's largest entry"""
    ev = abs(float(got_val) - float(ref_val)) / max(abs(float(ref_val)), 1e-300)
    print("%s: value %.9e vs %.9e (rel %.2e)" % (what, float(got_val), float(ref_val), ev))
    errs = []
    for k, (g, r) in enumerate(zip(got_g, ref_g)):
        g = g.detach().double().cpu().numpy() if torch.is_tensor(g) else np.asarray(g, dtype=np.float64)
        r = r.detach().double().cpu().numpy() if torch.is_tensor(r) else np.asarray(r, dtype=np.float64)
        assert np.isfinite(g).all(), what
        errs.append(np.abs(g - r).max() / np.abs(r).max())
        print("%s: g%d max err %.2e of max|g| %.3e" % (what, k + 1, errs[-1], np.abs(r).max()))
    assert ev <= VAL_RTOL, (what, ev)
    assert max(errs) <= GRAD_RTOL, (what, errs)


@pytest.mark.parametrize("name", NAMES)
def test_plain_kernel_against_the_reference_vectors(golden, name):
    """dist_small.npz: value and d/dlogits of every criterion in fp64, from the reference's own classes"""
    dev = _dev()
    from loss import get_prob_distance_criterion
    from mcdseg import ops
    fx = golden.npz("dist_small.npz")
    z1, z2 = torch.from_numpy(fx["z1"]).float().to(dev), torch.from_numpy(fx["z2"]).float().to(dev)
    losses, g1, g2 = ops.mcd_losses(z1, z2, None, None, diff_coef=1.0, dist=name)
    _held(name + " kernel", losses[2], fx[name + "_val"], (g1, g2), (fx[name + "_g1"], fx[name + "_g2"]))
    # through the criterion module and autograd, with an upstream gradient that is not 1
    a, b = z1.clone().requires_grad_(), z2.clone().requires_grad_()
    crit = get_prob_distance_criterion(name, n_class=int(fx["n_class"]))
    val = crit(a, b)
    (-2.5 * val).backward()
    _held(name + " criterion", val, fx[name + "_val"], (a.grad, b.grad), (-2.5 * fx[name + "_g1"], -2.5 * fx[name + "_g2"]))
    a2, b2 = z1.clone().requires_grad_(), z2.clone().requires_grad_()
    val2 = ops.prob_distance(a2, b2, ops.DIST_KINDS[name])
    (-2.5 * val2).backward()
    assert torch.equal(val2, val) and torch.equal(a2.grad, a.grad) and torch.equal(b2.grad, b.grad)
    # cross-entropy in the same call: its values and (alone) its gradients are the L1 entry's, bit for bit
    g = torch.Generator().manual_seed(3)
    y = torch.randint(0, 9, (2, 6, 10), generator=g)
    y[0, 0, :3] = -100
    y, cw = y.to(dev), (0.5 + torch.rand(9, generator=g)).to(dev)
    l1_l, l1_g1, l1_g2 = ops.mcd_losses(z1, z2, y, cw, ce_coef=1.0, diff_coef=0.0)
    ce_l, ce_g1, ce_g2 = ops.mcd_losses(z1, z2, y, cw, ce_coef=1.0, diff_coef=0.0, dist=name)
    assert torch.equal(ce_l[:2], l1_l[:2]) and torch.equal(ce_l[3], l1_l[3])
    assert torch.equal(ce_g1, l1_g1) and torch.equal(ce_g2, l1_g2)
    both_l, both_g1, both_g2 = ops.mcd_losses(z1, z2, y, cw, ce_coef=1.0, diff_coef=-1.0, dist=name)
    assert torch.equal(both_l[:2], l1_l[:2]) and torch.equal(both_l[2], losses[2])
    ref1 = l1_g1.double().cpu().numpy() - fx[name + "_g1"]
    ref2 = l1_g2.double().cpu().numpy() - fx[name + "_g2"]
    _held(name + " CE - dist", both_l[2], fx[name + "_val"], (both_g1, both_g2), (ref1, ref2))


def _torch_truth(name, z1, z2, c):
    """the product's torch criterion in fp64 on the CPU"""
    from loss import get_prob_distance_criterion
    a, b = z1.double().cpu().requires_grad_(), z2.double().cpu().requires_grad_()
    val = get_prob_distance_criterion(name, n_class=c)(a, b)
    val.backward()
    return val.detach(), a.grad, b.grad


@pytest.mark.parametrize("spread", [2.0, 30.0])
@pytest.mark.parametrize("c", [41, 19])
@pytest.mark.parametrize("name", KINDS)
def test_plain_kernel_at_full_resolution(name, c, spread):
    """2 x C x 480 x 640 seeded logits; spread 30 makes probabilities flush to zero, where nothing may divide by them or take their
    logarithm.  Identical heads: SYMKL and JSD are zero, value and gradients, exactly."""
    dev = _dev()
    from mcdseg import ops
    g = torch.Generator().manual_seed(1000 + c)
    z1 = (spread * torch.randn(2, c, 480, 640, generator=g)).to(dev)
    z2 = (spread * torch.randn(2, c, 480, 640, generator=g)).to(dev)
    losses, g1, g2 = ops.mcd_losses(z1, z2, None, None, diff_coef=1.0, dist=name)
    assert bool(torch.isfinite(losses[2])) and bool(torch.isfinite(g1).all()) and bool(torch.isfinite(g2).all())
    val, r1, r2 = _torch_truth(name, z1, z2, c)
    _held("%s C=%d spread %g" % (name, c, spread), losses[2], val, (g1, g2), (r1, r2))
    same, s1, s2 = ops.mcd_losses(z1, z1, None, None, diff_coef=1.0, dist=name)
    assert bool(torch.isfinite(s1).all()) and bool(torch.isfinite(s2).all())
    if name != "mis_symkl":
        assert float(same[2]) == 0.0 and float(s1.abs().max()) == 0.0 and float(s2.abs().max()) == 0.0


def _up_problem(shape, dev, seed=11, shared=False):
    n, c, hi, wi = shape
    g = torch.Generator().manual_seed(seed)
    s1 = (2 * torch.randn(n, c, hi, wi, generator=g)).to(dev)
    s2 = s1 if shared else (2 * torch.randn(n, c, hi, wi, generator=g)).to(dev)
    w1 = (torch.randn(c, 1, 16, 16, generator=g) * 0.2).to(dev)
    w2 = (torch.randn(c, 1, 16, 16, generator=g) * 0.2).to(dev)
    lab = torch.randint(0, c, (n, 8 * hi, 8 * wi), generator=g)
    lab[0, 0, :5] = -100
    cw = (0.5 + torch.rand(c, generator=g)).to(dev)
    return s1, w1, s2, w2, lab.to(dev), cw


# the shapes of test_up8_loss_fused_equals_two_pass (16 / 24 / 48-class instantiations, ragged segments, several patches per workgroup)
# and the benchmark's own
UP_SHAPES = [(2, 41, 5, 7), (1, 12, 3, 20), (2, 20, 4, 33), (1, 41, 2, 80), (5, 41, 30, 24), (3, 30, 33, 17), (16, 41, 60, 80)]


@pytest.mark.parametrize("shape", UP_SHAPES)
@pytest.mark.parametrize("dma", ["1", "0"])
@pytest.mark.parametrize("name", KINDS)
def test_fused_up8_kernels_equal_the_two_pass_result(name, dma, shape, libopt):
    dev = _dev()
    from mcdseg import ops
    libopt(UP8_LOSS_DMA=int(dma))
    n, c, hi, wi = shape
    kind = ops.DIST_KINDS[name]
    kname = ops.up8_loss_kernel_name(n, c, hi, wi, True, False, dist=name)
    ncmax = (16 if c <= 16 else 24 if c <= 24 else 41 if c == 41 else 48) if dma == "1" else (16 if c <= 16 else 24 if c <= 24 else 48)
    if dma == "1":
        assert kname == "up8_softmax_ce_dist_dma_kernel<%d, %s, %d>" % (ncmax, "true" if c == ncmax else "false", kind)
    else:
        assert kname == "up8_softmax_ce_dist_kernel<%d, %d>" % (ncmax, kind)
    seen = []

    class _Names:
        def wants(self, nm):
            seen.append(nm)
            return False
    s1, w1, s2, w2, lab, cw = _up_problem(shape, dev)
    z1, z2 = ops.up8(s1, w1), ops.up8(s2, w2)
    for labels, kw in ((None, dict(diff_coef=0.7)), (lab, dict(ce_coef=1.0, diff_coef=-1.0))):
        ref_l, ref_g1, ref_g2 = ops.mcd_losses(z1, z2, labels, cw if labels is not None else None, dist=name, **kw)
        ops.LAUNCH_TIMER = _Names()
        try:
            got_l, got_g1, got_g2 = ops.up8_mcd_losses(s1, w1, s2, w2, labels, cw if labels is not None else None, dist=name, **kw)
        finally:
            ops.LAUNCH_TIMER = None
        assert torch.equal(got_g1, ref_g1) and torch.equal(got_g2, ref_g2)
        for q in range(3):  # CE1, CE2, the distance, each against its own size (summation order only)
            assert abs(float(got_l[q]) - float(ref_l[q])) <= 2e-6 * abs(float(ref_l[q])), (q, float(got_l[q]), float(ref_l[q]))
        assert torch.equal(got_l[3], ref_l[3])
        vals, _, _ = ops.up8_mcd_losses(s1, w1, s2, w2, labels, cw if labels is not None else None, want_grad=False, dist=name, **kw)
        assert torch.equal(vals, got_l)
    assert ops.up8_loss_kernel_name(n, c, hi, wi, True, True, dist=name) in seen
    del z1, z2, ref_g1, ref_g2
    if dma == "1":  # the two forms of the fused kernel: the same sums in the same order
        libopt(UP8_LOSS_DMA=0)
        reg_l, reg_g1, reg_g2 = ops.up8_mcd_losses(s1, w1, s2, w2, lab, cw, dist=name, ce_coef=1.0, diff_coef=-1.0)
        assert torch.equal(reg_l, got_l) and torch.equal(reg_g1, got_g1) and torch.equal(reg_g2, got_g2)


def test_kind_zero_is_the_l1_entry_point(libopt):
    dev = _dev()
    from mcdseg import ops
    from mcdseg._lib import check, lib
    L = lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for shape, dma in (((2, 41, 5, 7), 1), ((2, 20, 4, 33), 1), ((5, 41, 30, 24), 0)):
        libopt(UP8_LOSS_DMA=dma)
        n, c, hi, wi = shape
        s1, w1, s2, w2, lab, cw = _up_problem(shape, dev)
        z1, z2 = ops.up8(s1, w1), ops.up8(s2, w2)
        old = ops.mcd_losses(z1, z2, lab, cw, ce_coef=1.0, diff_coef=-1.0)
        new_l, new_g1, new_g2 = torch.empty(4, device=dev), torch.empty_like(z1), torch.empty_like(z1)
        ws = ops._ws(L.mcdseg_loss_workspace_bytes(n, 64 * hi * wi), dev)
        check(L.mcdseg_softmax_ce_dist(p(z1), p(z2), p(lab), p(cw), -100, 1.0, -1.0, None, p(new_g1), p(new_g2), p(new_l), n, c, 64 * hi * wi,
                                       0, p(ws), ctypes.c_size_t(ws.numel() * 4), st), "softmax_ce_dist")
        assert torch.equal(new_l, old[0]) and torch.equal(new_g1, old[1]) and torch.equal(new_g2, old[2])
        old = ops.up8_mcd_losses(s1, w1, s2, w2, lab, cw, ce_coef=1.0, diff_coef=-1.0)
        ws = ops._ws(L.mcdseg_up8_loss_workspace_bytes(n, hi, wi), dev)
        check(L.mcdseg_up8_softmax_ce_dist(p(s1), p(w1), p(s2), p(w2), p(lab), p(cw), -100, 1.0, -1.0, None, p(new_g1), p(new_g2), p(new_l),
                                           n, c, hi, wi, 0, p(ws), ctypes.c_size_t(ws.numel() * 4), st), "up8_softmax_ce_dist")
        assert torch.equal(new_l, old[0]) and torch.equal(new_g1, old[1]) and torch.equal(new_g2, old[2])
        # ... and the single-head form of kind 0 stays what it was
        one = ops.mcd_losses(z1, None, lab, cw, ce_coef=1.0, dist="diff")
        ref = ops.mcd_losses(z1, None, lab, cw, ce_coef=1.0)
        assert torch.equal(one[0], ref[0]) and torch.equal(one[1], ref[1])


@pytest.mark.parametrize("name", KINDS)
def test_dma_kernel_is_deterministic_at_the_benchmark_shape(name):
    """the hand-waited kernel's contract: 50 launches, every output bitwise the first"""
    dev = _dev()
    from mcdseg import ops
    s1, w1, s2, w2, lab, cw = _up_problem((16, 41, 60, 80), dev, seed=23)
    assert ops.up8_loss_kernel_name(16, 41, 60, 80, True, True, dist=name) == "up8_softmax_ce_dist_dma_kernel<41, true, %d>" % ops.DIST_KINDS[name]
    first = ops.up8_mcd_losses(s1, w1, s2, w2, lab, cw, ce_coef=1.0, diff_coef=-1.0, dist=name)
    for _ in range(50):
        again = ops.up8_mcd_losses(s1, w1, s2, w2, lab, cw, ce_coef=1.0, diff_coef=-1.0, dist=name)
        assert all(torch.equal(a, b) for a, b in zip(again, first))
        del again


def _mcd_models(dev):
    from models.model_util import get_models
    g, f1, f2 = get_models("drn_d_38", 6, 41)
    for m, seed in ((g, 11), (f1, 12), (f2, 13)):
        fill_state_(m, seed)
        m.to(dev)
        m.train(True)
    return g, f1, f2


def _same_state(mod, ref, rtol):
    """test_model_gpu._check_state with the other model's checksums in the place of the stored ones"""
    got, want = state_checksums(mod), state_checksums(ref)
    assert got.keys() == want.keys()
    numel = {k: v.numel() for k, v in mod.state_dict().items()}
    bad = [(k, got[k][1], l2) for k, (s, l2) in want.items() if abs(got[k][1] - l2) > rtol * max(abs(l2), 1e-6)]
    assert not bad, bad[:5]
    bad = [(k, got[k][0], s) for k, (s, l2) in want.items() if abs(got[k][0] - s) > rtol * max(abs(l2), 1e-6) * max(numel[k], 1) ** 0.5]
    assert not bad, bad[:5]


@pytest.mark.parametrize("name", ["jsd", "symkl", "mis_symkl"])
def test_solver_matches_the_drop_in_loop(golden, name, monkeypatch):
    """the models, batch and optimizers of test_model_gpu.test_solver_matches_drop_in_loop, two iterations: ``MCDSolver.step`` against
    ``adapt_trainer.dropin_step`` with the torch statement of the criterion (the route this flag took before the kernels existed) on
    the HIP modules' logits"""
    dev = _dev()
    import adapt_trainer
    import loss as loss_mod
    from loss import CrossEntropyLoss2d, get_prob_distance_criterion
    from mcdseg import ops
    from models.model_util import get_optimizer
    from solvers.solver import MCDSolver
    tr = golden.json("traces.json")["mcd_small"]
    n, ch, h, w = tr["shape"]
    s, l, t = (v.to(dev) for v in make_batch(tr["seed_batch"], n, ch, h, w, 41))
    cw = torch.ones(41)
    cw[40] = 0
    ce = CrossEntropyLoss2d(cw.to(dev))
    g, f1, f2 = _mcd_models(dev)
    rg, rf1, rf2 = _mcd_models(dev)
    og = get_optimizer(g.parameters(), "sgd", 1e-3, 0.9, 2e-5)
    of = get_optimizer(list(f1.parameters()) + list(f2.parameters()), "sgd", 1e-3, 0.9, 2e-5)
    rog = get_optimizer(rg.parameters(), "sgd", 1e-3, 0.9, 2e-5)
    rof = get_optimizer(list(rf1.parameters()) + list(rf2.parameters()), "sgd", 1e-3, 0.9, 2e-5)
    solver = MCDSolver(g, f1, f2, og, of, ce, get_prob_distance_criterion(name, n_class=41), num_k=4)
    assert solver.fused_up
    torch_crit = get_prob_distance_criterion(name, n_class=41)
    seen = []

    class _Names:
        def wants(self, nm):
            seen.append(nm)
            return False
    for it in range(2):
        monkeypatch.setattr(ops, "LAUNCH_TIMER", _Names())
        c_loss, d_loss = solver.step(s, l, t)
        monkeypatch.setattr(ops, "LAUNCH_TIMER", None)
        with monkeypatch.context() as mp:
            mp.setattr(loss_mod, "_on_kernel", lambda *a, **k: False)  # the criterion's torch expression, as before this kernel
            rc, rd = adapt_trainer.dropin_step(rg, rf1, rf2, rog, rof, ce, torch_crit, s, l, t, 4, 1)
        c_loss, d_loss, rc, rd = float(c_loss), float(d_loss), float(rc), float(rd)
        print("%s iter %d: c_loss %.7f vs %.7f, d_loss %.6e vs %.6e" % (name, it, c_loss, rc, d_loss, rd))
        assert abs(c_loss - rc) <= 1e-4 * abs(rc)
        assert abs(d_loss - rd) <= 2e-3 * abs(rd)
    assert any(nm.startswith("up8_softmax_ce_dist") for nm in seen), sorted(set(seen))
    _same_state(g, rg, 3e-4), _same_state(f1, rf1, 3e-4), _same_state(f2, rf2, 3e-4)


@pytest.mark.parametrize("name", ["jsd", "symkl", "mis_symkl"])
def test_solver_matches_the_reference_trace(golden, name):
    """dist_traces.json (make_golden_dist_trace.py): the three-step loop of the "mcd_small" trace with the REFERENCE's criterion objects,
    in fp64.  The bars of test_model_gpu.test_solver_matches_drop_in_loop; a quantity in which the fp32 run of that loop is itself outside
    its bar would be held to twice that distance (stored in the fixture) -- none is: the fp32 oracle is within 1.1e-6 (c_loss), 3.6e-5
    (d_loss) and 7.7e-5 (state) of its fp64 run for all three distances."""
    dev = _dev()
    from loss import CrossEntropyLoss2d, get_prob_distance_criterion
    from models.model_util import get_optimizer
    from solvers.solver import MCDSolver
    tr = golden.json("dist_traces.json")[name]
    noise = tr["f32_distance"]

    def bar(base, own):
        return base if own <= base else 2 * own
    n, ch, h, w = tr["shape"]
    s, l, t = (v.to(dev) for v in make_batch(tr["seed_batch"], n, ch, h, w, 41))
    cw = torch.ones(41)
    cw[40] = 0
    g, f1, f2 = _mcd_models(dev)
    og = get_optimizer(g.parameters(), "sgd", 1e-3, 0.9, 2e-5)
    of = get_optimizer(list(f1.parameters()) + list(f2.parameters()), "sgd", 1e-3, 0.9, 2e-5)
    solver = MCDSolver(g, f1, f2, og, of, CrossEntropyLoss2d(cw.to(dev)), get_prob_distance_criterion(name, n_class=41), num_k=4)
    for k, it in enumerate(tr["iters"]):
        c_loss, d_loss = (float(v) for v in solver.step(s, l, t))
        ec, ed = abs(c_loss - it["c_loss"]) / abs(it["c_loss"]), abs(d_loss - it["d_loss"]) / abs(it["d_loss"])
        print("%s iter %d: c_loss %.7f vs %.7f (rel %.2e), d_loss %.6e vs %.6e (rel %.2e)" % (name, k, c_loss, it["c_loss"], ec, d_loss,
                                                                                             it["d_loss"], ed))
        assert ec <= bar(1e-4, noise["c_loss"][k])
        assert ed <= bar(2e-3, noise["d_loss"][k])
    for key, mod in (("g", g), ("f1", f1), ("f2", f2)):
        got, want = state_checksums(mod), tr[key]
        assert got.keys() == want.keys()
        rtol = bar(3e-4, noise["state"][key])
        numel = {k: v.numel() for k, v in mod.state_dict().items()}
        bad = [(k, got[k], want[k]) for k, (sm, l2) in want.items()
               if abs(got[k][1] - l2) > rtol * max(abs(l2), 1e-6) or abs(got[k][0] - sm) > rtol * max(abs(l2), 1e-6) * max(numel[k], 1) ** 0.5]
        assert not bad, bad[:5]


def test_mfnet_solver_matches_the_written_out_statements(golden, monkeypatch):
    """``MFNetMCDSolver`` with symkl on the models of the "mfnet_small" trace -- the materialised-logit branch of ``_loss_backward`` --
    against the statements of adapt_mfnet_trainer.py:174-244 (``oracle.ref_mcd.mfnet_mcd_step``, a plain statement loop over whatever
    modules it is given) run on a second copy of the HIP modules with the criterion's torch expression; two iterations"""
    dev = _dev()
    import loss as loss_mod
    from loss import CrossEntropyLoss2d, get_prob_distance_criterion
    from models.model_util import get_models, get_optimizer
    from oracle import ref_mcd
    from solvers.solver import MFNetMCDSolver
    tr = golden.json("traces.json")["mfnet_small"]
    n, ch, h, w = tr["shape"]
    s, l, t = (v.to(dev) for v in make_batch(tr["seed_batch"], n, ch, h, w, 41))
    cw = torch.ones(41)
    cw[40] = 0
    ce = CrossEntropyLoss2d(cw.to(dev))
    sets = []
    for _ in range(2):
        ms = get_models("drn_d_38", 6, 41, method="MFNet-ScoreAddFusion")
        for m, seed in zip(ms, (51, 52, 53, 54)):
            fill_state_(m, seed)
            m.to(dev).train()
        og = get_optimizer(list(ms[0].parameters()) + list(ms[1].parameters()), "sgd", 1e-3, 0.9, 2e-5)
        of = get_optimizer(list(ms[2].parameters()) + list(ms[3].parameters()), "sgd", 1e-3, 0.9, 2e-5)
        sets.append((ms, og, of))
    (ms, og, of), (rms, rog, rof) = sets
    solver = MFNetMCDSolver(ms[0], ms[1], ms[2], ms[3], og, of, ce, get_prob_distance_criterion("symkl", n_class=41), num_k=4)
    assert not solver.fused_up
    torch_crit = get_prob_distance_criterion("symkl", n_class=41)
    for it in range(2):
        c_loss, d_loss = (float(v) for v in solver.step(s, l, t))
        with monkeypatch.context() as mp:
            mp.setattr(loss_mod, "_on_kernel", lambda *a, **k: False)
            rc, rd = ref_mcd.mfnet_mcd_step(rms[0], rms[1], rms[2], rms[3], rog, rof, ce, torch_crit, s, l, t, num_k=4)
        print("mfnet symkl iter %d: c_loss %.7f vs %.7f, d_loss %.6e vs %.6e" % (it, c_loss, rc, d_loss, rd))
        assert abs(c_loss - rc) <= 1e-4 * abs(rc)
        assert abs(d_loss - rd) <= 2e-3 * abs(rd)
    for a, b in zip(ms, rms):
        _same_state(a, b, 3e-4)


def test_criteria_keep_their_torch_expression_past_48_classes():
    """the kernels keep at most 48 classes in registers; a criterion called with more stays what it was"""
    dev = _dev()
    from loss import get_prob_distance_criterion
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn(1, 60, 4, 6, generator=g).to(dev).requires_grad_(), torch.randn(1, 60, 4, 6, generator=g).to(dev)
    for name in KINDS:
        val = get_prob_distance_criterion(name, n_class=60)(a, b)
        want = get_prob_distance_criterion(name, n_class=60)(a.detach().double().cpu(), b.double().cpu())
        assert abs(float(val) - float(want)) <= 1e-5 * abs(float(want))
        val.backward()
    assert bool(torch.isfinite(a.grad).all())


COMMON = ["--input_ch", "6", "-b", "2", "--train_img_shape", "96", "64", "--synthetic", "--synthetic_len", "4",
          "--no_pretrained", "--no_tflog", "--epochs", "1", "--max_iter", "10"]


def test_adapt_trainer_runs_the_fused_kernel_for_jsd(tmp_path, monkeypatch):
    dev = _dev()
    import adapt_trainer
    from mcdseg import ops
    names = []

    class _Names:
        def wants(self, name):
            names.append(name)
            return False
    monkeypatch.setattr(ops, "LAUNCH_TIMER", _Names())
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        assert adapt_trainer.main(["suncg", "nyu", "--base_outdir", str(tmp_path / "out"), "--d_loss", "jsd"] + COMMON) == 0
    assert any(nm.startswith("up8_softmax_ce_dist") and nm.endswith(", 3>") for nm in names), sorted(set(names))
    aten = {e.key for e in prof.key_averages()}
    assert not any("softmax" in k for k in aten), sorted(k for k in aten if "softmax" in k)
    del dev


def test_adapt_mfnet_trainer_runs_with_symkl(tmp_path, monkeypatch):
    _dev()
    import adapt_mfnet_trainer
    from mcdseg import ops
    names = []

    class _Names:
        def wants(self, name):
            names.append(name)
            return False
    monkeypatch.setattr(ops, "LAUNCH_TIMER", _Names())
    assert adapt_mfnet_trainer.main(["suncg", "nyu", "--base_outdir", str(tmp_path / "out"), "--method_detail", "MFNet-ScoreAddFusion",
                                     "--d_loss", "symkl"] + COMMON) == 0
    assert "softmax_ce_dist_kernel" in names, sorted(set(names))
