"""GPU: the FuseNet-style generator (``--net drn_d_XX_fusenet``, middle fusion).

* ``mcdseg_stage_join`` bit for bit: y = a + b, y_bound = bound_a + bound_b, the companion = ``ops.split_companion(y, y_bound)``.
* ``ops.stage_join``: the gradient to both inputs, and MCDSEG_FUSED_JOIN=0 (add + split) against the kernel, bit for bit.
* ``models.dilated_fcn.FuseDRNSegBase`` on the reduced DRN-D against what the REAL reference produced (tests/golden/fusenet_small.npz):
  the score map, every gradient and the running statistics held to the fp64 truth in units of the reference's own fp32 distance from
  it, by the project's rule for tensors behind the trunk (tests/test_uncertain_gpu.py): a factor 2 on that unit, and a floor of 2e-5
  of the tensor's largest magnitude -- the split-precision convolutions' own accuracy bound -- since every tensor here lies behind
  convolutions.
* drn_d_22_fusenet: fused join against composed join, weight gradients on and off the side stream.
* one ``MCDSolver.step`` against one ``adapt_trainer.dropin_step``; the trainer, a resumed epoch and the tester end to end.
"""
import os

import numpy as np
import pytest
import torch

import fusenet_ref as R
from recipe import fill_state_, make_batch

pytestmark = pytest.mark.gpu

FACTOR, TRUNK_FLOOR = 2.0, 2e-5
# the COMMON flags of tests/test_trainers_gpu.py
COMMON = ["--input_ch", "6", "-b", "2", "--train_img_shape", "96", "64", "--synthetic", "--synthetic_len", "4",
          "--no_pretrained", "--no_tflog", "--epochs", "1", "--max_iter", "10"]
PIECES = {"f16x3": 2, "f16x1": 2, "bf16x6": 3}
# (h, w): HW = 1, 63 (one partial block), 256 (exact; the 16-byte form: HW % 4 == 0), 257 (a one-pixel tail), 527 (several blocks and a
# tail), and for the 16-byte form, whose workgroups cover 1024 pixels: 1028 (a one-quad tail), 2048 (exact blocks)
PLANES = ((1, 1), (7, 9), (16, 16), (1, 257), (17, 31), (4, 257), (32, 64))


@pytest.fixture(autouse=True)
def _no_pretrained(monkeypatch):
    monkeypatch.setenv("MCDSEG_PRETRAINED", "0")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _tiny_g(dev):
    from models.dilated_fcn import FuseDRNSegBase
    m = FuseDRNSegBase(R.register_tiny(), R.TINY["n_class"], pretrained=False, input_ch=6)
    return R.tiny_state(m).to(dev)


# ------------------------------------------------------------------------------------------------ the kernel, exact
def _values(kind, shape, gen):
    """(a, b, bound_a, bound_b) on the CPU"""
    a = torch.randn(shape, generator=gen) * 3.0
    b = torch.randn(shape, generator=gen) * 0.7 + 0.2
    if kind == "cancel":      # an all-zero sum under a non-zero bound
        b = -a
    elif kind == "subnormal":  # sums in the fp32 subnormal range
        a, b = a * 1e-39, b * 1e-39
    ba, bb = a.abs().max(), b.abs().max()
    if kind == "on_bound":    # entries with a = bound_a and b = bound_b: the sum sits exactly on the bound
        fa, fb = a.view(-1), b.view(-1)
        idx = torch.arange(0, fa.numel(), max(1, fa.numel() // 7))
        sign = torch.where(idx % 2 == 0, 1.0, -1.0)
        fa[idx], fb[idx] = ba * sign, bb * sign
    elif kind == "loose":     # bounds as a producer supplies them: upper bounds, not maxima
        ba, bb = ba * 3.3, bb * 1.9
    return a, b, ba.reshape(1).clone(), bb.reshape(1).clone()


def _raw_join(ops, a, ab, b, bb, want_cb, scaled):
    n, c, h, w = a.shape
    y = torch.full_like(a, float("nan"))
    cb = torch.full((PIECES[ops.CONV_MATH] * a.numel(),), 0x7e00, dtype=torch.int16, device=a.device) if want_cb else None
    yb = torch.full((1,), float("nan"), device=a.device) if scaled else None
    ops.check(ops.lib().mcdseg_stage_join(ops._p(a), ops._p(ab) if scaled else None, ops._p(b), ops._p(bb) if scaled else None, ops._p(y),
                                          ops._p(cb), ops._p(yb), ops.MATH_ID.get(ops.CONV_MATH, 0), n, c, h * w, None), "stage_join")
    return y, cb, yb


@pytest.mark.parametrize("kind", ["random", "loose", "cancel", "on_bound", "subnormal"])
@pytest.mark.parametrize("math", ["f16x3", "f16x1", "bf16x6", "f32"])
def test_stage_join_kernel_is_exact(math, kind, monkeypatch):
    dev = _dev()
    from mcdseg import ops
    monkeypatch.setattr(ops, "CONV_MATH", math)
    scaled, want_cb = math in ("f16x3", "f16x1"), math != "f32"
    gen = torch.Generator().manual_seed(5)
    channels = (16, 24, 512) + ((41,) if math == "f32" else ())
    seen = 0
    for c in channels:
        for h, w in PLANES:
            for n in (1, 3):
                if c == 512 and h * w > 600 and n == 3:
                    continue  # (the 16-byte form's block decoding is covered at the smaller widths)
                a, b, ba, bb = _values(kind, (n, c, h, w), gen)
                want_y = a + b  # IEEE fp32 on the host, subnormals kept
                want_bound = ba + bb
                a, b, ba, bb = (t.to(dev) for t in (a, b, ba, bb))
                torch.cuda.synchronize()  # (the kernel runs on the null stream)
                y, cb, yb = _raw_join(ops, a, ba, b, bb, want_cb, scaled)
                y2, cb2, yb2 = _raw_join(ops, a, ba, b, bb, want_cb, scaled)
                torch.cuda.synchronize()
                what = (math, kind, n, c, h, w)
                assert _same_bits(y.cpu(), want_y), what
                assert _same_bits(y, y2), what
                if kind == "cancel":
                    assert not y.any(), what
                if scaled:
                    assert _same_bits(yb.cpu(), want_bound) and _same_bits(yb, yb2), what
                if want_cb:
                    ref_cb, ref_bound = ops.split_companion(y, yb)
                    torch.cuda.synchronize()
                    assert ref_cb is not None and _same_bits(cb, ref_cb), what
                    assert _same_bits(cb, cb2), what
                    pieces = cb.view(torch.float16 if scaled else torch.bfloat16).float()
                    assert torch.isfinite(pieces).all(), what  # no piece overflows, on the bound included
                    if kind == "cancel":
                        assert not pieces.any(), what
                    if kind == "on_bound" and scaled:
                        assert float(y.abs().max()) == float(want_bound), what
                seen += 1
    assert seen >= 36


def test_stage_join_kernel_off_the_16_byte_grid(monkeypatch):
    """HW % 4 == 0 but pointers 4 bytes off the 16-byte grid: the one-pixel form, the same bits"""
    dev = _dev()
    from mcdseg import ops
    monkeypatch.setattr(ops, "CONV_MATH", "f16x3")
    gen = torch.Generator().manual_seed(6)
    n, c, h, w = 2, 24, 16, 20
    a, b, ba, bb = (t.to(dev) for t in _values("random", (n, c, h, w), gen))
    numel = a.numel()
    oa, ob = torch.empty(numel + 1, device=dev)[1:].view(n, c, h, w), torch.empty(numel + 1, device=dev)[1:].view(n, c, h, w)
    oa.copy_(a), ob.copy_(b)
    assert oa.data_ptr() % 16 == 4 and oa.is_contiguous()
    torch.cuda.synchronize()
    y, cb, yb = _raw_join(ops, a, ba, b, bb, True, True)
    y2, cb2, yb2 = _raw_join(ops, oa, ba, ob, bb, True, True)
    torch.cuda.synchronize()
    assert _same_bits(y, y2) and _same_bits(cb, cb2) and _same_bits(yb, yb2)
    assert _same_bits(y.cpu(), a.cpu() + b.cpu())


# ------------------------------------------------------------------------------------------------ ops.stage_join
@pytest.mark.parametrize("math", ["f16x3", "bf16x6", "f32"])
@pytest.mark.parametrize("bounds", ["measured", "supplied"])
def test_ops_stage_join_gradients_and_the_composed_form(math, bounds, monkeypatch):
    dev = _dev()
    from mcdseg import ops
    monkeypatch.setattr(ops, "CONV_MATH", math)
    gen = torch.Generator().manual_seed(7)
    out = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("MCDSEG_FUSED_JOIN", fused)
        a0, b0, ba, bb = (t.to(dev) for t in _values("loose", (3, 24, 9, 11), torch.Generator().manual_seed(7)))
        a, b = a0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
        ua, ub = a * 1.0, b * 1.0  # (non-leaf inputs, as the stage outputs are)
        if bounds == "supplied":
            ua._mcd_cb = (None, ba, ua._version, ua.data_ptr())
            ub._mcd_cb = (None, bb, ub._version, ub.data_ptr())
        y = ops.stage_join(ua, ub)
        cb, bound = ops._cb_of(y)
        g = torch.randn(y.shape, generator=gen).to(dev)
        y.backward(g)
        assert _same_bits(a.grad, g) and _same_bits(b.grad, g)
        assert _same_bits(y, a0 + b0)
        assert (cb is not None) == (math != "f32") and (bound is not None) == (math == "f16x3")
        if math == "f16x3":
            want = (ba + bb) if bounds == "supplied" else (a0.abs().max() + b0.abs().max()).reshape(1)
            assert _same_bits(bound, want)
        out[fused] = (y, cb, bound)
    for t1, t0 in zip(out["1"], out["0"]):
        assert (t1 is None) == (t0 is None)
        if t1 is not None:
            assert _same_bits(t1, t0)


def test_ops_stage_join_without_grad_on_bare_inputs_writes_y_only(monkeypatch):
    dev = _dev()
    from mcdseg import ops
    monkeypatch.setattr(ops, "CONV_MATH", "f16x3")
    a, b = torch.randn(1, 16, 5, 7, device=dev), torch.randn(1, 16, 5, 7, device=dev)
    with torch.no_grad():
        y = ops.stage_join(a, b)
    assert ops._cb_of(y) == (None, None) and _same_bits(y, a + b)


# ------------------------------------------------------------------------------------------------ the model against the reference
@pytest.fixture(scope="module")
def fx():
    return R.load_golden()[0]


def _hold(got, fx, case, names, what):
    worst = []
    for k in names:
        truth, unit = fx["%s/f64/%s" % (case, k)], float(fx["%s/unit/%s" % (case, k)])
        err = R.rel_to_max(got[k], truth)
        print("%s %-44s kernel %.3e  the reference's fp32 (the unit) %.3e  ratio %.2f  of the bound max(2 units, %.0e) %.2f"
              % (what, k, err, unit, err / unit if unit > 0 else float(err > 0), TRUNK_FLOOR, err / max(FACTOR * unit, TRUNK_FLOOR)))
        if err > max(FACTOR * unit, TRUNK_FLOOR):
            worst.append((k, err, unit))
    assert not worst, (what, worst)


@pytest.mark.parametrize("case", R.CASES)
def test_model_against_the_reference(case, fx, monkeypatch):
    dev = _dev()
    from mcdseg import ops
    g = _tiny_g(dev)
    before = {k: v.detach().clone() for k, v in g.state_dict().items()}
    names = []

    class _Names:
        def wants(self, nm):
            names.append(nm)
            return False
    monkeypatch.setattr(ops, "LAUNCH_TIMER", _Names())
    got = R.run_case(g, case, fx["x"], fx["dy"])
    torch.cuda.synchronize()
    monkeypatch.setattr(ops, "LAUNCH_TIMER", None)
    stored = [k[len(case) + 5:] for k in fx.files if k.startswith(case + "/f64/")]
    assert sorted(stored) == sorted(got)
    counters = [k for k in stored if k.endswith("num_batches_tracked")]
    assert len(counters) == 16
    for k in counters:
        assert int(got[k]) == int(fx["%s/f64/%s" % (case, k)]) == (2 if case == "train" else 0), k
    _hold(got, fx, case, [k for k in stored if k not in counters], "tiny-" + case)
    after = g.state_dict()
    if case != "train":  # fixed / eval-mode BatchNorms leave the running statistics bitwise alone
        for k in before:
            if k.split(".")[-1] in ("running_mean", "running_var", "num_batches_tracked"):
                assert torch.equal(before[k], after[k]), k
    for k in before:  # nothing of sub_layer* is ever touched
        if k.startswith("sub_layer"):
            assert torch.equal(before[k], after[k]), k
    # nine joins per forward; the no-grad eval forward runs them in the y-only form behind the folded-BN inference kernels
    assert names.count("stage_join") == 9, names.count("stage_join")


@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_sub_layers_stay_bitwise_through_an_optimizer_step(opt, fx):
    dev = _dev()
    from models.model_util import get_optimizer
    g = _tiny_g(dev)
    o = get_optimizer(g.parameters(), opt, 1e-2, 0.9, 1e-2)  # (a weight decay that would show)
    before = {k: v.detach().clone() for k, v in g.state_dict().items()}
    g.train()
    score = g(torch.as_tensor(fx["x"]).to(dev))
    score.backward(torch.as_tensor(fx["dy"]).to(dev))
    assert all(p.grad is None for k, p in g.named_parameters() if k.startswith("sub_layer"))
    assert all(p.grad is not None for k, p in g.named_parameters() if not k.startswith("sub_layer"))
    o.step()
    torch.cuda.synchronize()
    after = g.state_dict()
    moved = 0
    for k in before:
        if k.startswith("sub_layer"):
            assert torch.equal(before[k], after[k]), k
        elif k.split(".")[-1] in ("weight", "bias"):
            moved += int(not torch.equal(before[k], after[k]))
    assert moved == sum(1 for k, _ in g.named_parameters() if not k.startswith("sub_layer"))


# ------------------------------------------------------------------------------------------------ fused against composed
def _forward_backward(g, x, dy):
    g.zero_grad()
    score = g(x)
    score.backward(dy)
    torch.cuda.synchronize()
    out = {"score": score.detach().clone()}
    out.update(("grad/" + k, p.grad.detach().clone()) for k, p in g.named_parameters() if p.grad is not None)
    out.update(("state/" + k, v.detach().clone()) for k, v in g.state_dict().items() if "running_" in k or k.endswith("num_batches_tracked"))
    return out


def _differing(a, b, prefix=""):
    assert a.keys() == b.keys()
    return [k for k in a if k.startswith(prefix) and not (torch.equal(a[k], b[k]) if not a[k].dtype.is_floating_point else _same_bits(a[k], b[k]))]


def test_fused_join_against_composed_on_drn_d_22(monkeypatch):
    dev = _dev()
    from mcdseg import ops
    from models.model_util import get_models
    src, _, _ = make_batch(41, 2, 6, 64, 96, 41)
    x = src.to(dev)
    dy = (torch.randn(2, 41, 8, 12, generator=torch.Generator().manual_seed(3)) / (2 * 8 * 12)).to(dev)
    # what holds on the existing trunk decides what is claimed between the two weight-gradient modes
    base = get_models("drn_d_22", 6, 41)[0]
    fill_state_(base, 11)
    base.to(dev).train()
    state = {k: v.detach().clone() for k, v in base.state_dict().items()}
    runs = {}
    for overlap in ("0", "2"):
        monkeypatch.setattr(ops, "OVERLAP_WGRAD", overlap)
        base.load_state_dict(state)
        runs[overlap] = _forward_backward(base, x, dy)
    base_grads_differ = _differing(runs["0"], runs["2"], "grad/")
    print("DRNSegBase, MCDSEG_OVERLAP_WGRAD 0 against 2: %d gradients differ in bits" % len(base_grads_differ))
    del base, runs

    g = get_models("drn_d_22_fusenet", 6, 41)[0]
    fill_state_(g, 11)
    g.to(dev).train()
    state = {k: v.detach().clone() for k, v in g.state_dict().items()}
    runs = {}
    for overlap in ("0", "2"):
        for fused in ("1", "0"):
            monkeypatch.setattr(ops, "OVERLAP_WGRAD", overlap)
            monkeypatch.setenv("MCDSEG_FUSED_JOIN", fused)
            g.load_state_dict(state)
            runs[overlap, fused] = _forward_backward(g, x, dy)
    for overlap in ("0", "2"):
        assert not _differing(runs[overlap, "1"], runs[overlap, "0"]), overlap
        counters = [v for k, v in runs[overlap, "1"].items() if k.endswith("num_batches_tracked") and k.startswith("state/main")]
        assert counters and all(int(v) == 2 for v in counters)
        assert all(torch.isfinite(v).all() for v in runs[overlap, "1"].values())
    assert len([k for k in runs["0", "1"] if k.startswith("grad/")]) == sum(1 for k, _ in g.named_parameters() if not k.startswith("sub_layer"))
    across = _differing(runs["0", "1"], runs["2", "1"])
    print("FuseDRNSegBase, MCDSEG_OVERLAP_WGRAD 0 against 2: %d tensors differ in bits" % len(across))
    assert not _differing(runs["0", "1"], runs["2", "1"], "score") and not _differing(runs["0", "1"], runs["2", "1"], "state/")
    if not base_grads_differ:  # both weight gradients of every convolution are complete and summed, wherever the first one ran
        assert not across, across[:5]


# ------------------------------------------------------------------------------------------------ one MCD step
def _checksums(mod):
    return {k: (float(v.double().sum()), float(v.double().norm())) for k, v in mod.state_dict().items()}


def _same_state(mod, ref, rtol):
    """the comparison of tests/test_prob_distance_gpu.py: every state tensor's sum and norm"""
    got, want = _checksums(mod), _checksums(ref)
    assert got.keys() == want.keys()
    numel = {k: v.numel() for k, v in mod.state_dict().items()}
    bad = [(k, got[k][1], l2) for k, (s, l2) in want.items() if abs(got[k][1] - l2) > rtol * max(abs(l2), 1e-6)]
    assert not bad, bad[:5]
    bad = [(k, got[k][0], s) for k, (s, l2) in want.items() if abs(got[k][0] - s) > rtol * max(abs(l2), 1e-6) * max(numel[k], 1) ** 0.5]
    assert not bad, bad[:5]


def test_solver_step_against_the_drop_in_loop():
    dev = _dev()
    import adapt_trainer
    from loss import CrossEntropyLoss2d, get_prob_distance_criterion
    from models.dilated_fcn import DRNSegPixelClassifier
    from models.model_util import get_optimizer
    from solvers.solver import MCDSolver
    nc, num_k = R.TINY["n_class"], 2
    n, ch, h, w = R.TINY["shape"]
    s, l, t = (v.to(dev) for v in make_batch(31, n, ch, h, w, nc))
    cw = torch.ones(nc)
    cw[nc - 1] = 0
    ce = CrossEntropyLoss2d(cw.to(dev))

    def models():
        g = _tiny_g(dev).train()
        fs = [fill_state_(DRNSegPixelClassifier(n_class=nc), seed).to(dev).train() for seed in (12, 13)]
        og = get_optimizer(g.parameters(), "sgd", 1e-3, 0.9, 2e-5)
        of = get_optimizer(list(fs[0].parameters()) + list(fs[1].parameters()), "sgd", 1e-3, 0.9, 2e-5)
        return g, fs[0], fs[1], og, of
    g, f1, f2, og, of = models()
    rg, rf1, rf2, rog, rof = models()
    solver = MCDSolver(g, f1, f2, og, of, ce, get_prob_distance_criterion("diff"), num_k=num_k)
    assert not solver.reuse_tgt and not solver.fork_ok  # the literal schedule: HHA, RGB, HHA, RGB
    c_loss, d_loss = solver.step(s, l, t)
    rc, rd = adapt_trainer.dropin_step(rg, rf1, rf2, rog, rof, ce, get_prob_distance_criterion("diff"), s, l, t, num_k, 1)
    torch.cuda.synchronize()
    c_loss, d_loss, rc, rd = float(c_loss), float(d_loss), float(rc), float(rd)
    print("c_loss %.7f vs %.7f, d_loss %.6e vs %.6e" % (c_loss, rc, d_loss, rd))
    for m in (g, rg):
        counters = {k: int(v) for k, v in m.state_dict().items() if k.endswith("num_batches_tracked")}
        assert all(v == 2 * (3 + num_k) for k, v in counters.items() if k.startswith("main_layer")), counters
        assert all(v == 0 for k, v in counters.items() if k.startswith("sub_layer")), counters
    assert abs(c_loss - rc) <= 1e-4 * abs(rc)
    assert abs(d_loss - rd) <= 2e-3 * abs(rd)
    _same_state(g, rg, 3e-4), _same_state(f1, rf1, 3e-4), _same_state(f2, rf2, 3e-4)


# ------------------------------------------------------------------------------------------------ trainer, resume, tester
def test_trainer_resume_and_tester(tmp_path):
    _dev()
    import adapt_tester
    import adapt_trainer
    import util
    from PIL import Image
    out = str(tmp_path / "out")
    assert adapt_trainer.main(["suncg", "nyu", "--base_outdir", out, "--net", "drn_d_22_fusenet"] + COMMON) == 0
    d = os.path.join(out, "suncg-train2nyu-train_6ch")
    ck_fn = os.path.join(d, "pth", "MCD-normal-drn_d_22_fusenet-1.pth.tar")
    ck = util.load_checkpoint(ck_fn)
    assert sorted(ck.keys()) == ["args", "epoch", "f1_state_dict", "f2_state_dict", "g_state_dict", "optimizer_f", "optimizer_g"]
    assert ck["args"].net == "drn_d_22_fusenet" and ck["epoch"] == 1
    gsd = ck["g_state_dict"]
    assert "sub_layer8.0.weight" in gsd and "main_layer8.0.weight" in gsd and "seg.bias" in gsd
    assert int(gsd["main_layer0.1.num_batches_tracked"]) == 2 * 14  # 2 iterations x 7 forwards x 2 calls
    assert int(gsd["sub_layer0.1.num_batches_tracked"]) == 0
    assert all(torch.isfinite(v).all() for v in gsd.values() if v.dtype.is_floating_point)
    live = sum(1 for k in gsd if not k.startswith("sub_layer") and k.split(".")[-1] in ("weight", "bias"))
    assert len(ck["optimizer_g"]["state"]) == len(ck["optimizer_g"]["param_groups"][0]["params"]) == live
    ck["args"].epochs = 2
    util.save_checkpoint(ck, False, ck_fn)
    assert adapt_trainer.main(["suncg", "nyu", "--resume", ck_fn] + COMMON) == 0
    ck2 = util.load_checkpoint(os.path.join(d, "pth", "MCD-normal-drn_d_22_fusenet-2.pth.tar"))
    assert ck2["epoch"] == 2 and int(ck2["g_state_dict"]["main_layer0.1.num_batches_tracked"]) == 4 * 14
    assert all(torch.equal(ck2["g_state_dict"][k], gsd[k]) for k in gsd if k.startswith("sub_layer"))
    res = adapt_tester.main(["nyu", ck_fn, "--synthetic", "--synthetic_len", "2", "--outdir", str(tmp_path / "test"),
                             "--test_img_shape", "80", "56"])
    label_dir, ave_ent = res[:2]
    names = sorted(os.listdir(label_dir))
    assert len(names) == 2 and all(Image.open(os.path.join(label_dir, nm)).size == (80, 56) for nm in names)
    assert np.isfinite(ave_ent) and os.path.exists(os.path.join(os.path.dirname(label_dir), "eval_result.json"))
