"""GPU: the one-pass Monte-Carlo dropout loss (csrc/uncertain.hip, ops.up8_uncertain_loss / up8_std_sum), UncertainDRNSeg.get_loss in
its fused and literal forms, and the uncertain trainer / tester end to end.

The tolerance rule is the project's for grad_truth_*: per output tensor, the kernel's distance to the fp64 truth in units of the
distance of the fp32 LITERAL composition on the CPU (tests/uncertain_ref.literal, dtype float32) to the same truth, both relative to
the truth's largest magnitude.  The kernel may be a factor 2 further than that unit (it sums the T terms in another order); where the
literal form happens to be exact -- within 2 ulps of the truth itself -- the floor is 4 fp32 ulps of the tensor's largest magnitude, and
``hold`` names every output that passes on the floor and not on the factor.  Measured ratios: docs/MEASURED_HISTORY.md.
"""
import functools
import os

import numpy as np
import pytest
import torch

import uncertain_ref as R

pytestmark = pytest.mark.gpu

OUTPUTS = ("B", "U", "ds", "dw_up", "dw_std")
FACTOR = 2.0
FLOOR = 4 * 2.0 ** -23
# The gradients of the trunk's parameters pass the split-precision (f16x3) convolution kernels, which this variant does not touch.  The
# project's rule for them (tests/truth.summary, the grad_truth_* tests) puts a floor of 2e-5 of the tensor's scale -- those kernels' own
# accuracy bound -- under the fp32 oracle's distance; the same floor stands here in place of the 4 ulps.
TRUNK_FLOOR = 2e-5


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def run_kernel(d, dev):
    """ops.up8_uncertain_loss forward + backward under the upstream gradients of ``d``"""
    from mcdseg import ops
    t = lambda a, dt=torch.float32: torch.as_tensor(np.asarray(a)).to(dt).to(dev)
    s, w_up, w_std = (t(d[k]).requires_grad_(True) for k in ("s", "w_up", "w_std"))
    wsum = None if d.get("wsum") is None else t(d["wsum"])
    B, U = ops.up8_uncertain_loss(s, w_up, w_std, t(d["labels"], torch.int64), t(d["cw"]), t(d["keep"], torch.uint8), t(d["r"]), d["lam"],
                                  R.IGNORE, wsum=wsum)
    (B * float(d["gb"]) + (U * t(d["gu"])).sum()).backward()
    torch.cuda.synchronize()
    return {"B": B.detach().cpu().numpy(), "U": U.detach().cpu().numpy(), "ds": s.grad.cpu().numpy(), "dw_up": w_up.grad.cpu().numpy(),
            "dw_std": w_std.grad.cpu().numpy()}


def cpu_forms(d):
    """(fp64 truth, fp32 unit): the literal composition on the CPU in both precisions (tests/test_uncertain_host.py holds the one-pass
    formulas to the same truth on these inputs)"""
    a = (d["s"], d["w_up"], d["w_std"], d["labels"], d["cw"], d["keep"], d["r"])
    kw = dict(lam=d["lam"], gb=d["gb"], gu=d["gu"], wsum=d.get("wsum"))
    return R.literal(*a, dtype=torch.float64, **kw), R.literal(*a, dtype=torch.float32, **kw)


def hold(got, truth, lit32, what, outputs=OUTPUTS, floor=FLOOR):
    """every output within max(FACTOR units, floor); those beyond FACTOR units that pass on the floor alone -- the fp32 literal form
    then sits within floor / FACTOR of the truth itself -- are named in the output and returned"""
    worst, on_floor = [], []
    for k in outputs:
        err, unit = R.rel_to_max(got[k], truth[k]), R.rel_to_max(lit32[k], truth[k])
        by_floor = FACTOR * unit < err <= floor
        print("%s %-6s kernel %.3e  fp32 literal (the unit) %.3e  ratio %.2f  of the bound max(2 units, %.1e) %.2f%s"
              % (what, k, err, unit, err / unit if unit > 0 else float(err > 0), floor, err / max(FACTOR * unit, floor),
                 "  PASSES ON THE FLOOR, NOT THE FACTOR (%.1f ulp)" % (err * 2.0 ** 23) if by_floor else ""))
        if by_floor:
            on_floor.append(k)
        if err > max(FACTOR * unit, floor):
            worst.append((k, err, unit))
    if on_floor:
        print("%s: on the floor: %s" % (what, ", ".join(on_floor)))
    assert not worst, (what, worst)
    return on_floor


def golden_case(fx, name):
    d = {k: fx["%s/%s" % (name, k)] for k in ("s", "w_up", "w_std", "labels", "cw", "keep", "r")}
    d.update(lam=float(fx[name + "/lam"]), gb=float(fx[name + "/gb"]), gu=fx[name + "/gu"], wsum=None)
    return d


@pytest.mark.parametrize("name", ["a", "b"])
def test_kernel_against_the_references_fp64_results(golden, device, name):
    fx = golden.npz("uncertain_small.npz")
    d = golden_case(fx, name)
    assert R.conditions(d)
    _, lit32 = cpu_forms(d)
    hold(run_kernel(d, device), {k: fx["%s/f64/%s" % (name, k)] for k in OUTPUTS}, lit32, "golden-" + name)


@functools.lru_cache(maxsize=None)
def _extra(c, t, variant):
    d = R.extra_case(c, t, variant)
    assert R.conditions(d)
    return (d,) + cpu_forms(d)


@pytest.mark.parametrize("variant", R.VARIANTS)
@pytest.mark.parametrize("c,t", [(20, 1), (20, 4), (48, 1), (48, 4)])
def test_kernel_on_dropped_ignored_and_zero_gradient_inputs(device, c, t, variant):
    """a draw that drops the label's channel, a sample with every channel dropped in one draw, labels equal to ignore_index and to
    C, and per variant: wsum_in given / gb = 0 / gu = 0"""
    d, truth, lit32 = _extra(c, t, variant)
    got = run_kernel(d, device)
    hold(got, truth, lit32, "extra-%d-%d-%s" % (c, t, variant))
    if variant == "gu0":
        assert not got["dw_std"].any()  # GV carries b_t only
    if variant == "wsum":
        assert truth["W"] == 777.0


def test_results_are_bit_reproducible(device):
    d = R.extra_case(20, 4, "plain")
    first, second = run_kernel(d, device), run_kernel(d, device)
    for k in OUTPUTS:
        assert np.array_equal(first[k], second[k]), k


def test_std_sum(device):
    from mcdseg import ops
    d = R.extra_case(20, 1, "plain")
    s, w = torch.as_tensor(d["s"]).to(device), torch.as_tensor(d["w_std"]).to(device)
    for n_used in (19, 7):
        got = ops.up8_std_sum(s, w, n_used).cpu().numpy()
        truth = R.std_sum(d["s"], d["w_std"], n_used)
        lit32 = R.std_sum(d["s"], d["w_std"], n_used, dtype=torch.float32)
        hold({"std": got}, {"std": truth}, {"std": lit32}, "std_sum-%d" % n_used, outputs=("std",))
        two_step = torch.relu(ops.up8(s, w))[:, :n_used].sum(1).cpu().numpy()
        assert R.rel_to_max(got, two_step) <= FLOOR  # (the same multiply-adds; only the order of the class sum differs)
    assert tuple(ops.up8_std_sum(s, w).shape) == (2, 24, 72)


# ------------------------------------------------------------------------------------------------ the model: fused against literal
def _model_run(dev, fused, monkeypatch, x, gt, keep, r, state):
    from models.dilated_fcn import UncertainDRNSeg
    from loss import CrossEntropyLoss2d
    monkeypatch.setenv("MCDSEG_FUSED_UNCERTAIN", "1" if fused else "0")
    cw = torch.linspace(0.5, 1.5, 5)
    cw[-1] = 0.0
    model = UncertainDRNSeg("drn_d_22", 5, input_ch=3, pretrained=False, criterion=CrossEntropyLoss2d(cw), n_dropout_exp=3)
    if state is not None:
        model.load_state_dict(state)
    start = {k: v.clone() for k, v in model.state_dict().items()}
    model.to(dev).train()
    seen = []  # the scores of every trunk pass and their gradients

    def watch(mod, inp, out):
        slot = [out.detach(), None]
        seen.append(slot)

        def keep_grad(g):
            slot[1] = g.detach().clone()
        out.register_hook(keep_grad)
    model.seg.register_forward_hook(watch)
    base, unc = model.get_loss(x.to(dev), gt.to(dev), separately_returning=True, keep=keep.to(dev), r=r.to(dev))
    (base + unc.mean()).backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters()}
    buffers = {k: v.detach().cpu() for k, v in model.state_dict().items() if "running_" in k or "num_batches" in k}
    return dict(B=base.detach().cpu().numpy(), U=unc.detach().cpu().numpy(), grads=grads, buffers=buffers, start=start,
                scores=[s.cpu().numpy() for s, _ in seen], ds=sum(g for _, g in seen).cpu().numpy(), cw=cw.numpy())


def test_get_loss_fused_against_literal(device, monkeypatch):
    """drn_d_22, 3 channels, 32 x 40, N = 2, T = 3, the same keep and r in both forms.

    Both forms run the same trunk kernels on the same input, so the scores behind the trunk are the same bits (asserted).  Losses,
    d/dscores and the two up-samplers' gradients of BOTH forms are held to the fp64 truth of the head (CPU, from those scores), and
    every gradient of the trunk's parameters (base.*, seg.*) of BOTH forms to the fp64 truth of the whole network -- the CPU oracle's
    drn_d_22 from the same weights, run T times by tests/uncertain_ref.literal -- all by the rule at the top of this file, the unit
    being that literal composition in fp32 on the CPU (for the trunk's tensors with TRUNK_FLOOR as the floor).  The scores, the losses
    and the up-samplers' gradients are held to that whole-network truth as well.  Tensors that are zero up to rounding in the truth (a bias in front of a
    train-mode BatchNorm) are left out, as tests/truth.summary leaves them out."""
    monkeypatch.setenv("MCDSEG_PRETRAINED", "0")
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 3, 32, 40, generator=g)
    gt = torch.randint(0, 5, (2, 32, 40), generator=g)
    keep = (torch.rand(3, 2, 5, generator=g) >= 0.2).to(torch.uint8)
    keep[1, 0, 2] = 0
    r = torch.rand(3, generator=g)
    fused = _model_run(device, True, monkeypatch, x, gt, keep, r, None)
    literal = _model_run(device, False, monkeypatch, x, gt, keep, r, fused["start"])
    assert len(fused["scores"]) == 1 and len(literal["scores"]) == 3  # the literal form runs the trunk T times
    assert all(np.array_equal(s, fused["scores"][0]) for s in literal["scores"])
    # running means, variances and num_batches_tracked: bit for bit, and T updates
    assert sorted(fused["buffers"]) == sorted(literal["buffers"]) and fused["buffers"]
    for k, v in fused["buffers"].items():
        assert torch.equal(v, literal["buffers"][k]), k
        if k.endswith("num_batches_tracked"):
            assert int(v) == 3
    # the head of both forms against its fp64 truth
    st = fused["start"]
    d = dict(s=fused["scores"][0], w_up=st["up.weight"].numpy(), w_std=st["up_std.weight"].numpy(), labels=gt.numpy(), cw=fused["cw"],
             keep=keep.numpy(), r=r.numpy(), lam=0.1, gb=1.0, gu=np.full(2, 0.5), wsum=None)
    truth, lit32 = cpu_forms(d)
    for name, run in (("fused", fused), ("literal", literal)):
        got = dict(B=run["B"], U=run["U"], ds=run["ds"], dw_up=run["grads"]["up.weight"], dw_std=run["grads"]["up_std.weight"])
        hold(got, truth, lit32, "get_loss-" + name)
    # the trunk's parameter gradients against the fp64 truth of the whole network
    from oracle import ref_models
    forms = {}
    for dtype in (torch.float64, torch.float32):
        trunk = ref_models.DRNSegBase("drn_d_22", 5, 3)
        trunk.load_state_dict({k: v for k, v in st.items() if k.startswith(("base.", "seg."))})
        trunk.to(dtype).train()
        with torch.no_grad():
            forms[dtype, "scores"] = trunk(x.to(dtype)).numpy()
        trunk.load_state_dict({k: v for k, v in st.items() if k.startswith(("base.", "seg."))})  # (the running statistics moved)
        forms[dtype] = R.literal(x.numpy(), d["w_up"], d["w_std"], d["labels"], d["cw"], d["keep"], d["r"], lam=0.1, gb=1.0, gu=d["gu"],
                                 dtype=dtype, trunk=trunk)
    hold({"scores": fused["scores"][0]}, {"scores": forms[torch.float64, "scores"]}, {"scores": forms[torch.float32, "scores"]},
         "get_loss-trunk", outputs=("scores",))
    for name, run in (("fused", fused), ("literal", literal)):
        got = dict(B=run["B"], U=run["U"], dw_up=run["grads"]["up.weight"], dw_std=run["grads"]["up_std.weight"])
        hold(got, forms[torch.float64], forms[torch.float32], "get_loss-%s-network" % name, outputs=("B", "U", "dw_up", "dw_std"))
    truth_net, lit32_net = forms[torch.float64]["trunk"], forms[torch.float32]["trunk"]
    names = [k for k in fused["grads"] if k.startswith(("base.", "seg."))]
    assert sorted(names) == sorted(truth_net)
    top = max(float(np.abs(v).max()) for v in truth_net.values())
    live = [k for k in names if float(np.abs(truth_net[k]).max()) > 1e-9 * top]
    assert len(live) >= 40
    for name, run in (("fused", fused), ("literal", literal)):
        hold(run["grads"], truth_net, lit32_net, "get_loss-%s-trunk" % name, outputs=live, floor=TRUNK_FLOOR)


# ------------------------------------------------------------------------------------------------ trainer, resume, tester
def test_trainer_resume_and_tester(tmp_path, capsys):
    _need_gpu()
    import source_uncertain_tester
    import source_uncertain_trainer
    import util
    from PIL import Image
    out = str(tmp_path / "out")
    flags = ["--synthetic", "--no_pretrained", "-b", "2", "--train_img_shape", "64", "48", "--n_dropout", "3", "--max_iter", "2",
             "--epochs", "1", "--no_tflog", "--synthetic_len", "8"]
    assert source_uncertain_trainer.main(["suncg", "--base_outdir", out] + flags) == 0
    pth = os.path.join(out, "suncg-train_only_3ch_uncertain", "pth")
    ck_fn = os.path.join(pth, "normal-drn_d_38-1.pth.tar")
    ck = util.load_checkpoint(ck_fn)
    assert sorted(ck) == ["args", "epoch", "optimizer", "state_dict"] and ck["args"].n_dropout == 3
    assert "up_std.weight" in ck["state_dict"] and not any(k.startswith("module.") for k in ck["state_dict"])
    bn = next(k for k in ck["state_dict"] if k.endswith("num_batches_tracked"))
    steps = int(ck["state_dict"][bn]) // 3  # every step moves the running statistics as its 3 passes would
    assert steps >= 1 and int(ck["state_dict"][bn]) == 3 * steps
    printed = capsys.readouterr().out
    line = next(ln for ln in printed.splitlines() if ln.startswith("iter [0] TotalLoss:"))
    assert all(np.isfinite(float(tok.rstrip(")"))) for tok in line.replace("(", " ").split() if tok[0].isdigit() or tok[0] == "-")
    assert all(torch.isfinite(v).all() for v in ck["state_dict"].values() if v.dtype.is_floating_point)
    # resume: the uncertain model is rebuilt and loaded, and trains on
    ck["args"].epochs = 2
    util.save_checkpoint(ck, False, ck_fn)
    assert source_uncertain_trainer.main(["suncg", "--resume", ck_fn] + flags) == 0
    ck2 = util.load_checkpoint(os.path.join(pth, "normal-drn_d_38-2.pth.tar"))
    assert list(ck2["state_dict"]) == list(ck["state_dict"]) and int(ck2["state_dict"][bn]) == 2 * int(ck["state_dict"][bn])
    # the tester on that checkpoint
    test_out = str(tmp_path / "test")
    label_dir, unc_dir, ave_ent = source_uncertain_tester.main(["nyu", ck_fn, "--synthetic", "--synthetic_len", "2", "--outdir", test_out,
                                                                "--test_img_shape", "80", "56", "---saves_prob"])
    assert np.isfinite(ave_ent)
    base = os.path.dirname(label_dir)
    names = sorted(os.listdir(label_dir))
    assert len(names) == 2 and os.path.exists(os.path.join(base, "ave_ent_%s.txt" % ave_ent)) and os.path.exists(os.path.join(base, "param.json"))
    for name in names:
        stem = os.path.splitext(name)[0]
        assert Image.open(os.path.join(label_dir, name)).size == (80, 56)
        png = Image.open(os.path.join(unc_dir, stem + ".png"))
        assert png.size == (80, 56) and png.mode == "RGB"
        std = np.load(os.path.join(unc_dir, stem + ".npy"))
        assert std.shape == (48, 64) and std.dtype == np.float32 and np.isfinite(std).all() and (std >= 0).all()
        assert os.path.exists(os.path.join(base, "prob", stem + ".npy"))
    assert os.path.exists(os.path.join(base, "eval_result.json"))
