"""CPU: the uncertain source-only variant without a GPU -- the formulas against the reference's recorded fp64 results, the C ABI's new
entries and their argument errors, the trainer's parser / output layout / checkpoint keys, and UncertainDRNSeg's state dict."""
import argparse
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import uncertain_ref as R

CASES = ("a", "b")
OUTPUTS = ("B", "U", "ds", "dw_up", "dw_std")


def case_inputs(fx, name):
    d = {k: fx["%s/%s" % (name, k)] for k in ("s", "w_up", "w_std", "labels", "cw", "keep", "r")}
    d.update(lam=float(fx[name + "/lam"]), gb=float(fx[name + "/gb"]), gu=fx[name + "/gu"], wsum=None)
    return d


@pytest.fixture(scope="module")
def fx(golden):
    return golden.npz("uncertain_small.npz")


# ------------------------------------------------------------------------------------------------ the formulas
@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("form", ["one_pass", "literal"])
def test_restatement_equals_the_reference_in_fp64(fx, name, form):
    """one trunk pass + the closed-form gradients == the reference's T-pass loop (recorded from the real reference, fp64)"""
    d = case_inputs(fx, name)
    assert R.conditions(d)
    assert (d["keep"].min(2) == 0).any() and d["cw"][-1] == 0.0
    got = getattr(R, form)(d["s"], d["w_up"], d["w_std"], d["labels"], d["cw"], d["keep"], d["r"], lam=d["lam"], gb=d["gb"], gu=d["gu"])
    for k in OUTPUTS:
        assert R.rel_to_max(got[k], fx["%s/f64/%s" % (name, k)]) <= 1e-12, k


@pytest.mark.parametrize("variant", R.VARIANTS)
@pytest.mark.parametrize("c,t", [(20, 1), (20, 4), (48, 1), (48, 4)])
def test_one_pass_equals_the_literal_loop_on_the_extra_inputs(c, t, variant):
    """ignored labels, labels equal to C, a fully dropped sample, wsum given, gb = 0, gu = 0: the closed forms against T real passes"""
    d = R.extra_case(c, t, variant)
    a = (d["s"], d["w_up"], d["w_std"], d["labels"], d["cw"], d["keep"], d["r"])
    kw = dict(lam=d["lam"], gb=d["gb"], gu=d["gu"], wsum=d["wsum"])
    one, lit = R.one_pass(*a, **kw), R.literal(*a, **kw)
    for k in OUTPUTS + ("W",):
        assert R.rel_to_max(one[k], lit[k]) <= 1e-12, k


def test_conditions_hold_for_the_extra_inputs():
    for c in (20, 48):
        for t in (1, 4):
            d = R.extra_case(c, t, "plain")
            assert R.conditions(d)
            assert d["keep"][0, 0, d["labels"][0, 0, 0]] == 0 and d["keep"][t - 1, 1].max() == 0
            assert (d["labels"] == R.IGNORE).any() and (d["labels"] == c).any()


# ------------------------------------------------------------------------------------------------ the C ABI
NEW = ("mcdseg_up8_uncertain_loss_workspace_bytes", "mcdseg_up8_uncertain_loss_fwd", "mcdseg_up8_uncertain_loss_bwd", "mcdseg_up8_std_sum")


def test_new_symbols_are_exported_and_bound():
    import mcdseg
    from mcdseg import _lib
    L = mcdseg.lib()
    for name in NEW:
        assert name in _lib.EXPORTS
        assert getattr(L, name).argtypes is not None
    assert L.mcdseg_version() == 101
    assert "uncertain.hip" in _lib.NO_PACKED_F32


def _fwd(L, T=3, C=5, keep=1, ws_bytes=None, N=2, Hi=3, Wi=5):
    """forward entry with dummy non-null pointers: every call here must fail BEFORE anything is launched"""
    p = ctypes.c_void_p(64)
    need = L.mcdseg_up8_uncertain_loss_workspace_bytes(N, Hi, Wi)
    return L.mcdseg_up8_uncertain_loss_fwd(p, p, p, p, p, -100, ctypes.c_void_p(64) if keep else None, p, 1.25, None, 0.1, p, N, C, Hi, Wi, T,
                                           p, ctypes.c_size_t(need if ws_bytes is None else ws_bytes), None)


@pytest.mark.parametrize("kwargs,word", [(dict(N=65536), "65535 samples"), (dict(T=0), "draws"), (dict(T=33), "draws"), (dict(C=49), "48 classes"), (dict(keep=0), "keep"),
                                         (dict(ws_bytes=4), "workspace too small")])
def test_argument_errors_come_before_any_launch(kwargs, word):
    import mcdseg
    L = mcdseg.lib()
    rc = _fwd(L, **kwargs)
    assert rc < 0
    assert word in L.mcdseg_last_error().decode()


def test_backward_and_std_sum_argument_errors():
    import mcdseg
    L = mcdseg.lib()
    p = ctypes.c_void_p(64)
    for T, C, word in ((0, 5, "draws"), (33, 5, "draws"), (3, 49, "48 classes")):
        assert L.mcdseg_up8_uncertain_loss_bwd(p, p, p, p, p, -100, p, p, 1.25, p, 0.1, p, p, p, p, 2, C, 3, 5, T, None) < 0
        assert word in L.mcdseg_last_error().decode()
    assert L.mcdseg_up8_uncertain_loss_bwd(p, p, p, p, p, -100, p, p, 1.25, p, 0.1, None, p, p, p, 2, 5, 3, 5, 3, None) < 0  # gb NULL
    assert L.mcdseg_up8_std_sum(p, p, p, 2, 5, 6, 3, 5, None) < 0 and "C_used" in L.mcdseg_last_error().decode()
    assert L.mcdseg_up8_std_sum(p, p, None, 2, 5, 4, 3, 5, None) < 0


def test_workspace_bytes_is_positive_and_monotone():
    import mcdseg
    f = mcdseg.lib().mcdseg_up8_uncertain_loss_workspace_bytes
    assert f(0, 3, 5) == 0 and f(2, 0, 5) == 0
    last = 0
    for n, hi, wi in ((1, 1, 1), (1, 3, 5), (2, 3, 5), (2, 30, 40), (4, 30, 40), (4, 90, 160)):
        got = f(n, hi, wi)
        assert got > 0 and got >= last
        last = got


def test_ops_refuse_cpu_tensors_and_wrong_dtypes():
    from mcdseg import ops
    s, w = torch.zeros(1, 5, 2, 2), torch.zeros(5, 1, 16, 16)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.up8_uncertain_loss(s, w, w, torch.zeros(1, 16, 16, dtype=torch.int64), None, torch.ones(3, 1, 5, dtype=torch.uint8), torch.zeros(3))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.up8_std_sum(s, w)


# ------------------------------------------------------------------------------------------------ the trainer's declaration
def _args(extra=()):
    import source_uncertain_trainer as mod
    import trainer_common
    return trainer_common.parse_args(mod.get_parser(), ["suncg", "--base_outdir", "out"] + list(extra))


def test_parser_is_the_source_only_one_plus_n_dropout():
    import argmyparse
    plain = vars(argmyparse.get_src_only_training_parser().parse_args(["suncg"]))
    mine = vars(_args())
    assert mine["n_dropout"] == 10 and vars(_args(["--n_dropout", "3"]))["n_dropout"] == 3
    assert set(mine) - set(plain) == {"n_dropout", "n_class", "machine"} and set(plain) <= set(mine)


def test_output_layout_is_the_reference_scripts():
    import source_uncertain_trainer as mod
    import trainer_common
    for extra, model_name in (([], "normal-drn_d_38"), (["--net", "psp", "--res", "101"], "normal-psp-res101")):
        args = _args(["--input_ch", "6"] + extra)
        outdir = os.path.join("out", "suncg-train_only_6ch_uncertain")
        fresh = mod.TRAINER.layout(args, False)
        assert fresh == trainer_common.Layout(os.path.join(outdir, "pth"), os.path.join(outdir, "tflog", model_name),
                                              os.path.join(outdir, "param-%s.json" % model_name), model_name)
        assert trainer_common.checkpoint_fn(fresh, 1) == os.path.join(outdir, "pth", model_name + "-1.pth.tar")
        resumed = mod.TRAINER.layout(args, True)
        assert resumed[:2] == fresh[:2] and resumed.json_fn == os.path.join(outdir, "param_normal_resume.json")
    assert mod.TRAINER.sums == ("loss", "seg_loss", "uncertain_loss")


def test_backfill_covers_n_dropout():
    import source_uncertain_trainer as mod
    import trainer_common
    cli = _args(["--resume", "x", "--n_dropout", "4", "--seed", "7"])
    got = trainer_common.resumed_args(mod.TRAINER, argparse.Namespace(seed=5), cli)
    assert (got.n_dropout, got.seed) == (4, 5)
    assert trainer_common.resumed_args(mod.TRAINER, argparse.Namespace(n_dropout=6), cli).n_dropout == 6


class _Stub:
    def __init__(self, tag):
        self.tag, self.seed = tag, None

    def parameters(self):
        return []

    def state_dict(self):
        return {"tag": self.tag}

    def seed_draws(self, seed):
        self.seed = seed


def test_checkpoint_keys_and_the_uncertain_model_on_resume(monkeypatch):
    import source_uncertain_trainer as mod
    import trainer_common
    calls = []

    def factory(**kw):
        calls.append(kw)
        return _Stub("model")
    monkeypatch.setattr(mod, "get_full_uncertain_model", factory)
    monkeypatch.setattr(mod, "get_optimizer", lambda *a, **k: _Stub("optimizer"))
    args = _args(["--input_ch", "6", "--n_dropout", "3", "--seed", "11"])
    modules, optimizers = mod.TRAINER.build(args)  # (trainer_common builds a resumed run through the same function)
    assert list(modules) + list(optimizers) == ["state_dict", "optimizer"]
    assert calls[0]["n_dropout"] == 3 and calls[0]["is_data_parallel"] is False and calls[0]["input_ch"] == 6
    assert modules["state_dict"].seed == 11
    dic = trainer_common.checkpoint_dict(args, 2, modules, optimizers)
    assert set(dic) == {"epoch", "args", "state_dict", "optimizer"} and dic["state_dict"] == {"tag": "model"}


# ------------------------------------------------------------------------------------------------ the model
def test_state_dict_keys_and_shapes_are_the_reference_models(fx, monkeypatch):
    monkeypatch.setenv("MCDSEG_PRETRAINED", "0")
    from models.model_util import get_full_uncertain_model
    model = get_full_uncertain_model("drn_d_22", "50", 5, 3, criterion=None, is_data_parallel=False, n_dropout=3)
    want = json.loads(str(fx["keys"]))
    assert [[k, list(v.shape)] for k, v in model.state_dict().items()] == want
    assert {k for k, _ in want if not k.startswith("base.")} == {"seg.weight", "seg.bias", "up.weight", "up_std.weight"}
    assert model.n_dropout_exp == 3 and model.uncertain_weight == 0.1 and model.dropout.p == 0.2
    assert all(p.requires_grad for p in (model.up.weight, model.up_std.weight))
    wrapped = get_full_uncertain_model("drn_d_22", "50", 5, 3, criterion=None, n_dropout=3)
    assert all(k.startswith("module.") for k in wrapped.state_dict())
    with pytest.raises(NotImplementedError):
        get_full_uncertain_model("psp", "50", 5, 3, criterion=None)
    from models.dilated_fcn import UncertainDRNSeg
    with pytest.raises(NotImplementedError):
        UncertainDRNSeg("drn_d_22", 5, pretrained=False, use_torch_up=True)


def test_draws_honour_an_eval_mode_dropout(monkeypatch):
    monkeypatch.setenv("MCDSEG_PRETRAINED", "0")
    from models.dilated_fcn import UncertainDRNSeg
    from models.model_util import fix_dropout_when_training
    model = UncertainDRNSeg("drn_d_22", 5, pretrained=False, n_dropout_exp=4).train()
    model.seed_draws(3)
    keep, r, scale = model.draw(2, 5, torch.device("cpu"))
    assert keep.dtype == torch.uint8 and tuple(keep.shape) == (4, 2, 5) and scale == pytest.approx(1.25)
    assert np.array_equal(r.numpy(), np.random.RandomState(3).random_sample(4).astype(np.float32))
    fix_dropout_when_training(model)
    keep, r, scale = model.draw(2, 5, torch.device("cpu"))
    assert int(keep.min()) == 1 and scale == 1.0


def test_jet_is_matplotlibs():
    import source_uncertain_tester as tester
    a = np.linspace(-2.0, 5.0, 256).reshape(16, 16)
    got = tester.jet_u8(a)
    assert got.shape == (16, 16, 3) and got.dtype == np.uint8
    assert tuple(got[0, 0]) == (0, 0, 128) and tuple(got[-1, -1]) == (128, 0, 0)  # jet's ends: dark blue, dark red
    assert tuple(tester.jet_u8(np.ones((2, 2)))[0, 0]) == (0, 0, 128)
    mid = got[8, 0].astype(int)  # ~0.5: green dominates
    assert mid[1] == 255 and abs(int(mid[0]) - int(mid[2])) < 40
