"""CPU: the FuseNet-style generator (``--net drn_d_XX_fusenet``, middle fusion) -- tests/fusenet_ref against the golden the REAL
reference's ``FuseDRNSegBase`` produced (tests/golden/fusenet_small.npz, made by make_fusenet_golden.py), the state-dict layout of
``models.dilated_fcn.FuseDRNSegBase`` against the reference's, the dead ``sub_layer*`` parameters and the optimizer, the factory and
its refusals, and the export and the argument refusals of ``mcdseg_stage_join``.  No kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import fusenet_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _no_pretrained(monkeypatch):
    monkeypatch.setenv("MCDSEG_PRETRAINED", "0")


@pytest.mark.parametrize("case", R.CASES)
def test_fusenet_ref_equals_the_golden(case):
    fx, _ = R.load_golden()
    got = R.run_case(R.tiny_model(torch.float64), case, fx["x"], fx["dy"])
    names = [k[len(case) + 5:] for k in fx.files if k.startswith(case + "/f64/")]
    assert sorted(names) == sorted(got) and len(names) == (49 if case == "eval" else 99)
    for k in names:
        truth = fx["%s/f64/%s" % (case, k)]
        # (the other machine's fp64 sums run in another order; convolution-weight gradients are stored rounded to fp32)
        tol = 1e-7 if truth.dtype == np.float32 else 1e-9
        assert R.rel_to_max(got[k], truth) <= tol, (case, k, R.rel_to_max(got[k], truth))
        assert float(fx["%s/unit/%s" % (case, k)]) < 1e-4, (case, k)
    nbt = [int(got[k]) for k in names if k.endswith("num_batches_tracked")]
    assert len(nbt) == 16 and set(nbt) == {2 if case == "train" else 0}
    assert float(fx["min_variance"]) > 1e-2


def test_state_dict_is_the_references():
    from models.dilated_fcn import FuseDRNSegBase
    _, keys = R.load_golden()
    m = FuseDRNSegBase(R.register_tiny(), R.TINY["n_class"], pretrained=False, input_ch=6)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == keys
    assert sum(k.startswith("sub_layer") for k, _ in keys) == sum(k.startswith("main_layer") for k, _ in keys) > 0
    assert not hasattr(m, "optim_parameters") and not hasattr(m, "base")


def test_sub_layers_are_dead_weight():
    from models.dilated_fcn import FuseDRNSegBase
    from models.model_util import get_optimizer
    m = FuseDRNSegBase(R.register_tiny(), R.TINY["n_class"], pretrained=False, input_ch=6)
    sub = {id(p) for k, p in m.named_parameters() if k.startswith("sub_layer")}
    live = {id(p) for k, p in m.named_parameters() if not k.startswith("sub_layer")}
    assert sub and all(not p.requires_grad for p in m.parameters() if id(p) in sub)
    assert all(p.requires_grad for p in m.parameters() if id(p) in live)
    for opt in ("sgd", "adam"):
        o = get_optimizer(m.parameters(), opt, 1e-3, 0.9, 2e-5)
        held = {id(p) for g in o.param_groups for p in g["params"]}
        assert held == live, opt


def test_factory_builds_the_class():
    from models.dilated_fcn import DRNSegPixelClassifier, FuseDRNSegBase
    from models.model_util import get_models
    g, f1, f2 = get_models("drn_d_22_fusenet", 6, 7)
    assert type(g) is FuseDRNSegBase and type(f1) is DRNSegPixelClassifier and type(f2) is DRNSegPixelClassifier
    assert g.seg.out_channels == 7 and g.seg.in_channels == 512
    assert g.main_layer0[0].in_channels == 3 and g.sub_layer0[0].in_channels == 3


def test_solver_takes_the_literal_schedule():
    """one forward standing for two would update the running statistics HHA, HHA, RGB, RGB: the class is not on the solver's list"""
    from solvers import solver
    assert "FuseDRNSegBase" not in solver._REPEATABLE_GENERATORS


def test_refusals():
    from models.dilated_fcn import FuseDRNSegBase
    from models.model_util import get_models
    with pytest.raises(ValueError, match="input_ch == 6"):
        get_models("drn_d_22_fusenet", 4, 7)
    with pytest.raises(NotImplementedError, match="DRN-D"):
        get_models("drn_c_26_fusenet", 6, 7)
    with pytest.raises(NotImplementedError, match="ver2"):
        get_models("drn_d_22_ver2_fusenet", 6, 7)
    with pytest.raises(NotImplementedError, match="ver2"):
        FuseDRNSegBase("drn_d_22", 7, pretrained=False, input_ch=6, ver="ver2")
    with pytest.raises(NotImplementedError, match="MCD"):
        get_models("drn_d_22_fusenet", 6, 7, method="MFNet-AddFusion")


def test_forward_refuses_compact_storage(monkeypatch):
    from mcdseg import ops
    from models.dilated_fcn import FuseDRNSegBase
    m = FuseDRNSegBase(R.register_tiny(), R.TINY["n_class"], pretrained=False, input_ch=6)
    monkeypatch.setattr(ops, "ACT_STORAGE", "compact")
    with pytest.raises(NotImplementedError, match="MCDSEG_ACT_STORAGE=compact"):
        m(torch.zeros(1, 6, 16, 16))


def test_stage_join_export_and_refusals():
    import mcdseg
    from mcdseg import _lib
    mcdseg.build()
    header = open(os.path.join(ROOT, "include", "mcdseg.h")).read()
    assert re.search(r"\bmcdseg_stage_join\s*\(", header)
    assert "models/dilated_fcn.py:308-328" in header[header.index("The stage join"):header.index("int mcdseg_stage_join")]
    assert "mcdseg_stage_join" in _lib.EXPORTS and "join.hip" in _lib.NO_PACKED_F32
    L = mcdseg.lib()
    p = ctypes.c_void_p(4096)  # never read: every refusal is answered before anything is launched
    F16X3, BF16X6 = 3, 6

    def refused(why, *args):
        assert L.mcdseg_stage_join(*args, None) == -22, why
        msg = L.mcdseg_last_error().decode()
        assert msg.startswith("stage_join"), (why, msg)
        return msg

    refused("null a", None, p, p, p, p, p, p, F16X3, 2, 16, 64)
    refused("null y", p, p, p, p, None, p, p, F16X3, 2, 16, 64)
    assert "multiple of 8" in refused("C = 12 with a companion", p, p, p, p, p, p, p, F16X3, 2, 12, 64)
    assert "grid limit" in refused("N * C/8 = 65536", p, p, p, p, p, p, p, F16X3, 8192, 64, 4)
    assert "bound" in refused("f16x3 without bounds", p, None, p, None, p, p, None, F16X3, 2, 16, 64)
    assert "bound" in refused("f16x3 with one bound missing", p, p, p, None, p, p, p, F16X3, 2, 16, 64)
    assert "bound" in refused("f16x1 without bounds", p, None, p, None, p, p, None, 1, 2, 16, 64)
    assert "math" in refused("unknown math with a companion", p, None, p, None, p, p, None, 4, 2, 16, 64)
    refused("no pixels", p, None, p, None, p, None, None, BF16X6, 2, 16, 0)


def test_ops_stage_join_refuses_cpu_tensors():
    from mcdseg import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.stage_join(torch.zeros(1, 16, 4, 4), torch.zeros(1, 16, 4, 4))
    with pytest.raises(ValueError, match="one shape"):
        ops.stage_join(torch.zeros(1, 16, 4, 4), torch.zeros(1, 16, 4, 5))
