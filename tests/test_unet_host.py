"""CPU: the U-Net generator and classifiers (``--net unet``) -- the state-dict layout of ``models.unet`` against the REAL reference's
(tests/golden/unet_keys.json, made by make_unet_golden.py), the factory and what it still refuses, the refusals of the modules and of
the ops, the fixture's own shape, and the export and the argument refusals of the kernels of csrc/unet.hip.  No kernel is launched here."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import unet_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("mcdseg_maxpool2_fwd", "mcdseg_maxpool2_bwd", "mcdseg_relu_fwd", "mcdseg_relu_bwd", "mcdseg_deconv2x2_fwd",
               "mcdseg_deconv2x2_bwd_data", "mcdseg_deconv2x2_bwd_weight_workspace_bytes", "mcdseg_deconv2x2_bwd_weight")


@pytest.fixture(autouse=True)
def _no_pretrained(monkeypatch):
    monkeypatch.setenv("MCDSEG_PRETRAINED", "0")


# ------------------------------------------------------------------------------------------------ modules and factory
@pytest.mark.parametrize("feature_scale", [4, 8])
def test_state_dicts_are_the_references(feature_scale):
    from models.unet import UNetBase, UNetClassifier
    keys = R.load_keys()
    g = UNetBase(feature_scale=feature_scale, input_ch=6)
    f = UNetClassifier(feature_scale=feature_scale, n_classes=5)
    assert R.keys_shapes(g) == keys["base/%d" % feature_scale]
    assert R.keys_shapes(f) == keys["classifier/%d" % feature_scale]
    sd = g.state_dict()
    assert "conv1.conv1.0.weight" in sd and "conv1.conv1.1.running_mean" in sd and "center.conv2.1.num_batches_tracked" in sd
    c = 1024 // feature_scale
    assert tuple(f.state_dict()["up_concat4.up.weight"].shape) == (c, c // 2, 2, 2)  # torch's [Cin, Cout, 2, 2], no repack
    if feature_scale == 4:  # the sizes the issue quotes: 1.2 M + 0.76 M parameters
        assert sum(p.numel() for p in g.parameters()) == 1181184 and sum(p.numel() for p in f.parameters()) == 762405


def test_constructor_arguments_and_default_initialisation():
    from models import drn
    from models.unet import UNetBase, UNetClassifier, UNetConv, UNetUp
    g = UNetBase()
    assert (g.feature_scale, g.is_deconv, g.input_ch, g.is_batchnorm) == (4, True, 3, True)
    f = UNetClassifier()
    assert (f.feature_scale, f.is_deconv) == (4, True) and f.final.out_channels == 21
    assert isinstance(g.conv1, UNetConv) and isinstance(f.up_concat1, UNetUp) and isinstance(g.maxpool1, torch.nn.MaxPool2d)
    assert isinstance(g.conv1.conv1[0], drn.Conv2d) and isinstance(g.conv1.conv1[1], drn.BatchNorm2d)
    assert isinstance(f.up_concat1.up, torch.nn.ConvTranspose2d) and len(f.up_concat1.conv.conv1) == 2
    # torch's defaults: BatchNorm at (1, 0), a convolution bias within 1 / sqrt(fan_in)
    bn = g.center.conv2[1]
    assert torch.equal(bn.weight.detach(), torch.ones(256)) and not bn.bias.detach().any()
    conv = g.conv2.conv1[0]
    assert float(conv.bias.detach().abs().max()) <= 1.0 / (16 * 9) ** 0.5 and float(conv.weight.detach().abs().max()) <= 1.0 / (16 * 9) ** 0.5


def test_factory_builds_the_classes():
    from models.model_util import get_models
    from models.unet import UNetBase, UNetClassifier
    g, f1, f2 = get_models("unet", 6, 7)
    assert type(g) is UNetBase and type(f1) is UNetClassifier and type(f2) is UNetClassifier and f1 is not f2
    assert g.input_ch == 6 and g.conv1.conv1[0].in_channels == 6 and g.feature_scale == 4
    assert f1.final.out_channels == 7 and f2.final.out_channels == 7
    g, f1, f2 = get_models("unet", 6, 7, is_data_parallel=True)
    assert type(g).__name__ == "DataParallel" and type(g.module) is UNetBase and type(f2.module) is UNetClassifier


def test_what_the_factories_still_refuse():
    from models.model_util import get_full_model, get_models
    with pytest.raises(NotImplementedError, match="MCD"):
        get_models("unet", 6, 7, method="MFNet-AddFusion")
    with pytest.raises(NotImplementedError, match="are supported"):
        get_full_model("unet", "50", 7, 6)
    for net in ("segnet", "fcnvgg", "fusenet", "fcn", "psp"):
        with pytest.raises(NotImplementedError, match="are supported"):
            get_models(net, 6, 7)
    from models.model_util import get_dann_models
    with pytest.raises(NotImplementedError):
        get_dann_models("unet", 6, 7, (64, 64))


def test_solver_takes_the_literal_schedule():
    from solvers import solver
    assert "UNetBase" not in solver._REPEATABLE_GENERATORS
    d = solver._detached({"a": torch.zeros(2, requires_grad=True) * 2})
    assert isinstance(d, dict) and not d["a"].requires_grad


def test_module_refusals(monkeypatch):
    from mcdseg import ops
    from models.unet import UNetBase, UNetClassifier, UNetUp
    for bad in (lambda: UNetBase(is_deconv=False), lambda: UNetClassifier(is_deconv=False), lambda: UNetUp(32, 16, False)):
        with pytest.raises(NotImplementedError, match="is_deconv=False"):
            bad()
    g, f = UNetBase(input_ch=6), UNetClassifier(n_classes=5)
    for shape in ((1, 6, 40, 64), (1, 6, 64, 24), (1, 6, 17, 16)):
        with pytest.raises(ValueError, match="multiples of 16"):
            g(torch.zeros(shape))
    with pytest.raises(ValueError, match="multiples of 16"):
        f({"conv1": torch.zeros(1, 16, 24, 32)})
    monkeypatch.setattr(ops, "ACT_STORAGE", "compact")
    with pytest.raises(NotImplementedError, match="MCDSEG_ACT_STORAGE=compact"):
        g(torch.zeros(1, 6, 32, 32))
    with pytest.raises(NotImplementedError, match="MCDSEG_ACT_STORAGE=compact"):
        f({"conv1": torch.zeros(1, 16, 32, 32)})


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    from mcdseg import ops
    for fn in (ops.max_pool2, ops.relu):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(torch.zeros(1, 8, 4, 4))
        with pytest.raises(ValueError, match="NCHW"):
            fn(torch.zeros(8, 4, 4))
    with pytest.raises(ValueError, match="even H and W"):  # ahead of everything else: nothing (a bound's measurement included) is launched
        ops.max_pool2(torch.zeros(1, 8, 3, 4))
    w, b = torch.zeros(8, 4, 2, 2), torch.zeros(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.up_join(torch.zeros(1, 4, 8, 8), torch.zeros(1, 8, 4, 4), w, b)
    with pytest.raises(ValueError, match="twice the size"):
        ops.up_join(torch.zeros(1, 4, 8, 10), torch.zeros(1, 8, 4, 4), w, b)
    with pytest.raises(ValueError, match=r"\[Cin, Cout, 2, 2\]"):
        ops.up_join(torch.zeros(1, 4, 8, 8), torch.zeros(1, 6, 4, 4), w, b)
    assert ops.fused_unet() is True


def test_fused_unet_switch_is_read_per_call(monkeypatch):
    from mcdseg import ops
    monkeypatch.setenv("MCDSEG_FUSED_UNET", "0")
    assert ops.fused_unet() is False
    monkeypatch.setenv("MCDSEG_FUSED_UNET", "1")
    assert ops.fused_unet() is True


# ------------------------------------------------------------------------------------------------ the fixture
def test_fixture_holds_what_the_gpu_test_reads():
    fx, units = R.load_golden()
    spec = json.loads(str(fx["spec"]))
    assert {k: spec[k] for k in ("n", "input_ch", "h", "w", "n_class", "feature_scale")} == dict(n=2, input_ch=6, h=32, w=48, n_class=5,
                                                                                               feature_scale=8)
    x, labels = R.inputs(spec)  # nothing of the inputs is stored: the draw must be the one the fixture was made from
    assert abs(float(x.double().sum()) - float(fx["x_sum"])) <= 1e-6 * x.numel() and int(labels.sum()) == int(fx["labels_sum"])
    names = [k[4:] for k in fx.files if k.startswith("f64/")]
    assert sorted(names) == sorted(units)
    for k in ("feat/center", "feat/conv1", "feat/conv2", "feat/conv3", "feat/conv4", "o1", "o2", "loss/ce", "loss/diff", "grad_ce/x",
              "grad_diff/x", "state/conv1.conv1.1.running_mean", "grad_ce/f1.up_concat4.up.weight", "grad_diff/g.center.conv2.0.weight"):
        assert k in names, k
    assert fx["f64/o1"].shape == (2, 5, 32, 48) and fx["f64/feat/center"].shape == (2, 128, 2, 3)
    assert fx["f64/grad_ce/f1.up_concat4.up.weight"].shape == (2048,)  # 128 x 64 x 2 x 2 at every 16th flat index
    assert len(R.stored_index(128 * 64 * 4)) == 2048 and R.stored_index(2048) is None and len(R.stored_index(2304)) == 1152
    # the draw was chosen so that the fp32 reference takes no other side of a ReLU or a maximum than fp64 does
    assert max(units.values()) < 1e-3
    # the bias of a convolution in front of a train-mode BatchNorm: zero in exact arithmetic, held relative to its terms
    scales = [k for k in fx.files if k.startswith("scale/")]
    assert len(scales) == 20 and all(float(np.abs(fx["f64/" + k[6:]]).max()) < 1e-12 * float(fx[k]) for k in scales)
    assert os.path.getsize(R.GOLDEN) < 1500000


# ------------------------------------------------------------------------------------------------ the C ABI
def test_exports_and_argument_refusals():
    import mcdseg
    from mcdseg import _lib
    mcdseg.build()
    header = open(os.path.join(ROOT, "include", "mcdseg.h")).read()
    L = mcdseg.lib()
    for name in NEW_EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.EXPORTS and hasattr(L, name), name
    block = header[header.index("The operators of the U-Net"):header.index("int mcdseg_maxpool2_fwd")]
    for cite in ("models/unet.py", ":122-171", ":29-43", ":174-199"):
        assert cite in block, cite
    assert "unet.hip" in _lib.NO_PACKED_F32 and os.path.exists(os.path.join(_lib.CSRC, "unet.hip"))
    p = ctypes.c_void_p(4096)  # never read: every refusal is answered before anything is launched
    F16X3, BF16X6 = 3, 6

    def refused(fn, who, *args):
        assert fn(*args) == -22, (who, args)
        msg = L.mcdseg_last_error().decode()
        assert msg.startswith(who), (who, msg)
        return msg

    pool, relu = L.mcdseg_maxpool2_fwd, L.mcdseg_relu_fwd
    refused(pool, "maxpool2_fwd", None, p, p, p, p, F16X3, 2, 16, 8, 8, None)
    refused(pool, "maxpool2_fwd", p, p, None, p, p, F16X3, 2, 16, 8, 8, None)
    assert "even" in refused(pool, "maxpool2_fwd", p, p, p, p, p, F16X3, 2, 16, 7, 8, None)
    assert "even" in refused(pool, "maxpool2_fwd", p, None, p, None, None, 0, 2, 16, 8, 6 + 1, None)
    assert "multiple of 8" in refused(pool, "maxpool2_fwd", p, p, p, p, p, F16X3, 2, 12, 8, 8, None)
    assert "grid limit" in refused(pool, "maxpool2_fwd", p, p, p, p, p, F16X3, 8192, 64, 4, 4, None)
    assert "bound" in refused(pool, "maxpool2_fwd", p, None, p, p, None, F16X3, 2, 16, 8, 8, None)
    assert "bound" in refused(pool, "maxpool2_fwd", p, None, p, p, None, 1, 2, 16, 8, 8, None)
    assert "bound" in refused(pool, "maxpool2_fwd", p, p, p, p, None, BF16X6, 2, 16, 8, 8, None)
    assert "math" in refused(pool, "maxpool2_fwd", p, None, p, p, None, 4, 2, 16, 8, 8, None)
    refused(L.mcdseg_maxpool2_bwd, "maxpool2_bwd", p, None, p, 2, 16, 8, 8, None)
    assert "even" in refused(L.mcdseg_maxpool2_bwd, "maxpool2_bwd", p, p, p, 2, 16, 8, 9, None)

    refused(relu, "relu_fwd", None, p, p, p, p, F16X3, 2, 16, 64, None)
    assert "multiple of 8" in refused(relu, "relu_fwd", p, p, p, p, p, F16X3, 2, 12, 64, None)
    assert "grid limit" in refused(relu, "relu_fwd", p, p, p, p, p, F16X3, 8192, 64, 4, None)
    assert "bound" in refused(relu, "relu_fwd", p, None, p, p, None, F16X3, 2, 16, 64, None)
    assert "math" in refused(relu, "relu_fwd", p, None, p, p, None, 5, 2, 16, 64, None)
    refused(relu, "relu_fwd", p, None, p, None, None, 0, 2, 16, 0, None)
    refused(L.mcdseg_relu_bwd, "relu_bwd", p, p, None, 64, None)
    refused(L.mcdseg_relu_bwd, "relu_bwd", p, p, p, 0, None)

    fwd, bwd_d, bwd_w = L.mcdseg_deconv2x2_fwd, L.mcdseg_deconv2x2_bwd_data, L.mcdseg_deconv2x2_bwd_weight
    n, cin, cout, h, w = 2, 8, 4, 3, 5
    plane = 4 * h * w
    refused(fwd, "deconv2x2_fwd", None, p, p, p, 8 * plane, 8, 4, n, cin, cout, h, w, None)
    refused(fwd, "deconv2x2_fwd", p, p, p, None, 8 * plane, 8, 4, n, cin, cout, h, w, None)
    assert "slice" in refused(fwd, "deconv2x2_fwd", p, p, p, p, 8 * plane, 8, 5, n, cin, cout, h, w, None)   # [5, 9) of 8 channels
    assert "slice" in refused(fwd, "deconv2x2_fwd", p, p, p, p, 8 * plane, 8, -1, n, cin, cout, h, w, None)
    assert "slice" in refused(fwd, "deconv2x2_fwd", p, p, p, p, 8 * plane - 1, 8, 4, n, cin, cout, h, w, None)  # images overlap
    refused(fwd, "deconv2x2_fwd", p, p, p, p, 8 * plane, 8, 4, n, 0, cout, h, w, None)
    assert L.mcdseg_deconv2x2_fwd.argtypes[2] is ctypes.c_void_p  # (a NULL bias is allowed: no refusal to test)
    refused(bwd_d, "deconv2x2_bwd_data", None, 8 * plane, 8, 4, p, p, n, cin, cout, h, w, None)
    assert "slice" in refused(bwd_d, "deconv2x2_bwd_data", p, 8 * plane, 8, 6, p, p, n, cin, cout, h, w, None)
    ws = L.mcdseg_deconv2x2_bwd_weight_workspace_bytes(n, cin, cout, h, w)
    assert ws > 0 and ws % 8 == 0 and L.mcdseg_deconv2x2_bwd_weight_workspace_bytes(n, 0, cout, h, w) == 0
    # at the trainer's sizes the partials stay small: the largest layer (256 -> 128 at 30 x 40) and the full-resolution one (32 -> 16)
    assert L.mcdseg_deconv2x2_bwd_weight_workspace_bytes(16, 256, 128, 30, 40) <= 4 << 20
    assert L.mcdseg_deconv2x2_bwd_weight_workspace_bytes(16, 32, 16, 240, 320) <= 4 << 20
    refused(bwd_w, "deconv2x2_bwd_weight", p, p, 8 * plane, 8, 4, None, p, n, cin, cout, h, w, p, ws, None)
    refused(bwd_w, "deconv2x2_bwd_weight", p, p, 8 * plane, 8, 4, p, p, n, cin, cout, h, w, None, ws, None)
    assert "slice" in refused(bwd_w, "deconv2x2_bwd_weight", p, p, 8 * plane, 8, 5, p, p, n, cin, cout, h, w, p, ws, None)
    assert "workspace" in refused(bwd_w, "deconv2x2_bwd_weight", p, p, 8 * plane, 8, 4, p, p, n, cin, cout, h, w, p, ws - 1, None)


def test_a_producer_asks_its_reader_before_it_writes_a_companion(monkeypatch):
    """``ops.conv_reads_companion``: no for a biased thin 3x3 convolution (the library would route it to the window kernel, which takes no
    bias), for a channel count off the layout, and under the f32 arithmetic; yes for the wider biased layers and for an unbiased thin one"""
    import mcdseg
    from mcdseg import ops
    from models import drn
    mcdseg.build()
    monkeypatch.setattr(ops, "CONV_MATH", "f16x3")
    biased16, plain16 = drn.Conv2d(16, 16, 3, 1, 1), drn.Conv2d(16, 16, 3, 1, 1, bias=False)
    assert ops.lib().mcdseg_conv_split_window_ok(ops.ctypes.byref(ops.conv_desc((2, 16, 32, 48), biased16.weight.shape, 1, 1, 1)), 3, 1, 0) == 1
    assert not ops.conv_reads_companion(biased16, (2, 16, 32, 48)) and ops.conv_reads_companion(plain16, (2, 16, 32, 48))
    assert ops.conv_reads_companion(drn.Conv2d(128, 64, 3, 1, 1), (2, 128, 8, 12))
    assert ops.conv_reads_companion(drn.Conv2d(16, 5, 1), (2, 16, 32, 48))          # the 1x1 head: not a window geometry
    assert not ops.conv_reads_companion(drn.Conv2d(12, 16, 3, 1, 1), (2, 12, 8, 12))  # C % 8
    assert not ops.conv_reads_companion(drn.Conv2d(8, 16, 3, 1, 1), (2, 8, 8, 12))    # below the split path's 16 channels
    monkeypatch.setattr(ops, "CONV_MATH", "f32")
    assert not ops.conv_reads_companion(plain16, (2, 16, 32, 48))
