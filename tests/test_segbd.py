"""CPU: the segmentation + boundary ("segbd") multitask variant -- exports, the torch statement of ``loss.bce2d`` /
``get_boundary_loss`` against what the REAL reference returned (tests/golden/segbd_small.npz, made by make_segbd_golden.py),
state-dict layouts, the factory's errors, the two command lines' flags and the solver's step order.  No kernel is launched here."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_EXPORTS = ("mcdseg_label_boundary", "mcdseg_boundary_head_fwd", "mcdseg_boundary_head_bwd", "mcdseg_bce2d_workspace_bytes",
               "mcdseg_bce2d", "mcdseg_bce2d_bwd", "mcdseg_boundary_head_bce_fwd", "mcdseg_boundary_head_bce_bwd")


@pytest.fixture(autouse=True)
def _no_pretrained(monkeypatch):
    monkeypatch.setenv("MCDSEG_PRETRAINED", "0")


def test_new_exports_are_in_the_header_and_the_library():
    import mcdseg
    from mcdseg import _lib
    mcdseg.build()
    header = open(os.path.join(ROOT, "include", "mcdseg.h")).read()
    L = mcdseg.lib()
    for name in NEW_EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(L, name), name
    # every entry cites the reference lines it replaces
    block = header[header.index("Boundary branch of the segmentation + boundary"):header.index("int mcdseg_label_boundary")]
    for cite in ("models/dilated_fcn.py:770-774", ":1118-1128", "loss.py:131-138", ":743-787"):
        assert cite in block, cite
    assert L.mcdseg_bce2d_workspace_bytes(0) == 0
    assert L.mcdseg_bce2d_workspace_bytes(1) == 24 and L.mcdseg_bce2d_workspace_bytes(16 * 480 * 640) == 1200 * 24
    # argument checks happen before any launch
    assert L.mcdseg_boundary_head_fwd(None, None, None, None, 1, 8, 8, None) != 0
    assert b"boundary_head_fwd" in L.mcdseg_last_error()


def test_ops_refuse_cpu_tensors_and_other_dtypes():
    from mcdseg import ops
    z = torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 2, 2), torch.zeros(1, 1, 1, 1)
    lab = torch.zeros(1, 8, 8, dtype=torch.int64)
    for call in (lambda: ops.label_boundary(lab), lambda: ops.boundary_head(*z), lambda: ops.boundary_head_bce(*z, lab),
                 lambda: ops.bce2d(torch.zeros(1, 1, 8, 8), torch.zeros(1, 8, 8))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="target"):
        ops.bce2d(torch.zeros(4), torch.zeros(4, requires_grad=True))


def test_loss_bce2d_cpu_path_agrees_with_the_reference(golden):
    import loss
    fx = golden.npz("segbd_small.npz")
    p, soft = torch.from_numpy(fx["p"]), torch.from_numpy(fx["soft"])
    hard = torch.from_numpy(fx["get_boundary"])  # [N,H,W] against the [N,1,H,W] input: the shape difference old torch took
    for tag, dt, tol in (("f64", torch.float64, 1e-14), ("f32", torch.float32, 4e-7)):
        for name, t in (("bce2d_hard", hard), ("bce2d_soft", soft)):
            got = float(loss.bce2d(p.to(dt), t.to(dt)))
            want = float(fx["%s/%s" % (tag, name)])
            assert abs(got - want) <= tol * abs(want), (tag, name, got, want)
    # uint8 targets (what ops.label_boundary writes) take the same expression on the CPU
    assert float(loss.bce2d(p.double(), hard)) == float(loss.bce2d(p.double(), hard.double()))
    # gradient flows to the input only; a target that asks for one is refused as in the reference
    x = p.double().requires_grad_()
    loss.bce2d(x, hard).backward()
    assert x.grad is not None and bool(torch.isfinite(x.grad).all())
    with pytest.raises(AssertionError):
        loss.bce2d(p, soft.clone().requires_grad_())


def test_get_boundary_loss_cpu_path_agrees_with_the_reference(golden):
    from models.dilated_fcn import _get_boundary, get_boundary_loss
    fx = golden.npz("segbd_small.npz")
    lab_a, lab_b = torch.from_numpy(fx["lab_a"]), torch.from_numpy(fx["lab_b"])
    p, soft = torch.from_numpy(fx["p"]), torch.from_numpy(fx["soft"])
    assert np.array_equal(_get_boundary(lab_a).numpy().astype(np.uint8), fx["get_boundary"])
    assert np.array_equal(_get_boundary(lab_a.to(torch.uint8)).numpy().astype(np.uint8), fx["get_boundary"])
    for tag, dt, tol in (("f64", torch.float64, 1e-14), ("f32", torch.float32, 4e-7)):
        cases = (("boundary_loss_semseg", get_boundary_loss(lab_b, lab_a)),
                 ("boundary_loss_boundary", get_boundary_loss(pred=p.to(dt), gt=lab_a, pred_type="boundary")),
                 ("boundary_loss_gt_boundary", get_boundary_loss(pred=lab_b, gt=soft.to(dt), gt_type="boundary")))
        for name, got in cases:
            want = float(fx["%s/%s" % (tag, name)])
            assert abs(float(got) - want) <= max(tol, 4e-7 if "semseg" in name or "gt_" in name else 0) * abs(want), (tag, name, float(got), want)
    with pytest.raises(AssertionError):
        get_boundary_loss(lab_b, lab_a, pred_type="depth")


def test_state_dict_layouts_are_the_reference_s(golden):
    from loss import CrossEntropyLoss2d, Diff2d
    from models.model_util import get_segbd_multitask_models
    keys = golden.json("segbd_keys.json")
    enc, dec = get_segbd_multitask_models("drn_d_22", 6, 5)  # (input_ch is ignored: the encoder is RGB)
    assert [[k, list(v.shape)] for k, v in enc.state_dict().items()] == keys["encoder_drn_d_22"]
    assert [[k, list(v.shape)] for k, v in dec.state_dict().items()] == keys["decoder"]
    assert enc.main_layer0[0].in_channels == 3
    _, dec = get_segbd_multitask_models("drn_d_22", 3, 5, add_pred_seg_boundary_loss=True)
    assert [[k, list(v.shape)] for k, v in dec.state_dict().items()] == keys["decoder_pred_seg_boundary"]
    assert [n for n, _ in enc.named_children()] == ["main_layer%d" % k for k in range(9)]
    # with its criteria the decoder also carries the class weights, as the multitask decoder does
    _, dec = get_segbd_multitask_models("drn_d_22", 3, 5, CrossEntropyLoss2d(torch.ones(5)), Diff2d())
    assert "semseg_criterion.nll_loss.weight" in dec.state_dict()
    std = dec.get_task_weights()
    assert len(std) == 2 and abs(float(std[1].reshape(-1)[0]) - float(np.e)) < 1e-6  # sqrt(exp(2 * 1)): the boundary task's


def test_factory_errors():
    from models.dilated_fcn import MCDSegBDMultiTaskDecoder
    from models.model_util import get_segbd_multitask_models
    with pytest.raises(NotImplementedError, match="Only FCN"):
        get_segbd_multitask_models("fcn", 3, 5)
    with pytest.raises(NotImplementedError):
        get_segbd_multitask_models("drn_d_22", 3, 5, is_src_only=True)
    with pytest.raises(NotImplementedError, match="semseg_shortcut"):
        get_segbd_multitask_models("drn_d_22", 3, 5, semseg_shortcut=True)
    with pytest.raises(NotImplementedError, match="use_seg2bd_conv"):
        MCDSegBDMultiTaskDecoder(5, 3, use_seg2bd_conv=True)
    dec = MCDSegBDMultiTaskDecoder(5, 3, depth_shortcut=True)  # accepted and ignored, as in the reference
    assert dec.depth_shortcut and not hasattr(dec, "s_pred_seg_boundary")
    with pytest.raises(AssertionError):
        dec.get_psuedo_boundary_loss({})


def test_encoder_refuses_compact_storage(monkeypatch):
    from mcdseg import ops
    from models.dilated_fcn import MultiTaskEncoderReturningMultipleFeaturemaps
    enc = MultiTaskEncoderReturningMultipleFeaturemaps("drn_d_22", pretrained=False)
    monkeypatch.setattr(ops, "ACT_STORAGE", "compact")
    with pytest.raises(NotImplementedError, match="MCDSEG_ACT_STORAGE=compact"):
        enc(torch.zeros(1, 3, 16, 16))


def test_parsers_accept_the_reference_flags():
    import adapt_segbd_multitask_trainer as trainer
    a = trainer.get_parser().parse_args(["suncg", "nyu"])
    assert (a.depth_shortcut, a.semseg_shortcut, a.add_pred_seg_boundary_loss, a.use_seg2bd_conv) == (False,) * 4
    assert (a.boundary_loss_converging_epoch, a.scale_bd_loss, a.input_ch) == (5, 1, 3)
    a = trainer.get_parser().parse_args(["suncg", "nyu", "--add_pred_seg_boundary_loss", "--boundary_loss_converging_epoch", "0",
                                         "--scale_bd_loss", "3", "--depth_shortcut", "--opt", "adam", "--net", "drn_d_22"])
    assert a.add_pred_seg_boundary_loss and a.depth_shortcut and (a.boundary_loss_converging_epoch, a.scale_bd_loss, a.opt) == (0, 3, "adam")
    import adapt_segbd_multitask_tester as tester
    import argmyparse
    t = argmyparse.get_da_mcd_testing_parser().parse_args(["nyu", "x/pth/MCD-normal-drn_d_22-1.pth.tar", "--saves_prob"])
    assert t.saves_prob and callable(tester.main)


class _Log(list):
    pass


def _stub_solver(log, num_k=2, **kw):
    from solvers.solver import SegBDMultiTaskMCDSolver

    class Enc(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(1))

        def forward(self, x):
            log.append(("enc", tuple(x.shape), torch.is_grad_enabled()))
            return {"h8": x.mean() * self.w}

    class Dec(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.v = torch.nn.Parameter(torch.ones(1))

        def get_loss(self, f, gt, separately_returning=False):
            log.append(("get_loss",))
            return f["h8"] * self.v, f["h8"] * self.v * 2

        def get_psuedo_boundary_loss(self, f, separately_returning=False):
            log.append(("psuedo", f["h8"].requires_grad))
            return torch.tensor(5.0)

        def get_cls_descrepancy(self, f):
            log.append(("disc",))
            return f["h8"] * self.v * 3

    class Opt:
        def __init__(self, name):
            self.name = name

        def zero_grad(self):
            log.append((self.name, "zero"))

        def step(self):
            log.append((self.name, "step"))

    return SegBDMultiTaskMCDSolver(Enc(), Dec(), Opt("oe"), Opt("od"), num_k=num_k, **kw)


def test_solver_step_order_on_stub_modules():
    log = _Log()
    solver = _stub_solver(log, num_k=2, num_multiply_d_loss=4, add_pred_seg_boundary_loss=True, boundary_loss_converging_epoch=5,
                          scale_bd_loss=3)
    src, tgt, gt = torch.ones(2, 4, 8, 8), torch.full((2, 4, 8, 8), 2.0), torch.zeros(2, 8, 8, dtype=torch.int64)
    c, d, parts = solver.step(src, gt, tgt, epoch=5)  # epoch 5 is not yet past the converging epoch
    names = [e[:2] if e[0] in ("oe", "od") else e[:1] for e in log]
    A = [("oe", "zero"), ("od", "zero"), ("enc",), ("enc",), ("get_loss",), ("oe", "step"), ("od", "step")]
    B = [("oe", "zero"), ("od", "zero"), ("enc",), ("get_loss",), ("enc",), ("disc",), ("od", "step")]
    C = [("oe", "zero"), ("enc",), ("disc",), ("oe", "step")] * 2
    assert names == A + B + C, names
    # only the RGB channels reach the encoder; tapes exist where the encoder's gradient is used: step A's source pass and step C
    encs = [e for e in log if e[0] == "enc"]
    assert all(e[1] == (2, 3, 8, 8) for e in encs)
    assert [e[2] for e in encs] == [True, False, False, False, True, True]
    assert float(c) == 3.0 and parts[2] == 0 and float(parts[0]) == 1.0 and float(parts[1]) == 2.0
    assert float(d) == 2.0 * 3 * 4 / 2  # the last inner loss (mean 2, head factor 3, num_multiply_d_loss 4) over num_k
    # past the converging epoch the (gradient-free) pseudo-boundary loss joins step A, scaled
    del log[:]
    c, d, parts = solver.step(src, gt, tgt, epoch=6)
    assert [e for e in log if e[0] == "psuedo"] == [("psuedo", False)] and log.index(("psuedo", False)) < log.index(("oe", "step"))
    assert float(c) == 3.0 + 15.0 and float(parts[2]) == 15.0
    # ... and only when the flag is set
    del log[:]
    solver = _stub_solver(log, num_k=1)
    solver.step(src, gt, tgt, epoch=50)
    assert not [e for e in log if e[0] == "psuedo"]
