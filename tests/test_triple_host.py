"""CPU: the segmentation + depth + boundary ("triple") multitask variant -- exports and the seg2bd workspace bound, state-dict layouts
against the REAL reference's (tests/golden/triple_keys.json, made by make_triple_golden.py), the factory's errors, the command lines'
flags and back-fill, the output layout, the 7-channel synthetic source and the solver's step order.  No kernel is launched here."""
import argparse
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "multichannel-semseg-with-uda_amd")

NEW_EXPORTS = ("mcdseg_boundary_head_bce_target_fwd", "mcdseg_boundary_head_bce_target_bwd", "mcdseg_seg2bd_bce_workspace_bytes",
               "mcdseg_seg2bd_bce_fwd", "mcdseg_seg2bd_bce_bwd")


@pytest.fixture(autouse=True)
def _no_pretrained(monkeypatch):
    monkeypatch.setenv("MCDSEG_PRETRAINED", "0")


def test_new_exports_header_and_workspace_bound():
    import mcdseg
    from mcdseg import _lib
    mcdseg.build()
    header = open(os.path.join(ROOT, "include", "mcdseg.h")).read()
    L = mcdseg.lib()
    for name in NEW_EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(L, name), name
    block = header[header.index("Boundary losses of the triple multitask decoder"):header.index("int mcdseg_boundary_head_bce_target_fwd")]
    for cite in ("models/dilated_fcn.py:790-1024", ":1002-1004", ":960-981", ":863-864"):
        assert cite in block, cite
    assert "seg2bd.hip" in _lib.NO_PACKED_F32
    # the workspace holds one-channel full-resolution planes, 25 low-resolution planes per image and head, and partials: at the
    # trainer's size it stays below an eighth of ONE head's full-resolution logits, which the unfused path keeps twice per head
    ws = L.mcdseg_seg2bd_bce_workspace_bytes(16, 41, 60, 80)
    assert 0 < ws <= 16 * 41 * 480 * 640 * 4 // 8, ws
    assert ws >= 2 * 16 * 480 * 640 * 4  # (v of both heads is in there)
    assert L.mcdseg_seg2bd_bce_workspace_bytes(0, 41, 60, 80) == 0
    # argument checks happen before any launch
    assert L.mcdseg_seg2bd_bce_fwd(None, None, None, None, None, 0, 0, None, 1, 1, 1, 1, None, 0, None) != 0
    assert b"seg2bd_bce_fwd" in L.mcdseg_last_error()
    assert L.mcdseg_boundary_head_bce_target_fwd(None, None, None, None, 0, 0, None, 1, 8, 8, None, 0, None) != 0
    assert b"boundary_head_bce_target_fwd" in L.mcdseg_last_error()


def test_ops_refuse_cpu_tensors():
    from mcdseg import ops
    s = torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 2, 2), torch.zeros(1, 1, 1, 1)
    z, w, b = torch.zeros(1, 3, 1, 1), torch.zeros(1, 3, 5, 5), torch.zeros(1)
    for call in (lambda: ops.boundary_head_bce_target(*s, torch.zeros(1, 1, 8, 8)), lambda: ops.seg2bd_bce(z, z, w, b, torch.zeros(1, 1, 8, 8))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_target_planes_takes_a_channel_slice_in_place():
    from mcdseg.ops import _target_planes
    t = torch.empty_strided((3, 1, 8, 16), (7 * 128, 128, 16, 1), device="meta")

    class Cuda:  # a stand-in that answers is_cuda: the function only reads dtype, shape and strides before it decides
        def __init__(self, t):
            self.t = t
            self.is_cuda, self.dtype, self.shape = True, t.dtype, t.shape

        def stride(self):
            return self.t.stride()

        def contiguous(self):
            return Cuda(torch.empty(self.t.shape, device="meta"))

    got, stride = _target_planes(Cuda(t), 3, 8, 16, "target")
    assert got.t is t and stride == 7 * 128
    got, stride = _target_planes(Cuda(t[:, 0]), 3, 8, 16, "target")
    assert stride == 7 * 128
    got, stride = _target_planes(Cuda(torch.empty(3, 1, 8, 16, device="meta")), 3, 8, 16, "target")
    assert stride == 128
    tr = torch.empty(3, 1, 16, 8, device="meta").transpose(2, 3)  # another layout: copied
    got, stride = _target_planes(Cuda(tr), 3, 8, 16, "target")
    assert got.t is not tr and stride == 128
    with pytest.raises(ValueError, match="does not match"):
        _target_planes(Cuda(t), 3, 16, 16, "target")


def test_state_dict_layouts_are_the_reference_s(golden):
    from models.model_util import get_triple_multitask_models
    keys = golden.json("triple_keys.json")
    segbd = golden.json("segbd_keys.json")
    for pred in (False, True):
        for s2b in (False, True):
            enc, dec = get_triple_multitask_models("drn_d_22", 6, 5, add_pred_seg_boundary_loss=pred, use_seg2bd_conv=s2b)
            got = [[k, list(v.shape)] for k, v in dec.state_dict().items()]
            assert got == keys["pred%d_seg2bd%d" % (pred, s2b)], (pred, s2b)
            names = [k for k, _ in got]
            assert ("s_pred_seg_boundary" in names) == pred and ("seg2bd_conv.weight" in names) == s2b
    assert names[:4] == ["s_semsegcls", "s_deprgr", "s_boundary", "s_pred_seg_boundary"] and names[-2:] == ["seg2bd_conv.weight", "seg2bd_conv.bias"]
    assert any(k.startswith("nmlrgr_dec.") for k in names)
    assert list(dec.state_dict()["seg2bd_conv.weight"].shape) == [1, 5, 5, 5]
    assert [[k, list(v.shape)] for k, v in enc.state_dict().items()] == segbd["encoder_drn_d_22"]  # the segbd variant's encoder
    assert enc.main_layer0[0].in_channels == 3  # (input_ch is ignored: the encoder is RGB)
    std = dec.get_task_weights()
    assert len(std) == 2 and abs(float(std[1].reshape(-1)[0]) - 2.718281828) < 1e-6


def test_factory_errors_and_refusals():
    from models.dilated_fcn import MCDSegBDMultiTaskDecoder, MCDTripleMultiTaskDecoder
    from models.model_util import get_triple_multitask_models
    with pytest.raises(NotImplementedError, match="Only FCN"):
        get_triple_multitask_models("fcn", 6, 5)
    with pytest.raises(NotImplementedError, match="source-only"):
        get_triple_multitask_models("drn_d_22", 6, 5, is_src_only=True)
    with pytest.raises(NotImplementedError, match="semseg_shortcut"):
        get_triple_multitask_models("drn_d_22", 6, 5, semseg_shortcut=True)
    with pytest.raises(NotImplementedError, match="depth_shortcut"):
        MCDTripleMultiTaskDecoder(5, 3, depth_shortcut=True)
    dec = MCDTripleMultiTaskDecoder(5, 3)
    with pytest.raises(AssertionError):
        dec.get_boundary_loss_by_extra_conv({})
    with pytest.raises(AssertionError):
        dec.get_psuedo_boundary_loss({})
    assert "TypeError" in MCDTripleMultiTaskDecoder.get_psuedo_boundary_loss.__doc__
    with pytest.raises(NotImplementedError, match="use_seg2bd_conv"):  # the segbd decoder keeps refusing the flag
        MCDSegBDMultiTaskDecoder(5, 3, use_seg2bd_conv=True)


def test_parsers_flags_layout_and_backfill(tmp_path):
    import adapt_triple_multitask_tester as tester
    import adapt_triple_multitask_trainer as trainer
    from trainer_common import parse_args
    a = parse_args(trainer.get_parser(), ["suncg", "nyu", "--input_ch", "6"])
    assert (a.depth_shortcut, a.semseg_shortcut, a.add_pred_seg_boundary_loss, a.use_seg2bd_conv) == (False,) * 4
    assert (a.boundary_loss_converging_epoch, a.scale_bd_loss) == (5, 1)
    a = parse_args(trainer.get_parser(), ["suncg", "nyu", "--input_ch", "6", "--use_seg2bd_conv", "--boundary_loss_converging_epoch", "-1",
                                          "--scale_bd_loss", "3", "--opt", "adam", "--net", "drn_d_22", "--base_outdir", str(tmp_path)])
    assert a.use_seg2bd_conv and (a.boundary_loss_converging_epoch, a.scale_bd_loss, a.opt) == (-1, 3, "adam")
    assert trainer.check_inputs(a) is a
    lay = trainer.TRAINER.layout(a, False)
    assert lay.pth_dir == os.path.join(str(tmp_path), "suncg-train2nyu-train_6ch_MCD_triple_multitask", "pth")
    assert lay.model_name == "MCD-normal-drn_d_22" and lay.json_fn.endswith("param-MCD-normal-drn_d_22.json")
    assert trainer.TRAINER.layout(a, True).json_fn.endswith("param-MCD-normal-drn_d_22_resume.json")
    assert trainer.TRAINER.src_input_ch == 7 and trainer.TRAINER.sums == (
        "c_loss", "d_loss", "src_semseg_loss", "src_depth_loss", "tgt_depth_loss", "src_boundary_loss", "tgt_psuedo_boundary_loss",
        "src_extra_boundary_loss")
    assert set(trainer.TRAINER.backfill) == {"depth_shortcut", "semseg_shortcut", "add_pred_seg_boundary_loss", "use_seg2bd_conv",
                                             "boundary_loss_converging_epoch", "scale_bd_loss"}
    # what this trainer cannot be fed is refused with a message that says why
    for extra, word in ((["--synthetic_raw"], "synthetic_raw"), (["--src_file_list", "x.txt"], "file_list"), (["--tgt_file_list", "x.txt"], "file_list")):
        with pytest.raises(SystemExit, match=word) as e:
            trainer.check_inputs(parse_args(trainer.get_parser(), ["suncg", "nyu", "--input_ch", "6"] + extra))
        assert "boundary column" in str(e.value)
    with pytest.raises(SystemExit, match="input_ch"):
        trainer.check_inputs(parse_args(trainer.get_parser(), ["suncg", "nyu"]))
    assert trainer.check_inputs(parse_args(trainer.get_parser(), ["suncg", "nyu", "--resume", "x.pth.tar"])).resume  # the checkpoint's decide
    # the tester back-fills use_seg2bd_conv for checkpoints written before the flag existed
    old = argparse.Namespace(net="drn_d_22")
    assert tester.backfill(old).use_seg2bd_conv is False
    assert tester.backfill(argparse.Namespace(use_seg2bd_conv=True)).use_seg2bd_conv is True
    # the other trainers' declarations keep today's behaviour
    import adapt_segbd_multitask_trainer
    assert adapt_segbd_multitask_trainer.TRAINER.src_input_ch is None


def test_seven_channel_synthetic_sample_carries_its_labels_boundary():
    from datasets import SyntheticRGBD, get_dataset
    ds7 = SyntheticRGBD(4, 7, (24, 16), 5, seed=3)
    ds6 = SyntheticRGBD(4, 6, (24, 16), 5, seed=3)
    for i in range(3):
        img, lbl = ds7[i]
        assert tuple(img.shape) == (7, 16, 24) and img.dtype == torch.float32 and tuple(lbl.shape) == (16, 24)
        v = lbl.float()[None, None]
        want = (F.max_pool2d(v, 3, 1, 1) != -F.max_pool2d(-v, 3, 1, 1))[0, 0].float()
        assert torch.equal(img[6], want) and set(img[6].unique().tolist()) <= {0.0, 1.0}
        img6, lbl6 = ds6[i]
        assert tuple(img6.shape) == (6, 16, 24) and torch.equal(lbl6, ds6[i][1])  # the 6-channel sample draws as before
    assert 0 < float(ds7[0][0][6].mean()) <= 1
    with pytest.raises(NotImplementedError, match="boundary column"):
        SyntheticRGBD(4, 7, (24, 16), 5, seed=3, raw=True)
    d = get_dataset("suncg", "train", None, None, test=True, input_ch=7, synthetic=dict(length=2, img_shape=[24, 16], n_class=5, seed=1))
    assert len(d[0]) == 3 and tuple(d[0][0].shape) == (7, 16, 24)


def test_make_loader_gives_the_source_its_own_channel_count():
    import trainer_common
    args = argparse.Namespace(synthetic=True, synthetic_raw=False, synthetic_len=4, train_img_shape=[24, 16], n_class=5, seed=1, input_ch=6,
                              batch_size=2, background_id=255, src_file_list=None, tgt_file_list=None)
    run = argparse.Namespace(rank=0)
    pairs = [("suncg", "train"), ("nyu", "train")]
    src, tgt = next(iter(trainer_common.make_loader(args, run, pairs, src_input_ch=7)))
    assert tuple(src[0].shape) == (2, 7, 16, 24) and tuple(tgt[0].shape) == (2, 6, 16, 24)
    src, tgt = next(iter(trainer_common.make_loader(args, run, pairs)))
    assert tuple(src[0].shape) == (2, 6, 16, 24) and tuple(tgt[0].shape) == (2, 6, 16, 24)


def test_product_imports_no_oracle():
    code = ("import sys; sys.path.insert(0, %r); import adapt_triple_multitask_trainer, adapt_triple_multitask_tester; "
            "assert not [m for m in sys.modules if m == 'oracle' or m.startswith('oracle.')], 'oracle imported'" % PKG)
    env = dict(os.environ, MCDSEG_PRETRAINED="0")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=PKG)
    assert r.returncode == 0, r.stderr[-2000:]
    for fn in ("adapt_triple_multitask_trainer.py", "adapt_triple_multitask_tester.py", "csrc/seg2bd.hip"):
        assert "oracle" not in open(os.path.join(PKG, fn)).read(), fn


# ---------------------------------------------------------------------------------------------- the solver's step order, on stubs
def _stub_solver(log, num_k=2, **kw):
    from solvers.solver import TripleMultiTaskMCDSolver

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

        def _semseg_logits(self, f):
            from mcdseg import ops
            log.append(("logits", ops.BN_RUNNING_REPEAT))
            return "L"

        def get_loss(self, f, gt, dep, bd, separately_returning=False, logits=None):
            log.append(("get_loss", tuple(dep.shape), tuple(bd.shape), logits))
            return f["h8"] * self.v, f["h8"] * self.v * 2, f["h8"] * self.v * 4

        def _semseg_task_loss(self, f, gt, logits=None):
            log.append(("semseg_task", torch.is_grad_enabled()))
            return f["h8"] * self.v

        def depth_forward(self, f):
            log.append(("depth_forward", torch.is_grad_enabled()))

        def get_depth_loss(self, f, dep):
            log.append(("depth", tuple(dep.shape), f["h8"].requires_grad))
            return f["h8"] * self.v * 8

        def get_boundary_loss_by_extra_conv(self, f, gt_bdry=None, separately_returning=False, logits=None):
            log.append(("extra", None if gt_bdry is None else tuple(gt_bdry.shape), logits))
            return f["h8"] * self.v * (16 if gt_bdry is not None else 32)

        def get_psuedo_boundary_loss(self, f, separately_returning=False):
            log.append(("psuedo",))
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

    return TripleMultiTaskMCDSolver(Enc(), Dec(), Opt("oe"), Opt("od"), num_k=num_k, **kw)


def test_solver_step_order_on_stub_modules():
    log = []
    src, tgt, gt = torch.ones(2, 7, 8, 8), torch.full((2, 6, 8, 8), 2.0), torch.zeros(2, 8, 8, dtype=torch.int64)
    solver = _stub_solver(log, num_k=2, num_multiply_d_loss=4, boundary_loss_converging_epoch=5, scale_bd_loss=3)
    c, d, parts = solver.step(src, gt, tgt, epoch=9)  # no flag: no target term at any epoch
    names = [e[:2] if e[0] in ("oe", "od") else e[:1] for e in log]
    A = [("oe", "zero"), ("od", "zero"), ("enc",), ("enc",), ("get_loss",), ("depth",), ("oe", "step"), ("od", "step")]
    B = [("oe", "zero"), ("od", "zero"), ("enc",), ("semseg_task",), ("depth_forward",), ("enc",), ("disc",), ("od", "step")]
    C = [("oe", "zero"), ("enc",), ("disc",), ("oe", "step")] * 2
    assert names == A + B + C, names
    encs = [e for e in log if e[0] == "enc"]
    assert all(e[1] == (2, 3, 8, 8) for e in encs)  # only the RGB channels reach the encoder
    assert [e[2] for e in encs] == [True, True, False, False, True, True]  # step A tapes BOTH passes: the target's depth loss reaches the encoder
    gl = [e for e in log if e[0] == "get_loss"][0]
    assert gl[1] == (2, 3, 8, 8) and gl[2] == (2, 1, 8, 8) and gl[3] is None  # HHA = channels 3..5 of 7, boundary = channel 6
    assert [e for e in log if e[0] == "depth"] == [("depth", (2, 3, 8, 8), True)]
    assert ("semseg_task", True) in log and ("depth_forward", False) in log
    assert float(c) == 1 + 2 + 4 + 8 * 2 and parts[4] == 0 and parts[5] == 0
    assert [float(p) for p in parts[:4]] == [1.0, 2.0, 16.0, 4.0]
    assert float(d) == 2.0 * 3 * 4 / 2
    # use_seg2bd_conv: one pass of the segmentation decoders under two running-statistics updates feeds both consumers; the target term
    # joins once the epoch is past the converging epoch
    del log[:]
    solver = _stub_solver(log, num_k=1, use_seg2bd_conv=True, boundary_loss_converging_epoch=5, scale_bd_loss=3)
    c, d, parts = solver.step(src, gt, tgt, epoch=5)
    assert ("logits", 2) in log and [e for e in log if e[0] == "extra"] == [("extra", (2, 1, 8, 8), "L")]
    assert [e for e in log if e[0] == "get_loss"][0][3] == "L"
    assert float(parts[5]) == 16.0 and parts[4] == 0 and float(c) == 1 + 2 + 4 + 16 + 16
    del log[:]
    c, d, parts = solver.step(src, gt, tgt, epoch=6)
    assert [e for e in log if e[0] == "extra"] == [("extra", (2, 1, 8, 8), "L"), ("extra", None, None)]
    assert float(parts[4]) == 2 * 32 * 3 and float(c) == 1 + 2 + 4 + 16 + 16 + 2 * 32 * 3
    # both flags: the seg2bd target term overwrites the pseudo term in the loss, the logged sum takes both (:222-234)
    del log[:]
    solver = _stub_solver(log, num_k=1, use_seg2bd_conv=True, add_pred_seg_boundary_loss=True, boundary_loss_converging_epoch=5, scale_bd_loss=3)
    c, d, parts = solver.step(src, gt, tgt, epoch=6)
    assert ("psuedo",) in log and float(parts[4]) == 15.0 + 192.0 and float(c) == 1 + 2 + 4 + 16 + 16 + 192
