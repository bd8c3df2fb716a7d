"""CPU: the multitask / source-only testers' host side -- the depth-image cast rule against the reference's own outputs
(tests/golden/depth_image_small.npz), the command lines of the reference, the no-GPU exit, and the C ABI of the fused tails."""
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

from infer_tail_ref import numpy_u8, unnormalize_u8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("cd", [3, 1])
def test_depth_rule_reproduces_the_reference_bytes(golden, cd):
    """the rule of mcdseg_depth_image_u8, restated without numpy's cast, gives the reference's unnormalize bytes -- wrapped values,
    NaN, +-inf and values beyond the int32 range included -- and Pillow's BILINEAR resize of them gives the recorded PNG content"""
    fx = golden.npz("depth_image_small.npz")
    x, ref = fx["map_%dch" % cd], fx["img_%dch" % cd]
    assert x.dtype == np.float32 and x.shape[-1] == cd and not np.isfinite(x).all()
    got = unnormalize_u8(x)
    assert got.shape == ref.shape == (24, 32, 3)
    assert np.array_equal(got, ref), int((got != ref).sum())
    t = ((x.astype(np.float64) * np.array([.229, .224, .225])) + np.array([.485, .456, .406])) * 255
    assert ((t < 0) | (t >= 256)).mean() > 0.15  # a fifth of the bytes wrapped or zeroed: the rule, not the plain range, is under test
    for k, (ow, oh) in enumerate(fx["sizes"]):
        assert np.array_equal(np.asarray(Image.fromarray(got).resize((int(ow), int(oh)), Image.BILINEAR)), fx["resized%d_%dch" % (k, cd)])


def test_numpy_u8_edge_values():
    v = np.array([-1.0, -200.2, 256.0, 300.7, np.nan, np.inf, -np.inf, 2.0 ** 31 - 0.5, -2.0 ** 31, 3e9 + 7, 2.0 ** 40 + 300, 255.9, -0.5])
    assert numpy_u8(v).tolist() == [255, 56, 0, 44, 0, 0, 0, 255, 0, 0, 0, 255, 0]


def test_multitask_tester_parser_takes_the_reference_flags():
    from argmyparse import get_da_mcd_testing_parser
    a = get_da_mcd_testing_parser().parse_args(["nyu", "train_output/x/pth/MCD-normal-drn_d_38-40.pth.tar", "--split", "test",
                                                "--outdir", "o", "--test_img_shape", "640", "480", "--saves_prob", "--use_f2",
                                                "--synthetic", "--synthetic_len", "3", "-b", "2"])
    assert (a.tgt_dataset, a.split, a.outdir, a.test_img_shape, a.saves_prob, a.use_f2, a.synthetic, a.batch_size) == \
        ("nyu", "test", "o", [640, 480], True, True, True, 2)


@pytest.mark.parametrize("flag", ["---saves_prob", "--saves_prob", None])
def test_source_tester_parser_takes_the_reference_flags(flag):
    import source_tester
    argv = ["suncg", "--split", "test", "train_output/suncg-train_only_6ch/pth/normal-drn_d_38-1.pth.tar", "--outdir", "o",
            "--test_img_shape", "320", "240", "--synthetic", "--synthetic_len", "2", "-b", "2"] + ([flag] if flag else [])
    a = source_tester.get_parser().parse_args(argv)
    assert (a.tgt_dataset, a.split, a.outdir, a.test_img_shape, a.synthetic, a.batch_size) == ("suncg", "test", "o", [320, 240], True, 2)
    assert a.saves_prob is (flag is not None)
    assert source_tester.get_parser().parse_args(["nyu", "ck.pth.tar"]).split == "val"


def test_source_tester_subdir_quirk():
    import source_tester
    assert source_tester.add_subdir_if_necessary("out/label", "0001", "suncg") == os.path.join("out/label", "0001")
    assert source_tester.add_subdir_if_necessary("out/label", "0001", "nyu") == "out/label"


@pytest.mark.parametrize("which", ["adapt_multitask_tester", "source_tester"])
def test_testers_exit_cleanly_without_a_gpu(which, monkeypatch, tmp_path):
    import importlib
    mod = importlib.import_module(which)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit) as e:
        mod.main(["nyu", str(tmp_path / "missing.pth.tar"), "--outdir", str(tmp_path / "o"), "--synthetic"])
    assert "MI355X" in str(e.value.code)
    assert not (tmp_path / "o").exists()


def test_fused_tail_entry_points_are_declared_and_bound():
    from mcdseg import _lib
    hdr = open(os.path.join(ROOT, "include", "mcdseg.h")).read()
    for name in ("mcdseg_predict_up8_workspace_bytes", "mcdseg_predict_labels_up8", "mcdseg_depth_image_u8"):
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in _lib.EXPORTS, name
    from mcdseg import ops
    for fn in ("predict_labels_up8", "predict_labels_bilinear8", "depth_image_u8"):
        assert callable(getattr(ops, fn))


def test_fused_tail_wrappers_refuse_cpu_tensors():
    from mcdseg import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.predict_labels_bilinear8(torch.zeros(1, 3, 2, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.depth_image_u8(torch.zeros(1, 1, 2, 2))
