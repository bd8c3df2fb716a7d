"""GPU: ``--refine_by_boundary`` of the segbd and the triple testers and ``tools/refine_seg_by_boundary.py``, end to end: what they
write is the numpy restatement (tests/refine_ref.py) applied to the PNGs of the same run, byte for byte; without the flag the testers
write what they wrote before."""
import importlib
import importlib.util
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import refine_ref as R
from conftest import PKG

pytestmark = pytest.mark.gpu

# the command lines of tests/test_segbd_gpu.py::test_segbd_trainer_resume_and_tester and its triple counterpart, restated
NET = "drn_d_22"
CLI = ["-b", "2", "--train_img_shape", "96", "64", "--synthetic", "--synthetic_len", "4", "--no_pretrained", "--no_tflog",
       "--max_iter", "0", "--net", NET]
VARIANTS = {
    "segbd": ("adapt_segbd_multitask_trainer", "adapt_segbd_multitask_tester", "suncg-train2nyu-train_3ch_MCD_segbd_multitask",
              ["--add_pred_seg_boundary_loss", "--boundary_loss_converging_epoch", "-1", "--opt", "sgd"]),
    "triple": ("adapt_triple_multitask_trainer", "adapt_triple_multitask_tester", "suncg-train2nyu-train_6ch_MCD_triple_multitask",
               ["--input_ch", "6", "--use_seg2bd_conv", "--boundary_loss_converging_epoch", "-1", "--opt", "sgd"]),
}
TESTER = ["--synthetic", "--synthetic_len", "3", "-b", "2", "--test_img_shape", "80", "56"]
LO, HI = 4, 2000


def _png(path):
    return np.array(Image.open(path))


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_tester_writes_the_restatement_of_its_own_pngs(variant, tmp_path, device):
    trainer, tester, run, extra = VARIANTS[variant]
    trainer, tester = importlib.import_module(trainer), importlib.import_module(tester)
    out = str(tmp_path / "out")
    assert trainer.main(["suncg", "nyu", "--base_outdir", out, "--epochs", "1"] + extra + CLI) == 0
    ck_fn = os.path.join(out, run, "pth", "MCD-normal-%s-1.pth.tar" % NET)

    def dirs(result):
        d = result[0] if isinstance(result[0], dict) else {"label": result[0], "boundary": result[1]}
        return d["label"], d["boundary"]

    first = tester.main(["nyu", ck_fn, "--outdir", str(tmp_path / "plain")] + TESTER)
    assert len(first) == (2 if variant == "triple" else 3)  # what main() returned before the flag existed
    label1, boundary1 = dirs(first)
    base1 = os.path.dirname(label1)
    names = sorted(os.listdir(label1))
    assert len(names) == 3 and not os.path.exists(os.path.join(base1, "refined_label"))
    assert not os.path.exists(os.path.join(base1, "eval_result_refined.json"))
    with open(os.path.join(base1, "param.json")) as f:
        assert not {"refine_by_boundary", "boundary_thre", "min_thre", "max_thre"} & set(json.load(f))
    thre = int(np.median(np.concatenate([_png(os.path.join(boundary1, n)).reshape(-1) for n in names])))
    masks = [_png(os.path.join(boundary1, n)) > thre for n in names]
    assert any(m.any() for m in masks) and not all(m.all() for m in masks), "the median threshold must cut the boundary images"

    second = tester.main(["nyu", ck_fn, "--outdir", str(tmp_path / "refined"), "--refine_by_boundary", "--boundary_thre", str(thre),
                          "--min_thre", str(LO), "--max_thre", str(HI)] + TESTER)
    assert len(second) == len(first)
    label2, boundary2 = dirs(second)
    base2 = os.path.dirname(label2)
    refined_dir = os.path.join(base2, "refined_label")
    assert sorted(os.listdir(refined_dir)) == names == sorted(os.listdir(label2)) == sorted(os.listdir(boundary2))
    changed = 0
    for n in names:
        assert _bytes(os.path.join(label2, n)) == _bytes(os.path.join(label1, n)), n
        assert _bytes(os.path.join(boundary2, n)) == _bytes(os.path.join(boundary1, n)), n
        seg, bd = _png(os.path.join(label2, n)), _png(os.path.join(boundary2, n))
        got = _png(os.path.join(refined_dir, n))
        assert got.dtype == np.uint8 and got.shape == (56, 80)
        want = R.refine_by_boundary(seg, bd, thre, LO, HI)
        assert np.array_equal(got, want), n
        changed += int((want != seg).sum())
    print("%s: threshold %d, %d pixels relabelled" % (variant, thre, changed))
    with open(os.path.join(base2, "eval_result_refined.json")) as f:
        result = json.load(f)
    assert sorted(result) == ["after", "before"] and "mIoU" in result["before"] and "mIoU" in result["after"]
    with open(os.path.join(base2, "eval_result.json")) as f, open(os.path.join(base1, "eval_result.json")) as g:
        assert json.load(f) == json.load(g)
    with open(os.path.join(base2, "param.json")) as f:
        assert json.load(f)["refine_by_boundary"] is True


def _tool():
    spec = importlib.util.spec_from_file_location("refine_seg_by_boundary_tool", os.path.join(PKG, "tools", "refine_seg_by_boundary.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tool_reproduces_the_golden_outputs(tmp_path, golden, device):
    fx = golden.npz("refine_small.npz")
    tool = _tool()
    small = [k[2:] for k in fx.files if k.startswith("b_") and fx[k].shape == R.GOLDEN_SHAPE]
    assert len(small) == 12
    for group, names in (("small", small), ("spiral", ["spiral_130x200"])):
        base = tmp_path / group
        for sub in ("label", "boundary", "gt"):
            os.makedirs(str(base / sub))
        for n in names:
            Image.fromarray(fx["s_" + n]).save(str(base / "label" / (n + ".png")))
            Image.fromarray(fx["b_" + n]).save(str(base / "boundary" / (n + ".png")))
            Image.fromarray(fx["s_" + n]).save(str(base / "gt" / (n + ".png")))  # the labels as their own ground truth
        thre, lo, hi = (int(v) for v in fx["p_" + names[0]])
        outdir = tool.main([str(base / "label"), str(base / "boundary"), "--thre", str(thre), "--min_thre", str(lo), "--max_thre", str(hi),
                            "--gt_dir", str(base / "gt"), "--n_class", "41", "-b", "5"])
        assert outdir == str(base / "refined_label") and sorted(os.listdir(outdir)) == sorted(n + ".png" for n in names)
        for n in names:
            assert np.array_equal(_png(os.path.join(outdir, n + ".png")), fx["o_" + n]), n
        with open(str(base / "eval_result_refined.json")) as f:
            result = json.load(f)
        assert sorted(result) == ["after", "before"] and result["before"]["pixAcc"] == 100.0 and result["after"]["pixAcc"] < 100.0


def test_tool_names_the_boundary_image_of_another_size(tmp_path, device):
    for sub in ("label", "boundary"):
        os.makedirs(str(tmp_path / sub))
    Image.fromarray(np.zeros((8, 9), np.uint8)).save(str(tmp_path / "label" / "a.png"))
    Image.fromarray(np.zeros((9, 8), np.uint8)).save(str(tmp_path / "boundary" / "a.png"))
    with pytest.raises(ValueError, match=r"boundary.a\.png is 8 x 9"):
        _tool().main([str(tmp_path / "label"), str(tmp_path / "boundary")])
