"""GPU: the multitask and source-only testers end to end -- train one synthetic epoch, run the tester at a test shape different
from the train shape, and hold its outputs against the CPU oracle evaluating the same checkpoint."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

COMMON = ["-b", "2", "--train_img_shape", "96", "64", "--synthetic", "--synthetic_len", "4", "--no_pretrained", "--no_tflog",
          "--epochs", "1", "--max_iter", "10"]
TEST_WH = (80, 56)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _check_labels(got, o, n_used, safe_margin=2e-3):
    """the rule of test_adapt_tester_label_maps_match_oracle, at the test shape: exact where the oracle's top-2 margin exceeds
    ``safe_margin``; returns the count of agreeing pixels"""
    top2 = o[:n_used].topk(2, dim=0).values
    safe = Image.fromarray(((top2[0] - top2[1]) > safe_margin).numpy().astype(np.uint8)).resize(TEST_WH, Image.NEAREST)
    ref = np.asarray(Image.fromarray(o[:n_used].argmax(0).numpy().astype(np.uint8)).resize(TEST_WH, Image.NEAREST))
    assert got.shape == ref.shape == (TEST_WH[1], TEST_WH[0]) and got.max() < n_used
    safe = np.asarray(safe).astype(bool)
    assert safe.mean() > 0.5
    assert (got == ref)[safe].all()
    return int((got == ref).sum())


def _check_eval(base, gts, refs):
    """eval_result.json: the ground-truth side exactly, the prediction side within what the label agreement allows"""
    res = json.load(open(os.path.join(base, "eval_result.json")))
    gt = np.concatenate([g.flatten() for g in gts])
    ref = np.concatenate([r.flatten() for r in refs])
    keep = gt != 40
    counts = np.bincount(gt[keep], minlength=41)
    used = np.where(counts != 0)[0]
    assert res["used_class_ids"] == used.tolist()
    assert res["gt_distribution"] == counts[used].tolist()
    assert abs(res["pixAcc"] - 100.0 * float((gt[keep] == ref[keep]).mean())) <= 1.0
    assert 0.0 <= res["mIoU"] <= 100.0


@pytest.mark.parametrize("ch", [6, 4])
def test_adapt_multitask_tester_matches_oracle(tmp_path, ch):
    _need_gpu()
    import adapt_multitask_tester
    import adapt_multitask_trainer
    import util
    from datasets import SyntheticRGBD
    from oracle import ref_multitask
    out = str(tmp_path / "out")
    assert adapt_multitask_trainer.main(["suncg", "nyu", "--base_outdir", out, "--input_ch", str(ch)] + COMMON) == 0
    ck_fn = os.path.join(out, "suncg-train2nyu-train_%dch_MCDmultitask" % ch, "pth", "MCD-normal-drn_d_38-1.pth.tar")
    label_dir, depth_dir, ent = adapt_multitask_tester.main(["nyu", ck_fn, "--outdir", str(tmp_path / "test"), "--synthetic",
                                                             "--synthetic_len", "3", "-b", "2", "--use_f2", "--saves_prob",
                                                             "--test_img_shape", str(TEST_WH[0]), str(TEST_WH[1])])
    base = os.path.join(str(tmp_path / "test"), "suncg-train2nyu-train_%dch_MCDmultitask---nyu-val" % ch, "MCD-normal-drn_d_38-1.tar-use_f2")  # ".pth" dropped, ".tar" kept
    assert label_dir == os.path.join(base, "label") and depth_dir == os.path.join(base, "depth")
    assert os.path.exists(os.path.join(base, "param.json"))
    assert len([f for f in os.listdir(base) if f.startswith("ave_ent_")]) == 1
    ck = util.load_checkpoint(ck_fn)
    from oracle import ref_loss
    enc, dec = ref_multitask.get_multitask_models("drn_d_38", ch, 41, semseg_criterion=ref_loss.CrossEntropyLoss2d(torch.ones(41)))
    enc.load_state_dict(ck["enc_state_dict"]), dec.load_state_dict(ck["dec_state_dict"])
    enc.eval(), dec.eval()
    ds = SyntheticRGBD(3, ch, [96, 64], 41, seed=4321, test=True)
    ents, agree, total, depth_ok, depth_total, gts, refs = [], 0, 0, 0, 0, [], []
    for i in range(3):
        img, lbl, name = ds[i]
        gts.append(lbl.numpy())
        with torch.no_grad():
            p1, _, pd = dec(enc(img[None, :3]))
        p = torch.softmax(p1, dim=1)
        ents.append(float(-(p * torch.log(p + 1e-6)).mean()))
        got = np.array(Image.open(os.path.join(label_dir, name)))
        agree += _check_labels(got, p1[0], 40)
        refs.append(p1[0, :40].argmax(0).numpy())
        total += got.size
        # the reference's depth tail (adapt_multitask_tester.py:151-154) on the oracle's full-resolution depth map
        with np.errstate(invalid="ignore", over="ignore"):
            u8 = np.uint8(((pd[0].numpy().transpose(1, 2, 0).astype(np.float64) * np.array([.229, .224, .225])) +
                           np.array([.485, .456, .406])) * 255)
        ref_d = np.asarray(Image.fromarray(u8).resize(TEST_WH, Image.BILINEAR))
        got_d = np.array(Image.open(os.path.join(depth_dir, name)))
        assert got_d.shape == ref_d.shape == (TEST_WH[1], TEST_WH[0], 3) and got_d.dtype == np.uint8
        diff = (got_d.astype(np.int64) - ref_d) % 256
        depth_ok += int(((diff <= 1) | (diff == 255)).sum())
        depth_total += diff.size
        prob = np.load(os.path.join(base, "prob", name.replace("png", "npy")))
        assert prob.shape == (41, 64, 96)
        assert np.abs(prob - p1[0].numpy()).max() <= 1e-3 * max(1.0, float(p1.abs().max()))
    assert agree / total >= 0.995
    assert depth_ok / depth_total >= 0.99, depth_ok / depth_total
    assert abs(ent - sum(ents) / 3) <= 1e-4 * abs(sum(ents) / 3)
    _check_eval(base, gts, refs)


def test_source_tester_matches_oracle(tmp_path):
    _need_gpu()
    import source_tester
    import source_trainer
    import util
    from datasets import SyntheticRGBD
    from oracle import ref_models
    out = str(tmp_path / "out")
    assert source_trainer.main(["suncg", "--base_outdir", out, "--input_ch", "6"] + COMMON) == 0
    ck_fn = os.path.join(out, "suncg-train_only_6ch", "pth", "normal-drn_d_38-1.pth.tar")
    ck = util.load_checkpoint(ck_fn)
    assert all(k.startswith("module.") for k in ck["state_dict"])
    label_dir, ent = source_tester.main(["nyu", ck_fn, "--outdir", str(tmp_path / "test"), "--synthetic", "--synthetic_len", "3",
                                         "-b", "2", "---saves_prob", "--test_img_shape", str(TEST_WH[0]), str(TEST_WH[1])])
    base = os.path.join(str(tmp_path / "test"), "suncg-train_only_6ch---nyu-val", "normal-drn_d_38-1.tar")
    assert label_dir == os.path.join(base, "label")
    assert os.path.getsize(os.path.join(base, "data_list.txt")) == 0
    assert os.path.exists(os.path.join(base, "param.json"))
    assert len([f for f in os.listdir(base) if f.startswith("ave_ent_")]) == 1
    model = ref_models.DRNSeg("drn_d_38", 41, input_ch=6)
    model.load_state_dict({k[len("module."):]: v for k, v in ck["state_dict"].items()})
    model.eval()
    ds = SyntheticRGBD(3, 6, [96, 64], 41, seed=4321, test=True)
    ents, agree, total, gts, refs = [], 0, 0, [], []
    for i in range(3):
        img, lbl, name = ds[i]
        gts.append(lbl.numpy())
        with torch.no_grad():
            o = model(img[None])
        p = torch.softmax(o, dim=1)
        ents.append(float(-(p * torch.log(p + 1e-6)).mean()))
        got = np.array(Image.open(os.path.join(label_dir, name)))
        agree += _check_labels(got, o[0], 40)
        refs.append(o[0, :40].argmax(0).numpy())
        total += got.size
        prob = np.load(os.path.join(base, "prob", name.replace("png", "npy")))
        assert prob.shape == (41, 64, 96)
        assert np.abs(prob - o[0].numpy()).max() <= 1e-3 * max(1.0, float(o.abs().max()))
    assert agree / total >= 0.995
    assert abs(ent - sum(ents) / 3) <= 1e-4 * abs(sum(ents) / 3)
    _check_eval(base, gts, refs)
