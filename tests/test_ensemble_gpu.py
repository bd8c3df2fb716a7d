"""GPU: ``ops.ensemble_probs`` / ``ops.label_resize_colorize`` (csrc/ensemble.hip), the tool built on them and the
testers' ``--vis``, against the numpy / Pillow oracle of tests/ensemble_ref.py.

Everything is compared bit for bit.  The one liberty is the oracle's (``ensemble_ref.canon``): the payload of a NaN that an addition makes
is left to the implementation by IEEE 754 and is the host's in numpy, so the oracle's NaNs are mapped to 0x7FC00000, which is what the
device writes for every NaN; every other float is compared by its 32 bits, NaN positions included."""
import importlib.util
import json
import os
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import ensemble_ref as R
from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu

KS = (2, 3, 5, 16)
CS = (1, 3, 20, 41)
PLANES = ((1, 1), (3, 5), (7, 9), (4, 8), (16, 32), (33, 64))  # (H, W): W % 4 != 0 and == 0; one pixel; more than one block
NAIVE_FAILS = ((2, 7), (4, 6), (8, 6), (14, 5))                  # (in, out) where floor((x + 0.5) in / out) is not Pillow's index

_oracle = {}


def oracle(kind, k, n, c, h, w, method):
    """(maps, canon(combined) [N,C,H,W]) computed once per case and left unchanged"""
    key = (kind, k, n, c, h, w)
    if key not in _oracle:
        _oracle[key] = {"maps": R.make_maps(kind, k, n, c, h, w, seed=zlib.crc32(repr(key).encode()))}
    entry = _oracle[key]
    if method not in entry:
        entry[method] = R.canon(R.combine(entry["maps"], method))
        entry[method].setflags(write=False)
    return entry["maps"], entry[method]


def off_grid(t, device):
    """a contiguous device copy of ``t`` whose base lies 4 bytes off the 16-byte grid"""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=device)
    out = buf[1:1 + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def n_used_of(c):
    return sorted({1, max(c - 1, 1), c})


def run(maps_dev, method, n_used, want_prob=True):
    from mcdseg import ops
    prob, lab = ops.ensemble_probs(maps_dev, method, n_used, want_prob=want_prob)
    assert lab.dtype == torch.uint8 and tuple(lab.shape) == tuple(maps_dev[0].shape[:1] + maps_dev[0].shape[2:])
    assert (prob is None) == (not want_prob)
    return (None if prob is None else prob.cpu().numpy()), lab.cpu().numpy()


def hold_case(kind, k, n, c, h, w, method, device, aligned=True):
    maps, want = oracle(kind, k, n, c, h, w, method)
    dev = [torch.from_numpy(m).to(device) for m in maps]
    if not aligned:
        dev[k // 2] = off_grid(dev[k // 2], device)
    what = (kind, method, k, n, c, h, w, aligned)
    for n_used in n_used_of(c):
        prob, lab = run(dev, method, n_used)
        assert prob.dtype == np.float32 and R.bits(prob).tobytes() == R.bits(want).tobytes(), what
        assert np.array_equal(lab, R.labels_of(want, n_used)), what + (n_used,)
        none, lab_alone = run(dev, method, n_used, want_prob=False)
        assert np.array_equal(lab_alone, lab), what + (n_used, "out = NULL")
    again, lab_again = run(dev, method, n_used_of(c)[-1])
    assert R.bits(again).tobytes() == R.bits(prob).tobytes() and np.array_equal(lab_again, lab), what + ("second run",)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("method", R.METHODS)
def test_ensemble_probs_shapes(method, k, device):
    for c in CS:
        for h, w in PLANES:
            for n in (1, 3):
                hold_case("random", k, n, c, h, w, method, device)
        hold_case("random", k, 3, c, 16, 32, method, device, aligned=False)  # W % 4 == 0 but one base 4 bytes off: the scalar path
        hold_case("random", k, 1, c, 7, 9, method, device, aligned=False)


@pytest.mark.parametrize("kind", [kd for kd in R.KINDS if kd != "random"])
@pytest.mark.parametrize("method", R.METHODS)
def test_ensemble_probs_inputs(method, kind, device):
    for k, n, c, h, w in ((2, 1, 3, 7, 9), (3, 2, 20, 16, 32), (5, 1, 41, 33, 64)):
        maps, want = oracle(kind, k, n, c, h, w, method)
        if kind == "saturated" and method == "averaging":
            assert np.isnan(want).any() and np.isinf(want).any()  # inf - inf and overflow are both there
        if kind == "nan":
            assert np.isnan(want).any() and not np.isnan(want).all()
        if kind == "equal":
            assert (want == want[:, :1]).all()
        hold_case(kind, k, n, c, h, w, method, device)
        hold_case(kind, k, n, c, h, w, method, device, aligned=False)


def test_oracle_fixture_on_the_device(device):
    """tests/golden/ensemble_small.npz (the oracle's output; see make_ensemble_golden.py): both ops reproduce it"""
    from mcdseg import ops
    fx = np.load(os.path.join(GOLDEN, "ensemble_small.npz"))
    maps = [torch.from_numpy(fx["p%d" % k]).to(device) for k in range(3)]
    n_used, wh = int(fx["n_used"]), tuple(int(v) for v in fx["out_wh"])
    pal = torch.from_numpy(R.voc_palette(n_used + 1)).to(device)
    for method in R.METHODS:
        prob, lab = ops.ensemble_probs(maps, method, n_used)
        assert tuple(prob.shape) == (20, 12, 16) and tuple(lab.shape) == (12, 16)
        assert R.bits(prob.cpu().numpy()).tobytes() == R.bits(fx["prob_" + method]).tobytes()
        out, vis = ops.label_resize_colorize(lab[None], wh, pal)
        assert np.array_equal(out[0].cpu().numpy(), fx["label_" + method]) and np.array_equal(vis[0].cpu().numpy(), fx["vis_" + method])


def test_ensemble_probs_refusals(device):
    from mcdseg import ops
    z = torch.zeros(2, 3, 4, 4, device=device)
    for bad in (0, 4):
        with pytest.raises(ValueError, match="n_used"):
            ops.ensemble_probs([z, z], "averaging", bad)
    with pytest.raises(ValueError, match="n_used"):
        ops.ensemble_probs([torch.zeros(1, 300, 2, 2, device=device)] * 2, "nms", 257)
    with pytest.raises(ValueError, match="map 1"):
        ops.ensemble_probs([z, z[:, :, :3].contiguous()], "nms")
    with pytest.raises(TypeError):
        ops.ensemble_probs([z.double(), z.double()], "nms")
    wide = torch.randn(1, 300, 2, 2, device=device)
    prob, lab = ops.ensemble_probs([wide, wide], "nms", 256)  # the largest n_used: labels up to 255 fit the byte
    assert np.array_equal(lab.cpu().numpy(), R.labels_of(wide.cpu().numpy(), 256))


@pytest.mark.parametrize("method", R.METHODS)
def test_offset_outputs_take_the_scalar_path(method, device):
    """through the C ABI, where the outputs' bases can be chosen: ``out`` 4 bytes off the 16-byte grid, then ``labels`` 1 byte off it,
    with every map aligned and W % 4 == 0 -- each alone sends the call to the one-pixel path, and the bits are those of the 16-byte path"""
    import ctypes
    import mcdseg
    L = mcdseg.lib()
    k, n, c, h, w = 3, 2, 5, 8, 12
    maps, want = oracle("nan", k, n, c, h, w, method)
    dev = [torch.from_numpy(m).to(device) for m in maps]
    assert all(t.data_ptr() % 16 == 0 for t in dev)
    host = (ctypes.c_void_p * k)(*[t.data_ptr() for t in dev])
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    numel, pixels = n * c * h * w, n * h * w
    for out_off, lab_off in ((0, 0), (4, 0), (0, 1), (4, 3)):
        out_buf = torch.full((numel + 8,), 7.0, dtype=torch.float32, device=device)
        lab_buf = torch.full((pixels + 8,), 99, dtype=torch.uint8, device=device)
        assert out_buf.data_ptr() % 16 == 0 and lab_buf.data_ptr() % 16 == 0
        rc = L.mcdseg_ensemble_probs(ctypes.cast(host, ctypes.c_void_p), k, 0 if method == "averaging" else 1,
                                     ctypes.c_void_p(out_buf.data_ptr() + out_off), ctypes.c_void_p(lab_buf.data_ptr() + lab_off), c - 1, n, c, h, w,
                                     stream)
        assert rc == 0, L.mcdseg_last_error()
        torch.cuda.synchronize()
        o, b = out_off // 4, lab_off
        got, lab = out_buf.cpu().numpy(), lab_buf.cpu().numpy()
        assert R.bits(got[o:o + numel]).tobytes() == R.bits(want).tobytes(), (out_off, lab_off)
        assert np.array_equal(lab[b:b + pixels].reshape(n, h, w), R.labels_of(want, c - 1)), (out_off, lab_off)
        assert (got[:o] == 7.0).all() and (got[o + numel:] == 7.0).all() and (lab[:b] == 99).all() and (lab[b + pixels:] == 99).all()


# ------------------------------------------------------------------------------------------------ label_resize_colorize
RESIZES = [((h, w), (w, h)) for h, w in ((1, 1), (5, 3), (16, 32))]                       # identity
RESIZES += [((a, b), (pb, pa)) for (a, pa), (b, pb) in zip(NAIVE_FAILS, NAIVE_FAILS[::-1])]  # both axes at ratios the naive rule gets wrong
RESIZES += [((3, 5), (13, 7)), ((7, 9), (4, 3)), ((16, 32), (1280, 720))]                  # (H, W) -> (OW, OH): up, down, and to the reference's test size


@pytest.mark.parametrize("n_pal", (2, 20, 256))
def test_label_resize_colorize(n_pal, device):
    from mcdseg import ops
    rng = np.random.RandomState(n_pal)
    pal = rng.randint(0, 256, size=(n_pal, 3)).astype(np.uint8)
    pal_dev = torch.from_numpy(pal).to(device)
    for (h, w), wh in RESIZES:
        lab = rng.randint(0, 256, size=(3, h, w)).astype(np.uint8)
        if h * w >= 256:
            lab[0].reshape(-1)[:256] = np.arange(256)  # every label 0..255 is there
        lab_dev = torch.from_numpy(lab).to(device)
        out, vis = ops.label_resize_colorize(lab_dev, wh, pal_dev)
        assert out.dtype == torch.uint8 and vis.dtype == torch.uint8 and tuple(out.shape) == (3, wh[1], wh[0]) and tuple(vis.shape) == (3, wh[1], wh[0], 3)
        out, vis = out.cpu().numpy(), vis.cpu().numpy()
        for i in range(3):
            assert np.array_equal(out[i], R.resize_nearest(lab[i], wh)), ((h, w), wh, i)
            # the reference's order: colour at the map's size, then resize the RGB image
            assert np.array_equal(vis[i], R.resize_nearest(R.colorize(lab[i], pal), wh)), ((h, w), wh, i)
        if n_pal < 256:
            assert (vis[out >= n_pal] == 0).all() and ((out >= n_pal).any() or h * w < 256)
        only_lab, none = ops.label_resize_colorize(lab_dev, wh, None, want_vis=False)
        assert none is None and np.array_equal(only_lab.cpu().numpy(), out)
        none, only_vis = ops.label_resize_colorize(lab_dev, wh, pal_dev, want_labels=False)
        assert none is None and np.array_equal(only_vis.cpu().numpy(), vis)
    with pytest.raises(ValueError):
        ops.label_resize_colorize(lab_dev, wh, pal_dev, want_labels=False, want_vis=False)
    with pytest.raises(TypeError):
        ops.label_resize_colorize(lab_dev, wh, torch.zeros(257, 3, dtype=torch.uint8, device=device))
    with pytest.raises(ValueError):
        ops.label_resize_colorize(lab_dev, (0, 4), pal_dev)


def test_naive_rule_would_fail_here():
    """the sizes of RESIZES taken from NAIVE_FAILS do tell the two rules apart (no device needed, but it belongs to the cases above)"""
    for n_in, n_out in NAIVE_FAILS:
        naive = np.floor((np.arange(n_out) + 0.5) * n_in / n_out).astype(np.int64)
        assert not np.array_equal(R.nearest_indices_pillow(n_in, n_out), naive), (n_in, n_out)


# ------------------------------------------------------------------------------------------------ the memory contract
def test_memory_contract(device):
    """stock / 0xFF / 0x00 (tests/guards_hold.hold, 64 KiB guard bands): both ops keep inside their outputs and the workspace, and no
    result depends on what those held before -- on the 16-byte path, on the scalar path (ragged W), and with ``out`` NULL"""
    from guards_hold import hold
    from mcdseg import ops
    for method in R.METHODS:
        for k, n, c, h, w in ((3, 2, 5, 7, 9), (2, 3, 20, 16, 32)):
            maps, want = oracle("nan", k, n, c, h, w, method)

            def combine(put):
                dev = [put(torch.from_numpy(m)) for m in maps]
                prob, lab = ops.ensemble_probs(dev, method, c - 1)
                _, lab_alone = ops.ensemble_probs(dev, method, c - 1, want_prob=False)
                return dict(prob=prob, labels=lab, labels_alone=lab_alone)
            ref = hold(device, combine, family="ensemble_probs %s %dx%dx%dx%dx%d" % (method, k, n, c, h, w))
            assert R.bits(ref["prob"].cpu().numpy()).tobytes() == R.bits(want).tobytes() and torch.equal(ref["labels"], ref["labels_alone"])
    rng = np.random.RandomState(11)
    lab = rng.randint(0, 30, size=(2, 7, 9)).astype(np.uint8)
    pal = R.voc_palette(20)

    def colour(put):
        lab_dev, pal_dev = put(torch.from_numpy(lab)), put(torch.from_numpy(pal))
        out, vis = ops.label_resize_colorize(lab_dev, (13, 5), pal_dev)
        only, _ = ops.label_resize_colorize(lab_dev, (13, 5), None, want_vis=False)
        _, only_vis = ops.label_resize_colorize(lab_dev, (13, 5), pal_dev, want_labels=False)
        return dict(labels=out, vis=vis, labels_alone=only, vis_alone=only_vis)
    ref = hold(device, colour, workspace=True, family="label_resize_colorize")
    assert torch.equal(ref["labels"], ref["labels_alone"]) and torch.equal(ref["vis"], ref["vis_alone"])


# ------------------------------------------------------------------------------------------------ the tool, end to end
def _tool():
    spec = importlib.util.spec_from_file_location("ensemble_tool", os.path.join(PKG, "tools", "ensemble_predict_from_npy.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


NAMES = ("a", "b", "c", "d")


@pytest.fixture(scope="module")
def members(tmp_path_factory):
    """three member directories of four 5 x 24 x 32 maps each, and ground truth at 36 x 20"""
    root = tmp_path_factory.mktemp("members")
    maps = R.make_maps("random", 3, 4, 5, 24, 32, seed=77)  # [K][4 images, 5, 24, 32]
    dirs = []
    for k in range(3):
        d = str(root / ("m%d" % k) / "prob")
        os.makedirs(d)
        dirs.append(d)
        for i, name in enumerate(NAMES):
            np.save(os.path.join(d, name + ".npy"), maps[k][i])
        with open(os.path.join(d, "notes.txt"), "w") as f:  # not a map: ignored
            f.write("x")
    gt = str(root / "gt")
    os.makedirs(gt)
    rng = np.random.RandomState(5)
    for i, name in enumerate(NAMES):
        truth = R.resize_nearest(R.labels_of(R.combine([maps[k][i] for k in range(3)], "averaging"), 5), (36, 20)).copy()
        truth[rng.random_sample(truth.shape) < 0.1] = 255  # background
        truth[rng.random_sample(truth.shape) < 0.2] = 1
        Image.fromarray(truth).save(os.path.join(gt, name + ".png"))
    return dirs, maps, gt


def _read(fn):
    with open(fn, "rb") as f:
        return f.read()


@pytest.mark.parametrize("method", R.METHODS)
def test_tool_end_to_end(method, members, tmp_path, device):
    dirs, maps, _ = members
    out = str(tmp_path / "out")
    assert _tool().main(["--npydirs"] + dirs + ["--method", method, "-d", out]) == out
    assert sorted(os.listdir(out)) == ["label", "prob", "vis"]
    for i, name in enumerate(NAMES):
        prob, label, vis = R.ensemble_predict([maps[k][i] for k in range(3)], method)
        saved = np.load(os.path.join(out, "prob", name + ".npy"))
        assert saved.dtype == np.float32 and saved.shape == (5, 24, 32) and saved.tobytes() == prob.tobytes()
        png = Image.open(os.path.join(out, "label", name + ".png"))
        assert png.mode == "L" and np.array_equal(np.asarray(png), label) and label.shape == (24, 32)
        png = Image.open(os.path.join(out, "vis", name + ".png"))
        assert png.mode == "RGB" and np.array_equal(np.asarray(png), vis)
        assert (vis != 0).any()
    # -b 3 (a last batch of one), --out_shape, --n_used, --no_prob, a palette file: the same pictures as one at a time
    pal = np.random.RandomState(1).randint(0, 256, size=(3, 3)).astype(np.uint8)
    with open(str(tmp_path / "pal.json"), "w") as f:
        json.dump({"palette": pal.tolist()}, f)
    out2 = str(tmp_path / "out2")
    _tool().main(["--npydirs"] + dirs + ["--method", method, "-d", out2, "-b", "3", "--out_shape", "36", "20", "--n_used", "4", "--no_prob",
                                         "--palette_json", str(tmp_path / "pal.json")])
    assert sorted(os.listdir(out2)) == ["label", "vis"]
    for i, name in enumerate(NAMES):
        _, label, vis = R.ensemble_predict([maps[k][i] for k in range(3)], method, 4, (36, 20), pal)
        assert np.array_equal(np.asarray(Image.open(os.path.join(out2, "label", name + ".png"))), label) and label.shape == (20, 36)
        assert np.array_equal(np.asarray(Image.open(os.path.join(out2, "vis", name + ".png"))), vis)
        assert label.max() == 3 and (vis[label == 3] == 0).all()  # a label beyond the three colours is black


def test_tool_mode_and_evaluation(members, tmp_path, device):
    import eval as E
    dirs, maps, gt = members
    out = str(tmp_path / "out")
    _tool().main(["--npydirs"] + dirs + ["-d", out, "--out_shape", "36", "20", "--gt_dir", gt, "--n_class", "5", "-b", "3", "--no_prob"])
    with open(os.path.join(out, "eval_result_ensemble.json")) as f:
        result = json.load(f)
    assert sorted(result) == ["ensemble", "members"] and len(result["members"]) == 3
    # eval.py's numbers on the written PNGs (and, for the members, on what the oracle gives for each member alone)
    truth = np.stack([np.asarray(Image.open(os.path.join(gt, name + ".png"))) for name in NAMES])
    written = np.stack([np.asarray(Image.open(os.path.join(out, "label", name + ".png"))) for name in NAMES])
    preds = [written] + [np.stack([R.resize_nearest(R.labels_of(maps[k][i], 5), (36, 20)) for i in range(4)]) for k in range(3)]
    for pred, got in zip(preds, [result["ensemble"]] + result["members"]):
        meter = E.ConfusionMeter(5, background_id=255, device=device)
        meter.update(torch.from_numpy(pred).to(device), torch.from_numpy(truth).to(device))
        want = json.loads(json.dumps(meter.summary()))
        assert got == want
    assert result["ensemble"]["pixAcc"] < 100.0 and result["ensemble"]["pixAcc"] > max(m["pixAcc"] for m in result["members"])
    # --mode passes the reference's sizes
    out3 = str(tmp_path / "out3")
    _tool().main(["--npydirs"] + dirs[:2] + ["-d", out3, "--mode", "test", "--no_prob", "-b", "4"])
    img = Image.open(os.path.join(out3, "label", "a.png"))
    assert img.size == (1280, 720)
    _, label, vis = R.ensemble_predict([maps[k][0] for k in range(2)], "averaging", None, (1280, 720))
    assert np.array_equal(np.asarray(img), label) and np.array_equal(np.asarray(Image.open(os.path.join(out3, "vis", "a.png"))), vis)


# ------------------------------------------------------------------------------------------------ the testers' --vis
UNET = ["--net", "unet", "--input_ch", "6", "-b", "2", "--train_img_shape", "96", "64", "--synthetic", "--synthetic_len", "4", "--no_tflog",
        "--epochs", "1", "--max_iter", "10"]  # the smallest synthetic case of tests/test_unet_gpu.py::test_trainer_resume_and_tester


def test_tester_vis(tmp_path, device):
    import adapt_tester
    import adapt_trainer
    out = str(tmp_path / "out")
    assert adapt_trainer.main(["suncg", "nyu", "--base_outdir", out] + UNET) == 0
    ck_fn = os.path.join(out, "suncg-train2nyu-train_6ch", "pth", "MCD-normal-unet-1.pth.tar")
    common = ["nyu", ck_fn, "--synthetic", "--synthetic_len", "2", "--test_img_shape", "80", "64"]
    plain_dir = adapt_tester.main(common + ["--outdir", str(tmp_path / "plain")])[0]
    base = os.path.dirname(plain_dir)
    assert not os.path.exists(os.path.join(base, "vis"))
    with open(os.path.join(base, "param.json")) as f:
        assert not {"vis", "palette_json"} & set(json.load(f))
    label_dir = adapt_tester.main(common + ["--outdir", str(tmp_path / "vis"), "--vis"])[0]
    vis_dir = os.path.join(os.path.dirname(label_dir), "vis")
    names = sorted(os.listdir(label_dir))
    assert len(names) == 2 and sorted(os.listdir(vis_dir)) == names == sorted(os.listdir(plain_dir))
    with open(os.path.join(os.path.dirname(label_dir), "param.json")) as f:
        assert json.load(f)["vis"] is True
    n_class = 41  # nyu
    for name in names:
        assert _read(os.path.join(label_dir, name)) == _read(os.path.join(plain_dir, name))
        lab = np.asarray(Image.open(os.path.join(label_dir, name)))
        img = Image.open(os.path.join(vis_dir, name))
        assert img.mode == "P" and img.size == (80, 64) and np.array_equal(np.asarray(img), lab)
        assert np.array_equal(np.asarray(img.convert("RGB")), R.colorize(lab, R.voc_palette(n_class)))  # n_used + 1 = 41 colours


def test_uncertain_tester_vis_with_a_palette_file(tmp_path, device):
    """the source-only testers take the flag through ``source_tester.get_parser``: ``source_uncertain_tester.py --vis --palette_json``
    (the smallest synthetic case of tests/test_uncertain_gpu.py's trainer run)"""
    import source_uncertain_tester
    import source_uncertain_trainer
    out = str(tmp_path / "out")
    flags = ["--synthetic", "--no_pretrained", "-b", "2", "--train_img_shape", "64", "48", "--n_dropout", "3", "--max_iter", "2",
             "--epochs", "1", "--no_tflog", "--synthetic_len", "8"]
    assert source_uncertain_trainer.main(["suncg", "--base_outdir", out] + flags) == 0
    ck_fn = os.path.join(out, "suncg-train_only_3ch_uncertain", "pth", "normal-drn_d_38-1.pth.tar")
    pal = np.random.RandomState(4).randint(0, 256, size=(7, 3)).astype(np.uint8)
    with open(str(tmp_path / "pal.json"), "w") as f:
        json.dump({"palette": pal.tolist()}, f)
    common = ["nyu", ck_fn, "--synthetic", "--synthetic_len", "2", "--test_img_shape", "80", "56"]
    plain_dir = source_uncertain_tester.main(common + ["--outdir", str(tmp_path / "plain")])[0]
    assert not os.path.exists(os.path.join(os.path.dirname(plain_dir), "vis"))
    with open(os.path.join(os.path.dirname(plain_dir), "param.json")) as f:
        assert not {"vis", "palette_json"} & set(json.load(f))
    label_dir = source_uncertain_tester.main(common + ["--outdir", str(tmp_path / "vis"), "--vis", "--palette_json", str(tmp_path / "pal.json")])[0]
    vis_dir = os.path.join(os.path.dirname(label_dir), "vis")
    names = sorted(os.listdir(label_dir))
    assert len(names) == 2 and sorted(os.listdir(vis_dir)) == names
    for name in names:
        assert _read(os.path.join(label_dir, name)) == _read(os.path.join(plain_dir, name))
        lab = np.asarray(Image.open(os.path.join(label_dir, name)))
        img = Image.open(os.path.join(vis_dir, name))
        assert img.mode == "P" and img.size == (80, 56) and np.array_equal(np.asarray(img), lab)
        assert np.array_equal(np.asarray(img.convert("RGB")), R.colorize(lab, pal))  # a label beyond the seven colours is black
