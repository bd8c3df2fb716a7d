"""CPU: the ensembling oracle (tests/ensemble_ref.py) against hand-worked cases, the default palette, the tool's parser and refusals,
the C-ABI exports, and Pillow's NEAREST rule against the index rule the library shares (csrc/nearest_index.h, restated in
oracle/ref_io.nearest_index)."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest

import ensemble_ref as R
from conftest import GOLDEN, PKG, ROOT
from oracle import ref_io

F = np.float32
# (in, out) at which floor((x + 0.5) * in / out) is NOT Pillow's NEAREST index somewhere along the axis (Pillow adds in/out step by step)
NAIVE_FAILS = ((2, 7), (4, 6), (8, 6), (14, 5))


def _tool():
    spec = importlib.util.spec_from_file_location("ensemble_tool", os.path.join(PKG, "tools", "ensemble_predict_from_npy.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------ the oracle, by hand
def test_oracle_averaging_by_hand():
    nz = np.array([-0.0], dtype=F)
    mean = R.combine([nz, nz], "averaging")
    assert mean.dtype == F and R.bits(mean)[0] == 0x00000000          # 0 + -0.0 is +0.0: Python's sum starts from the integer 0
    assert R.bits(R.combine([nz, nz], "nms"))[0] == 0x80000000         # the maximum of two -0.0 is -0.0
    a, b, c = (np.array([v], dtype=F) for v in (1e8, -1e8, 1.0))       # (a + b) + c = 1, a + (b + c) = 0 in fp32
    assert F(1e8) + (F(-1e8) + F(1.0)) == 0.0 and (F(1e8) + F(-1e8)) + F(1.0) == 1.0
    assert R.combine([a, b, c], "averaging")[0] == F(1.0) / F(3.0)     # left to right, then ONE division
    assert R.combine([b, c, a], "averaging")[0] == 0.0
    x = np.array([1.0], dtype=F)                                       # x / 3 is not x * (1/3) in fp32: 1/3 rounds up, times 3 values
    third = F(1.0) / F(3.0)
    vals = np.array([5.0, 7.0, 1e-3, 2.5e10], dtype=F)
    assert (vals / F(3.0) != vals * third).any()
    assert R.combine([x, x, x], "averaging")[0] == F(3.0) / F(3.0)


def test_oracle_nan_ties_and_zeros_by_hand():
    nan = np.nan
    p0 = np.array([[[1.0, nan, 0.0, -0.0]], [[2.0, 5.0, -0.0, 0.0]], [[2.0, nan, 0.0, 0.0]]], dtype=F)  # [C=3, H=1, W=4]
    assert R.labels_of(p0, 3).tolist() == [[1, 0, 0, 0]]              # first of ties; the first NaN wins; +0 == -0
    assert R.labels_of(p0, 2).tolist() == [[1, 0, 0, 0]]
    assert R.labels_of(p0, 1).tolist() == [[0, 0, 0, 0]]
    a = np.array([nan, 1.0, 0.0, -0.0], dtype=F)
    b = np.array([2.0, nan, -0.0, 0.0], dtype=F)
    m = R.combine([a, b], "nms")
    assert np.isnan(m[:2]).all()                                       # a NaN in any map wins
    assert R.bits(m)[2:].tolist() == [0x80000000, 0x00000000]          # of +0 and -0 the later map's stays
    assert np.isnan(R.combine([a, b], "averaging")[:2]).all()
    inf = np.array([np.inf], dtype=F)
    made = R.combine([inf, -inf], "averaging")                         # inf - inf: a NaN the addition MAKES; its bits are the host's
    assert np.isnan(made[0]) and R.bits(R.canon(made))[0] == 0x7FC00000
    assert R.bits(R.canon(np.array([1.5, nan], dtype=F))).tolist() == [0x3FC00000, 0x7FC00000]


def test_oracle_colorize_and_resize_commute():
    """NEAREST of the palette image and the palette of the NEAREST label are the same picture (what lets the device do one gather)"""
    rng = np.random.RandomState(3)
    lab = rng.randint(0, 24, size=(9, 7)).astype(np.uint8)
    pal = R.voc_palette(20)
    assert (R.colorize(lab, pal)[lab >= 20] == 0).all() and (lab >= 20).any()
    for wh in ((7, 9), (4, 3), (13, 17), (6, 5)):
        assert np.array_equal(R.resize_nearest(R.colorize(lab, pal), wh), R.colorize(R.resize_nearest(lab, wh), pal)), wh


def test_oracle_reproduces_the_fixture():
    """tests/golden/ensemble_small.npz is the ORACLE's output (make_ensemble_golden.py says why not the reference's): numpy and Pillow
    still compute what they computed when it was written"""
    fx = np.load(os.path.join(GOLDEN, "ensemble_small.npz"))
    maps = [fx["p%d" % k] for k in range(3)]
    assert maps[0].shape == (20, 12, 16) and int(fx["n_used"]) == 19
    for method in R.METHODS:
        prob, label, vis = R.ensemble_predict(maps, method, int(fx["n_used"]), tuple(fx["out_wh"]))
        assert R.bits(prob).tobytes() == R.bits(fx["prob_" + method]).tobytes()
        assert np.array_equal(label, fx["label_" + method]) and np.array_equal(vis, fx["vis_" + method])
        assert label.shape == (17, 21) and vis.shape == (17, 21, 3)
    assert R.bits(fx["prob_averaging"])[3, 5, 7] == 0 and R.bits(fx["prob_nms"])[3, 5, 7] == 0x80000000


# ------------------------------------------------------------------------------------------------ the palette
def test_default_palette():
    import ensemble
    assert [tuple(c) for c in ensemble.default_palette(21).tolist()] == list(R.VOC21)
    pal = ensemble.default_palette(256)
    assert pal.dtype == np.uint8 and pal.shape == (256, 3)
    assert [tuple(c) for c in pal.tolist()] == [R.voc_colour(label) for label in range(256)]
    assert len({tuple(c) for c in pal.tolist()}) == 256
    assert np.array_equal(ensemble.default_palette(20), pal[:20])
    for bad in (0, 257):
        with pytest.raises(ValueError):
            ensemble.default_palette(bad)


def test_palette_json(tmp_path):
    import ensemble
    fn = str(tmp_path / "info.json")
    with open(fn, "w") as f:
        json.dump({"palette": [[1, 2, 3], [255, 0, 9]], "classes": ["a", "b"]}, f)
    assert ensemble.load_palette(fn).tolist() == [[1, 2, 3], [255, 0, 9]] and ensemble.load_palette(fn).dtype == np.uint8
    with open(fn, "w") as f:
        json.dump({"palette": [[1, 2, 300]]}, f)
    with pytest.raises(ValueError):
        ensemble.load_palette(fn)


def test_save_colorized_lbl(tmp_path):
    from PIL import Image
    import util
    lab = np.arange(256, dtype=np.uint8).reshape(16, 16)  # labels far beyond the five colours keep their index (and are black)
    fn = str(tmp_path / "v.png")
    util.save_colorized_lbl(Image.fromarray(lab), fn, R.voc_palette(5))
    img = Image.open(fn)
    assert img.mode == "P" and np.array_equal(np.asarray(img), lab)
    assert np.array_equal(np.asarray(img.convert("RGB")), R.colorize(lab, R.voc_palette(5)))  # beyond the palette: black


# ------------------------------------------------------------------------------------------------ the tool's parser and refusals
def test_parser_takes_the_reference_flags():
    tool = _tool()
    a = tool.get_parser().parse_args(["--npydirs", "a", "b", "c", "--method", "nms", "-d", "out", "--mode", "valid"])
    assert (a.npydirs, a.method, a.out_directory, a.mode) == (["a", "b", "c"], "nms", "out", "valid")
    assert tool.check_args(a) == (2048, 1024)
    a = tool.get_parser().parse_args(["--npydirs", "a", "b"])
    assert (a.method, a.out_directory, a.mode, a.n_used, a.out_shape, a.no_prob, a.batch_size) == ("averaging", "ensemble_results", None, None,
                                                                                                   None, False, 1)
    assert tool.check_args(a) is None  # neither --mode nor --out_shape: the maps' size
    assert tool.check_args(tool.get_parser().parse_args(["--npydirs", "a", "b", "--mode", "test"])) == (1280, 720)
    a = tool.get_parser().parse_args(["--npydirs", "a", "b", "--out_shape", "36", "20", "--n_used", "19", "--no_prob", "-b", "3",
                                      "--palette_json", "p.json", "--gt_dir", "g", "--n_class", "20"])
    assert tool.check_args(a) == (36, 20) and (a.n_used, a.no_prob, a.batch_size, a.palette_json, a.gt_dir, a.n_class) == (19, True, 3, "p.json",
                                                                                                                           "g", 20)
    with pytest.raises(SystemExit):
        tool.get_parser().parse_args(["--npydirs", "a", "b", "--method", "median"])


def test_refusals_before_any_device_work(tmp_path):
    tool = _tool()
    dirs = [str(tmp_path / d) for d in ("m0", "m1", "m2")]
    for d in dirs:
        os.makedirs(d)
        for name in ("x", "y"):
            np.save(os.path.join(d, name + ".npy"), np.zeros((5, 4, 6), dtype=F))
    with pytest.raises(SystemExit, match="at least two"):
        tool.main(["--npydirs", dirs[0]])
    with pytest.raises(SystemExit, match="--gt_dir needs --n_class"):
        tool.main(["--npydirs"] + dirs + ["--gt_dir", str(tmp_path)])
    with pytest.raises(SystemExit, match="1..256"):
        tool.main(["--npydirs"] + dirs + ["--n_used", "257"])
    with pytest.raises(SystemExit, match="1..256"):
        tool.main(["--npydirs"] + dirs + ["--n_used", "0"])
    with pytest.raises(SystemExit):
        tool.main(["--npydirs"] + dirs + ["-b", "0"])
    assert tool.list_names(dirs) == ["x", "y"]
    assert [m.shape for m in tool.load_member_maps(dirs, "x", 5)] == [(5, 4, 6)] * 3
    with pytest.raises(ValueError, match="--n_used 6 exceeds the 5 classes"):
        tool.load_member_maps(dirs, "x", 6)
    np.save(os.path.join(dirs[2], "y.npy"), np.zeros((5, 4, 7), dtype=F))
    with pytest.raises(ValueError, match=re.escape(os.path.join(dirs[2], "y.npy"))):
        tool.load_member_maps(dirs, "y")
    os.remove(os.path.join(dirs[1], "y.npy"))
    with pytest.raises(FileNotFoundError, match=re.escape(os.path.join(dirs[1], "y.npy"))):
        tool.main(["--npydirs"] + dirs + ["-d", str(tmp_path / "out")])  # before the device is asked for
    assert not os.path.exists(str(tmp_path / "out"))


def test_ops_refuse_on_the_host():
    import torch
    from mcdseg import ops
    z = torch.zeros(3, 2, 2)
    with pytest.raises(ValueError):
        ops.ensemble_probs([z], "averaging")
    with pytest.raises(ValueError):
        ops.ensemble_probs([z] * 17, "averaging")
    with pytest.raises(ValueError):
        ops.ensemble_probs([z, z], "median")
    with pytest.raises(TypeError):
        ops.ensemble_probs(z, "averaging")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ensemble_probs([z, z], "averaging")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.label_resize_colorize(torch.zeros(1, 2, 2, dtype=torch.uint8), (4, 4), torch.zeros(2, 3, dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------ the C ABI
def test_exports_and_declarations():
    import mcdseg
    from mcdseg import _lib
    mcdseg.build()
    with open(os.path.join(ROOT, "include", "mcdseg.h")) as f:
        header = f.read()
    L = mcdseg.lib()
    for name in ("mcdseg_ensemble_probs", "mcdseg_label_resize_colorize_workspace_bytes", "mcdseg_label_resize_colorize"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.EXPORTS and hasattr(L, name), name
    block = header[header.index("Ensembling of saved predictions"):header.index("int mcdseg_ensemble_probs")]
    flat = " ".join(block.replace("*", " ").split())
    for cite in ("tools/ensemble_predict_from_npy.py:17-56", "section 4.14", "2 <= K <= MCDSEG_ENSEMBLE_MAX_K", "#define MCDSEG_ENSEMBLE_MAX_K 16",
                 "no [K,C,H,W] copy", "0x7FC00000", "transform.py:155-165", "mcdseg_resize_nearest_u8"):
        assert cite in flat, cite
    from mcdseg import ops
    assert ops.ENSEMBLE_MAX_K == 16 and ops.ENSEMBLE_METHODS == {"averaging": 0, "nms": 1}
    assert "ensemble.hip" in _lib.NO_PACKED_F32 and os.path.exists(os.path.join(_lib.CSRC, "ensemble.hip"))
    assert L.mcdseg_label_resize_colorize_workspace_bytes(720, 1280) == 4 * 2000
    assert L.mcdseg_label_resize_colorize_workspace_bytes(0, 5) == 0


def test_library_refuses_before_launching():
    """every refusal is -EINVAL from the argument checks: none of these calls reaches a launch, so they need no device"""
    import ctypes
    import mcdseg
    mcdseg.build()
    L = mcdseg.lib()
    fake = ctypes.c_void_p(4096)  # never dereferenced: each call below is refused first
    maps = (ctypes.c_void_p * 17)(*([4096] * 17))
    mp = ctypes.cast(maps, ctypes.c_void_p)

    def probs(k=2, method=0, n_used=3, n=1, c=3, h=4, w=4, m=mp, labels=fake):
        return L.mcdseg_ensemble_probs(m, k, method, None, labels, n_used, n, c, h, w, None)
    for kw, word in ((dict(k=1), "K = 1"), (dict(k=17), "K = 17"), (dict(method=2), "method"), (dict(n_used=0), "n_used"),
                     (dict(n_used=4), "n_used"), (dict(c=300, n_used=257), "n_used"), (dict(h=0), "dims"), (dict(n=65536), "dims"),
                     (dict(m=None), "null"), (dict(labels=None), "null")):
        assert probs(**kw) == -22, kw
        assert word in L.mcdseg_last_error().decode(), (kw, L.mcdseg_last_error())
    holes = (ctypes.c_void_p * 3)(4096, None, 4096)
    assert probs(k=3, m=ctypes.cast(holes, ctypes.c_void_p)) == -22 and "map 1 is null" in L.mcdseg_last_error().decode()
    odd = (ctypes.c_void_p * 2)(4096, 4098)
    assert probs(m=ctypes.cast(odd, ctypes.c_void_p)) == -22 and "aligned" in L.mcdseg_last_error().decode()

    def colorize(pal=fake, n_pal=20, lab=fake, out=fake, vis=fake, n=1, h=4, w=4, oh=4, ow=4, ws=fake, nbytes=32):
        return L.mcdseg_label_resize_colorize(lab, pal, n_pal, out, vis, n, h, w, oh, ow, ws, ctypes.c_size_t(nbytes), None)
    for kw in (dict(lab=None), dict(ws=None), dict(out=None, vis=None), dict(pal=None), dict(n_pal=0), dict(n_pal=257), dict(oh=0), dict(w=0),
               dict(nbytes=31), dict(ws=ctypes.c_void_p(4098))):
        assert colorize(**kw) == -22, kw


# ------------------------------------------------------------------------------------------------ Pillow's NEAREST and the shared rule
def test_pillow_nearest_is_the_shared_index_rule():
    """for every (in, out) in 1..64 x 1..64 Pillow's NEAREST resize of arange(in) is the index sequence of the library's rule
    (nearest_index_kernel, restated in oracle/ref_io.nearest_index); the naive floor((x + 0.5) in / out) is not"""
    naive_wrong = set()
    for n_in in range(1, 65):
        for n_out in range(1, 65):
            pil = R.nearest_indices_pillow(n_in, n_out)
            assert np.array_equal(pil, ref_io.nearest_index(n_in, n_out)), (n_in, n_out)
            naive = np.floor((np.arange(n_out) + 0.5) * n_in / n_out).astype(np.int64)
            if not np.array_equal(pil, naive):
                naive_wrong.add((n_in, n_out))
    assert set(NAIVE_FAILS) <= naive_wrong, sorted(naive_wrong)[:20]
