"""CPU: the oracle of the colorization depth inpainting (tests/fill_ref.py) held to its own honesty conditions
on every scene tests/test_fill_depth_gpu.py uses, and the contract outside the kernels: the C ABI's declarations and refusals, the
Python op's refusals, the pipeline's method, the tools' parsers and their exit without a GPU.  No kernel is launched here.

Measured here (numpy/scipy, fp64): iterations 16 ... 120, ||M^-1 1||_inf 2.7 ... 1.3e3, ||x - x*||_inf between 0.01 and 0.7 of its bound."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import fill_ref as R
from conftest import PKG, ROOT

ALL = [(name, k) for name in R.CASES for k in range(len(R.case(name)[1]))]
NAMES = ("mcdseg_fill_depth_workspace_bytes", "mcdseg_fill_depth_setup", "mcdseg_fill_depth_iterate", "mcdseg_fill_depth_finish")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(PKG, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_scenes_are_what_their_names_say():
    for name in R.CASES:
        rgb, depth = R.case(name)
        assert rgb.dtype == np.uint8 and depth.dtype == np.float32 and rgb.shape == depth.shape + (3,), name
    known = lambda name, k=0: R.known_mask(R.case(name)[1][k])  # noqa: E731
    assert R.case("clipped_8x12")[1].shape == (1, 8, 12) and 0.3 < 1 - known("clipped_8x12").mean() < 0.5
    assert R.case("odd_37x53")[1].shape == (1, 37, 53) and not known("odd_37x53")[:, :4].any()
    assert R.case("two_48x64")[1].shape == (2, 48, 64) and R.truth("two_48x64", 0)["zmax"] != R.truth("two_48x64", 1)["zmax"]
    assert R.case("holes_96x128")[1].shape == (1, 96, 128)
    assert known("one_known_16x16").sum() == 1
    assert len(np.unique(R.case("flat_gray_16x16")[0])) == 1
    w = R.truth("flat_gray_16x16", 0)["weights"]
    assert set(np.unique(w)) == {0.0, 1 / 3, 0.2, 0.125}  # variance 0: the 2e-6 floor, uniform weights over 3, 5 or 8 neighbours
    isl = R.luma(R.case("island_32x32")[0][0])
    assert not known("island_32x32")[12:20, 12:20].any() and known("island_32x32").sum() == 32 * 32 - 64
    assert isl[12:20, 12:20].min() > 0.9 and isl[0, 0] < 0.1
    w = R.truth("island_32x32", 0)["weights"]
    assert 0 < w[w > 0].min() < 1e-7  # what crosses the luma edge
    assert R.case("row_1x40")[1].shape == (1, 1, 40)
    assert not known("missing_beside_valid", 0).any() and known("missing_beside_valid", 1).any()
    assert R.truth("missing_beside_valid", 0)["zmax"] == 0.0 and R.truth("missing_beside_valid", 0)["x_star"] is None


@pytest.mark.parametrize("name,k", ALL)
def test_system_is_the_m_matrix_the_bound_rests_on(name, k):
    t = R.truth(name, k)
    M, D = t["M"], t["D"]
    rgb, depth = R.case(name)
    n = M.shape[0]
    off = (M - sp.diags(M.diagonal())).tocsr()
    off.eliminate_zeros()
    assert off.nnz and off.data.max() < 0  # every off-diagonal entry is a weight, negated; none is zero (counted below)
    assert np.array_equal(M.diagonal(), D)
    alpha_k = np.where(R.known_mask(depth[k]).reshape(-1), 1.0, 0.0)
    rows = np.asarray(M.sum(axis=1)).reshape(-1)
    assert np.abs(rows - alpha_k).max() <= 4 * np.finfo(np.float64).eps, (name, np.abs(rows - alpha_k).max())  # 4 ulp of alpha k = 1
    w = t["weights"]
    inside = R.weights(rgb[k])[1]
    assert (w[inside] > 0).all() and not w[~inside].any() and np.isfinite(w).all()
    assert w[inside].min() >= np.exp(-30.0) / 8 * 0.99  # the exponent never goes below -30
    assert np.abs(w.sum(0) - 1).max() <= 4 * np.finfo(np.float64).eps
    assert off.nnz == inside.sum() and n == depth[k].size


@pytest.mark.parametrize("name,k", [(n, k) for n, k in ALL if R.truth(n, k)["zmax"] > 0])
def test_oracle_is_honest(name, k):
    """the direct solve leaves a residual of rounding size; the statement's own iteration converges well inside the limit and obeys
    the error bound the GPU test asserts of the device.  A scene the reference iteration cannot solve is replaced, not tolerated."""
    t = R.truth(name, k)
    M, b = t["M"], t["b"]
    r_star = b - M @ t["x_star"]
    bn = np.linalg.norm(b)
    assert np.linalg.norm(r_star) <= 1e-13 * bn
    x, status, its, res = t["it"]
    assert status == R.CONVERGED and 0 < its <= 4000 // 4 and its % 8 == 0 and res <= 1e-10
    r = b - M @ x
    assert np.linalg.norm(r) <= 1e-10 * bn
    err, bound = np.abs(x - t["x_star"]).max(), t["minv"] * (np.abs(r).max() + np.abs(r_star).max())
    print("%s[%d]: %d iterations, |M^-1 1| = %.3g, |x - x*| = %.3g of the allowed %.3g" % (name, k, its, t["minv"], err, bound))
    assert err <= bound
    assert (t["x_star"] > 0).all() and t["x_star"].max() <= 1 + 1e-12  # M^-1 >= 0 and the maximum principle: a fill is inside (0, zmax]


def test_two_48x64_counts_differ_by_a_check_interval():
    a, b = R.truth("two_48x64", 0)["it"][2], R.truth("two_48x64", 1)["it"][2]
    assert abs(a - b) >= 8, (a, b)  # what exercises the freeze of a finished image beside a running one


def test_statuses_of_the_statement():
    rgb, depth = R.case("holes_96x128")
    out = R.fill(rgb[0], depth[0], max_iter=8)
    assert out["status"] == R.NOT_CONVERGED and out["iterations"] == 8 and np.isfinite(out["filled"]).all()
    out = R.fill(rgb[0], np.zeros_like(depth[0]))
    assert out["status"] == R.EMPTY and not out["filled"].any()
    keep = R.fill(rgb[0], depth[0], keep_known=True)
    k = R.known_mask(depth[0])
    assert np.array_equal(keep["filled"][k], depth[0][k]) and (keep["filled"][~k] > 0).all()
    # max_valid_cm: the clipped pixels become missing ones
    far = float(np.sort(depth[0][k])[-50])
    m = R.system(rgb[0], depth[0], max_valid_cm=far)
    z = np.where(depth[0] < far, depth[0], 0)
    m0 = R.system(rgb[0], z)
    assert m[3] == m0[3] < far and np.array_equal(m[1], m0[1]) and (m[0] != m0[0]).nnz == 0


def test_exports_declarations_and_refusals():
    import mcdseg
    from mcdseg import _lib, ops
    mcdseg.build()
    with open(os.path.join(ROOT, "include", "mcdseg.h")) as f:
        header = f.read()
    L = mcdseg.lib()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.EXPORTS and hasattr(L, name), name
    for k, name in enumerate(("RUNNING", "CONVERGED", "EMPTY", "NOT_CONVERGED", "BREAKDOWN")):
        assert re.search(r"#define MCDSEG_FILL_%s %d\b" % (name, k), header) and getattr(ops, "FILL_" + name) == k == getattr(R, name)
        assert ops.FILL_STATUS_NAMES[k] == name.lower()
    assert L.mcdseg_version() == 101
    assert "fill.hip" in _lib.NO_PACKED_F32 and os.path.exists(os.path.join(_lib.CSRC, "fill.hip"))
    with open(os.path.join(_lib.CSRC, "block_reduce.h")) as f:
        assert "fill.hip" in f.read()

    size = L.mcdseg_fill_depth_workspace_bytes
    pad = lambda b: (b + 255) // 256 * 256  # noqa: E731
    tiles = lambda h, w: -(-h // 8) * -(-w // 32)  # noqa: E731
    want = lambda n, h, w: pad(88 * n) + pad(16 * n * tiles(h, w)) + pad(4 * n * h * w) + pad(64 * n * h * w) + 8 * pad(8 * n * h * w)  # noqa: E731
    for dims in ((1, 8, 12), (2, 37, 53), (16, 480, 640), (1, 1, 2), (1, 4096, 4096)):
        assert size(*dims) == want(*dims), dims
    assert size(1, 480, 640) < 133 * 480 * 640  # "about 128 B per pixel": 8 weights + 8 vectors in fp64, and the known depth in fp32
    for dims in ((0, 4, 4), (1, 0, 4), (1, 4, -1), (65536, 2, 1), (1, 5000, 5000), (1, 1, 1)):
        assert size(*dims) == 0, dims

    p = ctypes.c_void_p(4096)  # never read: every refusal is answered before anything is launched (there is no GPU here to launch on)
    big = 1 << 40

    def refused(call, why, **kw):
        a = dict(rgb=p, depth=p, alpha=1.0, max_valid=0.0, n=1, h=4, w=4, ws=p, ws_bytes=big, n_iter=8, rtol=1e-10, status=p, filled=p,
                 x=p, weights=p, zmax=p)
        a.update(kw)
        if call == "setup":
            rc = L.mcdseg_fill_depth_setup(a["rgb"], a["depth"], a["alpha"], a["max_valid"], a["n"], a["h"], a["w"], a["ws"], a["ws_bytes"], None)
        elif call == "iterate":
            rc = L.mcdseg_fill_depth_iterate(a["n_iter"], a["rtol"], a["n"], a["h"], a["w"], a["ws"], a["ws_bytes"], a["status"], None)
        else:
            rc = L.mcdseg_fill_depth_finish(a["n"], a["h"], a["w"], a["ws"], a["ws_bytes"], a["filled"], a["x"], a["weights"], a["zmax"], 0, None)
        msg = L.mcdseg_last_error().decode()
        assert rc == -22 and msg.startswith("fill_depth_%s:" % call) and why in msg, (call, why, rc, msg)

    need = size(1, 4, 4)
    for call in ("setup", "iterate", "finish"):
        refused(call, "null pointer", ws=None)
        refused(call, "bad dims", n=0)
        refused(call, "bad dims", h=0)
        refused(call, "bad dims", w=-3)
        refused(call, "at most 65535", n=65536, h=2, w=1)
        refused(call, "too large", h=5000, w=5000)  # H*W > 2^24
        refused(call, "too small", h=1, w=1)        # H*W < 2
        refused(call, "workspace too small", ws_bytes=need - 1)
        refused(call, "16-byte aligned", ws=ctypes.c_void_p(4096 + 8), ws_bytes=need)
    refused("setup", "null pointer", rgb=None)
    refused("setup", "null pointer", depth=None)
    refused("iterate", "null pointer", status=None)
    refused("finish", "null pointer", filled=None)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused("setup", "alpha must be positive and finite", alpha=bad)
        refused("iterate", "rtol must be positive and finite", rtol=bad)
    refused("setup", "max_valid_cm", max_valid=-1.0)
    refused("setup", "max_valid_cm", max_valid=float("nan"))
    refused("setup", "4-byte aligned", depth=ctypes.c_void_p(4098))
    refused("iterate", "n_iter", n_iter=-1)
    refused("iterate", "8-byte aligned", status=ctypes.c_void_p(4100))
    refused("finish", "4-byte aligned", filled=ctypes.c_void_p(4097))
    refused("finish", "8-byte aligned", x=ctypes.c_void_p(4100))
    # the optional outputs may be NULL: with them null and everything else in order the next refusal is the workspace's
    refused("finish", "workspace too small", x=None, weights=None, zmax=None, ws_bytes=0)


def test_op_refuses_the_cpu_and_bad_arguments():
    from mcdseg import ops
    rgb = torch.zeros(1, 4, 4, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.fill_depth(rgb, torch.ones(1, 4, 4))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.fill_depth(rgb, torch.ones(1, 4, 4, dtype=torch.int32), unit_m=0.001)
    for bad in (torch.ones(4, 4), torch.ones(1, 1, 4, 4), torch.ones(0, 4, 4), np.ones((1, 4, 4), np.float32)):
        with pytest.raises(TypeError, match=r"fill_depth takes a non-empty depth batch \[N,H,W\]"):
            ops.fill_depth(rgb, bad)
    with pytest.raises(TypeError, match="uint16, int32 or fp32"):
        ops.fill_depth(rgb, torch.ones(1, 4, 4, dtype=torch.float64))
    # ... the conversion is depth_to_hha's own code, which still names itself
    with pytest.raises(TypeError, match=r"depth_to_hha takes a non-empty depth batch \[N,H,W\]"):
        ops.depth_to_hha(torch.ones(4, 4), (1, 1, 1, 1))


def test_pipeline_method_composes_the_two_ops(monkeypatch):
    import datasets
    from mcdseg import ops
    seen = []
    monkeypatch.setattr(ops, "depth_to_hha", lambda depth, camera, unit_m=None, return_parts=False: seen.append(("hha", depth, camera, unit_m)) or "the part")
    monkeypatch.setattr(ops, "fill_depth", lambda rgb, depth, unit_m=None, **kw: seen.append(("fill", rgb, depth, unit_m, kw)) or "filled")
    pipe = datasets.DeviceInputPipeline(6, 41, torch.device("cpu"))
    d, rgb = torch.ones(1, 4, 4, dtype=torch.int32), torch.zeros(1, 4, 4, 3, dtype=torch.uint8)
    assert pipe.hha(d, (1, 2, 3, 4), 0.001) == "the part"
    assert len(seen) == 1 and seen[0][0] == "hha" and seen[0][1] is d and seen[0][3] == 0.001  # without fill_rgb: today's call
    del seen[:]
    assert pipe.hha(d, (1, 2, 3, 4), 0.001, fill_rgb=rgb, rtol=1e-8, keep_known=True) == "the part"
    assert [s[0] for s in seen] == ["fill", "hha"]
    assert seen[0][1] is rgb and seen[0][2] is d and seen[0][3] == 0.001 and seen[0][4] == dict(rtol=1e-8, keep_known=True)
    assert seen[1][1] == "filled" and seen[1][2] == (1, 2, 3, 4) and seen[1][3] is None  # the filled batch is centimetres
    with pytest.raises(TypeError, match="without fill_rgb"):
        pipe.hha(d, (1, 2, 3, 4), rtol=1e-8)
    with pytest.raises(TypeError, match="HHA part alone"):
        pipe.hha(d, (1, 2, 3, 4), fill_rgb=rgb, return_parts=True)


def test_tool_parsers_and_their_refusals(tmp_path):
    tool = _tool("fill_depth")
    a = tool.get_parser().parse_args(["depth", "rgb", "out"])
    assert (a.depth_dir, a.rgb_dir, a.out_dir, a.unit_m, a.alpha, a.rtol, a.max_iter, a.max_valid_m, a.keep_known, a.batch_size) == \
        ("depth", "rgb", "out", 0.001, 1.0, 1e-10, 4000, None, False, 1)
    a = tool.get_parser().parse_args(["d", "r", "o", "--unit_m", "0.0002", "--alpha", "2", "--rtol", "1e-8", "--max_iter", "50",
                                      "--max_valid_m", "10", "--keep_known", "-b", "16"])
    assert tool.solver_kwargs(a) == dict(alpha=2.0, rtol=1e-8, max_iter=50, keep_known=True, max_valid_cm=1000.0)
    assert (a.unit_m, a.batch_size) == (0.0002, 16)
    with pytest.raises(SystemExit):
        tool.get_parser().parse_args(["depth", "out"])  # the RGB directory is required
    for bad, why in ((["-b", "0"], "batch_size"), (["--unit_m", "0"], "unit_m"), (["--alpha", "0"], "alpha"), (["--rtol", "-1"], "rtol"),
                     (["--max_valid_m", "0"], "max_valid_m")):
        with pytest.raises(SystemExit, match=why):
            tool.main(["d", "r", "o"] + bad)
    # floor(cm / (100 unit_m) + 0.5), clipped
    cm = np.array([[0.0, 0.04999, 0.05, 123.44, 123.46, 6553.5, 7000.0]], np.float32)
    assert tool.to_units(cm, 0.001).tolist() == [[0, 0, 1, 1234, 1235, 65535, 65535]]
    assert tool.to_units(cm, 0.001).dtype == np.uint16
    from PIL import Image
    Image.fromarray(np.zeros((3, 4, 3), np.uint8)).save(str(tmp_path / "a.jpg"))
    assert tool.read_rgb(str(tmp_path), "a.png", (3, 4)).shape == (3, 4, 3)
    with pytest.raises(ValueError, match="its depth map"):
        tool.read_rgb(str(tmp_path), "a.png", (4, 4))
    with pytest.raises(FileNotFoundError):
        tool.read_rgb(str(tmp_path), "b.png", (3, 4))

    hha = _tool("depth_to_hha")
    a = hha.get_parser().parse_args(["depth", "out", "--camera", "1", "2", "3", "4"])
    assert a.fill is None and (a.alpha, a.rtol, a.max_iter, a.max_valid_m, a.keep_known) == (1.0, 1e-10, 4000, None, False)
    a = hha.get_parser().parse_args(["depth", "out", "--camera", "1", "2", "3", "4", "--fill", "rgb", "--rtol", "1e-9"])
    assert a.fill == "rgb" and a.rtol == 1e-9
    with pytest.raises(SystemExit, match="alpha"):
        hha.main(["depth", "out", "--camera", "1", "2", "3", "4", "--fill", "rgb", "--alpha", "-1"])


def test_tools_without_a_gpu_are_a_system_exit(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="MI355X"):
        _tool("fill_depth").main([str(tmp_path), str(tmp_path), str(tmp_path / "out")])
    with pytest.raises(SystemExit, match="MI355X"):
        _tool("depth_to_hha").main([str(tmp_path), str(tmp_path / "out"), "--camera", "500", "500", "320", "240", "--fill", str(tmp_path)])
    assert not os.path.exists(str(tmp_path / "out"))
