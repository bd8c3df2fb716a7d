"""CPU: the edge-map oracle (tests/edge_ref.py) against hand-derived cases, the C-ABI exports and the library's refusals (none of which
reaches a launch), the refusals of ``ops`` and of tools/edge_detect.py on the host, and the coverage the GPU test's inputs must have."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

import edge_ref as R
from conftest import PKG, ROOT

NEW = ("mcdseg_edge_maps", "mcdseg_canny_hysteresis_workspace_bytes", "mcdseg_canny_hysteresis")


def _tool():
    spec = importlib.util.spec_from_file_location("edge_detect_tool", os.path.join(PKG, "tools", "edge_detect.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------ the oracle, by hand
def test_luma_by_hand():
    rgb = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [254, 255, 253], [0, 0, 0], [255, 255, 255]], dtype=np.uint8)
    assert R.luma(rgb).tolist() == [76, 150, 29, 254, 0, 255]
    g = np.arange(256, dtype=np.uint8)
    assert np.array_equal(R.luma(R.grey(g)), g)  # a grey pixel maps to itself: 4899 + 9617 + 1868 = 2^14


def _step():
    y = np.zeros((5, 6), dtype=np.uint8)
    y[:, 3:] = 255
    return y


def test_vertical_step_by_hand():
    """columns 3..5 are 255: the second difference is +255 left of the step and -255 right of it; dx = 4 * 255 on both sides of it and 0
    at the borders (REFLECT_101 mirrors about the border pixel, so the difference of the two mirrored columns vanishes); of the two
    equal magnitudes the LEFT one survives: `mag > left && mag >= right`"""
    m = R.edge_maps(R.grey(_step()), 100, 200)
    assert np.array_equal(m["luma"], _step())
    for row in range(5):
        assert m["laplacian"][row].tolist() == [128, 128, 255, 0, 128, 128]
        assert m["sobel"][row].tolist() == [0, 0, 255, 255, 0, 0]
        assert m["canny_cls"][row].tolist() == [0, 0, 2, 0, 0, 0]
        assert m["canny"][row].tolist() == [0, 0, 255, 0, 0, 0]
    t = R.edge_maps(R.grey(_step().T.copy()), 100, 200)  # the transpose: `mag > upper && mag >= lower` keeps the upper row
    assert np.array_equal(t["laplacian"], m["laplacian"].T) and np.array_equal(t["sobel"], m["sobel"].T)
    assert np.array_equal(t["canny"], m["canny"].T) and (t["canny"][2] == 255).all() and (t["canny"][[0, 1, 3, 4, 5]] == 0).all()


def test_thresholds_by_hand():
    """the step's magnitude is 1020: strong below a high of 1020, weak (and so no edge: nothing strong to hang on) at or above it, gone
    at a low of 1020; low and high swap when given in the wrong order"""
    rgb = R.grey(_step())
    assert (R.edge_maps(rgb, 100, 1019)["canny_cls"][:, 2] == 2).all()
    weak = R.edge_maps(rgb, 100, 1020)
    assert (weak["canny_cls"][:, 2] == 1).all() and (weak["canny"] == 0).all()
    assert (R.edge_maps(rgb, 1019, 2000)["canny_cls"][:, 2] == 1).all()
    assert (R.edge_maps(rgb, 1020, 2000)["canny_cls"] == 0).all()
    for lo, hi in ((100, 200), (6, 100), (100, 1020), (0, 0)):
        a, b = R.edge_maps(rgb, lo, hi), R.edge_maps(rgb, hi, lo)
        assert all(np.array_equal(a[k], b[k]) for k in R.KINDS), (lo, hi)


MAIN_DIAGONAL = ["01000000", "01100000", "00110000", "00011000", "00001100", "00000110", "00000011", "00000000"]


def test_diagonal_steps_by_hand():
    """255 above the main diagonal: dx > 0 > dy there, so s = -1 and a band pixel is compared with its upper-right and lower-left
    neighbours, which lie OFF the two-pixel band (magnitude 510 against 1530): the whole band stays.  With the other s the neighbours
    would be band pixels of equal magnitude and both strict comparisons would fail.  The mirrored image has dx, dy > 0 and s = +1."""
    yy, xx = np.mgrid[0:8, 0:8]
    want = np.array([[int(c) for c in row] for row in MAIN_DIAGONAL], dtype=np.uint8) * 255
    main = np.where(xx > yy, 255, 0).astype(np.uint8)
    got = R.edge_maps(R.grey(main), 100, 200)
    assert np.array_equal(got["canny"], want)
    dx, dy = R.gradients(main, "nearest")
    assert ((dx ^ dy)[want == 255] < 0).all()
    anti = main[::-1].copy()  # 255 where x + y > 7
    assert np.array_equal(anti, np.where(xx + yy > 7, 255, 0))
    got = R.edge_maps(R.grey(anti), 100, 200)
    assert np.array_equal(got["canny"], want[::-1])
    dx, dy = R.gradients(anti, "nearest")
    assert ((dx ^ dy)[want[::-1] == 255] >= 0).all()
    _, branch = R.canny_branches(main, 100, 200)
    assert (branch[want == 255] == 2).all() and branch[0, 0] == 0 and branch[7, 7] == 1


def test_border_rules_by_hand():
    """one bright pixel in a corner: REFLECT_101 sees it mirrored about the border (so the Sobel gradient at the corner vanishes),
    REPLICATE sees it repeated (so Canny's does not), and magnitudes outside the image are 0, not those of replicated pixels"""
    y = np.zeros((4, 4), dtype=np.uint8)
    y[0, 0] = 200
    m = R.edge_maps(R.grey(y), 100, 200)
    assert m["sobel"][0, 0] == 0 and m["laplacian"][0, 0] == 0 and m["laplacian"][0, 1] == 255  # -4 * 200 + 128; 200 + 128
    dx, dy = R.gradients(y, "nearest")
    assert (dx[0, 0], dy[0, 0]) == (-600, -600) and m["canny_cls"][0, 0] == 2  # a maximum only because off-image magnitudes are 0
    one = R.edge_maps(R.grey(np.full((1, 1), 77, dtype=np.uint8)))
    assert [int(one[k][0, 0]) for k in R.KINDS] == [77, 128, 0, 0, 0]


def test_sobel_root_is_exact():
    s = np.arange(0, 2 * 1020 * 1020 + 1, dtype=np.int64)
    r = R.isqrt(s)
    assert (r * r <= s).all() and ((r + 1) * (r + 1) > s).all()
    assert np.array_equal(r, np.floor(np.sqrt(s.astype(np.float32))).astype(np.int64))  # fp32 is exact over the whole range too


def test_hysteresis_by_hand():
    cls = np.array([[1, 0, 0, 1, 1], [0, 1, 0, 0, 0], [0, 0, 2, 0, 3], [0, 0, 0, 0, 255], [1, 1, 0, 0, 1]], dtype=np.uint8)
    want = np.array([[1, 0, 0, 0, 0], [0, 1, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]], dtype=np.uint8) * 255
    assert np.array_equal(R.hysteresis(cls), want)  # joined diagonally; 3 and 255 are no candidates; weak-only components vanish
    m, last = R.serpentine(7, 5)
    assert last == (6, 0) and m.sum() == 4 * 5 + 3 and R.components(m)[1] == 1
    assert (R.hysteresis(m) == 0).all()
    m[last] = 2
    assert np.array_equal(R.hysteresis(m), np.where(m > 0, 255, 0))


# ------------------------------------------------------------------------------------------------ what the GPU cases must hold
@pytest.mark.parametrize("shape", ((33, 65), (64, 96)), ids=lambda s: "%dx%d" % s)
def test_smooth_inputs_cover_the_cases(shape):
    """every "smooth" image the GPU test compares at (100, 200) holds a weak-only component (which vanishes), a kept component with weak
    pixels in it (which the hysteresis, not the threshold, keeps) and pixels decided by each branch of the non-maximum suppression"""
    rgb = R.make_rgb("smooth", R.BATCH, shape[0], shape[1], seed=0)
    for k in range(R.BATCH):
        c = R.coverage(rgb[k], 100, 200)
        assert c["weak_only"] >= 1 and c["kept_with_weak"] >= 1 and min(c["branches"]) >= 1, (shape, k, c)
        assert c["kept"] + c["weak_only"] == c["components"] and c["edges"] > c["strong"] >= c["kept"]


def test_tie_inputs_hold_ties():
    for content in ("blocks", "alphabet"):
        rgb = R.make_rgb(content, 1, 33, 65, seed=0)[0]
        dx, dy = R.gradients(R.luma(rgb), "nearest")
        mag = np.abs(dx) + np.abs(dy)
        assert (mag == 0).any() and ((mag[:, 1:] == mag[:, :-1]) & (mag[:, 1:] > 0)).any(), content


# ------------------------------------------------------------------------------------------------ the C ABI
def test_exports_and_declarations():
    import mcdseg
    from mcdseg import _lib
    mcdseg.build()
    with open(os.path.join(ROOT, "include", "mcdseg.h")) as f:
        header = f.read()
    L = mcdseg.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.EXPORTS and hasattr(L, name), name
    block = header[header.index("Edge maps of RGB images"):header.index("int mcdseg_edge_maps")]
    flat = " ".join(block.replace("*", " ").split())
    for cite in ("tools/edge_detect.py:33-53", "sample_scripts/refine_seg_by_boundary.sh:6", "section 4.15", "neither claimed nor tested",
                 "BORDER_REFLECT_101", "BORDER_REPLICATE", "13573"):
        assert cite in flat, cite
    assert "edge.hip" in _lib.NO_PACKED_F32 and os.path.exists(os.path.join(_lib.CSRC, "edge.hip"))
    for name in ("edge.hip", "refine.hip"):
        with open(os.path.join(_lib.CSRC, name)) as f:
            text = f.read()
        assert '#include "union_find.h"' in text and "rf_union_lds(int" not in text, name  # shared, not copied


def test_workspace_bytes():
    import mcdseg
    mcdseg.build()
    L = mcdseg.lib()
    assert L.mcdseg_canny_hysteresis_workspace_bytes(3, 64, 96) == 4 * 3 * 64 * 96
    assert L.mcdseg_canny_hysteresis_workspace_bytes(16, 480, 640) == 4 * 16 * 480 * 640
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, -1)):
        assert L.mcdseg_canny_hysteresis_workspace_bytes(*bad) == 0


def test_library_refuses_before_launching():
    """every refusal is -EINVAL from the argument checks: none of these calls reaches a launch, so they need no device"""
    import mcdseg
    mcdseg.build()
    L = mcdseg.lib()
    fake, other = ctypes.c_void_p(4096), ctypes.c_void_p(8192)  # never dereferenced: each call below is refused first

    def maps(rgb=fake, luma=None, lap=fake, sob=None, cls=None, n=1, h=4, w=4):
        return L.mcdseg_edge_maps(rgb, luma, lap, sob, cls, 100, 200, n, h, w, None)
    for kw, word in ((dict(rgb=None), "null rgb"), (dict(lap=None), "no output"), (dict(h=0), "dims"), (dict(w=-3), "dims"), (dict(n=0), "dims"),
                     (dict(n=65536), "65535"), (dict(n=40000, h=400, w=400), "32 bits")):
        assert maps(**kw) == -22, kw
        assert word in L.mcdseg_last_error().decode(), (kw, L.mcdseg_last_error())

    def hyst(cls=fake, edges=other, n=1, h=4, w=4, ws=fake, nbytes=64):
        return L.mcdseg_canny_hysteresis(cls, edges, n, h, w, ws, ctypes.c_size_t(nbytes), None)
    for kw, word in ((dict(cls=None), "null"), (dict(edges=None), "null"), (dict(edges=fake), "must not be cls"), (dict(h=0), "dims"),
                     (dict(n=-1), "dims"), (dict(ws=None), "null workspace"), (dict(ws=ctypes.c_void_p(4098)), "aligned"),
                     (dict(nbytes=63), "too small"), (dict(nbytes=0), "too small")):
        assert hyst(**kw) == -22, kw
        assert word in L.mcdseg_last_error().decode(), (kw, L.mcdseg_last_error())


# ------------------------------------------------------------------------------------------------ ops and the tool on the host
def test_ops_refuse_on_the_host():
    import torch
    from mcdseg import ops
    rgb = torch.zeros(1, 4, 4, 3, dtype=torch.uint8)
    assert ops.EDGE_KINDS == R.KINDS
    with pytest.raises(ValueError):
        ops.edge_maps(rgb, want=("laplacian", "prewitt"))
    with pytest.raises(ValueError):
        ops.edge_maps(rgb, want=())
    with pytest.raises(TypeError):
        ops.edge_maps(rgb.float())
    with pytest.raises(TypeError):
        ops.edge_maps(rgb.numpy())
    for shape in ((4, 4, 3), (1, 4, 4, 4), (1, 3, 4, 4), (0, 4, 4, 3)):
        with pytest.raises(ValueError):
            ops.edge_maps(torch.zeros(shape, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.edge_maps(rgb)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.canny_hysteresis(torch.zeros(1, 4, 4, dtype=torch.uint8))


def test_parser_takes_the_reference_flags():
    tool = _tool()
    a = tool.get_parser().parse_args(["rgb"])
    assert (a.rgbdir, a.min_canny_thre, a.max_canny_thre, a.kinds, a.outdir, a.batch_size, a.refine) == ("rgb", 100, 200,
                                                                                                          ["laplacian", "canny", "sobel"], None, 8, None)
    assert (a.thre, a.min_thre, a.max_thre, a.gt_dir, a.n_class) == (50, 500, 79333, None, None)
    assert tool.check_args(a) == ("laplacian", "canny", "sobel")
    a = tool.get_parser().parse_args(["rgb", "--min_canny_thre", "6", "--max_canny_thre", "100", "--kinds", "sobel", "canny", "-b", "2",
                                      "--refine", "seg", "--gt_dir", "gt", "--n_class", "14", "--outdir", "o"])
    assert (a.min_canny_thre, a.max_canny_thre, a.batch_size, a.refine, a.gt_dir, a.n_class, a.outdir) == (6, 100, 2, "seg", "gt", 14, "o")
    assert tool.check_args(a) == ("canny", "sobel")
    assert "CV_64F" in tool.__doc__ and "--min_canny_thre 6 --max_canny_thre 100" in tool.__doc__  # the reference's threshold slip


def test_tool_refusals_before_any_device_work(tmp_path):
    tool = _tool()
    rgb = str(tmp_path / "rgb")
    os.makedirs(rgb)
    with pytest.raises(SystemExit, match="batch_size"):
        tool.main([rgb, "-b", "0"])
    with pytest.raises(SystemExit, match="--gt_dir needs --n_class"):
        tool.main([rgb, "--refine", str(tmp_path / "seg"), "--gt_dir", str(tmp_path)])
    with pytest.raises(SystemExit, match="--gt_dir needs --refine"):
        tool.main([rgb, "--gt_dir", str(tmp_path), "--n_class", "14"])
    with pytest.raises(SystemExit, match="unknown kind prewitt"):
        tool.main([rgb, "--kinds", "canny", "prewitt"])
    assert not os.path.exists(str(tmp_path / "edges"))


def test_read_rgb(tmp_path):
    from PIL import Image
    import edge_detect
    rng = np.random.RandomState(2)
    arr = rng.randint(0, 256, size=(5, 7, 3)).astype(np.uint8)
    Image.fromarray(arr).save(str(tmp_path / "a.png"))
    assert np.array_equal(edge_detect.read_rgb(str(tmp_path / "a.png")), arr)
    Image.fromarray(arr[..., 0]).save(str(tmp_path / "g.png"))  # a grey file decodes to three equal channels, as cv2.imread's
    assert np.array_equal(edge_detect.read_rgb(str(tmp_path / "g.png")), R.grey(arr[..., 0]))
    Image.fromarray((rng.randint(0, 65536, size=(5, 7))).astype(np.uint16)).save(str(tmp_path / "d.png"))
    with pytest.raises(ValueError, match="deeper than 8 bits"):
        edge_detect.read_rgb(str(tmp_path / "d.png"))
    with pytest.raises(ValueError):
        edge_detect.check_kinds(("canny", "prewitt"))
    assert edge_detect.check_kinds(("sobel", "laplacian")) == ("laplacian", "sobel")
    paths = []
    for k, shape in enumerate(((4, 6), (4, 6), (4, 6), (5, 6), (4, 6))):
        paths.append(str(tmp_path / ("b%d.png" % k)))
        Image.fromarray(rng.randint(0, 256, size=shape + (3,)).astype(np.uint8)).save(paths[-1])
    got = [(stems, batch.shape) for stems, batch in edge_detect.batches(paths, 2)]
    assert got == [(["b0", "b1"], (2, 4, 6, 3)), (["b2"], (1, 4, 6, 3)), (["b3"], (1, 5, 6, 3)), (["b4"], (1, 4, 6, 3))]
