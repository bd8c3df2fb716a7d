"""GPU: the edge-map kernels (csrc/edge.hip: luma, Laplacian, Sobel and Canny's classes in one launch; Canny's hysteresis by union-find)
against the numpy / scipy oracle of the definition (tests/edge_ref.py), and tools/edge_detect.py end to end.  Everything is integer: exact
equality throughout."""
import importlib.util
import itertools
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import edge_ref as R
from conftest import PKG
from guards_hold import hold

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    """{(content, shape): (rgb [3,H,W,3], {thresholds: {kind: [3,H,W]}})} by the oracle, computed once"""
    out = {}
    for content in R.CONTENTS:
        for shape in R.SHAPES:
            rgb = R.make_rgb(content, R.BATCH, shape[0], shape[1], seed=0)
            out[(content, shape)] = (rgb, {t: R.edge_maps(rgb, *t) for t in R.THRESHOLDS})
    return out


def _maps(rgb, device, low, high, want=R.KINDS):
    from mcdseg import ops
    got = ops.edge_maps(torch.from_numpy(rgb).to(device), low, high, want)
    return {k: v.cpu().numpy() for k, v in got.items()}


def _hyst(cls, device):
    from mcdseg import ops
    cls = cls if cls.ndim == 3 else cls[None]
    return ops.canny_hysteresis(torch.from_numpy(np.ascontiguousarray(cls)).to(device)).cpu().numpy()


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d" % s)
def test_all_maps_equal_the_oracle(ref, device, shape):
    for content in R.CONTENTS:
        rgb, want = ref[(content, shape)]
        for t in R.THRESHOLDS:
            got = _maps(rgb, device, *t)
            assert tuple(got) == R.KINDS
            for kind in R.KINDS:
                assert got[kind].dtype == np.uint8 and got[kind].shape == (R.BATCH,) + shape
                assert np.array_equal(got[kind], want[t][kind]), (content, shape, t, kind, int((got[kind] != want[t][kind]).sum()),
                                                                  np.argwhere(got[kind] != want[t][kind])[:4].tolist())


def test_swapped_thresholds_and_what_the_inputs_hold(ref):
    for content in R.CONTENTS:
        _, want = ref[(content, (64, 96))]
        assert all(np.array_equal(want[(100, 200)][k], want[(200, 100)][k]) for k in R.KINDS)
    _, want = ref[("smooth", (64, 96))]
    edges, cls = want[(100, 200)]["canny"], want[(100, 200)]["canny_cls"]
    assert (edges[cls == 2] == 255).all() and ((cls == 1) & (edges == 0)).any() and ((cls == 1) & (edges == 255)).any()
    assert set(np.unique(want[(0, 0)]["canny_cls"])) <= {0, 2}  # high = 0: whatever is kept is strong


def test_every_subset_of_outputs_gives_the_same_bits(ref, device):
    rgb, want = ref[("smooth", (33, 65))]
    full = want[(100, 200)]
    for r in range(1, len(R.KINDS) + 1):
        for subset in itertools.combinations(R.KINDS, r):
            got = _maps(rgb, device, 100, 200, subset)
            assert tuple(got) == subset
            for kind in subset:
                assert np.array_equal(got[kind], full[kind]), (subset, kind)
    got = _maps(rgb, device, 100, 200, ("canny", "luma"))  # the order of `want` does not matter; a single name may be a string
    assert tuple(got) == ("luma", "canny") and np.array_equal(got["canny"], full["canny"])
    assert np.array_equal(_maps(rgb, device, 100, 200, "sobel")["sobel"], full["sobel"])


def test_strided_input_is_made_dense(ref, device):
    from mcdseg import ops
    rgb, want = ref[("alphabet", (31, 33))]
    wide = torch.zeros((R.BATCH, 31, 40, 3), dtype=torch.uint8, device=device)
    wide[:, :, :33] = torch.from_numpy(rgb).to(device)
    got = ops.edge_maps(wide[:, :, :33], 6, 100)
    assert tuple(got) == ("laplacian", "sobel", "canny")
    for kind in got:
        assert np.array_equal(got[kind].cpu().numpy(), want[(6, 100)][kind]), kind


# ------------------------------------------------------------------------------------------------ the hysteresis alone
def _kept(cls):
    return np.where((cls == 1) | (cls == 2), 255, 0).astype(np.uint8)


def test_serpentine_through_every_tile(device):
    m, last = R.serpentine(70, 70)
    assert last == (68, 69) and R.components(m)[1] == 1  # row 2k is walked to the right for even k, to the left for odd k
    assert (_hyst(m, device) == 0).all()  # no strong pixel anywhere
    s = m.copy()
    s[last] = 2
    got = _hyst(s, device)[0]
    assert np.array_equal(got, _kept(s)) and np.array_equal(got, R.hysteresis(s))
    broken = s.copy()  # 3 and 255 are not candidates: the path is cut twice, only the stretch with the strong pixel stays
    broken[34, 20], broken[60, 50] = 3, 255
    got = _hyst(broken, device)[0]
    assert np.array_equal(got, R.hysteresis(broken))
    assert got[34, 20] == 0 and got[60, 50] == 0 and got[0, 0] == 0 and got[40, 5] == 0 and got[68, 5] == 255 and got[62, 5] == 255
    both = _hyst(np.stack([s, m]), device)  # two images of different content: the second holds nothing strong
    assert np.array_equal(both[0], _kept(s)) and (both[1] == 0).all()
    both = _hyst(np.stack([m, s]), device)
    assert (both[0] == 0).all() and np.array_equal(both[1], _kept(s))


@pytest.mark.parametrize("anti", (False, True), ids=("diagonal", "antidiagonal"))
def test_chains_that_meet_only_at_a_tile_corner(device, anti):
    from scipy import ndimage
    m = np.zeros((70, 70), dtype=np.uint8)
    if anti:
        m[31, 32:] = 1  # ends at (31, 32), in the upper right tile
        m[32, :32] = 1  # ends at (32, 31), in the lower left tile
    else:
        m[31, :32] = 1  # ends at (31, 31), in the upper left tile
        m[32, 32:] = 1  # ends at (32, 32), in the lower right tile
    assert ndimage.label(m)[1] == 2 and R.components(m)[1] == 1  # two chains 4-wise, one component 8-wise
    assert (_hyst(m, device) == 0).all()
    for strong in ((31, 69) if anti else (31, 0), (32, 0) if anti else (32, 69)):
        s = m.copy()
        s[strong] = 2
        assert np.array_equal(_hyst(s, device)[0], _kept(m)), strong


def test_weak_checkerboard_with_one_strong_pixel(device):
    yy, xx = np.mgrid[0:70, 0:70]
    m = ((yy + xx) % 2 == 0).astype(np.uint8)
    assert (_hyst(m, device) == 0).all()
    m[69, 69] = 2
    assert np.array_equal(_hyst(m, device)[0], _kept(m))
    m[:, 40] = 0  # a gap of one column: the left part is cut off from the strong pixel
    got = _hyst(m, device)[0]
    assert np.array_equal(got, R.hysteresis(m)) and (got[:, :40] == 0).all() and np.array_equal(got[:, 41:], _kept(m)[:, 41:])


def test_random_class_maps(device):
    rng = np.random.RandomState(5)
    for shape, p in (((1, 1), 0.5), ((2, 2), 0.5), ((33, 65), 0.35), ((70, 130), 0.4), ((70, 130), 0.25)):
        cls = (rng.rand(3, *shape) < p).astype(np.uint8)
        cls[(rng.rand(3, *shape) < 0.01) & (cls == 1)] = 2
        cls[rng.rand(3, *shape) < 0.02] = 200
        got = _hyst(cls, device)
        for k in range(3):
            assert np.array_equal(got[k], R.hysteresis(cls[k])), (shape, p, k)


def test_two_runs_are_bitwise_equal(ref, device):
    rgb, _ = ref[("smooth", (64, 96))]
    a, b = _maps(rgb, device, 100, 200), _maps(rgb, device, 100, 200)
    assert all(np.array_equal(a[k], b[k]) for k in R.KINDS)


def test_memory_contract(ref, device):
    from mcdseg import ops
    rgb, want = ref[("smooth", (33, 65))]
    m, last = R.serpentine(70, 70)
    m[last] = 2

    def work(put):
        out = ops.edge_maps(put(torch.from_numpy(rgb)), 100, 200, R.KINDS)
        out["canny_alone"] = ops.edge_maps(put(torch.from_numpy(rgb)), 100, 200, ("canny",))["canny"]
        out["hysteresis"] = ops.canny_hysteresis(put(torch.from_numpy(m[None])))
        return out
    got = hold(device, work, workspace=True, family="edge_maps + canny_hysteresis")
    for kind in R.KINDS:
        assert np.array_equal(got[kind].cpu().numpy(), want[(100, 200)][kind]), kind
    assert torch.equal(got["canny_alone"], got["canny"]) and np.array_equal(got["hysteresis"][0].cpu().numpy(), _kept(m))


def test_bad_calls_are_refused_and_launch_nothing(device):
    import ctypes
    import mcdseg
    L = mcdseg.lib()
    n, h, w = 1, 33, 65
    cls = torch.full((n, h, w), 2, dtype=torch.uint8, device=device)
    edges = torch.full((n, h, w), 99, dtype=torch.uint8, device=device)
    need = L.mcdseg_canny_hysteresis_workspace_bytes(n, h, w)
    assert need == 4 * n * h * w
    ws = torch.empty(need // 4, dtype=torch.int32, device=device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.mcdseg_canny_hysteresis(p(cls), p(edges), n, h, w, p(ws), need - 1, st) == -22
    assert L.mcdseg_canny_hysteresis(p(cls), p(cls), n, h, w, p(ws), need, st) == -22
    assert L.mcdseg_canny_hysteresis(p(cls), p(edges), n, h, w, None, need, st) == -22
    assert L.mcdseg_edge_maps(p(cls), None, None, None, None, 1, 2, n, h, w // 3, st) == -22
    torch.cuda.synchronize()
    assert (edges == 99).all()
    assert L.mcdseg_canny_hysteresis(p(cls), p(edges), n, h, w, p(ws), need, st) == 0
    torch.cuda.synchronize()
    assert (edges == 255).all()


# ------------------------------------------------------------------------------------------------ the tool, end to end
def _load(name):
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(PKG, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _png(path):
    return np.array(Image.open(path))


def _files(d):
    out = {}
    for name in sorted(os.listdir(d)):
        with open(os.path.join(d, name), "rb") as f:
            out[name] = f.read()
    return out


def test_tool_end_to_end(tmp_path, device):
    rng = np.random.RandomState(8)
    sizes = {"a": (64, 96), "b": (64, 96), "c": (64, 96), "d": (33, 65)}
    rgb = {stem: R.make_rgb("smooth", 1, s[0], s[1], seed=40 + k)[0] for k, (stem, s) in enumerate(sizes.items())}
    for sub in ("rgb", "label", "gt"):
        os.makedirs(str(tmp_path / sub))
    for stem, s in sizes.items():
        Image.fromarray(rgb[stem]).save(str(tmp_path / "rgb" / (stem + ".png")))
        seg = np.kron(rng.randint(0, 5, size=((s[0] + 3) // 4, (s[1] + 3) // 4)), np.ones((4, 4), dtype=np.int64))[:s[0], :s[1]].astype(np.uint8)
        Image.fromarray(seg).save(str(tmp_path / "label" / (stem + ".png")))
        Image.fromarray(np.where(rng.rand(*s) < 0.1, 255, seg).astype(np.uint8)).save(str(tmp_path / "gt" / (stem + ".png")))
    tool = _load("edge_detect")
    refine = ["--thre", "50", "--min_thre", "6", "--max_thre", "2500"]
    edge_dir = tool.main([str(tmp_path / "rgb"), "-b", "2", "--refine", str(tmp_path / "label"), "--gt_dir", str(tmp_path / "gt"), "--n_class",
                          "5"] + refine)
    assert edge_dir == str(tmp_path / "edges") and sorted(os.listdir(edge_dir)) == ["canny", "laplacian", "sobel"]
    for stem in sizes:
        want = R.edge_maps(rgb[stem], 100, 200)
        for kind in ("laplacian", "canny", "sobel"):
            assert np.array_equal(_png(os.path.join(edge_dir, kind, stem + ".png")), want[kind]), (stem, kind)
    mine = _files(str(tmp_path / "refined_label"))
    with open(str(tmp_path / "eval_result_refined.json")) as f:
        mine_json = json.load(f)
    assert sorted(mine) == sorted(stem + ".png" for stem in sizes)
    assert any(not np.array_equal(_png(str(tmp_path / "refined_label" / n)), _png(str(tmp_path / "label" / n))) for n in mine)  # it refined
    os.remove(str(tmp_path / "eval_result_refined.json"))
    for n in mine:
        os.remove(str(tmp_path / "refined_label" / n))
    _load("refine_seg_by_boundary").main([str(tmp_path / "label"), os.path.join(edge_dir, "canny"), "--gt_dir", str(tmp_path / "gt"), "--n_class",
                                          "5", "-b", "3"] + refine)
    assert _files(str(tmp_path / "refined_label")) == mine
    with open(str(tmp_path / "eval_result_refined.json")) as f:
        assert json.load(f) == mine_json
    assert sorted(mine_json) == ["after", "before"]

    # other thresholds, a subset of kinds, another directory; no refinement: nothing else is written
    out = tool.main([str(tmp_path / "rgb"), "--min_canny_thre", "6", "--max_canny_thre", "100", "--kinds", "canny", "--outdir", str(tmp_path / "e2")])
    assert out == str(tmp_path / "e2") and os.listdir(out) == ["canny"]
    for stem in sizes:
        assert np.array_equal(_png(os.path.join(out, "canny", stem + ".png")), R.edge_maps(rgb[stem], 6, 100)["canny"]), stem


def test_tool_names_the_label_image_of_another_size(tmp_path, device):
    for sub in ("rgb", "label"):
        os.makedirs(str(tmp_path / sub))
    Image.fromarray(np.zeros((8, 9, 3), np.uint8)).save(str(tmp_path / "rgb" / "a.png"))
    Image.fromarray(np.zeros((9, 8), np.uint8)).save(str(tmp_path / "label" / "a.png"))
    with pytest.raises(ValueError, match=r"label.a\.png is 8 x 9"):
        _load("edge_detect").main([str(tmp_path / "rgb"), "--refine", str(tmp_path / "label")])
