"""CPU: the boundary refinement contract (DESIGN.md "Refinement by predicted boundaries"; the reference's
sample_scripts/refine_seg_by_boundary.sh).  The numpy restatement (tests/refine_ref.py) against scipy's labelling where scipy is
installed, against the committed vectors (tests/golden/refine_small.npz) and against hand-written 5 x 5 cases; the flags of the two
testers and of tools/refine_seg_by_boundary.py.  No kernel is launched here."""
import importlib.util
import os

import numpy as np
import pytest

import refine_ref as R
from conftest import PKG


@pytest.fixture(scope="module")
def fx(golden):
    return golden.npz("refine_small.npz")


def _tool():
    spec = importlib.util.spec_from_file_location("refine_seg_by_boundary_tool", os.path.join(PKG, "tools", "refine_seg_by_boundary.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_restatement_equals_the_committed_vectors(fx):
    cases = R.golden_cases()
    assert len(cases) == 13 and sorted(k[2:] for k in fx.files if k.startswith("b_")) == sorted(c[0] for c in cases)
    for name, b, seg, thre, lo, hi in cases:
        assert np.array_equal(fx["b_" + name], b) and np.array_equal(fx["s_" + name], seg), name
        assert list(fx["p_" + name]) == [thre, lo, hi]
        reg = R.regions(b, thre)
        assert reg.dtype == np.int32 and np.array_equal(reg, fx["r_" + name]), name
        out = R.refine(seg, reg, lo, hi)
        assert out.dtype == np.uint8 and np.array_equal(out, fx["o_" + name]), name
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(R.__file__)), "golden", "refine_small.npz")) < 64 * 1024


def test_vectors_hold_what_they_should(fx):
    changed = {k[2:]: int((fx[k] != fx["s_" + k[2:]]).sum()) for k in fx.files if k.startswith("o_")}
    assert sum(1 for v in changed.values() if v > 0) >= 8  # the refinement does something in most cases ...
    assert changed["zeros"] == 0 and changed["full"] == 0 and changed["checker"] == 0  # ... too large, all frame, frame + single pixels
    assert (fx["r_full"] == -1).all() and (fx["r_zeros"] == 0).all()
    r, b = fx["r_checker_inset"], fx["b_checker_inset"]
    assert len(np.unique(r[b > 0])) == 1 and r[b > 0].min() >= 0
    r, b = fx["r_spiral_130x200"], fx["b_spiral_130x200"]
    assert len(np.unique(r[b == 0])) == 1 and (b == 0).sum() > 5000
    assert any((fx[k] == 255).any() for k in fx.files if k.startswith("s_"))


def _scipy_partition(b, thre):
    """(labels of the 4-connected components of ~m, labels of the 8-connected components of the framed m cropped back, the frame
    object's label) -- the bwboundaries route: objects 8-connected, holes 4-connected, the frame one object"""
    ndimage = pytest.importorskip("scipy.ndimage")
    m = R.mask_of(b, thre)
    holes, _ = ndimage.label(~m, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    framed = np.ones((m.shape[0] + 2, m.shape[1] + 2), bool)
    framed[1:-1, 1:-1] = m
    objects, _ = ndimage.label(framed, structure=np.ones((3, 3), int))
    return holes, objects[1:-1, 1:-1], objects[0, 0]


def _same_partition(reg, b, thre):
    holes, objects, frame = _scipy_partition(b, thre)
    m = R.mask_of(b, thre)
    assert np.array_equal(reg == -1, m & (objects == frame))
    # a key per pixel that is equal exactly for pixels of one scipy component (the frame object apart)
    key = np.where(m, objects.astype(np.int64), -holes.astype(np.int64) - 1)
    rest = reg != -1
    pairs = np.unique(np.stack([reg[rest].astype(np.int64), key[rest]]), axis=1)
    assert len(np.unique(pairs[0])) == pairs.shape[1] == len(np.unique(pairs[1]))  # a bijection between ids and components
    # and the id is the smallest row-major index of its component
    flat = reg.reshape(-1)
    ids = np.unique(flat[flat >= 0])
    first = np.array([np.flatnonzero(flat == i)[0] for i in ids])
    assert np.array_equal(ids, first)


def test_restatement_equals_scipy_labelling_on_the_golden_cases():
    pytest.importorskip("scipy.ndimage")
    for name, b, seg, thre, lo, hi in R.golden_cases():
        _same_partition(R.regions(b, thre), b, thre)


@pytest.mark.parametrize("density", (0.3, 0.5, 0.6))
def test_restatement_equals_scipy_labelling_on_random_masks(density):
    pytest.importorskip("scipy.ndimage")
    for seed, shape in enumerate(((1, 1), (1, 9), (9, 1), (17, 23), (40, 31))):
        b = R.bernoulli(shape[0], shape[1], density, seed=seed)
        _same_partition(R.regions(b, R.THRE), b, R.THRE)


def test_the_mask_is_strictly_above_the_threshold():
    b = np.array([[50, 51, 50], [50, 50, 50], [50, 50, 50]], np.uint8)
    assert np.array_equal(R.regions(b, 50), [[0, -1, 0], [0, 0, 0], [0, 0, 0]])
    assert (R.regions(b, 51) == 0).all() and (R.regions(b, 49) == -1).all()


# 5 x 5, hand-written: a ring of mask (X) strictly inside, one hole in the middle
RING = np.array([[0, 0, 0, 0, 0],
                 [0, 9, 9, 9, 0],
                 [0, 9, 0, 9, 0],
                 [0, 9, 9, 9, 0],
                 [0, 0, 0, 0, 0]], np.uint8) * 28  # 252 > 50
RING_REGIONS = np.array([[0, 0, 0, 0, 0],
                         [0, 6, 6, 6, 0],
                         [0, 6, 12, 6, 0],
                         [0, 6, 6, 6, 0],
                         [0, 0, 0, 0, 0]], np.int32)


def test_hand_written_regions():
    assert np.array_equal(R.regions(RING, 50), RING_REGIONS)  # outside 16 pixels, the ring 8 (not on the border: a region), the hole 1
    # two mask pixels touching by a corner are one object; the zeros they separate diagonally are NOT joined
    b = np.array([[0, 0, 0, 0, 0],
                  [0, 0, 0, 0, 0],
                  [0, 0, 0, 255, 0],
                  [0, 0, 255, 0, 255],
                  [0, 0, 0, 255, 0]], np.uint8)
    want = np.array([[0, 0, 0, 0, 0],
                     [0, 0, 0, 0, 0],
                     [0, 0, 0, -1, 0],
                     [0, 0, -1, 18, -1],
                     [0, 0, 0, -1, 24]], np.int32)  # (3,3) and (4,4) touch the other zeros by corners only
    assert np.array_equal(R.regions(b, 50), want)


def test_hand_written_ties_go_to_the_first_occurrence():
    seg = np.array([[7, 7, 7, 3, 3],
                    [3, 9, 2, 2, 0],
                    [0, 9, 5, 2, 0],
                    [0, 2, 9, 9, 0],
                    [0, 0, 0, 0, 0]], np.uint8)
    # outside (16 pixels): 0 x 8, 7 x 3, 3 x 3 -> 0.  ring (8): 9 x 4, 2 x 4, a tie: 9 occurs first although 2 is the smaller id
    want = np.array([[0, 0, 0, 0, 0],
                     [0, 9, 9, 9, 0],
                     [0, 9, 5, 9, 0],
                     [0, 9, 9, 9, 0],
                     [0, 0, 0, 0, 0]], np.uint8)
    assert np.array_equal(R.refine(seg, RING_REGIONS, 1, 100), want)  # the hole (1 pixel) is not above min_thre = 1
    # three ways: 9, 2, 4 twice each (+ 1 and 0 once): 9 first
    seg3 = seg.copy()
    seg3[1, 1:4], seg3[2, 1], seg3[2, 3], seg3[3, 1:4] = (9, 2, 4), 4, 9, (2, 1, 0)
    assert (R.refine(seg3, RING_REGIONS, 1, 100)[RING > 50] == 9).all()


def test_hand_written_size_thresholds_are_strict():
    seg = np.arange(25, dtype=np.uint8).reshape(5, 5)  # every value once: the winner of a region is its first pixel
    ring_won = np.where(RING > 50, 6, seg)
    assert np.array_equal(R.refine(seg, RING_REGIONS, 8, 16), seg)          # ring == min_thre, outside == max_thre: untouched
    assert np.array_equal(R.refine(seg, RING_REGIONS, 7, 16), ring_won)     # ring == min_thre + 1: refined
    assert np.array_equal(R.refine(seg, RING_REGIONS, 7, 8), seg)           # ring == max_thre: untouched
    both = np.where(RING_REGIONS == 0, 0, ring_won)
    assert np.array_equal(R.refine(seg, RING_REGIONS, 7, 17), both)
    assert np.array_equal(R.refine(seg, RING_REGIONS, 0, 2), seg)           # the hole: refined to its own value
    frame = np.where(RING_REGIONS == 0, -1, RING_REGIONS)
    assert np.array_equal(R.refine(seg, frame, 7, 17), ring_won)            # -1 is never a region, whatever its size


def test_hand_written_value_255_wins():
    seg = np.full((5, 5), 255, np.uint8)
    seg[1, 1], seg[1, 2], seg[2, 1] = 0, 1, 0
    out = R.refine(seg, RING_REGIONS, 1, 100)
    assert (out[RING > 50] == 255).all() and out.dtype == np.uint8


@pytest.mark.parametrize("which", ["adapt_segbd_multitask_tester", "adapt_triple_multitask_tester"])
def test_testers_take_the_flags_with_the_reference_defaults(which):
    import importlib
    parser = importlib.import_module(which).get_parser()
    a = parser.parse_args(["nyu", "x.pth.tar"])
    assert (a.refine_by_boundary, a.boundary_thre, a.min_thre, a.max_thre) == (False, 50, 500, 79333)
    a = parser.parse_args(["nyu", "x.pth.tar", "--refine_by_boundary", "--boundary_thre", "7", "--min_thre", "4", "--max_thre", "2000"])
    assert (a.refine_by_boundary, a.boundary_thre, a.min_thre, a.max_thre) == (True, 7, 4, 2000)


def test_other_testers_do_not_take_the_flag():
    from argmyparse import get_da_mcd_testing_parser
    with pytest.raises(SystemExit):
        get_da_mcd_testing_parser().parse_args(["nyu", "x.pth.tar", "--refine_by_boundary"])


def test_tool_parser_and_its_refusals(tmp_path):
    tool = _tool()
    a = tool.get_parser().parse_args(["seg", "bd"])
    assert (a.segdir, a.boundary_dir, a.thre, a.min_thre, a.max_thre, a.gt_dir, a.n_class) == ("seg", "bd", 50, 500, 79333, None, None)
    a = tool.get_parser().parse_args(["seg", "bd", "--thre", "9", "--min_thre", "1", "--max_thre", "5", "--gt_dir", "gt", "--n_class", "41", "-b", "3"])
    assert (a.thre, a.min_thre, a.max_thre, a.gt_dir, a.n_class, a.batch_size) == (9, 1, 5, "gt", 41, 3)
    with pytest.raises(SystemExit, match="n_class"):
        tool.main(["seg", "bd", "--gt_dir", "gt"])


def test_entry_points_are_declared_and_bound():
    from mcdseg import _lib
    with open(os.path.join(_lib.INCLUDE, "mcdseg.h")) as f:
        header = f.read()
    for name in ("mcdseg_refine_workspace_bytes", "mcdseg_boundary_regions", "mcdseg_refine_labels_by_regions"):
        assert name + "(" in header and name in _lib.EXPORTS
    import torch
    from mcdseg import ops
    with pytest.raises(RuntimeError, match="GPU"):
        ops.refine_labels_by_boundary(torch.zeros((1, 4, 4), dtype=torch.uint8), torch.zeros((1, 4, 4), dtype=torch.uint8))
