"""GPU: the boundary refinement kernels (csrc/refine.hip: connected-component labelling by union-find and the per-region vote) against
the numpy restatement (tests/refine_ref.py).  Everything is integer: exact equality throughout."""
import ctypes

import numpy as np
import pytest
import torch

import refine_ref as R

pytestmark = pytest.mark.gpu

LO, HI = 4, 600  # thresholds of the sweep: tiny, so that the small shapes hold eligible and ineligible regions alike


@pytest.fixture(scope="module")
def ref():
    """{(h, w): {pattern: (boundary, regions)}} by the restatement, computed once"""
    return {s: {name: (b, R.regions(b, R.THRE)) for name, b in R.patterns(*s).items()} for s in R.SHAPES}


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _regions(b, device, thre=R.THRE):
    from mcdseg import ops
    return ops.boundary_regions(_dev(b if b.ndim == 3 else b[None], device), thre).cpu().numpy()


def _refine(seg, reg, lo, hi, device):
    from mcdseg import ops
    seg, reg = (seg if seg.ndim == 3 else seg[None]), (reg if reg.ndim == 3 else reg[None])
    return ops.refine_labels(_dev(seg, device), _dev(reg.astype(np.int32), device), lo, hi).cpu().numpy()


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d" % s)
def test_regions_equal_the_restatement(ref, device, shape):
    for name, (b, want) in ref[shape].items():
        got = _regions(b, device)
        assert got.dtype == np.int32 and got.shape == (1,) + shape
        assert np.array_equal(got[0], want), (name, shape, int((got[0] != want).sum()))


def test_what_the_patterns_are_meant_to_hold(ref):
    big = ref[(130, 200)]
    b, r = big["checker"]
    assert (r[b > 0] == -1).all() and np.array_equal(r[b == 0], np.flatnonzero(b.reshape(-1) == 0))  # every zero pixel its own region
    b, r = big["checker_inset"]
    assert len(np.unique(r[b > 0])) == 1 and r[b > 0].min() >= 0
    b, r = big["spiral"]
    assert len(np.unique(r[b == 0])) == 1 and (b == 0).sum() > 5000  # ONE corridor through every tile
    b, r = big["diagonal"]
    assert len(np.unique(r[b == 0])) == 2 and (r[b > 0] == -1).all()
    b, r = big["diagonal_short"]
    assert len(np.unique(r[b == 0])) == 1 and len(np.unique(r[b > 0])) == 1 and r[b > 0].min() >= 0
    b, r = big["threshold"]
    assert (r[:, 1::2] == -1).all() and (r[:, 0::2] >= 0).all()
    b, r = big["comb"]
    assert len(np.unique(r[b == 0])) == 1


def test_regions_of_a_batch_carry_no_offset_and_do_not_leak(ref, device):
    pats = ref[(130, 200)]
    names = ("bernoulli_5", "spiral", "checker_inset")
    got = _regions(np.stack([pats[n][0] for n in names]), device)
    for k, n in enumerate(names):
        assert np.array_equal(got[k], pats[n][1]), n


def test_threshold_is_strict(device):
    b = R.threshold_pair(33, 65)
    assert np.array_equal(_regions(b, device, R.THRE)[0], R.regions(b, R.THRE))
    assert (_regions(b, device, R.THRE + 1)[0] == 0).all()  # nothing above thre + 1: one region whose smallest index is 0
    assert (_regions(b, device, R.THRE - 1)[0] == -1).all()  # everything above thre - 1: all frame


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d" % s)
def test_refined_labels_equal_the_restatement(ref, device, shape):
    for i, (name, (b, reg)) in enumerate(ref[shape].items()):
        seg = R.seeded_seg(shape[0], shape[1], seed=31 + i)
        got = _refine(seg, reg, LO, HI, device)[0]
        assert np.array_equal(got, R.refine(seg, reg, LO, HI)), (name, shape)


def _region_of_size(reg, lo, hi):
    ids, counts = np.unique(reg[reg >= 0], return_counts=True)
    ok = np.flatnonzero((counts >= lo) & (counts <= hi))
    assert ok.size, "the pattern holds no region of %d..%d pixels" % (lo, hi)
    rid = ids[ok[0]]
    return int(rid), int(counts[ok[0]]), np.flatnonzero(reg.reshape(-1) == rid)


def test_size_thresholds_are_strict_at_both_ends(ref, device):
    _, reg = ref[(33, 65)]["bernoulli_3"]
    rid, c, idx = _region_of_size(reg, 6, 200)
    seg = R.seeded_seg(33, 65, seed=5)
    flat = seg.reshape(-1)
    flat[idx] = 9
    flat[idx[0]] = 7  # refining the region must change this pixel
    for lo, hi, changed in ((c, 10 * c, False), (c - 1, 10 * c, True), (0, c, False), (0, c + 1, True)):
        got = _refine(seg, reg, lo, hi, device)[0]
        assert np.array_equal(got, R.refine(seg, reg, lo, hi)), (lo, hi)
        assert (got.reshape(-1)[idx[0]] == 9) == changed, (lo, hi, c)


@pytest.mark.parametrize("ways", (2, 3))
def test_ties_go_to_the_first_occurrence_not_the_smallest_id(ref, device, ways):
    _, reg = ref[(130, 200)]["bernoulli_3"]
    rid, c, idx = _region_of_size(reg, 12, 5000)
    seg = R.seeded_seg(130, 200, seed=6)
    flat = seg.reshape(-1)
    values = (200, 3) if ways == 2 else (200, 100, 3)  # the first to occur is the LARGEST id
    each = c // ways
    flat[idx[:each * ways]] = np.tile(np.array(values, np.uint8), each)
    flat[idx[each * ways:]] = np.arange(50, 50 + c - each * ways)  # the remainder: values that occur once
    got = _refine(seg, reg, 0, 10 ** 6, device)[0]
    assert np.array_equal(got, R.refine(seg, reg, 0, 10 ** 6))
    assert (got.reshape(-1)[idx] == 200).all()


def test_value_255_wins(ref, device):
    _, reg = ref[(33, 65)]["comb"]
    seg = np.full((33, 65), 255, np.uint8)
    seg[::3, ::2] = 254
    got = _refine(seg, reg, LO, 10 ** 6, device)[0]
    assert np.array_equal(got, R.refine(seg, reg, LO, 10 ** 6))
    rid, c, idx = _region_of_size(reg, 100, 10 ** 6)
    assert (got.reshape(-1)[idx] == 255).all() and (seg.reshape(-1)[idx] == 254).any()


def test_inner_boundary_component_is_refined_and_the_frame_object_never(ref, device):
    seg = R.seeded_seg(33, 65, seed=8)
    b, reg = ref[(33, 65)]["checker_inset"]
    got = _refine(seg, reg, LO, 2000, device)[0]
    assert np.array_equal(got, R.refine(seg, reg, LO, 2000))
    assert len(np.unique(got[b > 0])) == 1 and len(np.unique(seg[b > 0])) > 1
    b, reg = ref[(33, 65)]["checker"]
    assert LO < (reg == -1).sum() < 2000  # in range, and still not a region
    got = _refine(seg, reg, LO, 2000, device)[0]
    assert np.array_equal(got[b > 0], seg[b > 0]) and np.array_equal(got, R.refine(seg, reg, LO, 2000))


def test_min_thre_zero_fills_the_largest_vote_table(ref, device):
    _, reg = ref[(33, 65)]["bernoulli_5"]
    seg = R.seeded_seg(33, 65, seed=9)
    assert np.array_equal(_refine(seg, reg, 0, 33 * 65 + 1, device)[0], R.refine(seg, reg, 0, 33 * 65 + 1))
    _, reg = ref[(33, 65)]["checker"]  # 1072 one-pixel regions: every one eligible, nothing changes
    assert np.array_equal(_refine(seg, reg, 0, 2, device)[0], seg)
    assert np.array_equal(_refine(seg, reg, -5, 2, device)[0], seg)


def test_permuted_region_ids_give_the_same_labels(ref, device):
    _, reg = ref[(130, 200)]["bernoulli_6"]
    seg = R.seeded_seg(130, 200, seed=10)
    perm = np.random.RandomState(3).permutation(reg.size).astype(np.int32)
    other = np.where(reg >= 0, perm[np.maximum(reg, 0)], -1).astype(np.int32)
    assert not np.array_equal(other, reg)
    want = R.refine(seg, reg, LO, HI)
    assert np.array_equal(_refine(seg, reg, LO, HI, device)[0], want)
    assert np.array_equal(_refine(seg, other, LO, HI, device)[0], want)


def test_refinement_of_a_batch_and_by_boundary(ref, device):
    from mcdseg import ops
    pats = ref[(130, 200)]
    names = ("bernoulli_3", "spiral", "comb")
    b = np.stack([pats[n][0] for n in names])
    seg = np.stack([R.seeded_seg(130, 200, seed=20 + k, block=8) for k in range(3)])
    got = ops.refine_labels_by_boundary(_dev(seg, device), _dev(b, device), R.THRE, LO, 20000).cpu().numpy()
    for k in range(3):
        assert np.array_equal(got[k], R.refine_by_boundary(seg[k], b[k], R.THRE, LO, 20000)), names[k]


def test_two_runs_are_bitwise_equal(ref, device):
    b, _ = ref[(130, 200)]["bernoulli_5"]
    seg = R.seeded_seg(130, 200, seed=11)
    r1, r2 = _regions(b, device), _regions(b, device)
    assert np.array_equal(r1, r2)
    assert np.array_equal(_refine(seg, r1[0], LO, HI, device), _refine(seg, r2[0], LO, HI, device))


def test_bad_calls_are_refused_with_a_message_and_launch_nothing(device):
    import mcdseg
    L = mcdseg.lib()
    n, h, w = 1, 33, 65
    seg = torch.full((n, h, w), 7, dtype=torch.uint8, device=device)
    reg = torch.zeros((n, h, w), dtype=torch.int32, device=device)
    out = torch.full((n, h, w), 99, dtype=torch.uint8, device=device)
    need = L.mcdseg_refine_workspace_bytes(n, h, w, 0)
    assert need >= (h * w) * (4 + 256 * 8)  # a slot per pixel at min_thre = 0
    assert L.mcdseg_refine_workspace_bytes(n, h, w, 500) < L.mcdseg_refine_workspace_bytes(n, h, w, 4) < need
    assert L.mcdseg_refine_workspace_bytes(1, 425, 560, 500) == \
        -(-425 * 560 * 4 // 16) * 16 + 16 + -(-(425 * 560 // 501) // 16) * 16 + (425 * 560 // 501) * 2048
    ws = torch.empty(need // 4 + 1, dtype=torch.int32, device=device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def refused(rc, word):
        assert rc < 0
        assert word in L.mcdseg_last_error().decode()

    refused(L.mcdseg_refine_labels_by_regions(p(seg), p(reg), p(out), n, h, w, 0, 100, p(ws), need - 1, st), "workspace")
    refused(L.mcdseg_refine_labels_by_regions(None, p(reg), p(out), n, h, w, 0, 100, p(ws), need, st), "null")
    refused(L.mcdseg_refine_labels_by_regions(p(seg), p(reg), p(out), n, h, w, 0, 100, None, need, st), "null")
    refused(L.mcdseg_refine_labels_by_regions(p(seg), p(reg), p(out), n, 0, w, 0, 100, p(ws), need, st), "dims")
    refused(L.mcdseg_refine_labels_by_regions(p(seg), p(reg), p(out), 40000, 400, 400, 0, 100, p(ws), need, st), "32 bits")
    refused(L.mcdseg_boundary_regions(None, 50, p(reg), n, h, w, None, 0, st), "null")
    refused(L.mcdseg_boundary_regions(p(seg), 50, None, n, h, w, None, 0, st), "null")
    refused(L.mcdseg_boundary_regions(p(seg), 50, p(reg), n, h, -1, None, 0, st), "dims")
    refused(L.mcdseg_boundary_regions(p(seg), 50, p(reg), 40000, 400, 400, None, 0, st), "32 bits")
    torch.cuda.synchronize()
    assert (out == 99).all() and (reg == 0).all()
    assert L.mcdseg_refine_labels_by_regions(p(seg), p(reg), p(out), n, h, w, 0, 100, p(ws), need, st) == 0
    torch.cuda.synchronize()
    assert (out == 7).all()


def test_wrappers_refuse_what_is_not_a_map_batch(device):
    from mcdseg import ops
    with pytest.raises(RuntimeError):
        ops.boundary_regions(torch.zeros((1, 4, 4), dtype=torch.uint8), 50)
    with pytest.raises(TypeError):
        ops.boundary_regions(torch.zeros((4, 4), dtype=torch.uint8, device=device), 50)
    with pytest.raises(TypeError):
        ops.refine_labels(torch.zeros((1, 4, 4), dtype=torch.uint8, device=device), torch.zeros((1, 4, 4), dtype=torch.int64, device=device), 0, 9)
    with pytest.raises(ValueError):
        ops.refine_labels(torch.zeros((1, 4, 4), dtype=torch.uint8, device=device), torch.zeros((1, 4, 5), dtype=torch.int32, device=device), 0, 9)
