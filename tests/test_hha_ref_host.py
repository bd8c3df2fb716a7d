"""CPU: the depth -> HHA oracle (tests/hha_ref.py) against an analytically rendered box room, and the conditions
that keep the comparison of tests/test_hha_gpu.py with it honest.  No kernel is launched here.

Three statements of the issue that the definition itself does not allow are asserted in the form the definition gives them:

* the ceiling's angle byte.  N is a plane's normal up to its sign, and the sign is fixed by N_z >= 0: two parallel planes have the SAME
  N, so floor and ceiling get the same byte -- 38 with the camera pitched down (g_z > 0), not 38 and 218.  Walls are 128.
* g on the whole noiseless room.  The R = 10 windows that straddle an intersection of two planes fit neither plane, and their normals
  enter A like any other: the estimate lies 0.3 ... 3 degrees from the true direction (measured 0.6 degrees here).  With the normals
  whose window lies on ONE plane (``gravity_mask``) the same ten iterations give the true direction to 1e-6, the floor's height above
  the camera to 1e-6 relative and the bytes 38 / 128 / 38; that is what is asserted, next to a 2-degree bound on the unmasked run.
* the floor's height.  h = -g.P - y_min is the height above the LOWEST point: the floor is at -cam_height before y_min is taken off
  (asserted to 1e-6 relative) and at 0 after it.

The threshold clearance is 1e-5 where the issue says 1e-4: the normals of windows that straddle an intersection sweep every angle, and
among the first 4096 noise seeds of the 37 x 53 room none keeps all ten iterations 1e-4 clear.  The float bounds are capped at a tenth of
the clearance instead (hha_ref.CAP), which is what the condition is for: a device result inside its bounds has the oracle's sets F and W.
"""
import importlib.util
import os

import numpy as np
import pytest

import hha_ref as R
from conftest import PKG

EXACT = dict(h=72, w=96, front=600.0, ceiling=200.0, right=120.0, left=200.0, yaw=10.0)  # pitch 12, roll 5 (the defaults): floor, ceiling and the three walls in view


@pytest.fixture(scope="module")
def exact_room():
    depth, truth = R.room(**EXACT)
    one10 = R.single_plane(truth["plane"], R.R_LARGE)
    return depth, truth, one10, R.hha(depth, truth["camera"], gravity_mask=one10), R.hha(depth, truth["camera"])


def test_room_is_what_it_says():
    depth, truth = R.room(**EXACT)
    assert depth.dtype == np.float64 and depth.shape == (72, 96) and (depth > 0).all()
    assert sorted(np.unique(truth["plane"])) == [0, 1, 2, 3, 4]
    g = truth["gravity"]
    assert abs(np.linalg.norm(g) - 1) < 1e-15 and abs(np.degrees(np.arcsin(g[2])) - 12) < 1e-12  # pitched down: g_z = sin 12
    assert abs(np.degrees(np.arctan2(-g[0], g[1])) - 5) < 1e-12                                   # rolled by 5
    assert (truth["normal"][:, 2] >= 0).all() and np.allclose(truth["normal"][0], truth["normal"][1])
    # every pixel lies on its plane
    fx, fy, cx, cy = truth["camera"]
    v, u = np.mgrid[:72, :96]
    p = np.stack([(u - cx) / fx * depth, (v - cy) / fy * depth, depth], -1)
    assert np.abs((p[truth["plane"] == 0] @ g) - 120.0).max() < 1e-10
    assert np.abs((p[truth["plane"] == 1] @ -g) - 80.0).max() < 1e-10
    noisy, _ = R.room(noise=0.5, holes=((3, 4, 5, 6),), seed=3, **EXACT)
    assert (noisy[3:8, 4:10] == 0).all() and 0.4 < (noisy - depth)[20:, 20:].std() < 0.6
    again, _ = R.room(noise=0.5, holes=((3, 4, 5, 6),), seed=3, **EXACT)
    assert np.array_equal(noisy, again)


def test_normals_of_the_noiseless_room(exact_room):
    depth, truth, one10, res, _ = exact_room
    m = truth["interior"]
    assert m.mean() > 0.7 and res["ok3"].all() and res["ok10"].all()
    want = truth["normal"][truth["plane"]]
    assert np.abs(res["normals3"] - want)[m].max() < 1e-9
    assert np.abs(res["normals10"] - want)[one10].max() < 1e-8  # (441 pixels: the adjugate cancels a digit more)
    assert (res["normals3"][..., 2] >= 0).all() and np.abs(np.linalg.norm(res["normals3"], axis=-1) - 1).max() < 1e-12


def test_gravity_height_and_bytes_of_the_noiseless_room(exact_room):
    depth, truth, one10, res, plain = exact_room
    g = truth["gravity"]
    assert np.abs(res["gravity"] - g).max() < 1e-6
    floor = (truth["plane"] == 0) & truth["interior"]
    raw = res["height"] + res["y_min"]  # -g.P
    assert np.abs(raw[floor] + 120.0).max() < 1e-6 * 120.0
    assert abs(res["y_min"] + 120.0) < 1e-6 * 120.0 and np.abs(res["height"][floor]).max() < 1e-3
    ceil = (truth["plane"] == 1) & truth["interior"]
    assert np.abs(res["height"][ceil] - 200.0).max() < 1e-3
    walls = (truth["plane"] >= 2) & truth["interior"]
    assert floor.any() and ceil.any() and walls.any()
    ang = res["bytes"][..., 2]
    assert (ang[floor] == 38).all() and (ang[walls] == 128).all() and (ang[ceil] == 38).all()
    assert np.array_equal(res["bytes"][..., 0], R.round_u8(31000.0 / np.maximum(depth, 100.0)))
    # the definition on the whole room: the straddling windows pull g off by less than 2 degrees
    off = np.degrees(np.arccos(np.clip(plain["gravity"] @ g, -1, 1)))
    assert 0.05 < off < 2.0, off


def test_oracle_edges():
    z = np.zeros((9, 11), np.float32)
    res = R.hha(z, (10.0, 10.0, 5.0, 4.0))
    assert not res["bytes"].any() and res["gravity"].tolist() == [0.0, 1.0, 0.0] and res["y_min"] == -130 and not res["height"].any()
    assert not res["ok3"].any() and not res["normals3"].any()
    z[4, 5] = z[4, 6] = 300.0  # two valid pixels: no window reaches three
    z[0, 0] = np.nan
    z[8, 10] = np.inf
    z[1, 1] = -5.0
    res = R.hha(z, (10.0, 10.0, 5.0, 4.0))
    assert res["valid"].sum() == 2 and not res["ok10"].any() and res["gravity"].tolist() == [0.0, 1.0, 0.0]
    assert res["bytes"][4, 5].tolist() == [103, 130, 0] and res["bytes"][0, 0].tolist() == [0, 0, 0]  # 31000/300; b = 0: h = 0 - (-130)
    assert R.round_u8([0.5, 1.5, 2.49999, -0.5, 255.5, 300, -3]).tolist() == [1, 2, 2, 0, 255, 255, 0]
    d, c = R.case_depth("odd_37x53")
    r32 = R.hha(d[0], c[0], dtype=np.float32)
    assert all(r32[k].dtype == np.float32 for k in ("normals3", "gravity", "height", "pre")) and r32["bytes"].dtype == np.uint8
    assert R.rel_to_max(r32["gravity"], R.hha(d[0], c[0])["gravity"]) < 1e-3
    assert np.array_equal(R.box_sum(np.ones((5, 4)), 10), np.full((5, 4), 20.0))
    assert R.box_sum(np.ones((9, 9)), 3)[0, 0] == 16 and R.box_sum(np.ones((9, 9)), 3)[4, 4] == 49


def test_the_gpu_cases_are_honest():
    """for every image of every case of tests/test_hha_gpu.py: the eigen-gap, the threshold clearance, y_min's distance from -90, the
    share of pixels within the byte margin -- and the recorded seed is the first that has them"""
    assert sorted(R.CASES) == ["clipped_8x12", "noise_holes_96x128", "odd_37x53", "two_rooms_48x64"]
    assert R.CLEARANCE == 1e-5 and R.CAP == 1e-6 and R.FLOOR == 2.0 ** -23
    for name, rooms in R.CASES.items():
        depth, cams = R.case_depth(name)
        assert depth.dtype == np.float32 and depth.shape == (len(rooms), rooms[0]["h"], rooms[0]["w"]) and cams.shape == (len(rooms), 4)
        for k, kw in enumerate(rooms):
            gap, near, ymin_gap, share, r64, bounds, margins = R.honesty(depth[k], cams[k])
            print("%s[%d]: eigen-gap %.3g, clearance %.3g, |y_min + 90| %.3g cm, within the byte margin %.2f %%, bounds %s"
                  % (name, k, gap, near, ymin_gap, 100 * share, {b: "%.2e" % v for b, v in bounds.items()}))
            assert gap >= 1e-3 and near >= R.CLEARANCE and ymin_gap >= 1.0 and share <= 0.02, (name, k, gap, near, ymin_gap, share)
            assert all(R.FLOOR <= v <= R.CAP for v in bounds.values())
            assert kw["noise"] > 0 and R.first_honest_seed(kw) == kw["seed"], (name, k)
    holes = R.CASES["noise_holes_96x128"][0]["holes"]
    d, c = R.case_depth("noise_holes_96x128")
    res = R.hha(d[0], c[0])
    assert (9, 9) in [(r, w) for _, _, r, w in holes] and any(v0 == 0 for v0, _, _, _ in holes)
    assert not res["ok3"][44, 54] and not res["valid"][44, 54] and res["ok10"][44, 54]  # the 7 x 7 window inside the 9 x 9 hole is empty
    assert (res["bytes"][~res["valid"]] == 0).all()
    small, _ = R.case_depth("clipped_8x12")
    # no R = 10 window fits the image; of the R = 3 windows only those of 2 x 6 pixels do
    assert small.shape == (1, 8, 12) and max(small.shape[1:]) < 2 * R.R_LARGE + 1


def test_margins_follow_the_bounds():
    d, c = R.case_depth("odd_37x53")
    r64 = R.hha(d[0], c[0])
    b = {"normals3": 1e-6, "gravity": 1e-6, "height": 1e-6}
    m = R.byte_margins(r64, b)
    assert m.shape == r64["pre"].shape and (m >= 0).all()
    assert np.allclose(m[..., 1], 1e-6 * np.abs(r64["height"]).max()) and np.allclose(m[..., 0], R.FLOOR * r64["pre"][..., 0].max())
    dot = np.clip(r64["normals3"] @ r64["gravity"], -1, 1)
    side = np.abs(dot) < 0.5  # away from 0 and 180 degrees the angle moves by d / sin
    d_cos = np.sqrt(3) * 2e-6
    assert np.allclose(m[..., 2][side], np.degrees(d_cos / np.sqrt(1 - dot[side] ** 2)), rtol=1e-3)
    wide = R.byte_margins(r64, {k: 10 * v for k, v in b.items()})
    assert (wide >= m).all() and R.byte_margin_share(r64, wide) >= R.byte_margin_share(r64, m)
    assert R.near_rounding({"pre": np.array([[[1.5, 1.4999, 7.0]]])}, np.array([[[0.0, 1e-3, 0.4]]])).tolist() == [[[True, True, False]]]


def test_composed_form_of_the_timing_tool_is_the_definition():
    import torch
    spec = importlib.util.spec_from_file_location("time_depth_to_hha", os.path.join(PKG, "tools", "time_depth_to_hha.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    d, c = R.case_depth("two_rooms_48x64")
    got, g = tool.composed(torch.from_numpy(d), torch.from_numpy(c))
    for k in range(2):
        gap, near, ymin_gap, share, r64, bounds, margins = R.honesty(d[k], c[k])
        assert np.abs(g[k].numpy() - r64["gravity"]).max() < 1e-9
        sure = ~R.near_rounding(r64, margins)
        assert np.array_equal(got[k].numpy()[sure], r64["bytes"][sure])
        assert np.abs(got[k].numpy().astype(int) - r64["bytes"].astype(int)).max() <= 1
    syn, cam = tool.synthetic_depth(2, 24, 32, torch.device("cpu"), 1)
    assert syn.shape == (2, 24, 32) and syn.dtype == torch.float32 and cam.shape == (2, 4) and 0 < (syn == 0).float().mean() < 0.5
