"""GPU: ``ops.dense_crf`` (csrc/crf.hip) against the fp64 numpy oracle of tests/dense_crf_ref.py.

Q is held to fp64 within max(FACTOR * unit, FLOOR * max|Q|): ``unit`` is the distance of the SAME oracle run in fp32 from its fp64 run
on that case, computed here; FACTOR and FLOOR are the constants of tests/test_fusenet_gpu.py / test_unet_gpu.py.  Labels are equal to the
oracle's wherever its top-2 margin is at least MARGIN, and at most LEFT_OUT of the pixels may be left out by that rule."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import dense_crf_ref as R
from conftest import PKG
from guards import guarded

pytestmark = pytest.mark.gpu

FACTOR, FLOOR = 2.0, 2e-5
MARGIN, LEFT_OUT = 1e-3, 0.02
ITERS = (0, 1, 10)
#        B  H   W   C     what it probes
CASES = {"1x1x1": (1, 1, 1, 1),          # degenerate ends
         "12x16x5": (1, 12, 16, 5),      # ragged C; N below one tile
         "2x16x24x13": (2, 16, 24, 13),  # a batch of two different images
         "47x61x41": (1, 47, 61, 41)}    # N = 2867: several i- and j-tiles with ragged ends; the 64-column kernel
SXY_B = {"default": (49, 49), "sxy4": (4, 4)}

_inputs, _truth = {}, {}


def inputs(case):
    if case not in _inputs:
        b, h, w, c = CASES[case]
        _inputs[case] = R.make_case(b, h, w, c, seed=sorted(CASES).index(case))
    return _inputs[case]


def truth(case, image, sxy):
    """{np.float64 / np.float32: [per image {t: Q^t [C,H,W]}]} of the oracle, computed once per (case, image, sxy) and left unchanged"""
    key = (case, image, sxy if image else None)
    if key not in _truth:
        z, rgb = inputs(case)
        _truth[key] = {dt: [R.dense_crf(z[k], rgb[k] if image else None, sxy_bilateral=SXY_B[sxy], dtype=dt, keep=ITERS)
                            for k in range(z.shape[0])] for dt in (np.float64, np.float32)}
    return _truth[key]


def run(case, image, sxy, n_iters, device, **kw):
    z, rgb = inputs(case)
    from mcdseg import ops
    q, lab = ops.dense_crf(torch.from_numpy(z).to(device), torch.from_numpy(rgb).to(device) if image else None, n_iters=n_iters,
                           sxy_bilateral=SXY_B[sxy], **kw)
    torch.cuda.synchronize()
    assert q.dtype == torch.float32 and lab.dtype == torch.uint8 and tuple(q.shape) == z.shape and tuple(lab.shape) == rgb.shape[:3]
    return q.cpu().numpy(), lab.cpu().numpy()


def bound_of(case, image, sxy, t):
    tr = truth(case, image, sxy)
    q64 = np.stack([im[t] for im in tr[np.float64]])
    q32 = np.stack([im[t] for im in tr[np.float32]])
    unit = float(np.abs(q32.astype(np.float64) - q64).max())
    return q64, unit, max(FACTOR * unit, FLOOR * float(np.abs(q64).max()))


@pytest.mark.parametrize("n_iters", ITERS)
@pytest.mark.parametrize("sxy", sorted(SXY_B))
@pytest.mark.parametrize("image", (True, False), ids=("image", "noimage"))
@pytest.mark.parametrize("case", sorted(CASES))
def test_q_against_the_fp64_oracle(case, image, sxy, n_iters, device):
    q64, unit, bound = bound_of(case, image, sxy, n_iters)
    q, _ = run(case, image, sxy, n_iters, device)
    err = float(np.abs(q.astype(np.float64) - q64).max())
    print("%s image=%s %s n_iters=%d: |Q - fp64| %.3e, the fp32 oracle's %.3e, bound %.3e" % (case, image, sxy, n_iters, err, unit, bound))
    assert np.isfinite(q).all() and err <= bound, (err, unit, bound)
    if n_iters == 10 and CASES[case][1] > 1:  # the CRF does something: a kernel that returned softmax(z) would not pass
        moved = float(np.abs(q64 - np.stack([im[0] for im in truth(case, image, sxy)[np.float64]])).max())
        assert moved > 100 * bound, moved


@pytest.mark.parametrize("sxy", sorted(SXY_B))
@pytest.mark.parametrize("image", (True, False), ids=("image", "noimage"))
@pytest.mark.parametrize("case", sorted(CASES))
def test_labels_where_the_margin_allows(case, image, sxy, device):
    q64 = bound_of(case, image, sxy, 10)[0]
    _, lab = run(case, image, sxy, 10, device)
    want = np.stack([R.labels_of(q) for q in q64])
    sure = np.stack([R.margin_of(q) for q in q64]) >= MARGIN
    before = np.stack([R.labels_of(im[0]) for im in truth(case, image, sxy)[np.float64]])
    print("%s image=%s %s: %d of %d pixels left out by the margin rule, the CRF changed %d labels"
          % (case, image, sxy, int((~sure).sum()), sure.size, int((want != before).sum())))
    assert (~sure).mean() <= LEFT_OUT
    assert np.array_equal(lab[sure], want[sure])


def test_c_used_is_honoured(device):
    case = "2x16x24x13"
    q64 = bound_of(case, True, "sxy4", 10)[0]
    for c_used in (1, 4, 13):
        _, lab = run(case, True, "sxy4", 10, device, c_used=c_used)
        want = np.stack([R.labels_of(q, c_used) for q in q64])
        sure = np.stack([R.margin_of(q, c_used) for q in q64]) >= MARGIN
        # (among FEWER classes the two largest are often both small: the 2 % rule belongs to the labels over all classes)
        assert sure.mean() >= 0.25 and lab.max() < c_used
        assert np.array_equal(lab[sure], want[sure])
    assert (np.stack([R.labels_of(q, 4) for q in q64]) != np.stack([R.labels_of(q) for q in q64])).any()


def test_a_tie_goes_to_the_first_index(device):
    """two identical logit planes above a third, constant image: the two classes stay equal bit for bit and the label is the first"""
    from mcdseg import ops
    rng = np.random.RandomState(5)
    h, w = 12, 16
    top = rng.normal(0, 1.5, size=(h, w)).astype(np.float32) + 3
    z = np.stack([rng.normal(0, 1, size=(h, w)).astype(np.float32) - 3, top, top, top - 9])[None]
    rgb = np.full((1, h, w, 3), 77, np.uint8)
    for image in (True, False):
        for n_iters in ITERS:
            q, lab = ops.dense_crf(torch.from_numpy(z).to(device), torch.from_numpy(rgb).to(device) if image else None, n_iters=n_iters)
            q, lab = q.cpu().numpy(), lab.cpu().numpy()
            assert np.array_equal(q[0, 1], q[0, 2]) and (q[0, 1] > q[0, 0]).all() and (lab == 1).all(), (image, n_iters)
            want = R.dense_crf(z[0], rgb[0] if image else None, n_iters=n_iters)
            assert (R.labels_of(want) == 1).all()


@pytest.mark.parametrize("image", (True, False), ids=("image", "noimage"))
def test_two_runs_and_a_batch_are_bitwise_equal(image, device):
    from mcdseg import ops
    for case in ("2x16x24x13", "47x61x41"):
        q1, l1 = run(case, image, "sxy4", 10, device)
        q2, l2 = run(case, image, "sxy4", 10, device)
        assert q1.tobytes() == q2.tobytes() and l1.tobytes() == l2.tobytes()
    z, rgb = inputs("2x16x24x13")
    qb, lb = run("2x16x24x13", image, "sxy4", 10, device)
    assert not np.array_equal(qb[0], qb[1])
    for k in range(2):  # an image alone: what it gave in the batch
        q, lab = ops.dense_crf(torch.from_numpy(z[k:k + 1]).to(device), torch.from_numpy(rgb[k:k + 1]).to(device) if image else None,
                               sxy_bilateral=SXY_B["sxy4"])
        assert q.cpu().numpy().tobytes() == qb[k:k + 1].tobytes() and lab.cpu().numpy().tobytes() == lb[k:k + 1].tobytes()


@pytest.mark.parametrize("sxy", sorted(SXY_B))
@pytest.mark.parametrize("image", (True, False), ids=("image", "noimage"))
@pytest.mark.parametrize("case", ("12x16x5", "2x16x24x13"))
def test_composed_form_against_the_fused(case, image, sxy, device, monkeypatch):
    from mcdseg import ops
    for n_iters in ITERS:
        _, _, bound = bound_of(case, image, sxy, n_iters)
        monkeypatch.setenv("MCDSEG_FUSED_CRF", "1")
        assert ops.fused_crf()
        q, lab = run(case, image, sxy, n_iters, device)
        monkeypatch.setenv("MCDSEG_FUSED_CRF", "0")
        assert not ops.fused_crf()
        qc, labc = run(case, image, sxy, n_iters, device)
        err = float(np.abs(q.astype(np.float64) - qc).max())
        print("%s image=%s %s n_iters=%d: |fused - composed| %.3e, bound %.3e" % (case, image, sxy, n_iters, err, bound))
        assert err <= bound
        sure = np.stack([R.margin_of(x) for x in q.astype(np.float64)]) >= MARGIN
        assert np.array_equal(lab[sure], labc[sure])


@pytest.mark.parametrize("interior", (0xFF, 0x00))
@pytest.mark.parametrize("case", ("12x16x5", "47x61x41"))
def test_memory_contract(case, interior, device):
    """no guard byte changes, the results do not depend on what outputs and workspace held, and the workspace goes through ops._ws"""
    from mcdseg import ops
    z, rgb = inputs(case)
    for image in (True, False):
        for n_iters in (0, 3):
            want_q, want_l = run(case, image, "sxy4", n_iters, device)
            with guarded(device, interior=interior) as g:
                q, lab = ops.dense_crf(g.put(torch.from_numpy(z)), g.put(torch.from_numpy(rgb)) if image else None, n_iters=n_iters,
                                       sxy_bilateral=SXY_B["sxy4"])
                assert g.check() == []
                assert g.workspaces == 1 and g.count >= 4
                assert q.cpu().numpy().tobytes() == want_q.tobytes() and lab.cpu().numpy().tobytes() == want_l.tobytes()


def _tool():
    spec = importlib.util.spec_from_file_location("dense_crf_tool", os.path.join(PKG, "tools", "dense_crf.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tool_end_to_end(tmp_path, device):
    from mcdseg import ops
    z, rgb = R.make_case(3, 16, 24, 13, seed=9)
    names = ["a", "b", "c"]
    for sub in ("prob", "raw", "gt"):
        os.makedirs(str(tmp_path / sub))
    gt = np.stack([R.labels_of(x) for x in z])
    for k, n in enumerate(names):
        np.save(str(tmp_path / "prob" / (n + ".npy")), z[k])
        Image.fromarray(np.repeat(np.repeat(rgb[k], 2, 0), 2, 1)).save(str(tmp_path / "raw" / (n + ".png")))  # 32 x 48: resized NEAREST
        Image.fromarray(gt[k]).save(str(tmp_path / "gt" / (n + ".png")))
    out = str(tmp_path / "crf" / "label")
    got = _tool().main([str(tmp_path / "prob"), out, "--prob_outdir", str(tmp_path / "crf" / "prob"), "--raw_img_indir", str(tmp_path / "raw"),
                        "--outimg_shape", "36", "20", "--sxy_bilateral", "4", "4", "--gt_dir", str(tmp_path / "gt"), "--n_class", "13",
                        "-b", "2"])
    assert got == out and sorted(os.listdir(out)) == [n + ".png" for n in names]
    assert np.array_equal(np.array(Image.fromarray(rgb[0]).resize((48, 32), Image.NEAREST).resize((24, 16), Image.NEAREST)), rgb[0])
    q, lab = ops.dense_crf(torch.from_numpy(z).to(device), torch.from_numpy(rgb).to(device), sxy_bilateral=(4, 4))
    q, lab = q.cpu().numpy(), lab.cpu().numpy()
    for k, n in enumerate(names):
        png = np.array(Image.open(os.path.join(out, n + ".png")))
        assert png.dtype == np.uint8 and png.shape == (20, 36)
        assert np.array_equal(png, np.array(Image.fromarray(lab[k]).resize((36, 20), Image.NEAREST)))
        saved = np.load(str(tmp_path / "crf" / "prob" / (n + ".npy")))
        assert saved.dtype == np.float32 and saved.tobytes() == q[k].tobytes()  # an image alone or in a batch: the same bits
        want = R.dense_crf(z[k], rgb[k], sxy_bilateral=(4, 4))
        unit = float(np.abs(R.dense_crf(z[k], rgb[k], sxy_bilateral=(4, 4), dtype=np.float32) - want).max())
        assert float(np.abs(saved - want).max()) <= max(FACTOR * unit, FLOOR * float(want.max()))
    with open(str(tmp_path / "crf" / "eval_result_crf.json")) as f:
        result = json.load(f)
    assert sorted(result) == ["after", "before"] and result["before"]["pixAcc"] == 100.0 and result["after"]["pixAcc"] < 100.0
