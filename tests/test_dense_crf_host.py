"""CPU: the dense CRF's contract (the reference's tools/crf.py).  The numpy oracle's own properties, the
torch composition of ``MCDSEG_FUSED_CRF=0`` against it, the C ABI's declarations and refusals, the tool's parser.  No kernel is
launched here."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import dense_crf_ref as R
from conftest import PKG, ROOT


def _tool():
    spec = importlib.util.spec_from_file_location("dense_crf_tool", os.path.join(PKG, "tools", "dense_crf.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------ the oracle
def test_oracle_without_iterations_is_the_softmax():
    z, rgb = R.make_case(1, 6, 7, 5, seed=0)
    for img in (rgb[0], None):
        q = R.dense_crf(z[0], img, n_iters=0)
        assert q.dtype == np.float64 and np.abs(q - R.softmax(z[0].astype(np.float64), 0)).max() < 1e-15
        assert np.abs(q.sum(0) - 1).max() < 1e-14
    kept = R.dense_crf(z[0], rgb[0], n_iters=3, keep=(0, 1, 3))
    assert sorted(kept) == [0, 1, 3] and np.array_equal(kept[0], R.dense_crf(z[0], rgb[0], n_iters=0))
    assert np.array_equal(kept[3], R.dense_crf(z[0], rgb[0], n_iters=3)) and not np.allclose(kept[3], kept[1], atol=1e-3)
    assert R.dense_crf(z[0], rgb[0], n_iters=2, dtype=np.float32).dtype == np.float32


def test_oracle_constant_inputs_are_a_fixed_point():
    z = np.full((4, 5, 6), 0.7, np.float32)
    rgb = np.full((5, 6, 3), 90, np.uint8)
    for img in (rgb, None):
        q = R.dense_crf(z, img, n_iters=4)
        assert np.abs(q - 0.25).max() < 1e-15
    # and a message is at most the largest Q times n_i sum_j k n_j, which the symmetric normalisation keeps at or below ~1
    f = R.features(5, 6, (4, 4), rgb, (13, 13, 13))
    k = R.kernel_matrix(f)
    n = 1 / np.sqrt(k.sum(1) + 1e-20)
    assert np.allclose(k, k.T) and (np.diag(k) == 1).all() and (n[:, None] * k * n[None, :]).sum(1).max() < 1.2


def test_oracle_labels_and_margin():
    q = np.array([[[0.2, 0.5]], [[0.5, 0.5]], [[0.3, 0.0]]])
    assert R.labels_of(q).tolist() == [[1, 0]] and R.labels_of(q).dtype == np.uint8  # the first maximum on a tie
    assert R.labels_of(q, 1).tolist() == [[0, 0]]
    assert np.allclose(R.margin_of(q), [[0.2, 0.0]]) and np.isinf(R.margin_of(q, 1)).all()


def test_oracle_inputs_are_what_the_issue_describes():
    z, rgb = R.make_case(2, 12, 16, 5, seed=1)
    assert z.shape == (2, 5, 12, 16) and z.dtype == np.float32 and rgb.shape == (2, 12, 16, 3) and rgb.dtype == np.uint8
    z2, rgb2 = R.make_case(2, 12, 16, 5, seed=1)
    assert np.array_equal(z, z2) and np.array_equal(rgb, rgb2) and not np.array_equal(z[0], z[1])
    q0, q10 = R.dense_crf(z[0], rgb[0], n_iters=0), R.dense_crf(z[0], rgb[0], sxy_bilateral=(4, 4))
    changed = (R.labels_of(q0) != R.labels_of(q10)).mean()
    assert 0.2 < changed < 0.8  # the CRF changes about half of the labels: a kernel that did nothing would fail the parity test


# ------------------------------------------------------------------------------------------------ the torch composition
@pytest.mark.parametrize("image", (True, False))
def test_composed_form_is_the_definition(image):
    from mcdseg import ops
    z, rgb = R.make_case(2, 9, 11, 6, seed=2)
    params = (1.0, 1.0, 4.0, 4.0, 4.0, 5.0, 13.0, 13.0, 13.0)
    for n_iters in (0, 1, 5):
        q, lab = ops._crf_composed(torch.from_numpy(z), torch.from_numpy(rgb) if image else None, n_iters, params, 6)
        assert q.dtype == torch.float32 and lab.dtype == torch.uint8 and tuple(lab.shape) == (2, 9, 11)
        for k in range(2):
            want = R.dense_crf(z[k], rgb[k] if image else None, n_iters=n_iters, sxy_bilateral=(4, 4))
            unit = np.abs(R.dense_crf(z[k], rgb[k] if image else None, n_iters=n_iters, sxy_bilateral=(4, 4), dtype=np.float32) - want).max()
            assert np.abs(q[k].numpy() - want).max() <= max(2 * unit, 2e-5 * want.max())
            sure = R.margin_of(want) >= 1e-3
            assert np.array_equal(lab[k].numpy()[sure], R.labels_of(want)[sure])
    tie = torch.zeros(1, 3, 2, 2)
    assert ops._crf_composed(tie, None, 0, params, 3)[1].tolist() == [[[0, 0], [0, 0]]]
    assert ops._crf_composed(tie, None, 2, params, 2)[1].max() == 0


def test_op_refuses_the_cpu_and_gradients(monkeypatch):
    from mcdseg import ops
    assert ops.CRF_DEFAULTS == R.DEFAULTS
    assert ops.fused_crf() is True
    monkeypatch.setenv("MCDSEG_FUSED_CRF", "0")  # read at every call
    assert ops.fused_crf() is False
    monkeypatch.setenv("MCDSEG_FUSED_CRF", "1")
    assert ops.fused_crf() is True
    with pytest.raises(RuntimeError, match="GPU"):
        ops.dense_crf(torch.zeros(1, 3, 4, 4))
    with pytest.raises(RuntimeError, match="inference only"):
        ops.dense_crf(torch.zeros(1, 3, 4, 4, requires_grad=True))


# ------------------------------------------------------------------------------------------------ the C ABI
def test_exports_declarations_and_refusals():
    import mcdseg
    from mcdseg import _lib
    mcdseg.build()
    with open(os.path.join(ROOT, "include", "mcdseg.h")) as f:
        header = f.read()
    L = mcdseg.lib()
    for name in ("mcdseg_dense_crf_workspace_bytes", "mcdseg_dense_crf"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.EXPORTS and hasattr(L, name), name
    block = header[header.index("The fully connected CRF over saved logits"):header.index("size_t mcdseg_dense_crf_workspace_bytes")]
    for cite in ("tools/crf.py:14-60", "crf.py:14-21", "crf.py:51-52", "crf.py:55-57", "crf.py:112", "ceil(7.5 sx)", "2^-40"):
        assert cite in block, cite
    assert L.mcdseg_version() == 101
    assert "crf.hip" in _lib.NO_PACKED_F32 and os.path.exists(os.path.join(_lib.CSRC, "crf.hip"))

    size = L.mcdseg_dense_crf_workspace_bytes
    pad = lambda b: (b + 255) // 256 * 256
    assert size(2, 13, 16, 24, 1) == 4 * pad(768 * 32 * 4) + 2 * pad(768 * 4) + pad(768 * 8 * 4)
    assert size(2, 13, 16, 24, 0) == 4 * pad(768 * 32 * 4) + pad(768 * 4)
    assert size(1, 41, 47, 61, 1) == 4 * pad(2867 * 64 * 4) + 2 * pad(2867 * 4) + pad(2867 * 8 * 4)
    for dims in ((1, 0, 4, 4), (1, 65, 4, 4), (0, 3, 4, 4), (1, 3, 0, 4), (1, 3, 5000, 5000), (200, 41, 480, 640), (65536, 1, 1, 1)):
        assert size(*dims, 1) == 0, dims

    p = ctypes.c_void_p(4096)  # never read: every refusal is answered before anything is launched (there is no GPU here to launch on)
    good = (1.0, 1.0, 4.0, 49.0, 49.0, 5.0, 13.0, 13.0, 13.0, 0.0)

    def refused(why, logits=p, rgb=p, params=good, q=p, labels=p, c_used=3, b=1, c=3, h=4, w=4, n_iters=10, ws=p, ws_bytes=1 << 30):
        host = (ctypes.c_float * 10)(*params) if params is not None else None
        rc = L.mcdseg_dense_crf(logits, rgb, host, q, labels, c_used, b, c, h, w, n_iters, ws, ws_bytes, None)
        msg = L.mcdseg_last_error().decode()
        assert rc == -22 and msg.startswith("dense_crf:") and why in msg, (why, rc, msg)

    refused("null pointer", logits=None)
    refused("null pointer", params=None)
    refused("null pointer", ws=None)
    refused("neither q nor labels", q=None, labels=None)
    refused("C = 0", c=0, c_used=0)
    refused("C = 65", c=65)
    refused("C_used = 0", c_used=0)
    refused("C_used = 4", c_used=4)
    refused("C_used = -1", c_used=-1)
    refused("bad dims", b=0)
    refused("bad dims", h=0)
    refused("bad dims", w=-3)
    refused("too large", h=5000, w=5000)            # H*W > 2^24
    refused("too large", b=200, c=41, h=480, w=640)  # B*H*W*64 >= 2^31
    refused("too large", b=65536, h=1, w=1)
    refused("n_iters = -1", n_iters=-1)
    for k in (0, 1):
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            refused("sxy_gaussian", params=good[:k] + (bad,) + good[k + 1:])
            refused("sxy_gaussian", params=good[:k] + (bad,) + good[k + 1:], rgb=None)
    for k in (3, 4, 6, 7, 8):
        for bad in (0.0, -2.0, float("nan")):
            refused("sxy_bilateral and srgb_bilateral", params=good[:k] + (bad,) + good[k + 1:])
    need = size(1, 3, 4, 4, 1)
    refused("workspace too small", ws_bytes=need - 1)
    refused("workspace too small", rgb=None, ws_bytes=size(1, 3, 4, 4, 0) - 1)
    refused("16-byte aligned", ws=ctypes.c_void_p(4096 + 8), ws_bytes=need)
    refused("4-byte aligned", logits=ctypes.c_void_p(4098))


# ------------------------------------------------------------------------------------------------ the tool and the class
def test_tool_parser_and_its_refusals():
    tool = _tool()
    a = tool.get_parser().parse_args(["prob", "out"])
    assert (a.prob_indir, a.outdir, a.prob_outdir, a.outimg_shape, a.raw_img_indir, a.n_used, a.gt_dir, a.n_class, a.batch_size) == \
        ("prob", "out", None, None, None, None, None, None, 1)
    got = {k: (tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in vars(a).items() if k in R.DEFAULTS}
    assert got == R.DEFAULTS  # tools/crf.py:14-21
    a = tool.get_parser().parse_args(["prob", "out", "--prob_outdir", "po", "--outimg_shape", "1280", "720", "--raw_img_indir", "raw", "--n_iters", "3",
                                      "--sxy_gaussian", "2", "3", "--compat_gaussian", "1.5", "--sxy_bilateral", "40", "41", "--srgb_bilateral",
                                      "5", "6", "7", "--compat_bilateral", "9", "--n_used", "19", "--gt_dir", "gt", "--n_class", "41", "-b", "4"])
    assert (a.prob_outdir, a.outimg_shape, a.raw_img_indir, a.n_iters, a.n_used, a.gt_dir, a.n_class, a.batch_size) == \
        ("po", [1280, 720], "raw", 3, 19, "gt", 41, 4)
    assert (list(a.sxy_gaussian), a.compat_gaussian, list(a.sxy_bilateral), list(a.srgb_bilateral), a.compat_bilateral) == \
        ([2, 3], 1.5, [40, 41], [5, 6, 7], 9)
    with pytest.raises(SystemExit, match="n_class"):
        tool.main(["prob", "out", "--gt_dir", "gt"])
    with pytest.raises(SystemExit, match="batch_size"):
        tool.main(["prob", "out", "-b", "0"])


def test_tool_without_a_gpu_is_a_system_exit(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="MI355X"):
        _tool().main([str(tmp_path), str(tmp_path / "out")])
    assert not os.path.exists(str(tmp_path / "out"))


def test_class_holds_parameters_and_directories(tmp_path):
    import dense_crf
    assert dense_crf.DEFAULTS == R.DEFAULTS
    crf = dense_crf.DenseCRF(str(tmp_path / "run" / "crf_label"), str(tmp_path / "run" / "crf_prob"), (36, 20), 19, 41, None, n_iters=3)
    assert os.path.isdir(crf.outdir) and os.path.isdir(crf.prob_outdir) and crf.base_outdir == str(tmp_path / "run")
    assert crf.params == dict(R.DEFAULTS, n_iters=3) and crf.outimg_shape == (36, 20) and crf.n_used == 19
    assert crf.finish() is None
    with pytest.raises(TypeError, match="unknown"):
        dense_crf.DenseCRF(str(tmp_path / "x"), sxy=3)
    crf.save(torch.arange(12, dtype=torch.uint8).reshape(1, 3, 4), ["a"], torch.ones(1, 2, 3, 4))
    from PIL import Image
    png = np.array(Image.open(os.path.join(crf.outdir, "a.png")))
    assert png.shape == (20, 36) and png.dtype == np.uint8 and png[0, 0] == 0 and png[-1, -1] == 11
    assert np.load(os.path.join(crf.prob_outdir, "a.npy")).shape == (2, 3, 4)
