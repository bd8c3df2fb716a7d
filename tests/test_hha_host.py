"""CPU: the depth -> HHA encoding's contract outside the kernels: the C ABI's declarations and refusals, the
Python op's refusals, the pipeline's method, the tool's parser and its exit without a GPU.  No kernel is launched here."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT


def _tool():
    spec = importlib.util.spec_from_file_location("depth_to_hha_tool", os.path.join(PKG, "tools", "depth_to_hha.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_exports_declarations_and_refusals():
    import mcdseg
    from mcdseg import _lib
    mcdseg.build()
    with open(os.path.join(ROOT, "include", "mcdseg.h")) as f:
        header = f.read()
    L = mcdseg.lib()
    for name in ("mcdseg_depth_to_hha_workspace_bytes", "mcdseg_depth_to_hha"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.EXPORTS and hasattr(L, name), name
    block = header[header.index("Depth -> HHA"):header.index("size_t mcdseg_depth_to_hha_workspace_bytes")]
    flat = " ".join(block.replace("*", " ").split())  # (the comment's line breaks are not part of what it says)
    for cite in ("Gupta", "section 4.13", "tests/hha_ref.py", "adj(M) t", "ON THE HOST", "nothing is claimed about byte equality", "65535"):
        assert cite in flat, cite
    assert L.mcdseg_version() == 101
    assert "hha.hip" in _lib.NO_PACKED_F32 and os.path.exists(os.path.join(_lib.CSRC, "hha.hip"))

    size = L.mcdseg_depth_to_hha_workspace_bytes
    pad = lambda b: (b + 255) // 256 * 256
    # cameras, g, y_min | 12 sums and one minimum per reduction block (2048 pixels each, at most 128) | both normal maps, fp64
    assert size(2, 8, 12) == pad(64) + pad(48) + pad(16) + pad(2 * 12 * 8) + pad(2 * 8) + 2 * pad(2 * 96 * 24)
    assert size(1, 37, 53) == pad(32) + pad(24) + pad(8) + pad(12 * 8) + pad(8) + 2 * pad(1961 * 24)
    assert size(16, 480, 640) == pad(512) + pad(384) + pad(128) + pad(16 * 128 * 96) + pad(16 * 128 * 8) + 2 * pad(16 * 307200 * 24)
    for dims in ((0, 4, 4), (1, 0, 4), (1, 4, -1), (65536, 1, 1), (1, 5000, 5000), (100, 4096, 4096 // 2)):
        assert size(*dims) == 0, dims

    p = ctypes.c_void_p(4096)  # never read: every refusal is answered before anything is launched (there is no GPU here to launch on)

    def refused(why, depth=p, camera=(500.0, 500.0, 320.0, 240.0), hha=p, normals3=p, gravity=p, height=p, n=1, h=4, w=4, ws=p, ws_bytes=1 << 30):
        host = (ctypes.c_float * (4 * max(n, 1)))(*(tuple(camera) * max(n, 1))[:4 * max(n, 1)]) if camera is not None else None
        rc = L.mcdseg_depth_to_hha(depth, host, hha, normals3, gravity, height, n, h, w, ws, ws_bytes, None)
        msg = L.mcdseg_last_error().decode()
        assert rc == -22 and msg.startswith("depth_to_hha:") and why in msg, (why, rc, msg)

    refused("null pointer", depth=None)
    refused("null pointer", camera=None)
    refused("null pointer", hha=None)
    refused("null pointer", ws=None)
    refused("bad dims", n=0)
    refused("bad dims", h=0)
    refused("bad dims", w=-3)
    refused("at most 65535", n=65536, h=1, w=1)
    refused("too large", h=5000, w=5000)           # H*W > 2^24
    refused("too large", n=100, h=4096, w=2048)    # N*H*W*3 >= 2^31
    for k in (0, 1):
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            cam = [500.0, 500.0, 320.0, 240.0]
            cam[k] = bad
            refused("fx and fy must be positive and finite", camera=cam)
    refused("image 1", camera=(500.0, 500.0, 1.0, 1.0, 500.0, 0.0, 1.0, 1.0), n=2)  # every image's camera is looked at
    refused("cx and cy must be finite", camera=(500.0, 500.0, float("nan"), 240.0))
    refused("cx and cy must be finite", camera=(500.0, 500.0, 320.0, float("-inf")))
    need = size(1, 4, 4)
    refused("workspace too small", ws_bytes=need - 1)
    refused("16-byte aligned", ws=ctypes.c_void_p(4096 + 8), ws_bytes=need)
    refused("4-byte aligned", depth=ctypes.c_void_p(4098))
    refused("4-byte aligned", height=ctypes.c_void_p(4097))
    # the optional outputs may be NULL: with them null and everything else in order the next refusal is the workspace's
    refused("workspace too small", normals3=None, gravity=None, height=None, ws_bytes=0)


def test_op_refuses_the_cpu_and_bad_shapes():
    from mcdseg import ops
    cam = (500.0, 500.0, 320.0, 240.0)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.depth_to_hha(torch.ones(1, 4, 4), cam)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.depth_to_hha(torch.ones(1, 4, 4, dtype=torch.int32), cam, unit_m=0.001)
    with pytest.raises(TypeError, match=r"\[N,H,W\]"):
        ops.depth_to_hha(torch.ones(4, 4), cam)
    with pytest.raises(TypeError, match=r"\[N,H,W\]"):
        ops.depth_to_hha(torch.ones(1, 1, 4, 4), cam)
    with pytest.raises(TypeError, match=r"\[N,H,W\]"):
        ops.depth_to_hha(torch.ones(0, 4, 4), cam)
    with pytest.raises(TypeError, match=r"\[N,H,W\]"):
        ops.depth_to_hha(np.ones((1, 4, 4), np.float32), cam)
    with pytest.raises(TypeError, match="uint16, int32 or fp32"):
        ops.depth_to_hha(torch.ones(1, 4, 4, dtype=torch.float64), cam)
    with pytest.raises(TypeError, match="uint16, int32 or fp32"):
        ops.depth_to_hha(torch.ones(1, 4, 4, dtype=torch.int64), cam, unit_m=0.001)
    # the cameras: one for the batch or one per image
    assert list(ops._hha_cameras(cam, 3)) == list(cam) * 3
    assert list(ops._hha_cameras([[1, 2, 3, 4], [5, 6, 7, 8]], 2)) == [1, 2, 3, 4, 5, 6, 7, 8]
    assert list(ops._hha_cameras(torch.tensor([[1.0, 2, 3, 4]]), 1)) == [1, 2, 3, 4]
    for bad, n in (((1.0, 2.0, 3.0), 1), ([[1, 2, 3, 4]] * 3, 2), ((1, 2, 3, 4, 5), 1)):
        with pytest.raises(ValueError, match="one camera"):
            ops._hha_cameras(bad, n)


def test_pipeline_method_is_the_op(monkeypatch):
    import datasets
    from mcdseg import ops
    seen = {}

    def fake(depth, camera, unit_m=None, return_parts=False):
        seen.update(depth=depth, camera=camera, unit_m=unit_m, return_parts=return_parts)
        return "the part"

    monkeypatch.setattr(ops, "depth_to_hha", fake)
    pipe = datasets.DeviceInputPipeline(6, 41, torch.device("cpu"))
    d = torch.ones(1, 4, 4, dtype=torch.int32)
    assert pipe.hha(d, (1, 2, 3, 4), 0.001) == "the part"
    assert seen["depth"] is d and seen["camera"] == (1, 2, 3, 4) and seen["unit_m"] == 0.001 and seen["return_parts"] is False
    pipe.hha(d, (1, 2, 3, 4))
    assert seen["unit_m"] is None


def test_tool_parser_and_its_refusals(tmp_path):
    tool = _tool()
    a = tool.get_parser().parse_args(["depth", "out", "--camera", "518.8", "519.4", "325.5", "253.7"])
    assert (a.depth_dir, a.out_dir, a.camera, a.unit_m, a.batch_size) == ("depth", "out", [518.8, 519.4, 325.5, 253.7], 0.001, 1)
    a = tool.get_parser().parse_args(["depth", "out", "--camera", "1", "2", "3", "4", "--unit_m", "0.0002", "-b", "16"])
    assert (a.camera, a.unit_m, a.batch_size) == ([1, 2, 3, 4], 0.0002, 16)
    with pytest.raises(SystemExit):
        tool.get_parser().parse_args(["depth", "out"])  # --camera is required
    with pytest.raises(SystemExit, match="batch_size"):
        tool.main(["depth", "out", "--camera", "1", "2", "3", "4", "-b", "0"])
    with pytest.raises(SystemExit, match="positive"):
        tool.main(["depth", "out", "--camera", "0", "2", "3", "4"])
    with pytest.raises(SystemExit, match="positive"):
        tool.main(["depth", "out", "--camera", "1", "2", "3", "4", "--unit_m", "0"])
    from PIL import Image
    d = (np.arange(12, dtype=np.uint16).reshape(3, 4) * 5000)
    Image.fromarray(d).save(str(tmp_path / "d.png"))
    got = tool.read_depth(str(tmp_path / "d.png"))
    assert got.dtype == np.uint16 and np.array_equal(got, d)
    Image.fromarray(np.zeros((3, 4, 3), np.uint8)).save(str(tmp_path / "rgb.png"))
    with pytest.raises(ValueError, match="16-bit"):
        tool.read_depth(str(tmp_path / "rgb.png"))


def test_tool_without_a_gpu_is_a_system_exit(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="MI355X"):
        _tool().main([str(tmp_path), str(tmp_path / "out"), "--camera", "500", "500", "320", "240"])
    assert not os.path.exists(str(tmp_path / "out"))
