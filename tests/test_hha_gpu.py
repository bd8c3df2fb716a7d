"""GPU: ``ops.depth_to_hha`` (csrc/hha.hip) against the fp64 numpy oracle tests/hha_ref.py, computed here.

Bounds (tests/hha_ref.py ``float_bounds`` / ``byte_margins``; their honesty conditions are asserted on the CPU by
tests/test_hha_ref_host.py, where the deviation from the issue's 1e-4 clearance is explained):

* ``normals3``, ``gravity``, ``height``: ``rel_to_max`` to the fp64 oracle at most max(FLOOR, min(2 x the oracle's own fp32 run, CAP)).
  FLOOR = 2^-23 is the absolute floor for tensors whose fp32 unit is zero (the all-missing image: measured unit 0 for all three; the
  outputs are fp32, rounded once); CAP = 1e-6 is a tenth of the threshold clearance the scenes have (1e-5).  Measured fp32 units on
  the CPU: normals3 5e-6 ... 2.0, gravity 1e-7 ... 1e-5, height 2e-7 ... 1e-5 -- so every bound but the 8 x 12 gravity's (5.5e-7) is CAP.
* bytes: equal wherever the oracle's value before rounding is farther from a .5 boundary than the margin (the float bound of the channel
  in byte units; at most 2 % of a scene's pixels are nearer), and never more than 1 apart.

Measured on one MI355X: the three tensors 1.2e-8 ... 4.2e-8 from the oracle (0 on the all-missing image) -- the rounding of the fp32
outputs --, no byte differs on any scene (0 ... 174 pixels inside the margin).
"""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import hha_ref as R
from conftest import PKG

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(name):
    """(depth fp32 [N,H,W], cameras [N,4], per image (fp64 result, float bounds, byte margins)); computed once, never changed"""
    if name == "missing_beside_valid":
        d, c = R.case_depth("odd_37x53")
        depth, cams = np.concatenate([np.zeros_like(d), d]), np.concatenate([c, c])
    else:
        depth, cams = R.case_depth(name)
    depth.setflags(write=False)
    return depth, cams, [R.honesty(depth[k], cams[k])[4:] for k in range(len(depth))]


def _run(device, depth, cams, **kw):
    from mcdseg import ops
    out, parts = ops.depth_to_hha(torch.tensor(depth).to(device), cams, return_parts=True, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), {k: v.cpu().numpy() for k, v in parts.items()}


def _hold_to_the_oracle(name, out, parts):
    depth, cams, truth = _case(name)
    assert out.shape == depth.shape + (3,) and out.dtype == np.uint8
    for k, (r64, bounds, margins) in enumerate(truth):
        for key in ("normals3", "gravity", "height"):
            err = R.rel_to_max(parts[key][k], r64[key])
            print("%s[%d] %s: %.3g of the allowed %.3g" % (name, k, key, err, bounds[key]))
            assert err <= bounds[key], (name, k, key, err, bounds[key])
        sure = ~R.near_rounding(r64, margins)
        diff = np.abs(out[k].astype(np.int32) - r64["bytes"].astype(np.int32))
        print("%s[%d] bytes: %d of %d differ, %d inside the margin" % (name, k, (diff > 0).sum(), diff.size, (~sure).sum()))
        assert not diff[sure].any(), (name, k, np.argwhere(sure & (diff > 0))[:5].tolist())
        assert diff.max() <= 1
        assert not out[k][~r64["valid"]].any()


@pytest.mark.parametrize("name", ["clipped_8x12", "odd_37x53", "two_rooms_48x64", "noise_holes_96x128"])
def test_scenes_against_the_oracle(device, name):
    depth, cams, truth = _case(name)
    out, parts = _run(device, depth, cams)
    _hold_to_the_oracle(name, out, parts)
    if name == "noise_holes_96x128":
        r64 = truth[0][0]
        assert not r64["ok3"][44, 54] and not parts["normals3"][0][~r64["ok3"]].any()  # invalid inside the 9 x 9 hole: zeros
        assert (np.abs(np.linalg.norm(parts["normals3"][0][r64["ok3"]], axis=-1) - 1) < 1e-6).all()
    if name == "two_rooms_48x64":
        assert np.abs(parts["gravity"][0] - parts["gravity"][1]).max() > 0.05  # per-image g ...
        assert abs(truth[0][0]["y_min"] - truth[1][0]["y_min"]) > 20            # ... and per-image y_min


def test_all_missing_image_beside_a_valid_one(device):
    depth, cams, truth = _case("missing_beside_valid")
    out, parts = _run(device, depth, cams)
    _hold_to_the_oracle("missing_beside_valid", out, parts)
    assert not out[0].any() and parts["gravity"][0].tolist() == [0.0, 1.0, 0.0]
    assert not parts["normals3"][0].any() and not parts["height"][0].any()
    alone, alone_parts = _run(device, depth[1:], cams[1:])
    assert np.array_equal(out[1], alone[0])
    for k in alone_parts:
        assert np.array_equal(parts[k][1].view(np.int32), alone_parts[k][0].view(np.int32)), k


def test_depth_pointer_that_is_only_4_byte_aligned(device):
    from mcdseg import ops
    depth, cams, _ = _case("odd_37x53")
    want, want_parts = _run(device, depth, cams)
    buf = torch.empty(depth.size + 1, dtype=torch.float32, device=device)
    view = buf[1:].view(depth.shape)
    view.copy_(torch.tensor(depth))
    assert view.data_ptr() % 8 == 4 and view.is_contiguous()
    out, parts = ops.depth_to_hha(view, cams, return_parts=True)
    assert np.array_equal(out.cpu().numpy(), want)
    for k in want_parts:
        assert np.array_equal(parts[k].cpu().numpy().view(np.int32), want_parts[k].view(np.int32)), k


def test_same_bits_run_to_run_and_alone_or_in_a_batch(device):
    depth, cams, _ = _case("two_rooms_48x64")
    a, pa = _run(device, depth, cams)
    b, pb = _run(device, depth, cams)
    assert np.array_equal(a, b) and np.array_equal(pa["gravity"].view(np.int32), pb["gravity"].view(np.int32))
    for k in range(2):
        one, p1 = _run(device, depth[k:k + 1], cams[k:k + 1])
        assert np.array_equal(one[0], a[k]), k
        assert np.array_equal(p1["gravity"][0].view(np.int32), pa["gravity"][k].view(np.int32)), k
    one, p1 = _run(device, depth[:1], tuple(cams[0]))  # one camera for the batch
    assert np.array_equal(one[0], a[0])


def test_integer_depth_is_one_fp32_multiply(device):
    from mcdseg import ops
    depth, cams, _ = _case("odd_37x53")
    mm = np.round(depth * 10).astype(np.uint16)  # millimetres
    mm[0, 5, 7] = 0
    want, want_parts = ops.depth_to_hha(torch.from_numpy(mm.astype(np.float32)).to(device) * 0.1, cams, return_parts=True)
    assert not want[0, 5, 7].any() and want.any()
    for t in (torch.from_numpy(mm).to(device), torch.from_numpy(mm.astype(np.int32)).to(device)):
        got, parts = ops.depth_to_hha(t, cams, unit_m=0.001, return_parts=True)
        assert torch.equal(got, want), t.dtype
        for k in parts:
            assert torch.equal(parts[k].view(torch.int32), want_parts[k].view(torch.int32)), (t.dtype, k)
    metres = ops.depth_to_hha(torch.tensor(depth).to(device), cams, unit_m=0.01)  # fp32 with a unit: centimetres given as such
    assert torch.equal(metres, ops.depth_to_hha(torch.tensor(depth).to(device) * 1.0, cams))
    with pytest.raises(TypeError, match="unit_m"):
        ops.depth_to_hha(torch.from_numpy(mm.astype(np.int32)).to(device), cams)


def test_permuted_depth_is_read_through_its_strides(device):
    """a depth batch that is a permuted view ([H,W,N] storage) gives the bytes of its contiguous copy: with and without ``unit_m``, for
    every input type, through the op and through the pipeline"""
    import datasets
    from mcdseg import ops
    depth, cams, _ = _case("two_rooms_48x64")
    mm = np.round(depth * 10).astype(np.uint16)
    pipe = datasets.DeviceInputPipeline(6, 41, device)
    for src, unit in ((torch.tensor(depth), None), (torch.tensor(depth), 0.01), (torch.from_numpy(mm.astype(np.int32)), 0.001),
                      (torch.from_numpy(mm.copy()), 0.001)):
        dense = src.to(device)
        view = dense.permute(1, 2, 0).contiguous().permute(2, 0, 1)
        assert not view.is_contiguous() and torch.equal(view.double(), dense.double())
        want, want_parts = ops.depth_to_hha(dense, cams, unit_m=unit, return_parts=True)
        got, parts = ops.depth_to_hha(view, cams, unit_m=unit, return_parts=True)
        assert want.any() and torch.equal(got, want), (src.dtype, unit)
        for k in parts:
            assert torch.equal(parts[k].view(torch.int32), want_parts[k].view(torch.int32)), (src.dtype, unit, k)
        assert torch.equal(pipe.hha(view, cams, unit), want), (src.dtype, unit)
        assert torch.equal(pipe.hha(view.cpu(), cams, unit), want), (src.dtype, unit)


def test_memory_contract(device):
    """stock / 0xFF / 0x00 (tests/guards_hold.hold, 64 KiB guard bands): the output, the optional outputs and the workspace's first
    workspace_bytes keep inside their memory, and no result depends on what they held before"""
    from guards_hold import hold
    from mcdseg import ops
    for name in ("clipped_8x12", "two_rooms_48x64", "missing_beside_valid"):
        depth, cams, _ = _case(name)

        def encode(put):
            out, parts = ops.depth_to_hha(put(torch.tensor(depth)), cams, return_parts=True)
            plain = ops.depth_to_hha(put(torch.tensor(depth)), cams)
            return dict(parts, hha=out, hha_alone=plain)
        ref = hold(device, encode, workspace=True, family="depth_to_hha %s" % name)
        assert torch.equal(ref["hha"], ref["hha_alone"])


def test_tool_writes_what_the_op_gives(device, tmp_path, capsys):
    from PIL import Image
    from mcdseg import ops
    spec = importlib.util.spec_from_file_location("depth_to_hha_tool", os.path.join(PKG, "tools", "depth_to_hha.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    depth, cams, _ = _case("two_rooms_48x64")
    mm = np.round(depth * 10).astype(np.uint16)
    src, dst = tmp_path / "depth", tmp_path / "hha"
    os.makedirs(str(src))
    for k, name in enumerate(("a.png", "b.png")):
        Image.fromarray(mm[k]).save(str(src / name))
    cam = [float(c) for c in cams[0]]
    assert tool.main([str(src), str(dst), "--camera"] + [repr(c) for c in cam] + ["-b", "2"]) == str(dst)
    want, parts = ops.depth_to_hha(torch.from_numpy(mm.astype(np.int32)).to(device), cam, unit_m=0.001, return_parts=True)
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 2
    for k, name in enumerate(("a.png", "b.png")):
        png = np.array(Image.open(str(dst / name)))
        assert png.shape == (48, 64, 3) and png.dtype == np.uint8 and np.array_equal(png, want[k].cpu().numpy())
        g = parts["gravity"][k].tolist()
        assert lines[k] == "%s gravity %.6f %.6f %.6f" % (name, g[0], g[1], g[2])
    one_by_one = tmp_path / "hha1"
    tool.main([str(src), str(one_by_one), "--camera"] + [repr(c) for c in cam])
    for name in ("a.png", "b.png"):
        assert np.array_equal(np.array(Image.open(str(one_by_one / name))), np.array(Image.open(str(dst / name))))


def test_pipeline_takes_the_part(device):
    import datasets
    from mcdseg import ops
    depth, cams, _ = _case("two_rooms_48x64")
    pipe = datasets.DeviceInputPipeline(6, 41, device)
    rgb = torch.randint(0, 256, (2, 48, 64, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
    d = torch.tensor(depth)
    part = pipe.hha(d, cams)
    assert part.is_cuda and part.dtype == torch.uint8 and tuple(part.shape) == (2, 48, 64, 3)
    assert torch.equal(part, ops.depth_to_hha(d.to(device), cams))
    x = pipe.images(rgb, pipe.hha(d, cams))
    assert tuple(x.shape) == (2, 6, 48, 64) and x.dtype == torch.float32
    assert torch.equal(x, pipe.images(rgb, part.cpu()))
    mm = torch.from_numpy(np.round(depth * 10).astype(np.int32))
    assert torch.equal(pipe.hha(mm, cams, 0.001), ops.depth_to_hha(mm.to(device), cams, unit_m=0.001))
