"""GPU: ``ops.fill_depth`` (csrc/fill.hip) against the fp64 numpy/scipy oracle tests/fill_ref.py, computed here.

What is asserted of the device's fp64 solution x, per image, with the ORACLE's matrix M and right-hand side b:

* the status is ``converged`` (``empty`` for the image without a known pixel, whose output is all zero);
* ||b - M x||_2 <= 1.01 rtol ||b||_2: the device stops on the true residual; the 1 % covers the two sides' fp64 summation orders
  (about 1e-16 ||M|| ||x|| against 1e-10 ||b||);
* ||x - x*||_inf <= ||M^-1 1||_inf (||b - M x||_inf + ||b - M x*||_inf) with x* the sparse LU's solution: M^-1 >= 0, so this is a
  theorem, not a measured number (tests/test_fill_ref_host.py holds the oracle's own iteration to it);
* the weights within 1e-12 absolute of the oracle's (the exponent is at most 30 in magnitude: a few ulp of exp and of its argument stay
  below 1e-14), zmax bit-equal.

The iteration counts of the two sides are printed side by side; their equality is not asserted (the dot products are summed in other orders).
"""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import fill_ref as R
from conftest import PKG

pytestmark = pytest.mark.gpu

RTOL = 1e-10


def _tool(name):
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(PKG, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(device, rgb, depth, **kw):
    """(filled fp32 [N,H,W], parts) as numpy"""
    from mcdseg import ops
    out, parts = ops.fill_depth(torch.tensor(rgb).to(device), torch.tensor(depth).to(device),
                                return_parts=True, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), {k: v.cpu().numpy() for k, v in parts.items()}


@functools.lru_cache(maxsize=None)
def _default_run(name):
    """the default call on a case, once"""
    rgb, depth = R.case(name)
    return _run(torch.device("cuda", torch.cuda.current_device()), rgb, depth)


def _bits(a):
    return np.ascontiguousarray(a).view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


@pytest.mark.parametrize("name", list(R.CASES))
def test_against_the_oracles_system(device, name):
    rgb, depth = R.case(name)
    out, parts = _default_run(name)
    assert out.shape == depth.shape and out.dtype == np.float32 and parts["x"].dtype == np.float64
    assert parts["weights"].shape == (len(depth), 8) + depth.shape[1:]
    for k in range(len(depth)):
        t = R.truth(name, k)
        assert _bits(parts["zmax"][k:k + 1])[0] == _bits(np.array([t["zmax"]]))[0], (name, k)
        werr = np.abs(parts["weights"][k] - t["weights"]).max()
        print("%s[%d] weights: %.3g from the oracle's" % (name, k, werr))
        assert werr <= 1e-12
        if t["zmax"] == 0.0:
            assert parts["status"][k] == R.EMPTY and parts["iterations"][k] == 0 and not out[k].any() and not parts["x"][k].any()
            continue
        assert parts["status"][k] == R.CONVERGED, (name, k, parts["status"][k], parts["iterations"][k], parts["residual"][k])
        M, b = t["M"], t["b"]
        x = parts["x"][k].reshape(-1)
        r, r_star = b - M @ x, b - M @ t["x_star"]
        res, bn = np.linalg.norm(r), np.linalg.norm(b)
        err, bound = np.abs(x - t["x_star"]).max(), t["minv"] * (np.abs(r).max() + np.abs(r_star).max())
        print("%s[%d]: iterations device %d / oracle %d; residual %.3g (the device's own figure %.3g) of the allowed %.3g; |x - x*| = %.3g of "
              "the allowed %.3g" % (name, k, parts["iterations"][k], t["it"][2], res / bn, parts["residual"][k], 1.01 * RTOL, err, bound))
        assert res <= 1.01 * RTOL * bn
        assert err <= bound
        assert parts["iterations"][k] % 8 == 0 and 0 < parts["iterations"][k] <= 4000
        assert np.isfinite(out[k]).all() and (out[k] > 0).all()


@pytest.mark.parametrize("name", ["odd_37x53", "missing_beside_valid", "row_1x40"])
def test_fp32_output_and_keep_known(device, name):
    rgb, depth = R.case(name)
    out, parts = _default_run(name)
    want = (parts["x"] * parts["zmax"][:, None, None]).astype(np.float32)
    assert np.array_equal(_bits(out), _bits(want))
    kept, kparts = _run(device, rgb, depth, keep_known=True)
    known = R.known_mask(depth)
    assert np.array_equal(_bits(kept[known]), _bits(depth[known])) and np.array_equal(_bits(kept[~known]), _bits(out[~known]))
    assert np.array_equal(_bits(kparts["x"]), _bits(parts["x"]))
    from mcdseg import ops
    plain = ops.fill_depth(torch.tensor(rgb).to(device), torch.tensor(depth).to(device))
    assert torch.is_tensor(plain) and np.array_equal(_bits(plain.cpu().numpy()), _bits(out))


@pytest.mark.parametrize("name", ["two_48x64", "missing_beside_valid"])
def test_same_bits_run_to_run_and_alone_or_in_a_batch(device, name):
    rgb, depth = R.case(name)
    a, pa = _default_run(name)
    b, pb = _run(device, rgb, depth)
    assert np.array_equal(_bits(a), _bits(b))
    for key in pa:
        assert np.array_equal(_bits(pa[key]), _bits(pb[key])), key
    if name == "two_48x64":
        assert abs(int(pa["iterations"][0]) - int(pa["iterations"][1])) >= 8, pa["iterations"]  # one image was frozen beside a running one
    for k in range(len(depth)):
        one, p1 = _run(device, rgb[k:k + 1], depth[k:k + 1])
        assert np.array_equal(_bits(p1["x"][0]), _bits(pa["x"][k])), k
        assert np.array_equal(_bits(one[0]), _bits(a[k])), k
        assert p1["iterations"][0] == pa["iterations"][k] and p1["status"][0] == pa["status"][k], k
        assert _bits(p1["residual"])[0] == _bits(pa["residual"][k:k + 1])[0], k


def test_iteration_limit_is_a_status_not_an_exception(device):
    rgb, depth = R.case("holes_96x128")
    out, parts = _run(device, rgb, depth, max_iter=8)
    assert parts["status"].tolist() == [R.NOT_CONVERGED] and parts["iterations"].tolist() == [8]
    assert np.isfinite(out).all() and np.isfinite(parts["x"]).all() and np.isfinite(parts["residual"]).all() and parts["residual"][0] > RTOL
    out, parts = _run(device, rgb, depth, max_iter=12, check_every=5)  # the last call is cut to the limit
    assert parts["status"].tolist() == [R.NOT_CONVERGED] and parts["iterations"].tolist() == [12]
    out, parts = _run(device, rgb, depth, max_iter=0)
    assert parts["status"].tolist() == [R.NOT_CONVERGED] and parts["iterations"].tolist() == [0]
    t = R.truth("holes_96x128", 0)
    assert np.array_equal(_bits(parts["x"][0].reshape(-1)), _bits(t["b"] / t["D"]))  # x0 = b / D, bit for bit
    assert _default_run("holes_96x128")[1]["status"].tolist() == [R.CONVERGED]


def test_input_types_strides_and_alignment(device):
    from mcdseg import ops
    rgb, depth = R.case("two_48x64")
    t_rgb = torch.tensor(rgb).to(device)
    mm = np.round(depth * 10).astype(np.uint16)  # millimetres
    want, wp = ops.fill_depth(t_rgb, torch.from_numpy(mm.astype(np.float32)).to(device) * 0.1, return_parts=True)
    assert (wp["status"] == ops.FILL_CONVERGED).all()
    for t in (torch.from_numpy(mm).to(device), torch.from_numpy(mm.astype(np.int32)).to(device)):
        got, gp = ops.fill_depth(t_rgb, t, unit_m=0.001, return_parts=True)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), t.dtype
        assert torch.equal(gp["x"].view(torch.int64), wp["x"].view(torch.int64)) and torch.equal(gp["iterations"], wp["iterations"])
    with pytest.raises(TypeError, match="unit_m"):
        ops.fill_depth(t_rgb, torch.from_numpy(mm.astype(np.int32)).to(device))
    with pytest.raises(TypeError, match="uint8 RGB batch"):
        ops.fill_depth(t_rgb[:, :, :, :2], torch.tensor(depth).to(device))
    with pytest.raises(TypeError, match="uint8 RGB batch"):
        ops.fill_depth(t_rgb.float(), torch.tensor(depth).to(device))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.fill_depth(t_rgb.cpu(), torch.tensor(depth).to(device))
    with pytest.raises(ValueError, match="positive and finite"):
        ops.fill_depth(t_rgb, torch.tensor(depth).to(device), rtol=0.0)
    with pytest.raises(ValueError, match="at least 2 pixels"):
        ops.fill_depth(t_rgb[:1, :1, :1], torch.ones(1, 1, 1, device=device))
    # a permuted view and a pointer that is only 4-byte aligned give the contiguous run's bits
    want, wp = _default_run("two_48x64")
    dense = torch.tensor(depth).to(device)
    view = dense.permute(1, 2, 0).contiguous().permute(2, 0, 1)
    assert not view.is_contiguous()
    rgb_view = t_rgb.permute(3, 0, 1, 2).contiguous().permute(1, 2, 3, 0)
    assert not rgb_view.is_contiguous()
    got, gp = ops.fill_depth(rgb_view, view, return_parts=True)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)) and np.array_equal(_bits(gp["x"].cpu().numpy()), _bits(wp["x"]))
    buf = torch.empty(depth.size + 1, dtype=torch.float32, device=device)
    odd = buf[1:].view(depth.shape)
    odd.copy_(dense)
    assert odd.data_ptr() % 8 == 4 and odd.is_contiguous()
    got, gp = ops.fill_depth(t_rgb, odd, return_parts=True)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)) and np.array_equal(_bits(gp["x"].cpu().numpy()), _bits(wp["x"]))


def test_max_valid_cm_makes_the_clipped_pixels_missing(device):
    rgb, depth = R.case("odd_37x53")
    known = R.known_mask(depth)
    far = float(np.sort(depth[known])[-40])
    zeroed = np.where(depth < far, depth, 0).astype(np.float32)
    assert (zeroed > 0).sum() == known.sum() - 40
    got, gp = _run(device, rgb, depth, max_valid_cm=far)
    want, wp = _run(device, rgb, zeroed)
    assert gp["status"].tolist() == [R.CONVERGED] and gp["zmax"][0] < far
    for key in gp:
        assert np.array_equal(_bits(gp[key]), _bits(wp[key])), key
    assert np.array_equal(_bits(got), _bits(want))
    assert not np.array_equal(_bits(got), _bits(_default_run("odd_37x53")[0]))
    kept, _ = _run(device, rgb, depth, max_valid_cm=far, keep_known=True)  # a clipped pixel is not a known one: it is filled
    clipped = known & (depth >= far)
    assert np.array_equal(_bits(kept[clipped]), _bits(got[clipped])) and np.array_equal(_bits(kept[zeroed > 0]), _bits(depth[zeroed > 0]))


def test_memory_contract(device):
    """stock / 0xFF / 0x00 (tests/guards_hold.hold, 64 KiB guard bands): the outputs and the workspace's first workspace_bytes keep inside
    their memory, and no result depends on what they held before"""
    from guards_hold import hold
    from mcdseg import ops
    for name in ("clipped_8x12", "two_48x64", "missing_beside_valid"):
        rgb, depth = R.case(name)

        def fill(put):
            out, parts = ops.fill_depth(put(torch.tensor(rgb)), put(torch.tensor(depth)), return_parts=True)
            plain = ops.fill_depth(put(torch.tensor(rgb)), put(torch.tensor(depth)))
            return dict(parts, filled=out, filled_alone=plain)
        ref = hold(device, fill, workspace=True, family="fill_depth %s" % name)
        assert torch.equal(ref["filled"].view(torch.int32), ref["filled_alone"].view(torch.int32))
        assert np.array_equal(_bits(ref["filled"].cpu().numpy()), _bits(_default_run(name)[0]))


def test_pipeline_fills_then_encodes(device):
    import datasets
    from mcdseg import ops
    import hha_ref
    rgb, depth = R.case("holes_96x128")
    cams = hha_ref.default_camera(96, 128)
    pipe = datasets.DeviceInputPipeline(6, 41, device)
    t_rgb, t_depth = torch.tensor(rgb), torch.tensor(depth)
    got = pipe.hha(t_depth, cams, fill_rgb=t_rgb)
    want = ops.depth_to_hha(ops.fill_depth(t_rgb.to(device), t_depth.to(device)), cams)
    assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got, want)
    assert not bool((got == 0).all(dim=-1).any())  # no (0,0,0) pixel is left
    raw = ops.depth_to_hha(t_depth.to(device), cams)
    assert bool((raw == 0).all(dim=-1).any()) and torch.equal(pipe.hha(t_depth, cams), raw)
    mm = torch.from_numpy(np.round(depth * 10).astype(np.int32))
    assert torch.equal(pipe.hha(mm, cams, 0.001, fill_rgb=t_rgb, keep_known=True),
                       ops.depth_to_hha(ops.fill_depth(t_rgb.to(device), mm.to(device), unit_m=0.001, keep_known=True), cams))


def test_tools_write_what_the_ops_give(device, tmp_path, capsys):
    from PIL import Image
    from mcdseg import ops
    import hha_ref
    rgb, depth = R.case("two_48x64")
    mm = np.round(depth * 10).astype(np.uint16)
    src, img, dst = tmp_path / "depth", tmp_path / "rgb", tmp_path / "filled"
    os.makedirs(str(src))
    os.makedirs(str(img))
    for k, name in enumerate(("a.png", "b.png")):
        Image.fromarray(mm[k]).save(str(src / name))
        Image.fromarray(rgb[k], "RGB").save(str(img / name))
    t_rgb, t_mm = torch.tensor(rgb).to(device), torch.from_numpy(mm.astype(np.int32)).to(device)
    filled, parts = ops.fill_depth(t_rgb, t_mm, unit_m=0.001, return_parts=True)
    units = np.clip(np.floor(filled.cpu().numpy().astype(np.float64) / (100.0 * 0.001) + 0.5), 0, 65535).astype(np.uint16)

    tool = _tool("fill_depth")
    assert tool.main([str(src), str(img), str(dst), "-b", "2"]) == str(dst)
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 2
    for k, name in enumerate(("a.png", "b.png")):
        png = np.array(Image.open(str(dst / name)))
        assert png.shape == (48, 64) and png.dtype == np.uint16 and np.array_equal(png, units[k]) and (png > 0).all()
        assert lines[k] == "%s %d %.3e converged" % (name, int(parts["iterations"][k]), float(parts["residual"][k]))
    one_by_one = tmp_path / "filled1"
    tool.main([str(src), str(img), str(one_by_one)])
    for name in ("a.png", "b.png"):
        assert np.array_equal(np.array(Image.open(str(one_by_one / name))), np.array(Image.open(str(dst / name))))
    capsys.readouterr()
    with pytest.raises(SystemExit) as stop:  # an image at its limit: every file is still written, then exit status 1
        tool.main([str(src), str(img), str(tmp_path / "short"), "--max_iter", "8", "-b", "2"])
    assert stop.value.code == 1 and sorted(os.listdir(str(tmp_path / "short"))) == ["a.png", "b.png"]
    assert [ln.split()[-1] for ln in capsys.readouterr().out.strip().splitlines()] == ["not_converged"] * 2

    hha_tool = _tool("depth_to_hha")
    cam = [float(c) for c in hha_ref.default_camera(48, 64)]
    args = [str(src), str(tmp_path / "hha_fill"), "--camera"] + [repr(c) for c in cam] + ["-b", "2"]
    hha_tool.main(args + ["--fill", str(img)])
    lines = capsys.readouterr().out.strip().splitlines()
    want, hp = ops.depth_to_hha(filled, cam, return_parts=True)  # the filled centimetres, not the 16-bit values
    for k, name in enumerate(("a.png", "b.png")):
        assert np.array_equal(np.array(Image.open(str(tmp_path / "hha_fill" / name))), want[k].cpu().numpy())
        g = hp["gravity"][k].tolist()
        assert lines[k] == "%s gravity %.6f %.6f %.6f fill %d %.3e converged" % (name, g[0], g[1], g[2], int(parts["iterations"][k]),
                                                                                float(parts["residual"][k]))
    args[1] = str(tmp_path / "hha_raw")
    hha_tool.main(args)
    lines = capsys.readouterr().out.strip().splitlines()
    raw, rp = ops.depth_to_hha(t_mm, cam, unit_m=0.001, return_parts=True)
    for k, name in enumerate(("a.png", "b.png")):
        assert np.array_equal(np.array(Image.open(str(tmp_path / "hha_raw" / name))), raw[k].cpu().numpy())
        g = rp["gravity"][k].tolist()
        assert lines[k] == "%s gravity %.6f %.6f %.6f" % (name, g[0], g[1], g[2])
