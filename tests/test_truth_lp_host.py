"""Host: the low-precision yardsticks of BASELINE config 5's 2-byte chain (tests/golden/lowp.py, make_grad_truth.py --lp) -- the
straight-through rounder against a numpy restatement of the kernels' formats, its backward pass, the layer selection, and the
generator's --lp mode end to end at the --tiny size."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lowp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _np_f16s(x, bound):
    """numpy: fp16 (RNE) of x / s times s, s = 2^(e - 15) with frexp(bound) = (m, e)"""
    s = 2.0 ** (np.frexp(np.float64(bound))[1] - 15)
    return ((np.asarray(x, np.float32) / np.float32(s)).astype(np.float16).astype(np.float32) * np.float32(s)).astype(np.float32)


def _np_bf16(x):
    """numpy: bf16 with round-to-nearest-even on the fp32 bit pattern"""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16
    return u.astype(np.uint32).view(np.float32)


def test_scale_is_the_kernels_power_of_two():
    # frexp: bound = m 2^e, 0.5 <= m < 1 -- an exact power of two gets the NEXT exponent (2^e > bound strictly)
    assert lowp.scale_of(1.0) == 2.0 ** -14
    assert lowp.scale_of(0.75) == 2.0 ** -15
    assert lowp.scale_of(2.0 ** -20) == 2.0 ** -34
    assert lowp.scale_of(65504.0) == 2.0 ** 1
    assert lowp.scale_of(0.0) == 1.0 and lowp.scale_of(float("inf")) == 1.0 and lowp.scale_of(float("nan")) == 1.0


@pytest.mark.parametrize("bound", [1.0, 0.75, 3.0e-3, 2.0 ** -20, 1.7e4])
def test_f16s_matches_numpy_on_edge_values(bound):
    s = lowp.scale_of(bound)
    q = np.array([
        0.0, -0.0,
        2.0 ** 14, 2.0 ** 10, 1.0, 2.0 ** -14,            # exact powers of two (in units of s)
        bound / s, -bound / s,                           # the bound itself
        1024.5, 1025.5, 2047.5, -1024.5, -1025.5,        # ties to even (spacing 1 in [1024, 2048))
        1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11,          # ties to even (spacing 2^-10 in [1, 2))
        2.0 ** -15, 3 * 2.0 ** -25, 2.0 ** -25, 5 * 2.0 ** -26,   # fp16 subnormals after scaling, incl. ties and a flush to zero
        -(2.0 ** -15), -3 * 2.0 ** -25, 12345.678, -0.3333,
    ], dtype=np.float64)
    x = (q * s).astype(np.float32)
    x[x.size // 2] = np.float32(bound)  # (the tensor's max-abs: the bound the default scale comes from)
    x = np.clip(x, -bound, bound).astype(np.float32)
    got = lowp.round_f16s(torch.from_numpy(x)).numpy()
    ref = _np_f16s(x, np.abs(x).max())
    np.testing.assert_array_equal(got, ref)
    got_b = lowp.round_f16s(torch.from_numpy(x), bound=bound).numpy()
    np.testing.assert_array_equal(got_b, _np_f16s(x, bound))
    # hand-checked values at bound 1.0 (s = 2^-14): a tie goes to the even neighbour, the smallest subnormal's half flushes to zero
    if bound == 1.0:
        one = lambda v: float(lowp.round_f16s(torch.tensor([v, 1.0], dtype=torch.float32))[0])  # noqa: E731
        assert one(1024.5 * 2.0 ** -14) == 1024 * 2.0 ** -14
        assert one(1025.5 * 2.0 ** -14) == 1026 * 2.0 ** -14
        assert one(3 * 2.0 ** -39) == 2 * 2.0 ** -38      # 1.5 x the smallest subnormal (2^-24 s): tie -> 2 units
        assert one(2.0 ** -39) == 0.0                      # half the smallest subnormal: tie -> 0
        assert one(-(2.0 ** -14)) == -(2.0 ** -14)
        assert one(-0.0) == 0.0 and np.signbit(one(-0.0))


def test_bf16_matches_numpy_on_edge_values():
    x = np.array([0.0, -0.0, 1.0, -2.0, 2.0 ** -126, 2.0 ** -130, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8),
                  3.0e38, 1.2345e-20, -7.654321], dtype=np.float32)
    got = lowp.round_bf16(torch.from_numpy(x)).numpy()
    np.testing.assert_array_equal(got, _np_bf16(x))
    assert got[6] == 1.0 and got[7] == 1.0 + 2.0 ** -6 and got[8] == -1.0  # ties to even


def test_round_backward_rounds_the_gradient():
    torch.manual_seed(0)
    x = torch.randn(4, 8, 5, 5, requires_grad=True)
    g = torch.randn(4, 8, 5, 5) * 1e-3
    g[0, 0, 0, 0] = 1.0 + 2.0 ** -8  # (a tie of bf16)
    for fwd, bwd, expect in (("f16s", "bf16", lowp.round_bf16(g)), ("f16s", "f16s", lowp.round_f16s(g)), ("f16s", None, g),
                             (None, "bf16", lowp.round_bf16(g))):
        x.grad = None
        y = lowp.rnd(x, fwd, bwd)
        np.testing.assert_array_equal(y.detach().numpy(), (lowp.round_f16s(x) if fwd else x).detach().numpy())
        y.backward(g)
        np.testing.assert_array_equal(x.grad.numpy(), expect.numpy())
        if bwd is not None:
            assert not torch.equal(x.grad, g)  # where the chain rounds a gradient, the backward pass is NOT the identity


def test_chain_model_selects_the_half_layers():
    from oracle import ref_models
    import torch.nn as nn
    g = ref_models.get_models("drn_d_105", 6, 41)[0]
    lowp.chain_model(g)
    convs = [(n, m) for n, m in g.base.named_modules() if isinstance(m, nn.Conv2d)]
    patched = {n for n, m in convs if "forward" in vars(m)}
    assert patched == {n for n, m in convs if m.in_channels > 16 or n == "2.0"}, sorted(patched)
    assert "forward" not in vars(g.seg)  # the 41-class head stays fp32
    assert len([n for n, m in convs if m.in_channels > 16]) == 99 + 4 + 2  # 33 Bottlenecks x 3, their 4 shortcuts, layer7, layer8


def test_committed_lp_fixture_matches_its_truth():
    fx = np.load(os.path.join(GOLDEN, "grad_truth_cfg5n2.npz"))
    lp = np.load(os.path.join(GOLDEN, "grad_truth_cfg5n2_lp.npz"))
    names = [str(n) for n in fx["names"]]
    assert [str(n) for n in lp["names"]] == names and str(lp["recipe"]) == str(fx["recipe"])
    for k in names:
        for key in ("dmodel", "damp", "nmodel", "namp"):
            assert np.isfinite(float(lp["%s/%s" % (k, key)])) and float(lp["%s/%s" % (k, key)]) > 0, (k, key)
    assert "Cin > 16" in str(lp["recipe_model"]) and "bfloat16" in str(lp["recipe_amp"])


def test_make_grad_truth_lp_tiny_end_to_end(tmp_path):
    script = os.path.join(GOLDEN, "make_grad_truth.py")
    env = dict(os.environ, OMP_NUM_THREADS=os.environ.get("OMP_NUM_THREADS", "4"))
    subprocess.run([sys.executable, script, "--tiny", "--out", str(tmp_path), "cfg5n2"], check=True, env=env, timeout=600)
    before = (tmp_path / "grad_truth_cfg5n2.npz").read_bytes()
    subprocess.run([sys.executable, script, "--tiny", "--lp", "--out", str(tmp_path), "cfg5n2"], check=True, env=env, timeout=600)
    assert (tmp_path / "grad_truth_cfg5n2.npz").read_bytes() == before  # the fp64 fixture is read, never rewritten
    fx = np.load(tmp_path / "grad_truth_cfg5n2.npz")
    lp = np.load(tmp_path / "grad_truth_cfg5n2_lp.npz")
    names = [str(n) for n in fx["names"]]
    expect = {"recipe", "names", "recipe_model", "recipe_amp", "loss_model", "loss_amp", "feat/e_model", "feat/e_amp", "logits1/e_model",
              "logits1/e_amp"} | {"%s/%s" % (k, key) for k in names for key in ("dmodel", "damp", "nmodel", "namp")}
    assert set(lp.files) == expect, sorted(set(lp.files) ^ expect)[:10]
    assert all(np.isfinite(float(lp[k])) for k in expect if not k.startswith(("recipe", "names")))
