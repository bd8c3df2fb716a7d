"""GPU: the fused inference tails of csrc/infer.hip against the unfused composition of the library's own kernels (bit for bit)
and against CPU torch + numpy."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from infer_tail_ref import unnormalize_u8

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


CASES = [(16, 41, 60, 80, 40), (1, 41, 8, 12, 41), (3, 19, 7, 9, 19)]


@pytest.mark.parametrize("learned", [True, False], ids=["up8", "bilinear8"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_fused_predict_equals_up_sampling_then_predict(case, learned):
    dev = _dev()
    from mcdseg import ops
    n, c, hi, wi, used = case
    g = torch.Generator().manual_seed(hi * 100 + c)
    s = (torch.randn(n, c, hi, wi, generator=g) * 3).to(dev)
    w = (torch.randn(c, 1, 16, 16, generator=g) * 0.1).to(dev) if learned else None
    with torch.no_grad():
        z = ops.up8(s, w) if learned else ops.bilinear8(s)
        ref_lab, ref_ent = ops.predict_labels(z, None, used)
        del z
        lab, ent = ops.predict_labels_up8(s, w, used) if learned else ops.predict_labels_bilinear8(s, used)
    assert lab.dtype == torch.uint8 and tuple(lab.shape) == (n, 8 * hi, 8 * wi)
    assert torch.equal(lab, ref_lab)
    assert int(lab.max()) < used
    assert abs(float(ent) - float(ref_ent)) <= 1e-6 * abs(float(ref_ent))


@pytest.mark.parametrize("learned", [True, False], ids=["up8", "bilinear8"])
def test_fused_predict_does_not_store_the_logits(learned):
    dev = _dev()
    from mcdseg import ops
    n, c, hi, wi = 16, 41, 60, 80
    s = torch.randn(n, c, hi, wi, device=dev)
    w = torch.randn(c, 1, 16, 16, device=dev) * 0.1 if learned else None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    lab, ent = ops.predict_labels_up8(s, w, c - 1) if learned else ops.predict_labels_bilinear8(s, c - 1)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated(dev) - base
    logits = n * c * 64 * hi * wi * 4  # 806 MB
    assert grew < logits // 100, (grew, logits)  # the labels (4.9 MB) and a few KB of partial sums


def _depth_input(n, cd, hi, wi, seed, special=True):
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(n, cd, hi, wi, generator=g) * 1.5
    d[torch.rand(n, cd, hi, wi, generator=g) < 0.1] *= 40  # far outside [0, 255] after scaling: wraps
    if special:
        d[0, 0, 1, 1], d[0, 0, 2, 5], d[-1, -1, hi - 1, wi - 1], d[-1, 0, hi // 2, 0] = float("nan"), float("inf"), -float("inf"), 3.6e7
    return d


@pytest.mark.parametrize("cd", [3, 1])
@pytest.mark.parametrize("shape", [(2, 8, 12), (3, 7, 9), (1, 60, 80)], ids=lambda s: "x".join(map(str, s)))
def test_depth_image_equals_the_numpy_tail_of_bilinear8(cd, shape):
    dev = _dev()
    from mcdseg import ops
    n, hi, wi = shape
    d = _depth_input(n, cd, hi, wi, seed=hi * 7 + cd)
    with torch.no_grad():
        img = ops.depth_image_u8(d.to(dev)).cpu().numpy()
        up = ops.bilinear8(d.to(dev)).cpu().numpy()
    assert img.shape == (n, 8 * hi, 8 * wi, 3) and img.dtype == np.uint8
    ref = unnormalize_u8(up.transpose(0, 2, 3, 1))
    assert np.array_equal(img, ref), int((img != ref).sum())
    assert (img == 0).mean() < 0.5 and len(np.unique(img)) > 200


@pytest.mark.parametrize("cd", [3, 1])
def test_depth_image_against_cpu_interpolate(cd):
    """bytes differ from CPU F.interpolate + numpy's own cast only where the two fp32 up-sampled values differ"""
    dev = _dev()
    from mcdseg import ops
    d = _depth_input(2, cd, 9, 13, seed=77 + cd)
    with torch.no_grad():
        img = ops.depth_image_u8(d.to(dev)).cpu().numpy()
        gpu_up = ops.bilinear8(d.to(dev)).cpu().numpy().transpose(0, 2, 3, 1)
    cpu_up = F.interpolate(d, scale_factor=8, mode="bilinear", align_corners=False).numpy().transpose(0, 2, 3, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        ref = np.uint8(((cpu_up.astype(np.float64) * np.array([.229, .224, .225])) + np.array([.485, .456, .406])) * 255)
    same = (gpu_up == cpu_up) | (np.isnan(gpu_up) & np.isnan(cpu_up))
    if cd == 1:
        same = np.broadcast_to(same, img.shape)
    assert same.mean() > 0.3
    assert np.array_equal(img[same], ref[same])
