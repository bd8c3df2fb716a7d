"""Host restatements of the inference tails, in torch-CPU and numpy only (nothing of ``mcdseg``):

* the depth-image tail of adapt_multitask_tester.py:148-155 (transform.py:285-294, ``unnormalize``): the rule
  ``mcdseg_depth_image_u8`` implements, written out in numpy without calling numpy's own float -> uint8 cast;
* the argmax / entropy tail of adapt_tester.py:104-124 and util.py:44-48 in float64 (``predict_truth``), with the two x8
  up-samplers that precede it in the multitask and source-only testers (``bilinear8_truth``, ``up8_truth``).
  ``tests/test_infer_tail_ref_host.py`` checks these statements themselves."""
import numpy as np
import torch
import torch.nn.functional as F

MEAN = np.array([.485, .456, .406])  # transform.py:287-288 (not the training transform's statistics)
STD = np.array([.229, .224, .225])


def numpy_u8(t):
    """np.uint8(t) of a float64 array on x86-64: truncate toward zero to int32 and keep the low 8 bits; NaN, +-inf and values
    outside the int32 range give 0."""
    t = np.asarray(t, dtype=np.float64)
    ok = (t > -2147483649.0) & (t < 2147483648.0)  # False for NaN
    return np.where(ok, np.trunc(np.where(ok, t, 0.0)).astype(np.int64) & 255, 0).astype(np.uint8)


def unnormalize_u8(hwc):
    """float32 [..., H, W, Cd] (Cd = 1 or 3) -> uint8 [..., H, W, 3]: (v * STD + MEAN) * 255 in float64, each operation rounded
    (numpy's promotion of the float32 map against the float64 constants), Cd = 1 broadcast into three channels"""
    return numpy_u8(((np.asarray(hwc, dtype=np.float32).astype(np.float64) * STD) + MEAN) * 255.0)


def bilinear8_truth(s):
    """MCDMultiTaskDecoder.upsample in float64: [N,C,Hi,Wi] -> [N,C,8Hi,8Wi]"""
    return F.interpolate(s.detach().cpu().double(), scale_factor=8, mode="bilinear", align_corners=False)


def up8_truth(s, w):
    """DRNSeg.up (ConvTranspose2d(C, C, 16, stride=8, padding=4, groups=C, bias=False)) in float64; w: [C,1,16,16]"""
    return F.conv_transpose2d(s.detach().cpu().double(), w.detach().cpu().double(), stride=8, padding=4, groups=s.shape[1])


def predict_truth(z1, z2, n_used):
    """(labels uint8 [N,H,W], entropy python float, margin float64 [N,H,W]) of logits z1 (and z2, or None), all in float64:
    o = z1 or (z1 + z2)/2; label = the FIRST index of the maximum over o[:, :n_used] (adapt_tester.py:121-124, ``max(0)[1]``);
    entropy = -mean(p log(p + 1e-6)) over all C classes and all pixels, p = softmax(o, 1) (util.py:44-48); margin = largest minus
    second-largest of o[:, :n_used] per pixel (0 at a tie, +inf where n_used = 1)."""
    o = z1.detach().cpu().double()
    if z2 is not None:
        o = (o + z2.detach().cpu().double()) / 2
    n, c, h, w = o.shape
    assert 1 <= n_used <= c
    ou = o[:, :n_used]
    top = ou.max(1, keepdim=True)[0]
    # first maximal index, written out (no argmax, whose choice among equals is the library's business): every later index
    # that attains the maximum is replaced by n_used before the minimum is taken
    idx = torch.arange(n_used).view(1, n_used, 1, 1).expand_as(ou)
    labels = torch.where(ou == top, idx, torch.full_like(idx, n_used)).min(1)[0]
    assert int(labels.max()) < n_used
    if n_used == 1:
        margin = torch.full((n, h, w), float("inf"), dtype=torch.float64)
    else:
        two = ou.topk(2, dim=1)[0]
        margin = two[:, 0] - two[:, 1]
    p = torch.softmax(o, 1)
    entropy = float(-(p * torch.log(p + 1e-6)).mean())
    return labels.to(torch.uint8), entropy, margin
