"""What the U-Net tests and tests/golden/make_unet_golden.py share: the case of tests/golden/unet_small.npz, the recipe of its parameters
and inputs (nothing of either is stored: both are drawn from seeded generators), the one procedure that is run on the reference's
modules (CPU, fp32 and fp64) and on ``models.unet`` (GPU), and the rule by which a large tensor is stored.

The case: N = 2, 6 x 32 x 48, 5 classes, ``feature_scale=8`` -- 8, 16, 32, 64 and 128 channels, so both sides of the 16-channel rule of
the split-precision convolutions, and of the multiple-of-8 rule of the pre-split companions, are met."""
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "unet_small.npz")
KEYS = os.path.join(HERE, "golden", "unet_keys.json")
SPEC = dict(n=2, input_ch=6, h=32, w=48, n_class=5, feature_scale=8, fill_seed=91, input_seed=92, max_stored=2048)
FEATURES = ("center", "conv1", "conv2", "conv3", "conv4")
LOSSES = ("ce", "diff")


def fill_models(models, seed=SPEC["fill_seed"]):
    """every floating tensor of the state dicts of ``models`` (G, F1, F2, in this order) from ONE generator, in state-dict order: fp32
    draws, cast to the tensor's dtype -- the ``fill_decoder`` pattern of make_triple_golden.py"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in models:
            for k, v in m.state_dict().items():
                if k.endswith("num_batches_tracked"):
                    continue
                if k.endswith("running_var"):
                    t = torch.rand(v.shape, generator=g) + 0.5
                elif k.endswith("running_mean"):
                    t = 0.1 * torch.randn(v.shape, generator=g)
                elif v.dim() >= 2:  # convolutions [Cout, Cin, 3, 3] and up-convolutions [Cin, Cout, 2, 2]
                    t = torch.randn(v.shape, generator=g) * (1.0 / (v[0].numel() ** 0.5))
                elif k.endswith(".1.weight"):  # BatchNorm scale (the Sequential holders: conv 0, BatchNorm 1)
                    t = 1 + 0.1 * torch.randn(v.shape, generator=g)
                else:
                    t = 0.1 * torch.randn(v.shape, generator=g)
                v.copy_(t.to(v.dtype))
    return models


def inputs(spec=SPEC):
    """(x [N, C, H, W] fp32, labels [N, H, W] int64): the two samples differ in gain and offset"""
    g = torch.Generator().manual_seed(spec["input_seed"])
    n, c, h, w = spec["n"], spec["input_ch"], spec["h"], spec["w"]
    x = torch.randn((n, c, h, w), generator=g)
    x = x * torch.tensor([1.0, 1.6]).view(n, 1, 1, 1) + torch.tensor([0.2, -0.3]).view(n, 1, 1, 1)
    labels = torch.randint(0, spec["n_class"], (n, h, w), generator=g)
    return x, labels


def stored_index(numel, most=SPEC["max_stored"]):
    """the flat indices a tensor of ``numel`` elements is stored at: all of them up to ``most``, else arange(0, numel, ceil(numel / most))"""
    return None if numel <= most else np.arange(0, numel, math.ceil(numel / most))


def stored(t, most=SPEC["max_stored"]):
    a = np.asarray(t, dtype=np.float64)
    idx = stored_index(a.size, most)
    return a if idx is None else a.reshape(-1)[idx]


def rel_to_max(a, b, scale=None):
    """max |a - b| relative to max |b| -- or to ``scale`` where the truth is a sum whose terms cancel (the gradient of a convolution bias
    in front of a train-mode BatchNorm is zero in exact arithmetic: its scale is the largest per-channel sum of the terms' magnitudes,
    the rule of tests/dann_ref.rel_to_max)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    den = float(np.abs(b).max()) if scale is None else float(scale)
    return float(np.abs(a - b).max() / max(den, 1e-300))


def losses(o1, o2, labels):
    """CE(o1) + CE(o2) (F.cross_entropy for the removed NLLLoss2d, as the triple golden does) and mean |softmax(o1) - softmax(o2)|"""
    return {"ce": F.cross_entropy(o1, labels) + F.cross_entropy(o2, labels),
            "diff": torch.mean(torch.abs(F.softmax(o1, dim=1) - F.softmax(o2, dim=1)))}


def run(g, f1, f2, x, labels, scales=False):
    """``scales`` (plain torch modules only: it hooks the convolutions): also "scale/grad_<loss>/g.<conv>.bias" for every convolution of G,
    the largest per-channel sum of |gradient of the convolution's output| -- the terms whose sum that bias gradient is.

    One train-mode forward of G, F1, F2 and the gradients of both losses, on any implementation with the reference's module API:
    {name: float64 array, large gradients at ``stored_index``} with the names
      feat/<map>, o1, o2          the five feature maps and both logits (whole)
      state/<key>                 G's running statistics after ONE forward
      loss/ce, loss/diff
      grad_<loss>/x, grad_<loss>/g.<key>, .../f1.<key>, .../f2.<key>     (a parameter a loss does not reach: zeros)
    Each loss gets a forward pass of its own (train-mode BatchNorm normalises with batch statistics: the two passes agree)."""
    p0 = next(g.parameters())
    x, labels = x.to(p0.device, p0.dtype), labels.to(p0.device)
    named = [("g." + k, p) for k, p in g.named_parameters()] + [("f1." + k, p) for k, p in f1.named_parameters()] + \
            [("f2." + k, p) for k, p in f2.named_parameters()]
    for m in (g, f1, f2):
        m.train()
    out = {}
    for which in LOSSES:
        for m in (g, f1, f2):
            m.zero_grad()
        xx = x.clone().requires_grad_(True)
        hooks = []
        for name, m in (g.named_modules() if scales else ()):
            if isinstance(m, torch.nn.Conv2d):
                def hook(mod, gin, gout, key="scale/grad_%s/g.%s.bias" % (which, name)):
                    out[key] = gout[0].detach().double().abs().sum(dim=(0, 2, 3)).max().cpu().numpy().copy()
                hooks.append(m.register_full_backward_hook(hook))
        feats = g(xx)
        o1, o2 = f1(feats), f2(feats)
        vals = losses(o1, o2, labels)
        if which == LOSSES[0]:
            for k in FEATURES:
                out["feat/" + k] = feats[k].detach().double().cpu().numpy().copy()
            out["o1"], out["o2"] = o1.detach().double().cpu().numpy().copy(), o2.detach().double().cpu().numpy().copy()
            for k, v in g.state_dict().items():
                if k.split(".")[-1] in ("running_mean", "running_var", "num_batches_tracked"):
                    out["state/" + k] = v.detach().double().cpu().numpy().copy()
            for k, v in vals.items():
                out["loss/" + k] = v.detach().double().cpu().numpy().copy()
        vals[which].backward()
        for h in hooks:
            h.remove()
        out["grad_%s/x" % which] = stored(xx.grad.detach().double().cpu().numpy())
        for k, p in named:
            grad = p.grad if p.grad is not None else torch.zeros_like(p)
            out["grad_%s/%s" % (which, k)] = stored(grad.detach().double().cpu().numpy())
    return out


def keys_shapes(m):
    return [[k, list(v.shape)] for k, v in m.state_dict().items()]


def load_golden(path=GOLDEN):
    fx = np.load(path)
    return fx, json.loads(str(fx["units"]))


def load_keys(path=KEYS):
    with open(path) as fh:
        return json.load(fh)
