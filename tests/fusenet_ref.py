"""Plain-torch CPU restatement of the reference's ``FuseDRNSegBase`` (models/dilated_fcn.py:253-337) over the oracle's DRN modules
(oracle/ref_models.py, imported as they are), in fp32 or fp64 -- the middle fusion of ``--net drn_d_XX_fusenet``:

    x_d0 = main_layer0(hha); x_dk = main_layerk(x_d(k-1))            the HHA channels through the MAIN stages, first
    x = main_layer0(rgb) + x_d0; x = main_layerk(x) + x_dk           the RGB channels through the SAME modules
    return seg(x)

``sub_layer0`` .. ``sub_layer8`` are built and never called, as there.  tests/golden/make_fusenet_golden.py asserts this file against
the real reference class (1e-12 of each tensor's maximum, fp64) on the reduced DRN-D below and stores the results; the host tests
re-check it against those, the GPU tests hold ``models.dilated_fcn.FuseDRNSegBase`` to them.

The reduced DRN-D (``TINY``): BasicBlock, one block or convolution per stage, widths (16, 16, 24, 24, 32, 32, 32, 32) -- all multiples
of 8 and at least 16, so every stage output has a pre-split companion; a 16-wide full-resolution stage (the thin layers' window
kernels); projection shortcuts that stride (layer3, layer4) and that only widen (layer5), an identity shortcut (layer6)."""
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(HERE, "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import ref_models as RM  # noqa: E402
from recipe import fill_state_  # noqa: E402

TINY = dict(name="drn_d_tiny", channels=(16, 16, 24, 24, 32, 32, 32, 32), reps=(1, 1, 1, 1, 1, 1, 1, 1), n_class=7, seed=21,
            shape=(2, 6, 32, 40))
GOLDEN = os.path.join(HERE, "golden", "fusenet_small.npz")
CASES = ("train", "fix_bn", "eval")


def drn_d_stages(channels, reps, kind="basic"):
    """layer0 .. layer8 of a DRN-D with these widths (models/drn.py:125-157), from the oracle's stage builders"""
    ch = channels
    stages = [nn.Sequential(nn.Conv2d(3, ch[0], 7, padding=3, bias=False), nn.BatchNorm2d(ch[0]), nn.ReLU(inplace=True))]
    c = ch[0]
    s, c = RM._plain_stage(c, ch[0], reps[0]); stages.append(s)
    s, c = RM._plain_stage(c, ch[1], reps[1], stride=2); stages.append(s)
    s, c = RM._res_stage(kind, c, ch[2], reps[2], stride=2); stages.append(s)
    s, c = RM._res_stage(kind, c, ch[3], reps[3], stride=2); stages.append(s)
    s, c = RM._res_stage(kind, c, ch[4], reps[4], dilation=2, new_level=False); stages.append(s)
    s, c = RM._res_stage(kind, c, ch[5], reps[5], dilation=4, new_level=False); stages.append(s)
    s, c = RM._plain_stage(c, ch[6], reps[6], dilation=2); stages.append(s)
    s, c = RM._plain_stage(c, ch[7], reps[7], dilation=1); stages.append(s)
    return stages, c


class FuseDRNSegBase(nn.Module):
    def __init__(self, channels=RM.WIDTHS, reps=RM.ARCH["drn_d_22"][1], n_class=41, kind="basic"):
        super().__init__()
        main, c = drn_d_stages(channels, reps, kind)
        sub, _ = drn_d_stages(channels, reps, kind)
        for prefix, stages in (("main", main), ("sub", sub)):
            for k, s in enumerate(stages):
                setattr(self, "%s_layer%d" % (prefix, k), s)
        self.seg = RM._seg_head(c, n_class)
        RM.he_normal_(self)

    def forward(self, x):
        rgb, depth = x[:, :3], x[:, 3:]
        x_d = []
        for k in range(9):
            depth = getattr(self, "main_layer%d" % k)(depth)
            x_d.append(depth)
        x = rgb
        for k in range(9):
            x = torch.add(getattr(self, "main_layer%d" % k)(x), x_d[k])
        return self.seg(x)


def fix_batchnorm(model):
    """``fix_batchnorm_when_training`` (models/model_util.py:305-310)"""
    for m in model.modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            m.training = False


def rel_to_max(a, b):
    """max |a - b| relative to max |b|"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(float(np.abs(b).max()), 1e-300))


def tiny_inputs(spec=TINY, attempt=0):
    """(x [N,6,H,W], dy [N,n_class,H/8,W/8]) fp32: the two samples differ in gain and offset, RGB and HHA in spread"""
    rs = np.random.RandomState(1000 + spec["seed"] + 97 * attempt)
    n, c, h, w = spec["shape"]
    x = rs.standard_normal((n, c, h, w))
    x = x * np.array([1.0, 1.7]).reshape(n, 1, 1, 1) + np.array([0.2, -0.4]).reshape(n, 1, 1, 1)
    x[:, 3:] *= 0.6
    dy = rs.standard_normal((n, spec["n_class"], h // 8, w // 8)) / (n * (h // 8) * (w // 8))
    return x.astype(np.float32), dy.astype(np.float32)


def tiny_state(model, spec=TINY):
    """the recipe state of the reduced net (tests/golden/recipe.fill_state_, fp32 values whatever the model's dtype)"""
    sd = {k: (v.detach().float().cpu().clone() if v.dtype.is_floating_point else v.detach().cpu().clone())
          for k, v in model.state_dict().items()}

    class _Bag:  # (fill_state_ asks its argument for a state dict and fills the tensors in place)
        def state_dict(self):
            return sd
    fill_state_(_Bag(), spec["seed"])
    own = model.state_dict()
    model.load_state_dict({k: v.to(own[k].dtype) for k, v in sd.items()})
    return model


def run_case(model, case, x, dy, watch=None):
    """one of CASES on ``model`` (any implementation with the reference's state-dict keys, in its initial state): the score map, under
    the upstream gradient ``dy`` every main_layer* / seg gradient, and the running statistics afterwards, as float64 arrays.
    ``watch(module, input)``: a forward pre-hook for every BatchNorm (the golden's variance condition)."""
    p0 = next(model.parameters())
    x, dy = torch.as_tensor(x).to(p0.device, p0.dtype), torch.as_tensor(dy).to(p0.device, p0.dtype)
    model.train()
    if case == "fix_bn":
        fix_batchnorm(model)
    elif case == "eval":
        model.eval()
    hooks = [m.register_forward_pre_hook(watch) for m in model.modules() if isinstance(m, nn.BatchNorm2d)] if watch else []
    out = {}
    if case == "eval":
        with torch.no_grad():
            out["score"] = model(x)
    else:
        model.zero_grad()
        score = model(x)
        score.backward(dy)
        out["score"] = score.detach()
        for k, p in model.named_parameters():
            if p.grad is not None:
                out["grad/" + k] = p.grad
            else:
                assert k.startswith("sub_layer"), k
    for h in hooks:
        h.remove()
    for k, v in model.state_dict().items():
        if k.startswith("main_layer") and k.split(".")[-1] in ("running_mean", "running_var", "num_batches_tracked"):
            out["state/" + k] = v
    return {k: v.detach().double().cpu().numpy().copy() for k, v in out.items()}


def tiny_model(dtype=torch.float64, spec=TINY):
    return tiny_state(FuseDRNSegBase(spec["channels"], spec["reps"], spec["n_class"]).to(dtype), spec)


def register_tiny(spec=TINY):
    """the reduced DRN-D in the PROJECT's ``models.drn`` namespace, where its ``FuseDRNSegBase`` looks the constructor up; returns the name"""
    from models import drn

    def drn_d_tiny(pretrained=False, input_ch=3, **kw):
        return drn._build(drn.BasicBlock, list(spec["reps"]), "D", "drn-d-tiny", False, input_ch, channels=tuple(spec["channels"]), **kw)
    setattr(drn, spec["name"], drn_d_tiny)
    return spec["name"]


def load_golden(path=GOLDEN):
    fx = np.load(path)
    return fx, json.loads(str(fx["keys"]))
