#!/usr/bin/env python3
"""Generate the fixtures of the segmentation + boundary ("segbd") multitask variant by running the REAL reference in memory, the
way make_golden.py does (same loader: lib2to3 on the reference's text, nothing copied).

    python tests/golden/make_segbd_golden.py            # needs /root/reference

Case: N = 2, 16 x 24, 5 classes.  Written:
  segbd_keys.json    state-dict key lists (with shapes) of MCDSegBDMultiTaskDecoder -- plain and with add_pred_seg_boundary_loss --
                     and of MultiTaskEncoderReturningMultipleFeaturemaps('drn_d_22')
  segbd_small.npz    inputs and the reference's outputs, each in fp32 ("f32/...") and fp64 ("f64/..."):
                       boundary_forward   of a decoder whose conv1/2/3 are stored, on stored h2 / h3 / h8
                       get_boundary       of a label map (the nested function of get_boundary_loss, taken from its code object)
                       bce2d              on a hard {0,1} target and on a soft target
                       get_boundary_loss  pred_type "semseg" (two label maps) and pred_type "boundary" (a probability map)

What the installed torch does not run, and how it was captured instead:
  * ``get_boundary_loss(pred_type="boundary")`` hands F.binary_cross_entropy an [N,1,H,W] input with an [N,H,W] target, which the torch
    of the reference's day took and today's refuses: that call is fed the label map as [N,1,H,W] (max_pool2d takes either).
  * ``MCDSegBDMultiTaskDecoder.get_semseg_loss`` / ``get_loss`` add get_boundary_loss(pred.max(1)[1], gt) to an NLLLoss2d criterion
    (removed from torch) and ``loss.data[0]`` style reads: not captured as a whole.  Their parts are: the criterion (loss_small.npz,
    make_golden.py), the arg-max boundary loss (the "semseg" case here) and the exp(-s) L + s weighting, which tests restate.
  * ``get_task_weights`` reads the non-existent ``s_deprgr`` and raises: nothing to capture.
The edge arithmetic recorded here is that of the installed torch's F.binary_cross_entropy (logs clamped at -100), not torch 0.4's.
"""
import json
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import load_reference  # noqa: E402

N, H, W, NC = 2, 16, 24, 5


def main():
    warnings.simplefilter("ignore")
    ref_loss, drn, dfcn, _, _ = load_reference()
    g = torch.Generator().manual_seed(20)
    keys = {}
    for tag, kw in (("decoder", {}), ("decoder_pred_seg_boundary", {"add_pred_seg_boundary_loss": True})):
        dec = dfcn.MCDSegBDMultiTaskDecoder(NC, 3, **kw)
        keys[tag] = [[k, list(v.shape)] for k, v in dec.state_dict().items()]
    enc = dfcn.MultiTaskEncoderReturningMultipleFeaturemaps("drn_d_22", pretrained=False, input_ch=3)
    keys["encoder_drn_d_22"] = [[k, list(v.shape)] for k, v in enc.state_dict().items()]
    with open(os.path.join(HERE, "segbd_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)

    # the nested get_boundary of get_boundary_loss, rebuilt from its code object with the reference module's globals
    code = [c for c in dfcn.get_boundary_loss.__code__.co_consts if isinstance(c, types.CodeType) and c.co_name == "get_boundary"][0]
    get_boundary = types.FunctionType(code, dfcn.__dict__)

    out = {}
    dec = dfcn.MCDSegBDMultiTaskDecoder(NC, 3)
    for name in ("conv1", "conv2", "conv3"):
        conv = getattr(dec, name)
        conv.weight.data.copy_(torch.randn(conv.weight.shape, generator=g) * 0.3)
        conv.bias.data.copy_(torch.randn(conv.bias.shape, generator=g))
        out[name + ".weight"], out[name + ".bias"] = conv.weight.detach().numpy().copy(), conv.bias.detach().numpy().copy()
    feats = {"h2": torch.randn(N, 32, H // 2, W // 2, generator=g), "h3": torch.randn(N, 64, H // 4, W // 4, generator=g),
             "h8": torch.randn(N, 512, H // 8, W // 8, generator=g) * 0.2}
    coarse = torch.randint(0, NC, (N, 1, H // 4, W // 4), generator=g).float()
    lab_a = torch.nn.functional.interpolate(coarse, size=(H, W), mode="nearest")[:, 0].long()
    lab_b = torch.roll(lab_a, shifts=(1, 2), dims=(1, 2))
    lab_b[:, 5:9, 7:15] = 3
    p = torch.rand(N, 1, H, W, generator=g) * 0.98 + 0.01
    soft = torch.rand(N, 1, H, W, generator=g) ** 3
    out.update({k: v.numpy() for k, v in feats.items()})
    out.update(lab_a=lab_a.numpy(), lab_b=lab_b.numpy(), p=p.numpy(), soft=soft.numpy())

    out["get_boundary"] = get_boundary(lab_a).numpy().astype(np.uint8)
    assert out["get_boundary"].shape == (N, H, W) and 0 < out["get_boundary"].mean() < 1
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        dec.to(dt)
        with torch.no_grad():
            out[tag + "/boundary_forward"] = dec.boundary_forward({k: v.to(dt) for k, v in feats.items()}).numpy()
            hard = get_boundary(lab_a)[:, None].to(dt)
            out[tag + "/bce2d_hard"] = ref_loss.bce2d(p.to(dt), hard).numpy()
            out[tag + "/bce2d_soft"] = ref_loss.bce2d(p.to(dt), soft.to(dt)).numpy()
            out[tag + "/boundary_loss_semseg"] = dfcn.get_boundary_loss(lab_b, lab_a).to(dt).numpy()
            out[tag + "/boundary_loss_boundary"] = dfcn.get_boundary_loss(pred=p.to(dt), gt=lab_a[:, None], pred_type="boundary").numpy()
            out[tag + "/boundary_loss_gt_boundary"] = dfcn.get_boundary_loss(pred=lab_b[:, None], gt=soft.to(dt), gt_type="boundary").numpy()
    assert out["f64/boundary_forward"].shape == (N, 1, H, W)
    np.savez_compressed(os.path.join(HERE, "segbd_small.npz"), **out)
    print({k: (v.shape if v.ndim else float(v)) for k, v in out.items() if "/" in k})
    print("wrote segbd_small.npz (%d bytes), segbd_keys.json" % os.path.getsize(os.path.join(HERE, "segbd_small.npz")))


if __name__ == "__main__":
    main()
