#!/usr/bin/env python3
"""Generate the fixtures of the segmentation + depth + boundary ("triple") multitask variant by running the REAL reference in memory,
the way make_golden.py does (same loader: lib2to3 on the reference's text, nothing copied).

    python tests/golden/make_triple_golden.py            # needs the reference checkout make_golden.py loads

Case: N = 2, 16 x 24, 5 classes.  Written:
  triple_keys.json   state-dict key lists (with shapes) of MCDTripleMultiTaskDecoder, one per combination of
                     add_pred_seg_boundary_loss / use_seg2bd_conv
  triple_small.npz   inputs (h2 / h3 / h8, labels, an HHA target, a {0,1} boundary target), the stored conv1/2/3 and seg2bd_conv
                     parameters, and the reference's results in train mode, each in fp32 ("f32/...") and fp64 ("f64/..."):
                       z1, z2               the two segmentation decoders' 1/8-resolution outputs (the seg2bd kernel's inputs)
                       forward              the four outputs of MCDTripleMultiTaskDecoder.forward
                       boundary_forward
                       boundary_loss        get_boundary_loss with the given target
                       extra_gt, extra_none get_boundary_loss_by_extra_conv(separately_returning=True) with the target and with None
                       loss_parts           get_loss(separately_returning=True)
                       d_h8, d_seg2bd_w, d_seg2bd_b   gradients of get_boundary_loss_by_extra_conv(x, target) (both heads summed)

The four ThreeLayerDecoders hold 9.5 M parameters, far beyond a fixture: ``fill_decoder`` draws every tensor of the state dict from one
seeded torch.Generator in state-dict order, and a test that builds the decoder here draws the same ones (the key lists above pin the
order).  conv1/2/3 and seg2bd_conv are stored all the same, for the tests that need no decoder.

What the installed torch does not run, and what was done instead:
  * the trainer's criterion is CrossEntropyLoss2d over nn.NLLLoss2d, which torch removed: ``get_loss`` ran with
    ``F.cross_entropy`` (unweighted, mean) as ``semseg_criterion``.
  * ``get_semseg_loss`` under add_pred_seg_boundary_loss calls ``.cuda()`` on its extra losses: it does not run on a CPU, and is not
    captured.  Its parts are get_boundary_loss(pred_type="semseg") of segbd_small.npz and the criterion.
  * ``get_psuedo_boundary_loss`` raises TypeError (it passes ``pred_semseg=`` to a function whose parameter is ``pred``): nothing to
    capture.
The edge arithmetic recorded here is that of the installed torch's F.binary_cross_entropy (logs clamped at -100), not torch 0.4's.
"""
import itertools
import json
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import load_reference  # noqa: E402

N, H, W, NC = 2, 16, 24, 5
FILL_SEED = 77


def fill_decoder(dec, seed=FILL_SEED):
    """every tensor of ``dec.state_dict()`` from one generator, in state-dict order (fp32 draws, cast to the tensor's dtype)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in dec.state_dict().items():
            if k.endswith("num_batches_tracked"):
                continue
            if k.endswith("running_var"):
                t = torch.rand(v.shape, generator=g) + 0.5
            elif k.endswith("bn.weight"):
                t = 1 + 0.1 * torch.randn(v.shape, generator=g)
            elif v.dim() >= 2:
                t = torch.randn(v.shape, generator=g) * (1.0 / (v[0].numel() ** 0.5))
            elif k.startswith("s_"):
                t = 1 + 0.3 * torch.randn(v.shape, generator=g)
            else:
                t = 0.1 * torch.randn(v.shape, generator=g)
            v.copy_(t.to(v.dtype))


def main():
    warnings.simplefilter("ignore")
    _, _, dfcn, _, _ = load_reference()
    keys = {}
    for pred, s2b in itertools.product((False, True), (False, True)):
        dec = dfcn.MCDTripleMultiTaskDecoder(NC, 3, add_pred_seg_boundary_loss=pred, use_seg2bd_conv=s2b)
        keys["pred%d_seg2bd%d" % (pred, s2b)] = [[k, list(v.shape)] for k, v in dec.state_dict().items()]
    with open(os.path.join(HERE, "triple_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)

    g = torch.Generator().manual_seed(21)
    feats = {"h2": torch.randn(N, 32, H // 2, W // 2, generator=g), "h3": torch.randn(N, 64, H // 4, W // 4, generator=g),
             "h8": torch.randn(N, 512, H // 8, W // 8, generator=g) * 0.2}
    coarse = torch.randint(0, NC, (N, 1, H // 4, W // 4), generator=g).float()
    labels = F.interpolate(coarse, size=(H, W), mode="nearest")[:, 0].long()
    gt_dep = torch.randn(N, 3, H, W, generator=g)
    v = labels.float()[:, None]
    gt_bd = (F.max_pool2d(v, 3, 1, 1) != -F.max_pool2d(-v, 3, 1, 1)).float()  # [N,1,H,W] in {0,1}, as datasets.py:680-695 yields it
    assert 0 < float(gt_bd.mean()) < 1

    out = {k: t.numpy() for k, t in feats.items()}
    out.update(labels=labels.numpy(), gt_dep=gt_dep.numpy(), gt_bd=gt_bd.numpy())
    dec = dfcn.MCDTripleMultiTaskDecoder(NC, 3, semseg_criterion=lambda p, t: F.cross_entropy(p, t), use_seg2bd_conv=True)
    fill_decoder(dec)
    for name in ("conv1", "conv2", "conv3", "seg2bd_conv"):
        conv = getattr(dec, name)
        out[name + ".weight"], out[name + ".bias"] = conv.weight.detach().numpy().copy(), conv.bias.detach().numpy().copy()
    state = {k: t.clone() for k, t in dec.state_dict().items()}
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        dec.load_state_dict(state)  # (train-mode forwards move the running statistics: every dtype starts from the same ones)
        dec.to(dt).train()
        x = {k: t.to(dt) for k, t in feats.items()}
        with torch.no_grad():
            out[tag + "/z1"] = dec.semsegcls_dec1(x["h8"]).numpy()
            out[tag + "/z2"] = dec.semsegcls_dec2(x["h8"]).numpy()
            for k, t in enumerate(dec(x)):
                out[tag + "/forward%d" % k] = t.numpy()
            out[tag + "/boundary_forward"] = dec.boundary_forward(x).numpy()
            out[tag + "/boundary_loss"] = dec.get_boundary_loss(x, gt_bd.to(dt)).numpy()
            out[tag + "/extra_gt"] = np.stack([t.numpy() for t in dec.get_boundary_loss_by_extra_conv(x, gt_bd.to(dt), True)])
            out[tag + "/extra_none"] = np.stack([t.numpy() for t in dec.get_boundary_loss_by_extra_conv(x, None, True)])
            out[tag + "/loss_parts"] = np.stack([t.numpy().reshape(()) for t in dec.get_loss(x, labels, gt_dep.to(dt), gt_bd.to(dt), True)])
        x["h8"] = x["h8"].clone().requires_grad_()
        loss = dec.get_boundary_loss_by_extra_conv(x, gt_bd.to(dt))
        grads = torch.autograd.grad(loss, [x["h8"], dec.seg2bd_conv.weight, dec.seg2bd_conv.bias])
        out[tag + "/d_h8"], out[tag + "/d_seg2bd_w"], out[tag + "/d_seg2bd_b"] = (t.numpy() for t in grads)
    assert out["f64/forward3"].shape == (N, 1, H, W) and out["f64/z1"].shape == (N, NC, H // 8, W // 8)
    np.savez_compressed(os.path.join(HERE, "triple_small.npz"), **out)
    print({k: (t.shape if t.ndim else float(t)) for k, t in out.items() if "/" in k})
    print("wrote triple_small.npz (%d bytes), triple_keys.json" % os.path.getsize(os.path.join(HERE, "triple_small.npz")))


if __name__ == "__main__":
    main()
