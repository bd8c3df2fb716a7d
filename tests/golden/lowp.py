"""Low-precision yardsticks of BASELINE config 5's 2-byte chain (test infrastructure: imports nothing of the product).

The chain (``bench.py --dtype f16``: CONV_MATH=f16x1, compact storage, ops.HALF_STORAGE; include/mcdseg.h "2-byte activation storage")
is held to the fp64 truth in units of what its FORMATS cost, measured on the CPU oracle:

* ``model``: the fp32 oracle with the chain's roundings inserted through the straight-through ``Round``, only where the kernels store
  or multiply a 16-bit value (``MODEL_RECIPE``);
* ``amp``: the oracle under ``torch.autocast("cpu", dtype=torch.bfloat16)``, what a PyTorch user means by "bf16" (``amp_recipe``).

Used by make_grad_truth.py --lp (the full-size fixture grad_truth_cfg5n2_lp.npz) and tests/test_model_gpu.py (the toy-size test).
"""
import functools
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

MODEL_RECIPE = (
    "fp32 oracle + straight-through roundings of the f16x1 2-byte chain; f16s = fp16 RNE of x / s times s, s = 2^(e-15) with "
    "frexp(max|x|) = (m, e) (csrc/split.h mcd_scale_of_bound), bf16 = RNE.  Convolutions of G's trunk with Cin > 16 (ops.py's half "
    "predicate: not the stem, layer1, layer2, not the 41-class head): operands x, w -> f16s (one-term MFMA on the leading companion "
    "piece); z -> f16s (z16) except at the trunk's last layer (fp32 output); dz -> f16s as the dgrad and wgrad operand; the gradient "
    "of x -> bf16 where x is an activation of the chain (not layer2's output, read by layer3.0's conv1 and shortcut).  Bottleneck and "
    "shortcut outputs -> f16s (the one-piece activation the residual add reads), their gradients -> bf16.  layer2 (16 -> 32, stride 2, "
    "no window kernel): forward and data gradient on the one-term GEMM, operands f16s; its weight gradient (thin_tr kernel) and the "
    "stem and layer1 (window, direct and thin_tr kernels: both companion pieces, 22 bits) stay fp32.  BatchNorm arithmetic, residual "
    "adds, the seg head, F1 / F2 and the loss: fp32")


def scale_of(bound):
    """2^(e - 15) with bound = m 2^e, 0.5 <= m < 1 (csrc/split.h mcd_scale_of_bound; 1 for a zero or non-finite bound)"""
    b = float(bound)
    if not (b > 0.0) or not (b <= 3.0e38):
        return 1.0
    _, e = math.frexp(b)
    return 2.0 ** max(-100, min(100, e - 15))


def round_f16s(t, bound=None):
    """the leading piece of an F16X3 / F16X1 companion: fp16 (RNE) of t / s, times s; s from ``bound`` (default: max |t|)"""
    if t.numel() == 0:
        return t.clone()
    s = scale_of(t.detach().abs().max() if bound is None else bound)
    return ((t.float() / s).half().float() * s).to(t.dtype)


def round_bf16(t):
    return t.bfloat16().to(t.dtype)


FORMATS = {None: lambda t: t.clone(), "f16s": round_f16s, "bf16": round_bf16}


class Round(torch.autograd.Function):
    """straight-through rounder: the forward pass rounds x to the format ``fwd``, the backward pass rounds the arriving gradient to
    ``bwd`` (None: passes it on unchanged)"""

    @staticmethod
    def forward(ctx, x, fwd, bwd):
        ctx.bwd = bwd
        return FORMATS[fwd](x)

    @staticmethod
    def backward(ctx, g):
        return FORMATS[ctx.bwd](g), None, None


def rnd(x, fwd, bwd=None):
    return Round.apply(x, fwd, bwd)


class _OneTermFwdDgrad(torch.autograd.Function):
    """a thin convolution whose forward pass and data gradient run the one-term GEMM (operands f16s) and whose weight gradient runs a
    kernel that multiplies both companion pieces (kept fp32)"""

    @staticmethod
    def forward(ctx, x, w, geom):
        ctx.save_for_backward(x, w)
        ctx.geom = geom
        return F.conv2d(round_f16s(x), round_f16s(w), None, *geom)

    @staticmethod
    def backward(ctx, dz):
        x, w = ctx.saved_tensors
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.nn.grad.conv2d_input(x.shape, round_f16s(w), round_f16s(dz), *ctx.geom)
        if ctx.needs_input_grad[1]:
            dw = torch.nn.grad.conv2d_weight(x, w.shape, dz, *ctx.geom)
        return dx, dw, None


def _chain_conv(m, x_bwd, z_fwd, x):
    z = F.conv2d(rnd(x, "f16s", x_bwd), rnd(m.weight, "f16s"), m.bias, m.stride, m.padding, m.dilation)
    return rnd(z, z_fwd, "f16s")


def _one_term_conv(m, x):
    return _OneTermFwdDgrad.apply(x, m.weight, (m.stride, m.padding, m.dilation))


def _round_output(mod, inp, out):
    return rnd(out, "f16s", "bf16")


def chain_model(g):
    """insert the 2-byte chain's roundings (MODEL_RECIPE) into the oracle generator ``g`` (oracle.ref_models.DRNSegBase of a Bottleneck
    DRN-D) in place"""
    base = g.base
    convs = [m for m in base.modules() if isinstance(m, nn.Conv2d)]
    first = base[3][0]  # the first Bottleneck: its input, layer2's output, is not an activation of the chain
    fed_by_layer2 = {first.conv1, first.downsample[0]}
    for m in convs:
        if m.in_channels > 16:
            m.forward = functools.partial(_chain_conv, m, None if m in fed_by_layer2 else "bf16", None if m is convs[-1] else "f16s")
        elif m.stride[0] != 1:
            m.forward = functools.partial(_one_term_conv, m)
    for stage in base[3:7]:
        for blk in stage:
            blk.register_forward_hook(_round_output)
            if blk.downsample is not None:
                blk.downsample.register_forward_hook(_round_output)
    return g


def amp_recipe(feat, logits, params):
    """what autocast did in a run (``feat``, ``logits``: G's and F1's outputs; ``params``: the parameters after backward)"""
    name = lambda dt: str(dt).replace("torch.", "")  # noqa: E731
    grads = "/".join(sorted({name(p.grad.dtype) for p in params if p.grad is not None}))
    return ("oracle forward under torch.autocast('cpu', dtype=torch.bfloat16), backward outside it: Conv2d, BatchNorm2d, ReLU and the "
            "ConvTranspose2d heads compute in bf16 (G's output %s, F1's %s); parameters stay fp32, their gradients are %s; the loss as "
            "autocast computes it" % (name(feat.dtype), name(logits.dtype), grads))
