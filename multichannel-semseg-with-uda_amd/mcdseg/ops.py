"""torch.autograd wrappers around the libmcdseg kernels.

PyTorch supplies device memory, the current HIP stream and the autograd tape; every arithmetic
pass over activations, gradients and parameters below is a hand-written HIP kernel.  The functions
mirror the ATen call sites of the reference's hot path:

  conv_bn_act      nn.Conv2d + nn.BatchNorm2d + ReLU (+ residual)   models/drn.py:43-59, 80-100, 195-205
  stage_join       torch.add between two stage outputs (+ the next stage's operand)   models/dilated_fcn.py:308-328
  max_pool2        nn.MaxPool2d(kernel_size=2) (+ the next convolution's operand)     models/unet.py:135-159
  up_join          torch.cat([shortcut, ConvTranspose2d k2 s2 (h)], 1)                models/unet.py:38-43
  relu             nn.ReLU behind a convolution without BatchNorm                     models/unet.py:18-21
  conv2d_bias      nn.Conv2d with bias (the 1x1 ``seg`` head)       models/dilated_fcn.py:226-232
  up8 / up8_dual   depthwise ConvTranspose2d k16 s8 p4              models/dilated_fcn.py:357-366, 479-491
  cross_entropy2d  log_softmax + weighted NLL                       loss.py:7-13
  diff2d           mean |softmax - softmax|                         loss.py:93-100
  mcd_losses       both of the above in one fused kernel            adapt_trainer.py:163-212
  prob_distance    the other distances of --d_loss (jsd, symkl, ...) loss.py:66-189
  up8_uncertain_loss  the T Monte-Carlo dropout passes of UncertainDRNSeg.get_loss in one kernel   models/dilated_fcn.py:169-214
  up8_std_sum      the uncertain tester's map, sum_c relu(up_std(s))   source_uncertain_tester.py:158-166
"""
import collections
import contextlib
import ctypes
import os
import threading
import types
import weakref

import torch

from . import _lib
from ._lib import ConvDesc, check, get_option, lib

# bumped by the optimizer after every in-place parameter update (the kernels write through raw
# pointers, so torch's own version counters do not move)
WEIGHT_EPOCH = 0


def bump_weight_epoch(params=None):
    """an in-place parameter update happened: of ``params`` (each carries its own counter, so that stepping one optimizer does not
    invalidate the packed images of another's parameters), or -- None -- of anything"""
    global WEIGHT_EPOCH
    if params is None:
        WEIGHT_EPOCH += 1
        return
    for p in params:
        p._mcd_epoch = getattr(p, "_mcd_epoch", 0) + 1


# Optional launch timer (bench.py): an object with ``wants(name) -> bool`` and ``add(name, work, start, stop)``.
# When set, the named kernel launches are bracketed by HIP events recorded on the launch stream.
LAUNCH_TIMER = None


class _timed:
    def __init__(self, name, work):
        self.on = LAUNCH_TIMER is not None and LAUNCH_TIMER.wants(name)
        self.name, self.work = name, work

    def __enter__(self):
        if self.on:
            self.t0 = torch.cuda.Event(enable_timing=True)
            self.t1 = torch.cuda.Event(enable_timing=True)
            self.t0.record()

    def __exit__(self, *exc):
        if self.on:
            self.t1.record()
            LAUNCH_TIMER.add(self.name, self.work, self.t0, self.t1)


def conv_work(desc):
    """(algorithmic FLOPs, algorithmic bytes) of one conv pass: 2*MACs; input read once + output written once."""
    macs = desc.N * desc.Ho * desc.Wo * desc.Cout * desc.Cin * desc.KH * desc.KW
    byts = 4 * (desc.N * desc.Cin * desc.H * desc.W + desc.N * desc.Cout * desc.Ho * desc.Wo)
    return 2 * macs, byts


POLICY = {"f16x3": "SplitF16x3", "bf16x6": "SplitBf16x6", "f16x1": "SplitF16x1"}


def gemm_kernel_name(m, k, dgrad, split=False, presplit=False, direct=False, pixels=0, math=None):
    """Template instantiation conv_fprop / conv_dgrad dispatch to (the launcher's own rule through
    ``mcdseg_conv_split_tile_config``; csrc/common.h mcd_bm / mcd_bk for the f32 kernels); the string equals the kernel name
    rocprofv3 prints, so profiles/*_pmc_traffic.json can be keyed by it."""
    bm = 32 if m <= 32 else (64 if m <= 64 else 128)
    cfg = {128: "2, 2, 2, 2", 64: "2, 2, 1, 4", 32: "1, 2, 1, 4"}[bm]
    if split and direct:
        return "conv_stem_x6_kernel"
    if split:
        code = "%04d" % lib().mcdseg_conv_split_tile_config(int(m), int(pixels), int(bool(presplit)))
        return "conv_gemm_split_kernel<%s, %s, %s, %s>" % (POLICY[math or CONV_MATH], ", ".join(code), "true" if dgrad else "false",
                                                           "true" if presplit else "false")
    return "conv_gemm_kernel<%s, %d, %s>" % (cfg, 8 if k <= 8 else 16, "true" if dgrad else "false")


def pingpong_kernel_name(dgrad, math=None, small=False, wide=0, deep=False):
    """rocprofv3's name of the 8-wave ping-pong kernel (csrc/conv_gemm_split_pp.hip): its 256 x 256 tile, the 256 x 128 one
    (``small``), the 256 x 320 one (``wide`` = 1), the 128 x 320 one (2) or the 256 x 160 one (3: what ``mcdseg_conv_split_wide_pingpong`` returns).
    ``deep`` (``mcdseg_conv_split_pp_deep``; never on the 256 x 128 tile): the one-term arithmetic with two K-steps per barrier interval"""
    tile = {0: "2, 2, 2, 2" if small else "4, 2, 1, 4", 1: "2, 5, 2, 2", 2: "1, 5, 2, 2", 3: "1, 5, 4, 1"}[int(wide)]
    policy = POLICY[math or CONV_MATH] + ("D" if (deep and not (small and not wide) and (math or CONV_MATH) == "f16x1") else "")
    return "conv_gemm_split_pp_kernel<%s, %s, %s>" % (policy, "true" if dgrad else "false", tile)


def _split_launches(d, presplit, dgrad, name, call, work=None):
    """One split-arithmetic convolution as the library would launch it, each kernel bracketed by its own timer: the pixels
    ``mcdseg_conv_split_parts`` gives to the ping-pong kernel (part 1) and the rest on the 4-wave tiles (part 2); ``call(part)``
    invokes the ``_part`` entry point.  Work is shared out by pixels."""
    if LAUNCH_TIMER is None:  # nobody asks which kernels ran: one call, the library launches both parts itself (and the host saves
        call(0)               # the plan queries below -- 700 convolutions per MCD step)
        return
    def plan():  # the library's answers, asked once per (descriptor, arithmetic, presplit, dgrad): part 1's pixels and kernel, part 2's
        L, r, m, g = lib(), ctypes.byref(d), MATH_ID[CONV_MATH], int(dgrad)
        pp = L.mcdseg_conv_split_parts(r, m, 1, g) if presplit else 0
        first = pingpong_kernel_name(dgrad, wide=L.mcdseg_conv_split_wide_pingpong(r, m, 1, g), deep=bool(L.mcdseg_conv_split_pp_deep(r, m, g))) \
            if pp > 0 else None
        rest = presplit and pp < pixels and L.mcdseg_conv_split_rest_pingpong(r, m, 1, g)
        return pp, first, pingpong_kernel_name(dgrad, small=True) if rest else None
    pixels = d.N * (d.H * d.W if dgrad else d.Ho * d.Wo)
    pp, first, rest = _memo(d, ("split", bool(presplit), bool(dgrad)), plan)
    flops, byts = (work or conv_work)(d)
    if pp > 0:
        with _timed(first, (flops * pp / pixels, byts * pp / pixels)):
            call(1)
    if pp < pixels:
        with _timed(rest or (name() if callable(name) else name), (flops * (pixels - pp) / pixels, byts * (pixels - pp) / pixels)):
            call(2 if pp > 0 else 0)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# the stream the next kernels are launched on when it is not torch's current one: the side stream while _conv_backward enqueues a
# weight gradient there.  torch's CURRENT stream stays the main one meanwhile, so every tensor still comes from the main stream's
# allocator pool, and whatever those kernels touch is collected in ``keep``: the caller holds the list until the main stream has
# waited for the side stream, which makes the memory reusable at once.  (Tensor.record_stream instead would return it only when
# the side stream has passed the point in WALL-CLOCK time; the host enqueues a whole backward pass ahead of the device, so the
# allocator kept growing -- 27 -> 116 GB reserved for drn_d_105 at N = 8 -- and cfg5 at N = 32, 232 of 288 GB, fell into its
# free-everything-and-retry path: 14-18 s per step instead of 3.8 s.)
class _LaunchStream(threading.local):  # (per thread: the autograd engine runs backward nodes on one worker thread per device)
    stream = None
    keep = None


_LAUNCH = _LaunchStream()


def _stream():
    s = _LAUNCH.stream
    return ctypes.c_void_p((s if s is not None else torch.cuda.current_stream()).cuda_stream)


def _on_launch_stream(*tensors):
    """tensors just handed to kernels on the launch stream: their memory must not be reused before those kernels have run"""
    if _LAUNCH.stream is not None:
        _LAUNCH.keep.extend(t for t in tensors if t is not None)


def _req(t, name, dtype=torch.float32):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("mcdseg: %s must live on the GPU -- the HIP kernels are the only implementation "
                           "(no CPU fallback)" % name)
    if t.dtype != dtype:
        raise TypeError("mcdseg: %s must be %s, got %s" % (name, dtype, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 4) // 4 + 1, dtype=torch.float32, device=device)


def conv_desc(x_shape, w_shape, stride, pad, dil):
    n, cin, h, w = x_shape
    cout, cin_w, kh, kw = w_shape
    if cin_w != cin:
        raise ValueError("mcdseg: conv expects %d input channels, got %d" % (cin_w, cin))
    ho = (h + 2 * pad - dil * (kh - 1) - 1) // stride + 1
    wo = (w + 2 * pad - dil * (kw - 1) - 1) // stride + 1
    return ConvDesc(n, cin, h, w, cout, kh, kw, stride, pad, dil, ho, wo)


# Matrix-pipe arithmetic of the convolutions (MCDSEG_CONV_MATH), csrc/split.h:
#   "f16x3" (default)   fp32 operands as s * (h1 + h2): two fp16 pieces and a power-of-two scale per tensor, three cross terms
#                       on v_mfma_f32_32x32x16_f16 -- fp32-grade against the reference's fp64 gradients (same noise-floor
#                       test as the other modes) at 5.3x the f32 matrix rate;
#   "bf16x6"            three bf16 pieces, the six largest cross terms on v_mfma_f32_32x32x16_bf16 (2.67x the f32 rate);
#   "f32"               v_mfma_f32_32x32x2_f32, the exact k-ordered fp32 FMA chain.
#   "f16x1"             REDUCED precision (BASELINE config 5's "bf16"; trainers / bench: --dtype f16): f16x3's operands -- same
#                       companions, weight images and bounds -- multiplied with the leading term only: one MFMA instead of three,
#                       operands rounded to fp16's 11 significant bits (bf16 would keep 8); accumulation, BatchNorm, loss and
#                       optimizer stay fp32.  NOT within north_star's 1e-3 of the fp32 reference: tests/test_model_gpu.py states
#                       what it keeps.
CONV_MATH = os.environ.get("MCDSEG_CONV_MATH", "f16x3")
# producers (BN apply / BN backward apply) also emit the split of what they write, so the convolution that gathers it
# does not re-split every activation inside its K loop (MCDSEG_PRESPLIT=0 turns this off)
PRESPLIT = os.environ.get("MCDSEG_PRESPLIT", "1") != "0"
if CONV_MATH not in ("f16x3", "bf16x6", "f32", "f16x1"):
    raise ValueError("MCDSEG_CONV_MATH must be f16x3, bf16x6, f32 or f16x1, got %r" % CONV_MATH)
MATH_ID = {"f16x3": 3, "bf16x6": 6, "f16x1": 1}   # MCDSEG_MATH_F16X3 / _BF16X6 / _F16X1 of include/mcdseg.h
PIECES = {"f16x3": 2, "bf16x6": 3, "f16x1": 2}    # (f16x1 stores what f16x3 stores)


# the stem's training forward on the LDS-window kernel (f16x3, 0.20 instead of 0.35 ms per launch at 14 x 480 x 640).  OFF by
# default: the stem's rounding is amplified by every BatchNorm behind it -- with the 22-bit f16x3 stem the weight updates of the
# small three-step trace sit at 1.7-4x the reference's own fp32-vs-fp64 spread, with the 24-bit bf16x6 direct kernel at 0.8-1.0x
# (tools/delta_report.py) -- and the layer is 0.4 % of the step
STEM_WINDOW = os.environ.get("MCDSEG_STEM_WINDOW", "0") != "0"

# Activation storage inside a DRN trunk (MCDSEG_ACT_STORAGE):
#   "fp32" (default)  every fused group writes its fp32 output y next to the pre-split companion;
#   "compact"         between the layers of a trunk only the companion is written (4 B/element with f16x3: the 22 leading bits
#                     of y) -- residual adds and ReLU masks read it, no fp32 y exists.  8 instead of 12 B/element are kept for
#                     backward, which is what lets BASELINE config 5 (drn_d_105, 32 x 720 x 1280 per GPU) fit 288 GB, and the
#                     BatchNorm passes move a third fewer bytes.  The trunk's last layer, and everything outside a trunk, stays fp32.
ACT_STORAGE = os.environ.get("MCDSEG_ACT_STORAGE", "fp32")
if ACT_STORAGE not in ("fp32", "compact"):
    raise ValueError("MCDSEG_ACT_STORAGE must be fp32 or compact, got %r" % ACT_STORAGE)
_TRUNK_DEPTH = 0


class trunk_internal:
    """context of the layers INSIDE a trunk whose outputs only other fused groups consume (models/dilated_fcn.py Trunk)"""

    def __enter__(self):
        global _TRUNK_DEPTH
        _TRUNK_DEPTH += 1

    def __exit__(self, *exc):
        global _TRUNK_DEPTH
        _TRUNK_DEPTH -= 1


def _compact_now():
    return ACT_STORAGE == "compact" and _TRUNK_DEPTH > 0 and _scaled()


# 2-byte activation storage (round 6; BASELINE config 5 "bf16"): in the one-term arithmetic f16x1 a compact group keeps ONE 16-bit value per
# element of everything its BatchNorm passes move -- the convolution writes z as scaled fp16 units (after taking the BatchNorm partial sums
# from its fp32 accumulators), the activation is the leading piece of the companion alone, the gradients between the groups travel as bf16
# units (include/mcdseg.h, "2-byte activation storage").  Such a group's output is a VIRTUAL tensor of dtype bfloat16: the dtype is the
# contract with autograd -- whoever consumes it owes its gradient as a bf16 tensor of the same logical shape whose BYTES are in the unit
# layout [N][C/8][HW][8] (element-wise sums of two such tensors, which is all autograd ever does to them, do not care).
# MCDSEG_HALF_STORAGE=0: f16x1 stores what f16x3 stores (round 5's form).
HALF_STORAGE = os.environ.get("MCDSEG_HALF_STORAGE", "1") != "0"


def _half_now():
    return HALF_STORAGE and CONV_MATH == "f16x1" and _compact_now()


def is_half(t):
    """an activation of the 2-byte chain (see HALF_STORAGE): virtual, dtype bfloat16"""
    return t is not None and t.dtype == torch.bfloat16 and is_virtual(t)


def pack_bf16_units(g):
    """fp32 NCHW gradient -> the bf16 unit layout (a gradient entering the 2-byte chain from a kernel without the 16-bit epilogue)"""
    n, c, h, w = g.shape
    out = torch.empty((n, c, h, w), dtype=torch.bfloat16, device=g.device)
    check(lib().mcdseg_pack_bf16_units(_p(_req(g, "gradient")), _p(out), n, c, h * w, _stream()), "pack_bf16_units")
    return out


def unpack_bf16_units(g):
    """the inverse of ``pack_bf16_units``"""
    n, c, h, w = g.shape
    out = torch.empty((n, c, h, w), dtype=torch.float32, device=g.device)
    check(lib().mcdseg_unpack_bf16_units(_p(_req(g, "gradient", torch.bfloat16)), _p(out), n, c, h * w, _stream()), "unpack_bf16_units")
    return out


# A fused ReLU group WITHOUT residual whose output only the next split convolution consumes (conv1 of a BasicBlock, conv1 / conv2
# of a Bottleneck: ``conv_bn_act(..., internal=True)``) need not write its fp32 output at all, in ANY storage mode and without
# changing a bit: the consumer's forward and weight gradient read the companion either way, and the group's own backward
# takes its ReLU mask from z (BN_ZMASK).  8 instead of 12 bytes written per element, 4 bytes per element less kept for backward.
# (Taken for more than 32 channels and un-cut batches only: there the consumer's forward, data and weight gradient all run on the
# split kernels.  A consumer that needs fp32 after all reconstructs it from the companion, 22 bits, as in compact storage.)
INTERNAL_SKIP_Y = os.environ.get("MCDSEG_INTERNAL_SKIP_Y", "1") != "0"
# ... and so need the groups of a trunk's plain convolution chains (models/drn.py:195-205: the stem, layer1, layer2, layer7) whose output
# only the next stage's convolutions read (round 5; models/drn.py run_fused / _reads_companions_only decide, "0": they write fp32 too).
# These include the 16- and 32-channel layers: their consumers' forward, data and weight gradients all read companions since the thin
# layers' window kernels (round 2) and the tap-pair weight gradient from 24 channels up (round 5).
INTERNAL_STAGES = os.environ.get("MCDSEG_INTERNAL_STAGES", "1") != "0"
# a block's 1x1 projection shortcut is read as a residual only (fp32): its companion is not written ("0": it is, as before round 5)
SHORTCUT_NO_CB = os.environ.get("MCDSEG_SHORTCUT_NO_CB", "1") != "0"


def _virtual(shape, device, dtype=torch.float32):
    """stand-in for an activation that exists only as its companion: right shape / device / dtype, 4 bytes of storage"""
    return torch.empty(1, dtype=dtype, device=device).expand(shape)


# how many times a train-mode BatchNorm forward applies its running-statistics update (solvers/solver.py: one generator
# forward standing for two identical ones of the reference's schedule)
BN_RUNNING_REPEAT = 1


class bn_running_updates:
    def __init__(self, k):
        self.k = int(k)

    def __enter__(self):
        global BN_RUNNING_REPEAT
        self.old, BN_RUNNING_REPEAT = BN_RUNNING_REPEAT, self.k

    def __exit__(self, *exc):
        global BN_RUNNING_REPEAT
        BN_RUNNING_REPEAT = self.old


def is_virtual(t):
    return t is not None and getattr(t, "_mcd_virtual", False)


def materialize(x, cb=None, bound=None):
    """fp32 tensor of an activation kept as its companion (value = scale * sum of pieces); ``x`` itself when it is real"""
    if cb is None:
        if not is_virtual(x):
            return x
        cb, bound = _cb_of(x)
    if cb is None:
        raise RuntimeError("mcdseg: a compact activation lost its companion (was it modified in place?)")
    n, c, h, w = x.shape
    out = torch.empty((n, c, h, w), dtype=torch.float32, device=cb.device)
    check(lib().mcdseg_unsplit_cb(_p(cb), _p(bound), MATH_ID[CONV_MATH], n, c, h * w, _p(out), _stream()), "unsplit_cb")
    return out


def _use_split(contraction_channels):
    return contraction_channels >= 16 and CONV_MATH in MATH_ID


def _scaled():
    """the active arithmetic needs per-tensor bound scalars (f16x3 and its one-term form f16x1)"""
    return CONV_MATH in ("f16x3", "f16x1")


def absmax(x):
    """device scalar max |x| -- the bound of a tensor whose producer did not supply one"""
    x = _req(x, "tensor")
    b = torch.empty(1, dtype=torch.float32, device=x.device)
    check(lib().mcdseg_absmax(_p(x), x.numel(), _p(b), _stream()), "absmax")
    _on_launch_stream(b)
    return b


def _bound_or_measure(x, bound):
    """bound scalar of ``x`` for the scaled arithmetic: the producer's if known, else measured (cached on the tensor)"""
    if not _scaled():
        return None
    if bound is not None:
        return bound
    rec = getattr(x, "_mcd_bound", None)
    if rec is not None and rec[1] == x._version and rec[2] == x.data_ptr():
        return rec[0]
    b = absmax(x)
    try:
        x._mcd_bound = (b, x._version, x.data_ptr())
    except AttributeError:
        pass
    return b


_PACK_REGISTRY = weakref.WeakSet()   # every PackedWeights alive
_PACK_TABLES = {}                    # (device, math) -> cached device tables of the last group pack
GROUP_PACK = os.environ.get("MCDSEG_GROUP_PACK", "1") != "0"
FUSED_UP_LOSS = os.environ.get("MCDSEG_FUSED_UP_LOSS", "1") != "0"  # MCDSolver: up-sampler folded into the loss kernel
# BatchNorm backward of a ReLU group without residual: the mask y > 0 recomputed from z (bit-identical), y never read
BN_ZMASK = os.environ.get("MCDSEG_BN_ZMASK", "1") != "0"
# BatchNorm backward of a ReLU group WITH residual: the mask y > 0 from a bit-plane the forward apply kernel wrote (1 bit per element)
# instead of from the fp32 y (32): the same mask, bit for bit; "0": read y (round 4's form)
RELU_MASK = os.environ.get("MCDSEG_RELU_MASK", "1") != "0"
# the gradient of a residual block's input has two producers (the first convolution's data gradient and the shortcut); autograd would
# add them with an element-wise kernel -- 80 adds of 40-160 MB tensors per MCD step, 7.3 ms at BASELINE config 2.  With this on the
# one that runs second folds the other's tensor into its own epilogue (``GradBox``); "0": autograd's add (same bits, tests compare)
FUSE_RES_ADD = os.environ.get("MCDSEG_FUSE_RES_ADD", "1") != "0"


class GradBox:
    """Mailbox between the producers of ONE tensor's gradient inside a residual block (models/drn.py BasicBlock / Bottleneck: the block
    input feeds the first convolution and the shortcut -- the identity, or the 1x1 projection).  Each producer ``attach``es in the
    forward pass; in the backward pass every producer but the last leaves its gradient here and reports None to autograd, the last
    one returns the sum -- formed in its convolution's data-gradient epilogue when it is one (``_conv_dgrad``'s ``addend``).  The sum
    is the one autograd's own accumulation would form, bit for bit (fp32 addition commutes), one kernel and three passes over the
    tensor earlier.  A box lives as long as the graph of its forward pass; it may see several backward passes -- also PARTIAL ones
    (``torch.autograd.grad(..., inputs=[...])``, ``backward(inputs=...)``, a pass that died in an exception) in which only some of
    the producers run: what such a pass left behind is dropped when a producer of ANOTHER pass arrives (the passes are told apart by
    the autograd engine's graph-task id), so a stale count or tensor never enters a later sum.  (In a partial pass the gradient of the
    block input is complete only if all its producers run -- which they do whenever the engine needs that gradient at all, since every
    producer lies on a path to it; a producer that runs only for its own weight's sake parks a tensor nobody asked for.)  Tensor hooks
    on the block input see ONE call, with the sum."""
    __slots__ = ("n", "seen", "g", "task")

    def __init__(self):
        self.n, self.seen, self.g, self.task = 0, 0, None, None

    def attach(self):
        self.n += 1
        return self

    def arrive(self):
        """(gradient left by the earlier producers or None, whether the caller is the last producer of this backward pass)"""
        task = _graph_task_id()
        if task != self.task:
            self.task, self.seen, self.g = task, 0, None
        self.seen += 1
        g, self.g = self.g, None
        last = self.seen >= self.n
        if last:
            self.seen = 0
        return g, last

    def leave(self, g):
        self.g = g


# (a private torch hook, resolved once: on a build without it the residual sums go back to autograd's own add -- same bits)
_GRAPH_TASK_ID = getattr(torch._C, "_current_graph_task_id", None)
if _GRAPH_TASK_ID is None:
    FUSE_RES_ADD = False


def _graph_task_id():
    """id of the backward pass the calling autograd node runs in (-1 outside one)"""
    return _GRAPH_TASK_ID()


def grad_box(x):
    """a ``GradBox`` for the gradient of ``x`` when there will be one (and the folding is on), else None"""
    return GradBox() if (FUSE_RES_ADD and torch.is_grad_enabled() and x.requires_grad) else None


class PackedWeights:
    """GEMM images of one conv kernel, refreshed when the parameter changes.  ``wf`` / ``wd``: forward / data-gradient image
    (fp32 for the f32 kernels, 16-bit pieces for the split kernels); ``w_bound``: device scalar max |w| (f16x3).

    An optimizer step invalidates every image of the model at once, so the first stale ``get`` of a forward pass re-packs ALL
    known convolutions of that device in two launches (``mcdseg_conv_split_pack_weights_multi``) instead of ~3 per conv."""

    def __init__(self):
        self.key = None
        self.wf = None
        self.wd = None
        self.w_bound = None
        self.mpf = 0
        self._weight = None   # weakref to the parameter, for group packs
        self._dims = None     # (Cout, Cin, taps, direct-stem?, math)
        _PACK_REGISTRY.add(self)

    @staticmethod
    def _key_of(weight):
        return (weight.data_ptr(), weight._version, WEIGHT_EPOCH, getattr(weight, "_mcd_epoch", 0), weight.device, CONV_MATH)

    def get(self, weight, desc, need_dgrad=True):
        key = self._key_of(weight)
        if key != self.key or (need_dgrad and self.wd is None):
            if GROUP_PACK and self._dims is not None and self.wd is not None and self._dims[4] == CONV_MATH:
                _pack_group(weight.device)
            if self._key_of(weight) != self.key or (need_dgrad and self.wd is None):
                self._pack_single(weight, desc)
        return self.wf, self.wd, self.mpf

    def _pack_single(self, weight, desc):
        L = lib()
        mpf, kpf, mpd, kpd = (ctypes.c_int32() for _ in range(4))
        check(L.mcdseg_conv_packed_dims(ctypes.byref(desc), mpf, kpf, mpd, kpd), "conv_packed_dims")
        taps = desc.KH * desc.KW
        w = _req(weight.detach(), "conv weight")
        dev = w.device
        fsp, dsp = _use_split(desc.Cin), _use_split(desc.Cout)
        direct = CONV_MATH in MATH_ID and bool(L.mcdseg_conv_split_direct_ok(ctypes.byref(desc)))
        if direct:
            fsp = True  # the stem: direct convolution on the split path although it contracts < 16 channels
        # f32 images (kept for whichever direction does not run on the split path)
        self.wf = None if fsp else torch.empty(taps * kpf.value * mpf.value, dtype=torch.float32, device=dev)
        self.wd = None if dsp else torch.empty(taps * kpd.value * mpd.value, dtype=torch.float32, device=dev)
        if self.wf is not None or self.wd is not None:
            check(L.mcdseg_conv_pack_weights(ctypes.byref(desc), _p(w), _p(self.wf), _p(self.wd), _stream()), "conv_pack_weights")
        self._dims = None
        if fsp or dsp:
            mid = MATH_ID[CONV_MATH]
            fb, db = ctypes.c_int64(), ctypes.c_int64()
            check(L.mcdseg_conv_split_packed_bytes(ctypes.byref(desc), mid, fb, db), "conv_split_packed_bytes")
            if fsp:
                self.wf = torch.empty(fb.value // 2, dtype=torch.int16, device=dev)
            if dsp:
                self.wd = torch.empty(db.value // 2, dtype=torch.int16, device=dev)
            if _scaled() and self.w_bound is None:
                self.w_bound = torch.empty(1, dtype=torch.float32, device=dev)
            with _timed("pack_weights_split_kernel", (0, 4 * w.numel() + (fb.value if fsp else 0) + (db.value if dsp else 0))):
                check(L.mcdseg_conv_split_pack_weights(ctypes.byref(desc), mid, _p(w), _p(self.wf) if fsp else None,
                                                       _p(self.wd) if dsp else None, _p(self.w_bound) if _scaled() else None,
                                                       _stream()), "conv_split_pack_weights")
            if fsp and dsp:  # both images on the split path: eligible for the group pack from now on
                self._weight = weakref.ref(weight)
                self._dims = (desc.Cout, desc.Cin, taps, direct, CONV_MATH)
        self.mpf = mpf.value
        self.key = self._key_of(weight)


def _pack_group(device):
    """re-pack every known split-path convolution on ``device`` whose image is stale: one table-driven absmax launch and one
    table-driven pack launch (plus the stem's own forward image)"""
    L = lib()
    members = []
    for pw in list(_PACK_REGISTRY):
        w = pw._weight() if pw._weight is not None else None
        if (w is None or pw._dims is None or pw._dims[4] != CONV_MATH or w.device != device or pw.wd is None or pw.wf is None
                or pw._dims[2] > 72):  # (the table-driven pack kernel stages up to 72 taps per tile)
            continue
        members.append((pw, w))
    if len(members) < 2:
        return
    members.sort(key=lambda m: m[1].data_ptr())
    sig = tuple((w.data_ptr(), pw.wf.data_ptr(), pw.wd.data_ptr()) + pw._dims for pw, w in members)
    tab = _PACK_TABLES.get((device, CONV_MATH))
    if tab is None or tab["sig"] != sig:
        n = len(members)
        bounds = torch.zeros(n, dtype=torch.float32, device=device)
        ptrs, dims = [], []
        for i, (pw, w) in enumerate(members):
            ptrs += [w.data_ptr(), pw.wf.data_ptr(), pw.wd.data_ptr(), bounds.data_ptr() + 4 * i]
            dims += [pw._dims[0], pw._dims[1], pw._dims[2], 0]
        tab = dict(sig=sig, bounds=bounds, ptrs=torch.tensor(ptrs, dtype=torch.int64).to(device),
                   dims=torch.tensor(dims, dtype=torch.int32).to(device))
        _PACK_TABLES[(device, CONV_MATH)] = tab
    if _scaled():
        for i, (pw, _) in enumerate(members):
            pw.w_bound = tab["bounds"][i:i + 1]
    n = len(members)
    nbytes = sum(4 * w.numel() + 2 * pw.wf.numel() + 2 * pw.wd.numel() for pw, w in members)
    with _timed("pack_weights_multi_kernel", (0, nbytes)):
        check(L.mcdseg_conv_split_pack_weights_multi(_p(tab["ptrs"]), _p(tab["dims"]), n, MATH_ID[CONV_MATH],
                                                     _p(tab["bounds"]) if _scaled() else None, _stream()), "conv_split_pack_weights_multi")
    for pw, w in members:
        if pw._dims[3]:  # the stem's direct-kernel forward image (behind the standard one) has its own layout
            d = ConvDesc(1, pw._dims[1], 8, 8, pw._dims[0], 7, 7, 1, 3, 1, 8, 8)
            check(L.mcdseg_conv_split_pack_weights(ctypes.byref(d), MATH_ID[CONV_MATH], _p(w.detach()), _p(pw.wf), None,
                                                   _p(pw.w_bound) if _scaled() else None, _stream()), "conv_split_pack_weights")
        pw.key = PackedWeights._key_of(w)


def _is_split(w_image):
    """packed image of the split kernels (16-bit pieces) rather than of the f32 kernels"""
    return w_image.dtype == torch.int16


# ------------------------------------------------------------------------------------------------ raw launchers
# The kernels address one conv operand with 32-bit buffer offsets, so a single launch takes operands below 2 GiB
# (+ a tile of slack).  Larger batches (cfg5: 32 x 720 x 1280) are cut along N on the host: conv is independent per
# image, the BN partial rows of the pieces are simply concatenated, weight gradients of the pieces are summed.
MAX_CONV_BYTES = int(os.environ.get("MCDSEG_MAX_CONV_BYTES", str((1 << 31) - (1 << 26))))


def _sub_desc(desc, n, ncb=0):
    """descriptor of ``n`` images of the batch; ``ncb``: batch size of the tensor the companions were written for (Ncb of mcdseg.h)"""
    return ConvDesc(n, desc.Cin, desc.H, desc.W, desc.Cout, desc.KH, desc.KW, desc.stride, desc.pad, desc.dil, desc.Ho, desc.Wo, ncb)


def _cb_slice(cb, a, channels, hw):
    """pointer to image ``a`` in piece 0 of a companion [piece][N][C/8][HW][8 x 16 bit] (None stays None)"""
    return None if cb is None else ctypes.c_void_p(cb.data_ptr() + a * (channels // 8) * hw * 16)


def _unit_slice(t, a, channels, hw):
    """pointer to image ``a`` of a 16-bit tensor in the unit layout [N][C/8][HW][8]"""
    return None if t is None else ctypes.c_void_p(t.data_ptr() + a * channels * hw * 2)


def _sl(t, a, b):
    return None if t is None else t[a:b]


def _launches(desc, pieces, whole_cb):
    """(first image, end, descriptor) of every launch of a convolution whose batch is cut into ``pieces``.  An uncut batch goes through on
    ``desc`` itself.  ``whole_cb``: the companions passed along were written for the whole batch -- a slice keeps them: piece p of a slice
    lies p * N * (C/8) * HW * 16 bytes behind its piece 0, which the kernels learn from Ncb"""
    for a, b in pieces:
        yield a, b, (desc if (a, b) == (0, desc.N) else _sub_desc(desc, b - a, desc.N if whole_cb else 0))


_PLAN_CACHE = {}


def _memo(desc, what, compute):
    """``compute()``, once per geometry, question, MAX_CONV_BYTES, arithmetic and state of the library's options: a group asks for its
    batch pieces and the library's plan answers several times per pass"""
    key = (desc.N, desc.Cin, desc.H, desc.W, desc.Cout, desc.KH, desc.KW, desc.stride, desc.pad, desc.dil, desc.Ncb, MAX_CONV_BYTES, CONV_MATH,
           _lib.OPTION_EPOCH) + what
    hit = _PLAN_CACHE.get(key)
    if hit is None:
        if len(_PLAN_CACHE) > 4096:
            _PLAN_CACHE.clear()
        hit = _PLAN_CACHE[key] = compute()
    return hit


def _wgrad_variant(desc, have_cb, math=None):
    """``mcdseg_conv_wgrad_variant``: the kernel the weight gradient of this geometry runs on -- 0..3 the f32 plans (128 / 64 / 32 tiles,
    tap-packed thin), 10 and up the split-arithmetic plans, from 11 on those that read both pre-split companions and nothing else, 15 the
    thin layers' window kernel.  ``math``: the active arithmetic, or 0 for what ``mcdseg_conv_wgrad`` launches."""
    math = MATH_ID.get(CONV_MATH, 0) if math is None else math
    return _memo(desc, ("wgrad", math, bool(have_cb)), lambda: lib().mcdseg_conv_wgrad_variant(ctypes.byref(desc), math, int(bool(have_cb))))


def _cut(desc, elem_bytes, slack, fits=None):
    """[(first image, end)]: the batch in the fewest equal launches whose operands -- ``elem_bytes`` per element, ``slack`` channels past the
    tensor -- stay below MAX_CONV_BYTES and whose image count ``fits``"""
    step = desc.N
    for c, hw in ((desc.Cin, desc.H * desc.W), (desc.Cout, desc.Ho * desc.Wo)):
        step = min(step, max(1, (MAX_CONV_BYTES - elem_bytes * slack * hw) // (elem_bytes * c * hw)))
    while fits is not None and step > 1 and not fits(step):
        step -= 1
    return [(i, min(i + step, desc.N)) for i in range(0, desc.N, step)]


def _batch_pieces(desc, wgrad_cb=None):
    """[(first image, end)] of the launches a convolution's batch is cut into.  ``wgrad_cb``: None for the forward pass and the data
    gradient; for the weight gradient, whether both pre-split companions will be passed."""
    def pieces():
        # the f32 kernels express padding and ragged channel tails as offsets the buffer range check rejects, up to a 128-channel tile
        # past the tensor: (N*C + 128) * H*W * 4 < 2 GiB per operand -- the tile of slack is per LAUNCH, not per image (charging it per
        # image cut the full-resolution 16-channel layers in two and lost their pre-split operands).  The split kernels mark such
        # accesses with an explicit out-of-range offset instead, so the forward pass and the data gradient of a layer that runs on them
        # (both channel counts multiples of 8, at least 16) need no slack: BASELINE config 5's 16- and 32-channel layers at
        # 32 x 720 x 1280 (1.89 GB per tensor) stay in one launch and keep their companions.  The WEIGHT gradient is slack-free only on
        # the plans that read both companions (mcdseg_conv_wgrad_fits states the library's own rule): the f32 plans of thin layers, the
        # split plan without companions and bf16x6's thin layers still gather fp32 values with the slack.
        math = MATH_ID.get(CONV_MATH, 0)
        variant = _wgrad_variant(desc, True) if wgrad_cb else 0
        # the thin layers' window weight gradient (csrc/conv_wgrad_thin_tr.hip) reads both companions of the WHOLE batch through one
        # descriptor each and nothing else: the library's own rule decides (round 6: the stem at BASELINE config 5's N = 32 -- a 1.9 GB dz,
        # two 0.9 GB pieces of its companion -- was cut by the fp32 kernels' slack rule and fell back to the f32 tap-packed kernel: 37 ms)
        if variant == 15 and lib().mcdseg_conv_wgrad_fits(ctypes.byref(desc), math, 1):
            return [(0, desc.N)]
        split_only = bool(math) and desc.Cin % 8 == 0 and desc.Cout % 8 == 0 and min(desc.Cin, desc.Cout) >= 16
        if wgrad_cb is None:
            return _cut(desc, 4, 0 if split_only else 128)
        return _cut(desc, 4, 0 if split_only and variant >= 11 else 128, lambda n: lib().mcdseg_conv_wgrad_fits(  # (the variant can change with N)
            ctypes.byref(_sub_desc(desc, n, desc.N if wgrad_cb else 0)), math, int(wgrad_cb)))
    return _memo(desc, ("pieces", wgrad_cb), pieces)


def _batch_pieces_half(desc):
    """[(first image, end)] of the launches of a convolution of the 2-byte chain: a launch addresses one piece of its pre-split operand
    through a 32-bit buffer resource (< 2 GiB, 2 bytes per element); the 16-bit output is addressed with 64-bit pointers"""
    return _cut(desc, 2, 0)


def half_conv_work(d):
    """(algorithmic FLOPs, algorithmic bytes) of one conv pass of the 2-byte chain: 16-bit operand in, 16-bit result out"""
    flops, byts = conv_work(d)
    return flops, byts // 2


def _window_name(d, presplit, dgrad):
    """rocprofv3's name of the LDS-window kernel when it takes this thin 3x3 geometry (csrc/conv_thin_window.hip), else None"""
    if not lib().mcdseg_conv_split_window_ok(ctypes.byref(d), MATH_ID.get(CONV_MATH, 0), int(presplit), int(dgrad)):
        return None
    m = d.Cin if dgrad else d.Cout
    stem = d.KH * d.KW == 49
    return "conv_thin_window_kernel<%d, %d, %d, %s>" % (1 if stem else 2, m // 16, 13 if stem else 5, "true" if dgrad else "false")


def _fprop(desc, x, x_cb, x_bound, wf, w_bound, bias, want_stats, mpf, half):
    """The forward convolution, fp32 result or -- ``half`` -- the 2-byte chain's (16-bit units from the companion alone): per launch the
    entry point, the slice of the output and of the BatchNorm partial rows, and the kernel name a launch timer is given"""
    L = lib()
    dev, hw_out = (x if x is not None else x_cb).device, desc.Ho * desc.Wo
    presplit, split = x_cb is not None, half or _is_split(wf)
    launches = list(_launches(desc, _batch_pieces_half(desc) if half else _batch_pieces(desc), presplit))
    y = torch.empty(desc.N * desc.Cout * hw_out, dtype=torch.int16, device=dev) if half \
        else torch.empty((desc.N, desc.Cout, desc.Ho, desc.Wo), dtype=torch.float32, device=dev)
    y_bound = torch.empty(1, dtype=torch.float32, device=dev) if half else None
    row_off = [0]  # BatchNorm partial rows: those of the launches, one behind the other
    for _, _, d in launches if want_stats else ():
        row_off.append(row_off[-1] + (L.mcdseg_conv_split_stat_rows_for(ctypes.byref(d), MATH_ID[CONV_MATH], int(presplit))
                                      if split else L.mcdseg_conv_stat_rows(ctypes.byref(d))))
    rows = row_off[-1]
    part = torch.empty(rows * 3 * mpf, dtype=torch.float32, device=dev) if want_stats else None
    direct = split and not half and bool(L.mcdseg_conv_split_direct_ok(ctypes.byref(desc)))
    if split and not direct and not half:
        x_bound = _bound_or_measure(x, x_bound)
    for i, (a, b, d) in enumerate(launches):
        pp = None if part is None else ctypes.c_void_p(part.data_ptr() + 4 * row_off[i] * 3 * mpf)
        xs = _cb_slice(x_cb, a, desc.Cin, desc.H * desc.W)
        def name():  # (formed only when a launch timer asks: it costs queries of the library's plan)
            return (_window_name(d, presplit, False) if split and not half else None) \
                or gemm_kernel_name(desc.Cout, desc.Cin, False, split, presplit, direct, d.N * hw_out)
        if half:
            _split_launches(d, True, False, name, lambda part_no: check(L.mcdseg_conv_split_fprop_half(
                ctypes.byref(d), MATH_ID[CONV_MATH], xs, _p(x_bound), _p(wf), _p(w_bound), _unit_slice(y, a, desc.Cout, hw_out), _p(y_bound),
                pp, part_no, _stream()), "conv_split_fprop_half"), half_conv_work)
        elif split:
            _split_launches(d, presplit, False, name, lambda part_no: check(L.mcdseg_conv_split_fprop_part(
                ctypes.byref(d), MATH_ID[CONV_MATH], _p(_sl(x, a, b)), xs, _p(x_bound), _p(wf), _p(w_bound), _p(bias), _p(y[a:b]), pp, part_no,
                _stream()), "conv_split_fprop"))
        else:
            with _timed(name() if LAUNCH_TIMER is not None else "", conv_work(d)):
                check(L.mcdseg_conv_fprop(ctypes.byref(d), _p(x[a:b]), _p(wf), _p(bias), _p(y[a:b]), pp, _stream()), "conv_fprop")
    return (y, y_bound, part, rows) if half else (y, part, rows)


def _conv_fprop(desc, x, wf, bias, want_stats, mpf, x_cb=None, x_bound=None, w_bound=None):
    return _fprop(desc, x, x_cb, x_bound, wf, w_bound, bias, want_stats, mpf, False)


def _conv_fprop_half(desc, x_cb, x_bound, wf, w_bound, mpf):
    """forward convolution of the 2-byte chain: (z16 units [int16], z_bound scalar, BatchNorm partial rows, row count)"""
    return _fprop(desc, None, x_cb, x_bound, wf, w_bound, None, True, mpf, True)


def _dgrad(desc, dy, dy_cb, dy_bound, wd, w_bound, addend, half):
    """The data gradient (+ ``addend``), fp32 or -- ``half`` -- the 2-byte chain's bf16 units: per launch the entry point and the kernel
    name a launch timer is given.  The sum is formed in the kernel's epilogue where the kernel can (``mcdseg_conv_split_dgrad_add``, the
    chain's entry point), by an element-wise add otherwise: the same bits either way."""
    L = lib()
    addend = _req(addend, "gradient addend", torch.bfloat16 if half else torch.float32)
    dx = torch.empty((desc.N, desc.Cin, desc.H, desc.W), dtype=torch.bfloat16 if half else torch.float32,
                     device=(dy if dy is not None else dy_cb).device)
    presplit, split = dy_cb is not None, half or _is_split(wd)
    if split and dy is not None:
        dy_bound = _bound_or_measure(dy, dy_bound)
    for a, b, d in _launches(desc, _batch_pieces_half(desc) if half else _batch_pieces(desc), presplit):
        ys = _cb_slice(dy_cb, a, desc.Cout, desc.Ho * desc.Wo)
        # the LDS-window kernel has no adding epilogue: asked once, for the entry point and for the name
        window = _window_name(d, presplit, True) if split and not half and (addend is not None or LAUNCH_TIMER is not None) else None
        def name():
            return window or gemm_kernel_name(desc.Cin, desc.Cout, True, split, presplit, False, d.N * d.H * d.W)
        fused_add = addend is not None and split and window is None
        if half:
            _split_launches(d, True, True, name, lambda part_no: check(L.mcdseg_conv_split_dgrad_half(
                ctypes.byref(d), MATH_ID[CONV_MATH], ys, _p(dy_bound), _p(wd), _p(w_bound), _unit_slice(addend, a, desc.Cin, desc.H * desc.W),
                _unit_slice(dx, a, desc.Cin, desc.H * desc.W), part_no, _stream()), "conv_split_dgrad_half"), half_conv_work)
        elif split:
            entry, sum_with = (L.mcdseg_conv_split_dgrad_add, (_p(addend[a:b]),)) if fused_add else (L.mcdseg_conv_split_dgrad_part, ())
            _split_launches(d, presplit, True, name, lambda part_no: check(entry(
                ctypes.byref(d), MATH_ID[CONV_MATH], _p(_sl(dy, a, b)), ys, _p(dy_bound), _p(wd), _p(w_bound), *sum_with, _p(dx[a:b]), part_no,
                _stream()), "conv_split_dgrad_add" if fused_add else "conv_split_dgrad"))
        else:
            with _timed(name() if LAUNCH_TIMER is not None else "", conv_work(d)):
                check(L.mcdseg_conv_dgrad(ctypes.byref(d), _p(dy[a:b]), _p(wd), _p(dx[a:b]), _stream()), "conv_dgrad")
        if addend is not None and not fused_add:
            dx[a:b].add_(addend[a:b])
    return dx


def _conv_dgrad(desc, dy, wd, dy_cb=None, dy_bound=None, w_bound=None, addend=None):
    """``dy`` may be None when its pre-split companion is given and the batch is not cut (the kernel reads only ``dy_cb``).
    ``addend``: another gradient of the same input (``GradBox``); the result is data gradient + addend"""
    return _dgrad(desc, dy, dy_cb, dy_bound, wd, w_bound, addend, False)


def _conv_dgrad_half(desc, dy_cb, dy_bound, wd, w_bound, addend16=None):
    """data gradient of the 2-byte chain: bf16 units (+ the other gradient of the same tensor, same layout, in the kernel's epilogue)"""
    return _dgrad(desc, None, dy_cb, dy_bound, wd, w_bound, addend16, True)


def _cb_wanted(channels):
    """Emit the pre-split (channel-blocked) companion of a tensor with this many channels?  Only when the conv that gathers
    it runs on the split path (contraction >= 16 channels) and the layout applies (multiple of 8)."""
    return PRESPLIT and _use_split(channels) and channels % 8 == 0


def _cb_alloc(n, c, hw, device):
    return torch.empty(PIECES[CONV_MATH] * n * c * hw, dtype=torch.int16, device=device)


def split_companion(x, bound=None):
    """pre-split companion of an fp32 NCHW tensor no fused BN group produced: (companion, bound scalar) -- (None, None) when
    the layout does not apply"""
    x = _req(x, "tensor to split")
    n, c, h, w = x.shape
    if not _cb_wanted(c) or n * (c // 8) > 65535:
        return None, None
    bound = _bound_or_measure(x, bound)
    cb = _cb_alloc(n, c, h * w, x.device)
    check(lib().mcdseg_split_cb(_p(x), _p(cb), _p(bound), MATH_ID[CONV_MATH], n, c, h * w, _stream()), "split_cb")
    return cb, bound


def split_companion_padded(x, bound=None):
    """companion of a tensor whose channel count is not a multiple of 8 (the 6-channel network input): ceil(C/8) channel groups,
    zeros in the missing channels -- read by the stem's window-forward and weight-gradient kernels.  Cached on the tensor object (same guard
    as ``_mcd_cb``): one MCD step back-propagates through the stem several times with the same batch."""
    rec = getattr(x, "_mcd_cbp", None)
    if rec is not None and rec[2] == x._version and rec[3] == x.data_ptr() and rec[4] == CONV_MATH:
        return rec[0], rec[1]
    x = _req(x, "tensor to split")
    n, c, h, w = x.shape
    bound = _bound_or_measure(x, bound)
    cb = torch.empty(PIECES[CONV_MATH] * n * ((c + 7) // 8) * 8 * h * w, dtype=torch.int16, device=x.device)
    check(lib().mcdseg_split_cb_padded(_p(x), _p(cb), _p(bound), MATH_ID[CONV_MATH], n, c, h * w, _stream()), "split_cb_padded")
    x._mcd_cbp = (cb, bound, x._version, x.data_ptr(), CONV_MATH)
    return cb, bound


# mcdseg_conv_wgrad_variant code -> the kernel name rocprofv3 prints (%s: the arithmetic's policy)
_WGRAD_NAMES = {0: "conv_wgrad_kernel<2, 2, 2, 2, 16>", 1: "conv_wgrad_kernel<1, 1, 2, 2, 32>", 2: "conv_wgrad_kernel<1, 1, 1, 1, 32>",
                10: "conv_wgrad_split_kernel<%s>", 11: "conv_wgrad_split_cb_kernel<%s>", 12: "conv_wgrad_split_tr_kernel<%s, 2, 2, 3>",
                13: "conv_wgrad_split_tr_kernel<%s, 4, 2, 3>", 14: "conv_wgrad_split_tr64_kernel<%s>",
                17: "conv_wgrad_split_pp_kernel<%s>", 18: "conv_wgrad_split_pp3_kernel<%s>"}


def _wgrad_name(d, v):
    """rocprofv3's name of the weight-gradient kernel with variant code ``v`` on this geometry"""
    if v == 3:   # the tap-packed f32 kernel of the thin layers: <padded input channels per tap, Cout <= 16>
        return "conv_wgrad_thin_kernel<%d, %s>" % (8 if d.Cin <= 8 else 16, "true" if d.Cout <= 16 else "false")
    if v == 15:  # csrc/conv_wgrad_thin_tr.hip: <channel groups of the input, row tiles, column tiles, tile rows> (no policy argument)
        cfg = lib().mcdseg_conv_wgrad_thin_tr_config(ctypes.byref(d))  # (the library's own choice, not a restatement of it)
        return "conv_wgrad_thin_tr_kernel<%d, %d, %d, %d>" % (cfg // 1000000, cfg // 10000 % 100, cfg // 100 % 100, cfg % 100)
    deep = v == 17 and CONV_MATH == "f16x1" and get_option("WGRAD_PP_DEEP")  # six logical stages (csrc/conv_wgrad_split_pp.hip)
    return _WGRAD_NAMES.get(v, "conv_wgrad<%s>").replace("%s", "SplitF16x1D" if deep else POLICY.get(CONV_MATH, ""))


def wgrad_kernel_name(cout, cin, taps=9):
    """rocprofv3's name of the f32 weight-gradient kernel ``mcdseg_conv_wgrad`` launches for these channel counts (the library's plan
    goes by them and the tap count alone: asked with a one-pixel geometry)"""
    d = conv_desc((1, cin, taps, 1), (cout, cin, taps, 1), 1, 0, 1)
    return _wgrad_name(d, _wgrad_variant(d, False, math=0))


def wgrad_split_kernel_name(d, have_cb):
    """rocprofv3's name of the split-arithmetic weight-gradient kernel the library launches for this geometry"""
    return _wgrad_name(d, _wgrad_variant(d, have_cb))


def _wgrad_thin_tr(desc):
    """the thin-layer window kernel (csrc/conv_wgrad_thin_tr.hip) takes this geometry when both companions exist"""
    return _wgrad_variant(desc, True) == 15


def _wgrad_split_plan(desc, have_cb=False):
    """a split-arithmetic plan of csrc/conv_wgrad.hip applies (else the f32 kernels run): the 128x128 plan for min(Cin, Cout) > 64, and -- from
    both pre-split companions only, f16x3 -- the 64-channel tap-pair plan for 32 < min <= 64 and the window kernel of the thin 3x3 layers"""
    return _wgrad_variant(desc, have_cb) >= 10


def _wgrad_reads_cb(desc):
    """the weight gradient has a plan that reads both pre-split companions and nothing else.  (The channel counts are the host's own rule: the
    stem, 6 input channels, is on plan 15 too, but from the zero-PADDED companion that only ``_plan_backward``'s ``stem_tr`` provides.)"""
    return _wgrad_variant(desc, True) >= 11 and desc.Cin % 8 == 0 and desc.Cout % 8 == 0


def _conv_wgrad(desc, x, dy, x_cb=None, dy_cb=None, x_bound=None, dy_bound=None):
    L, total = lib(), None
    if x_cb is None or dy_cb is None:
        x_cb = dy_cb = None  # both companions or none
    pieces = _batch_pieces(desc, wgrad_cb=x_cb is not None)
    if x_cb is not None and len(pieces) > 1 and desc.Cin <= 16:
        x_cb = dy_cb = None  # the thin layers' window kernel takes whole batches only: the cut batch gathers fp32 values (with the slack)
        pieces = _batch_pieces(desc, wgrad_cb=False)
    split = _wgrad_split_plan(desc, x_cb is not None)
    if split and x_cb is None:
        x_bound, dy_bound = _bound_or_measure(x, x_bound), _bound_or_measure(dy, dy_bound)
    for a, b, d in _launches(desc, pieces, x_cb is not None):
        ws = _ws(L.mcdseg_conv_wgrad_workspace_bytes(ctypes.byref(d)), (x if x is not None else x_cb).device)
        dw = torch.empty((desc.Cout, desc.Cin, desc.KH, desc.KW), dtype=torch.float32, device=ws.device)
        name = "" if LAUNCH_TIMER is None else (wgrad_split_kernel_name(d, x_cb is not None) if split else
                                                 wgrad_kernel_name(desc.Cout, desc.Cin, desc.KH * desc.KW))
        with _timed(name, conv_work(d)):
            if split:
                check(L.mcdseg_conv_split_wgrad(ctypes.byref(d), MATH_ID[CONV_MATH], _p(_sl(x, a, b)), _cb_slice(x_cb, a, desc.Cin, desc.H * desc.W),
                                                _p(x_bound), _p(_sl(dy, a, b)), _cb_slice(dy_cb, a, desc.Cout, desc.Ho * desc.Wo), _p(dy_bound),
                                                _p(dw), _p(ws), ctypes.c_size_t(ws.numel() * 4), _stream()), "conv_split_wgrad")
            else:
                check(L.mcdseg_conv_wgrad(ctypes.byref(d), _p(x[a:b]), _p(dy[a:b]), _p(dw), _p(ws), ctypes.c_size_t(ws.numel() * 4),
                                          _stream()), "conv_wgrad")
        _on_launch_stream(ws, dw)
        if total is None:
            total = dw
        else:
            with torch.cuda.stream(_LAUNCH.stream or torch.cuda.current_stream()):
                total.add_(dw)
    return total


# dgrad and wgrad of one layer are independent.  MCDSEG_OVERLAP_WGRAD:
#   "0"  both on the current stream;
#   "1"  wgrad on a second HIP stream, joined right behind dgrad (round 1; measured +1 %: both kernels are matrix-bound);
#   "2"  (default) wgrad on the second stream and NOT joined until the backward pass is nearly over: the weight gradient of layer k
#        then also runs beside the HBM-bound BatchNorm backward of layer k-1, which a power-metered matrix kernel hides
#        (tools/probes/overlap_probe.py: 20 forward launches + 20 bn_apply passes take as long as the 20 forward launches alone;
#        -4 % of the cfg2 step).  Correct by construction: a deferred gradient is handed to autograd through a ``_LateGrad``
#        identity node that sits between the parameter and the convolution and makes the main stream wait for the side stream
#        BEFORE it passes the gradient on -- nothing downstream (the engine's summation of several gradients of one weight,
#        AccumulateGrad's in-place add, hooks, torch.autograd.grad's capture) ever sees an unfinished tensor.  WHEN the wait
#        happens is a matter of the engine's ready queue (latest-created node first): ``late_weight_grads`` creates the identity
#        nodes at the start of a trunk's forward pass, so they run at the end of its backward pass; a convolution called outside
#        such a context gets no identity node and runs its weight gradient on the main stream.
OVERLAP_WGRAD = os.environ.get("MCDSEG_OVERLAP_WGRAD", "2")
if OVERLAP_WGRAD not in ("0", "1", "2"):
    raise ValueError("MCDSEG_OVERLAP_WGRAD must be 0, 1 or 2, got %r" % OVERLAP_WGRAD)
_SIDE = {}
_PENDING = {}  # device index -> (event behind the last weight gradient on the side stream, the stream that has to wait for it)


def _side_stream(device):
    # (a stream of HIP's lowest priority -- hipStreamCreateWithPriority through ctypes, wrapped as torch.cuda.ExternalStream -- was
    # measured too: 235.1 vs 236.2 ms on one box, 236.1 / 234.6 vs 234.8 / 235.0 on another; within the noise, not kept)
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in _SIDE:
        _SIDE[key] = torch.cuda.Stream(device=device)
    return _SIDE[key]


def join_side_streams(device_index=None):
    """The consumer stream of a device -- the stream its backward pass ran on when the weight gradients were deferred, recorded with
    the event -- waits for the weight gradients still running on that device's side stream.  A ``_LateGrad`` node joins its own
    device only (under nn.DataParallel every device has its own autograd thread, whose current stream says nothing about another
    device's); the final callback of a backward pass that deferred one joins all of them.  Safe at any time."""
    for key in ([device_index] if device_index is not None else list(_PENDING)):
        rec = _PENDING.pop(key, None)
        if rec is not None:
            rec[1].wait_event(rec[0])
            # backward passes of two sub-graphs may run on two streams (MFNet's encoders, solvers/solver.py) and share the side stream:
            # whoever joins waits too, whichever stream recorded the event last
            cur = torch.cuda.current_stream(rec[1].device)
            if cur != rec[1]:
                cur.wait_event(rec[0])
            _HELD.pop(key, None)  # (after the wait: the operands of the deferred launches go back to the allocator)


# ---- two independent forward passes side by side (MCD step B: the generator on the source and on the target batch, same weights).
# A forward pass on ONE stream alternates matrix-bound convolutions with HBM-bound BatchNorm passes and nothing runs beside either;
# two passes on two streams fill each other's gaps.  The only state they share is each BatchNorm's running statistics, which the
# reference updates source-first (adapt_trainer.py:187-200): the pass that leads (source, side stream) records an event behind every
# statistics launch, the pass that follows (target, main stream) waits for the layer's event before it touches the layer -- the same
# updates in the same order (and the lazily re-packed weight images of the leading pass are complete before the follower reads
# them).  MCDSEG_OVERLAP_STEPB=0: one after the other.
OVERLAP_STEPB = os.environ.get("MCDSEG_OVERLAP_STEPB", "1") != "0"
_FWD_SYNC = None  # "lead" / "follow" inside ForwardFork's contexts
_FWD_LEAD_DONE = None  # event behind the last launch of the leading pass


class ForwardFork:
    def __init__(self, device):
        self.device = device
        self.main = torch.cuda.current_stream(device)
        self.side = _side_stream(device)

    @contextlib.contextmanager
    def lead(self):
        """the pass that goes first in the reference's order: on the side stream, without a tape"""
        global _FWD_SYNC, _FWD_LEAD_DONE
        self.side.wait_stream(self.main)
        prev, _FWD_SYNC = _FWD_SYNC, "lead"
        try:
            with torch.cuda.stream(self.side), torch.no_grad():
                yield
            _FWD_LEAD_DONE = torch.cuda.Event()
            _FWD_LEAD_DONE.record(self.side)
        finally:
            _FWD_SYNC = prev

    @contextlib.contextmanager
    def follow(self):
        global _FWD_SYNC
        prev, _FWD_SYNC = _FWD_SYNC, "follow"
        try:
            yield
        finally:
            _FWD_SYNC = prev

    def join(self, tensors):
        """the main stream waits for the leading pass; its results (allocated from the side stream's pool) now belong to both"""
        global _FWD_LEAD_DONE
        _FWD_LEAD_DONE = None
        self.main.wait_stream(self.side)
        for t in tensors:
            t.record_stream(self.main)
            for c in (getattr(t, "_mcd_cb", None) or ())[:2]:
                if torch.is_tensor(c):
                    c.record_stream(self.main)


def forward_fork(device):
    """a ``ForwardFork`` when two forward passes may run side by side on ``device`` now, else None"""
    if not OVERLAP_STEPB or device.type != "cuda" or _LAUNCH.stream is not None:
        return None
    if LAUNCH_TIMER is not None and LAUNCH_TIMER.wants("conv_wgrad"):
        return None  # a step whose launches are bracketed by HIP events runs every kernel alone
    if not _room_to_defer(device):
        return None
    return ForwardFork(device)


def _fwd_sync_wait(anchor):
    ev = getattr(anchor, "_mcd_fwd_ev", None)
    if ev is not None:
        torch.cuda.current_stream().wait_event(ev)
        anchor._mcd_fwd_ev = None


def _fwd_sync_record(anchor):
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream())
    anchor._mcd_fwd_ev = ev


class _LateGrad(torch.autograd.Function):
    """identity on a convolution weight; its backward makes the main stream wait for the side stream, then passes the gradient on"""

    @staticmethod
    def forward(ctx, w):
        return w.view_as(w)

    @staticmethod
    def backward(ctx, g):
        join_side_streams(g.device.index)
        return g


class late_weight_grads:
    """Context around the forward pass of a trunk (``root``: an nn.Module): one ``_LateGrad`` alias per convolution weight, created
    NOW -- before every other node of this forward pass, hence executed after all of them in the backward pass -- and consumed by
    the first ``conv_bn_act`` call on that convolution.  Nothing is prepared without grad mode, for weights that do not require a
    gradient, for weights with foreign post-accumulate hooks (they want their gradients DURING the pass; FlatSGD's bucketed
    all-reduce takes deferred gradients through its ``_mcd_grad_sink`` instead) or when MCDSEG_OVERLAP_WGRAD is not "2"."""

    def __init__(self, root):
        self.root, self.mods = root, []

    def __enter__(self):
        if OVERLAP_WGRAD == "2" and torch.is_grad_enabled():
            for m in self.root.modules():
                if isinstance(getattr(m, "_packed", None), PackedWeights) and getattr(m, "_w_late", None) is None:
                    w = m.weight
                    # (a weight with post-accumulate hooks wants its gradient DURING the pass -- unless the hook's owner also left a
                    # ``_mcd_grad_sink`` on it, which receives a deferred gradient on the side stream: _conv_backward)
                    if w.is_cuda and w.requires_grad and (not getattr(w, "_post_accumulate_grad_hooks", None) or
                                                          getattr(w, "_mcd_grad_sink", None) is not None):
                        alias = _LateGrad.apply(w)
                        alias._mcd_param = w  # (the packed images are keyed by the parameter, see PackedWeights._key_of)
                        m._w_late = alias
                        self.mods.append(m)
        return self

    def __exit__(self, *exc):
        for m in self.mods:
            m._w_late = None


def _take_late(conv):
    """the weight tensor a fused group hands to autograd: the prepared ``_LateGrad`` alias (once), else the parameter itself"""
    alias = getattr(conv, "_w_late", None)
    if alias is None or not torch.is_grad_enabled():
        return conv.weight
    conv._w_late = None
    return alias


# What a deferred weight gradient reads and writes stays allocated until the main stream has waited for it.  At most MAX_LAG
# launches are left behind: before the next one is enqueued the main stream waits for the oldest (the side stream is rarely more
# than a layer or two behind, so this wait is almost always already satisfied) and its operands are released.  And nothing is
# deferred while the allocator holds more than DEFER_MEM_FRACTION of the device's memory (cfg5 at N = 32: 232 of 288 GB).
MAX_LAG = int(os.environ.get("MCDSEG_OVERLAP_WGRAD_LAG", "4"))
DEFER_MEM_FRACTION = float(os.environ.get("MCDSEG_OVERLAP_WGRAD_MEM", "0.6"))
DEFER_RESERVED_FRACTION = float(os.environ.get("MCDSEG_OVERLAP_WGRAD_RESERVED", "0.85"))
WGRAD_STREAM_STATS = {"deferred": 0, "no_room": 0}  # launches left on the side stream / kept on the main stream for lack of memory
_TOTAL_MEM = {}
_HELD = {}  # device index -> deque of (event behind a deferred weight gradient, [tensors it uses])


def _room_to_defer(device):
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in _TOTAL_MEM:
        _TOTAL_MEM[key] = torch.cuda.get_device_properties(key).total_memory
    # memory IN USE decides (with memory_reserved alone, cached-but-free blocks left by one large pass would latch deferral off for the
    # rest of the run) -- under a higher ceiling on what the allocator HOLDS: the side stream's pool (ForwardFork's leading pass) caches
    # blocks that cannot serve the main stream and that memory_allocated does not see; past the ceiling the allocator is one large
    # request away from its free-everything-and-retry path (14-18 s per step at BASELINE config 5)
    return (torch.cuda.memory_allocated(key) < DEFER_MEM_FRACTION * _TOTAL_MEM[key]
            and torch.cuda.memory_reserved(key) < DEFER_RESERVED_FRACTION * _TOTAL_MEM[key])


def _dgrad_any(desc, dy, wd, dy_cb, dy_bound, w_bound, addend, dx16):
    """the data gradient in the format its consumer is owed: fp32 NCHW, or -- ``dx16``: the convolution's input is an activation of the
    2-byte chain -- bf16 units, straight from the kernel's epilogue where it has one, converted otherwise"""
    if not dx16:
        return _conv_dgrad(desc, dy, wd, dy_cb, dy_bound, w_bound, addend)
    if dy_cb is not None and _is_split(wd) and lib().mcdseg_conv_split_half_ok(ctypes.byref(desc), MATH_ID.get(CONV_MATH, 0), 1):
        return _conv_dgrad_half(desc, dy_cb, dy_bound, wd, w_bound, addend)
    dx = pack_bf16_units(_conv_dgrad(desc, dy, wd, dy_cb, dy_bound, w_bound, None))
    return dx if addend is None else dx + addend


def _conv_backward(desc, x, dy, wd, need_dx, need_dw, dy_cb=None, x_cb=None, dy_bound=None, x_bound=None, w_bound=None, defer=False, param=None,
                   dx_addend=None, dx16=False):
    """(dx, dw).  ``defer``: dw goes to a ``_LateGrad`` node, so mode "2" may leave it on the side stream.  ``param``: the parameter
    behind that node; when its optimizer has left a ``_mcd_grad_sink`` on it (FlatSGD's bucketed all-reduce, MCDSEG_DP_OVERLAP=1) a
    deferred gradient is handed to the sink ON THE SIDE STREAM, right behind its kernels -- the exchange of a bucket then starts when
    its last weight gradient has been enqueued, long before the ``_LateGrad`` nodes pass the gradients on at the end of the pass."""
    mode = OVERLAP_WGRAD
    sink = getattr(param, "_mcd_grad_sink", None) if param is not None else None
    if mode == "2" and not (defer and x_cb is not None and dy_cb is not None):
        mode = "0"  # (without companions the weight gradient measures bounds and caches them on tensors the main stream reads)
    if mode != "0" and LAUNCH_TIMER is not None and LAUNCH_TIMER.wants("conv_wgrad"):
        mode = "0"  # a step whose launches are bracketed by HIP events runs every kernel alone, so that the pairs time kernels
    # (nothing is deferred while the allocator is close to its limit -- BASELINE config 5 -- also for a weight whose optimizer exchanges
    # gradients in buckets: its gradient then reaches the sink as "not early" (below), which spoils the bucket's early start on THIS rank
    # only; the collectives still start in bucket order on every rank, FlatSGD._drain)
    if mode == "2" and not _room_to_defer(x.device):
        mode = "0"
        WGRAD_STREAM_STATS["no_room"] += 1
    if not (need_dx and need_dw and mode != "0"):
        if sink is not None and need_dw:
            sink(param, None)  # this contribution to the weight's gradient reaches p.grad WITHOUT passing through the sink
        return ((_dgrad_any(desc, dy, wd, dy_cb, dy_bound, w_bound, dx_addend, dx16) if need_dx else None),
                (_conv_wgrad(desc, x, dy, x_cb, dy_cb, x_bound, dy_bound) if need_dw else None))
    main = torch.cuda.current_stream()
    side = _side_stream(x.device)
    key = side.device.index
    if _scaled() and dy is not None:
        dy_bound = _bound_or_measure(dy, dy_bound)  # measured once, on the main stream, for both consumers
    # (launching wgrad only once dgrad has finished -- so that it would run beside the next BatchNorm backward from its first
    # workgroup on -- is slower: 243 vs 237.6 ms per step; the weight gradient fills the data gradient's partial rounds as it is)
    side.wait_stream(main)
    _LAUNCH.stream, _LAUNCH.keep = side, [x, dy, x_cb, dy_cb, x_bound, dy_bound]
    try:
        dw = _conv_wgrad(desc, x, dy, x_cb, dy_cb, x_bound, dy_bound)
    finally:
        keep, _LAUNCH.stream, _LAUNCH.keep = _LAUNCH.keep, None, None
    dx = _dgrad_any(desc, dy, wd, dy_cb, dy_bound, w_bound, dx_addend, dx16)
    if mode == "1":
        main.wait_stream(side)
        if sink is not None:
            sink(param, None)
        return dx, dw
    if sink is not None:
        with torch.cuda.stream(side):
            sink(param, dw)
    WGRAD_STREAM_STATS["deferred"] += 1
    ev = torch.cuda.Event()
    ev.record(side)
    _PENDING[key] = (ev, main)
    held = _HELD.setdefault(key, collections.deque())
    held.append((ev, keep))
    while len(held) > MAX_LAG:
        main.wait_event(held.popleft()[0])  # (its tensors are dropped with the tuple: the main stream is behind their last use now)
    torch.autograd.Variable._execution_engine.queue_callback(join_side_streams)  # (backstop; the _LateGrad node has waited by then)
    return dx, dw


# Where the BatchNorm backward of a group takes its ReLU mask from: ONE value per group and pass, which ``_channel_reduce`` and
# ``_bn_bwd_apply`` map to their entry points -- the reduce and the apply kernel of a group must see the same mask.
MASK_NONE = "none"   # no ReLU
MASK_Y = "y"         # the fp32 activation
MASK_Y_CB = "y_cb"   # the sign of the leading piece of the activation's companion (compact storage, the 2-byte chain)
MASK_Z = "z"         # recomputed from z: y > 0 <=> the forward kernels' own map of z > 0 (csrc/bn.hip bn_forward_map; BN_ZMASK; no residual enters)
MASK_BITS = "bits"   # the bit-plane the forward pass wrote (RELU_MASK; an fp32 residual)


def _channel_reduce(dy, mask=MASK_NONE, src=None, z=None, mean=None, rstd=None, gamma=None, beta=None, want_bound=False, train=True):
    """(dgamma, dbeta) of a BN (z given) or just the per-channel sum of dy (z None); with ``want_bound`` also the device
    scalar bounding |dz| of the tensor bn_bwd_apply will write from these sums (include/mcdseg.h).  ``mask`` / ``src``: where the
    ReLU mask comes from (MASK_*) and the tensor that holds it -- y, its companion, the bit-plane; MASK_Z reads z and ``beta``."""
    L = lib()
    n, c, hw = dy.shape[0], dy.shape[1], dy.shape[2] * dy.shape[3]
    ws = _ws(L.mcdseg_bn_bwd_workspace_bytes(n, c, hw), dy.device)
    dgamma = torch.empty(c, dtype=torch.float32, device=dy.device) if z is not None else None
    dbeta = torch.empty(c, dtype=torch.float32, device=dy.device)
    bound = torch.empty(1, dtype=torch.float32, device=dy.device) if want_bound else None
    tail = (int(train), n, c, hw, _p(ws), ctypes.c_size_t(ws.numel() * 4), _stream())
    if mask == MASK_BITS:
        with _timed("bn_bwd_reduce", (0, 4 * n * c * hw * 2)):
            check(L.mcdseg_bn_bwd_reduce_mask(_p(dy), _p(src), _p(z), _p(mean), _p(rstd), _p(gamma) if want_bound else None, _p(dgamma),
                                              _p(dbeta), _p(bound), *tail), "bn_bwd_reduce_mask")
    elif mask == MASK_Z:
        with _timed("bn_bwd_reduce", (0, 4 * n * c * hw * 2)):
            check(L.mcdseg_bn_bwd_reduce_zmask(_p(dy), _p(z), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(dgamma), _p(dbeta), _p(bound),
                                               *tail), "bn_bwd_reduce_zmask")
    else:
        with _timed("bn_bwd_reduce", (0, 4 * n * c * hw * (1 + (mask == MASK_Y) + (z is not None)))):
            check(L.mcdseg_bn_bwd_reduce(_p(dy), _p(src) if mask == MASK_Y else None, _p(src) if mask == MASK_Y_CB else None,
                                         MATH_ID.get(CONV_MATH, 0), _p(z), _p(mean), _p(rstd), _p(dgamma), _p(dbeta),
                                         _p(gamma) if want_bound else None, _p(bound), int(train), n, c, hw, int(mask != MASK_NONE),
                                         *tail[4:]), "bn_bwd_reduce")
    return dgamma, dbeta, bound


def _bn_bwd_apply(dy, mask, src, use_cb, z, mean, rstd, gamma, beta, dgamma, dbeta, dz, dres, dz_bound, train):
    """the apply pass behind ``_channel_reduce``, with the same mask source: writes ``dz`` (unless None), ``dres`` (the residual's
    gradient, when the ReLU makes it differ from dy) and -- ``use_cb`` -- the pre-split companion of dz, which it returns.  The plain
    kernel has no form that recomputes the mask from z: for MASK_Z it reads ``src`` = y, which exists whenever it runs."""
    L = lib()
    n, c, hw = dy.shape[0], dy.shape[1], dy.shape[2] * dy.shape[3]
    elems, relu = n * c * hw, mask != MASK_NONE
    p_dres = _p(dres) if relu else None
    rd = 4 * elems * (2 + int(relu)) + 4 * elems * ((dz is not None) + (p_dres is not None))
    if not use_cb:
        with _timed("bn_bwd_apply", (0, rd)):
            check(L.mcdseg_bn_bwd_apply(_p(dy), _p(src), _p(z), _p(mean), _p(rstd), _p(gamma), _p(dgamma), _p(dbeta), _p(dz), p_dres, n, c,
                                        hw, int(relu), int(train), _stream()), "bn_bwd_apply")
        return None
    dz_cb = _cb_alloc(n, c, hw, dy.device)
    math, rd = MATH_ID[CONV_MATH], rd + 2 * PIECES[CONV_MATH] * elems
    if mask == MASK_Z:
        with _timed("bn_bwd_apply_cb", (0, rd - 4 * elems)):
            check(L.mcdseg_bn_bwd_apply_cb_zmask(_p(dy), _p(z), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(dgamma), _p(dbeta), _p(dz),
                                                 _p(dz_cb), _p(dz_bound), math, n, c, hw, int(train), _stream()), "bn_bwd_apply_cb_zmask")
    elif mask == MASK_BITS:
        with _timed("bn_bwd_apply_cb", (0, rd - 4 * elems)):
            check(L.mcdseg_bn_bwd_apply_cb_mask(_p(dy), _p(src), _p(z), _p(mean), _p(rstd), _p(gamma), _p(dgamma), _p(dbeta), _p(dz), p_dres,
                                                _p(dz_cb), _p(dz_bound), math, n, c, hw, int(train), _stream()), "bn_bwd_apply_cb_mask")
    else:
        with _timed("bn_bwd_apply_cb", (0, rd)):
            check(L.mcdseg_bn_bwd_apply_cb(_p(dy), _p(src) if mask == MASK_Y else None, _p(src) if mask == MASK_Y_CB else None, _p(z),
                                           _p(mean), _p(rstd), _p(gamma), _p(dgamma), _p(dbeta), _p(dz), p_dres, _p(dz_cb), _p(dz_bound),
                                           math, n, c, hw, int(relu), int(train), _stream()), "bn_bwd_apply_cb")
    return dz_cb


DEBUG_TAPE = None  # a list: _ConvBNAct.backward appends its intermediate tensors (development only)


# ------------------------------------------------------------------------------------------------ conv + BN + act
def _cb_grid_ok(n, c):
    """the companion kernels put N * C/8 on grid y"""
    return n * (c // 8) <= 65535


def _uncut(desc, wgrad_cb=None):
    """the batch goes through in one launch (arguments: ``_batch_pieces``)"""
    return len(_batch_pieces(desc, wgrad_cb)) == 1


class _GroupPlan:
    """Every host decision of one conv + BN + act group, as plain values: it hangs on ``ctx`` and must keep no tensor alive.
    ``_plan_forward`` fills the first row of slots when the group is called, ``_plan_backward`` the second at the top of a backward pass."""
    __slots__ = ("relu", "training", "has_bias", "has_res", "res_half", "storage", "want_cb", "bits", "y_bound", "stem_window", "x_fp32",
                 "x_virtual", "res_fp32",
                 "stem_tr", "use_cb", "mask", "want_bound", "wgrad_cb", "skip_dz", "y_fp32", "x_fp32_bwd")
    half = property(lambda self: self.storage == "half")        # the 2-byte chain (HALF_STORAGE)
    compact = property(lambda self: self.storage != "fp32")     # no fp32 y is written: the companion IS the activation (ACT_STORAGE)


def _plan_forward(desc, split_w, relu, training, has_bias, x_cb, x_virtual, has_res=False, res_virtual=False, res_cb=False, res_half=False,
                  compact=False, single_piece_only=False, thin_ok=False, no_cb=False, half=False, needs_grad=True):
    """The forward decisions of a group, from its descriptor, the module flags (read now) and what the caller passed.  Tensors enter as
    booleans -- ``x_cb`` / ``res_cb``: it came with a companion; ``*_virtual``: it exists as its companion only; ``res_half``: it is an
    activation of the 2-byte chain; ``split_w``: the packed weights are those of the split kernels -- so no GPU is needed to ask."""
    p = _GroupPlan()
    c, math = desc.Cout, MATH_ID.get(CONV_MATH, 0)
    p.relu, p.training, p.has_bias, p.has_res, p.res_half = relu, training, has_bias, has_res, res_half
    uncut, grid_ok = _uncut(desc), _cb_grid_ok(desc.N, c)
    # this consumer reads fp32: x is materialised first (a batch cut along N keeps its companions -- the split kernels take slices,
    # mcdseg.h Ncb -- except on the thin layers' window kernels, Cin <= 16)
    p.x_fp32 = bool(x_virtual and not (split_w and x_cb and (uncut or desc.Cin > 16)))
    p.x_virtual = bool(x_virtual and not p.x_fp32)
    # the stem: forward on the LDS-window kernel from the zero-padded companion of the network input
    p.stem_window = bool(STEM_WINDOW and split_w and not x_cb and not has_bias and PRESPLIT and desc.Cin % 8 != 0 and not p.x_virtual and uncut
                         and lib().mcdseg_conv_split_window_ok(ctypes.byref(desc), math, 1, 0))
    # the 2-byte chain: this group keeps z, y, dz and the gradients it hands on as one 16-bit value per element (not the thin layers,
    # Cin <= 16: their window weight gradient multiplies BOTH pieces of dz's companion whatever the arithmetic)
    is_half = bool(half and training and split_w and x_cb and not has_bias and _cb_wanted(c) and desc.Cin > 16 and grid_ok and not no_cb
                   and (not has_res or (res_half and res_cb)) and lib().mcdseg_conv_split_half_ok(ctypes.byref(desc), math, 0)
                   and _wgrad_reads_cb(desc))
    # the pre-split companion of y: the scaled arithmetic needs |y|'s bound BEFORE y is written -- train-mode statistics
    # give one (Samuelson), eval-mode running statistics do not (the consumer then measures y)
    p.want_cb = bool(_cb_wanted(c) and grid_ok and (training or not _scaled()) and not no_cb)
    is_compact = bool(compact and p.want_cb and training)
    if is_compact and single_piece_only and c <= 32 and not (thin_ok and c >= 16 and uncut):
        is_compact = False  # the consumer would run its weight gradient on the f32 kernels and read fp32
    p.storage = "half" if is_half else "compact" if is_compact else "fp32"
    p.res_fp32 = bool(res_virtual and not p.want_cb)  # plain bn_apply reads fp32: the residual is materialised first
    p.y_bound = bool(training and _scaled() and _use_split(c))  # with or without a companion: consumers that split y themselves use it too
    # the ReLU bit-plane for this group's backward pass (``_bn_apply`` takes it back where the geometry or the alignment has none)
    p.bits = bool(p.want_cb and RELU_MASK and relu and has_res and training and p.storage == "fp32" and not (res_virtual and res_cb)
                  and needs_grad)
    return p


def _plan_backward(p, desc, split_d, need_x, need_w, need_bias, x_cb, dy_aligned=True):
    """The backward decisions of a group, taken once at the top of a backward pass: what autograd asks for (``need_*``) and the
    alignment of ``dy`` are only known there.  ``split_d``: the data-gradient weights are those of the split kernels; ``x_cb``: the
    input came with a companion."""
    n, c = desc.N, desc.Cout
    if p.half:  # dz exists as the leading companion piece alone, and the convolution's gradients come from companions alone
        if need_w and not _wgrad_reads_cb(desc):
            raise RuntimeError("mcdseg: a group of the 2-byte chain needs a weight-gradient plan that reads companions (%d -> %d channels)"
                               % (desc.Cin, desc.Cout))
        p.stem_tr = p.y_fp32 = p.x_fp32_bwd = False
        p.use_cb = p.want_bound = p.wgrad_cb = p.skip_dz = True
        p.mask = MASK_NONE if not p.relu else MASK_Y_CB if p.has_res else MASK_Z
        return p
    # the stem: no input gradient and an input without a companion, but its weight gradient runs on split operands too
    # (conv_wgrad_thin_tr.hip) -- from the zero-padded companion of the network input and the companion of dz
    p.stem_tr = bool(need_w and not need_x and not x_cb and desc.Cin % 8 != 0 and PRESPLIT and not p.x_virtual and _uncut(desc, True)
                     and c % 8 == 0 and _cb_grid_ok(n, c) and _wgrad_thin_tr(desc))
    x_cb = x_cb or p.stem_tr
    p.use_cb = p.stem_tr or bool((need_x or (need_w and x_cb)) and split_d and _cb_wanted(c) and _cb_grid_ok(n, c))
    p.y_fp32 = p.compact and not p.use_cb  # the plain backward kernels read the fp32 activation for the ReLU mask: y is materialised
    if not p.relu:
        p.mask = MASK_NONE
    elif BN_ZMASK and not p.has_res and (not p.compact or p.use_cb):
        p.mask = MASK_Z
    elif p.bits and p.use_cb and dy_aligned:  # (where the four-pixel backward kernel will run)
        p.mask = MASK_BITS
    else:
        p.mask = MASK_Y_CB if (p.compact and p.use_cb) else MASK_Y
    p.want_bound = bool(_scaled() and (split_d or p.stem_tr or _wgrad_split_plan(desc)))
    # the fp32 dz is skipped when every consumer reads the split companion: dgrad (pre-split gather) and wgrad (pre-split plans); a conv
    # bias gradient or any fallback path still needs it (cut batches keep their companions, see ``_plan_forward``; the stem's window
    # weight gradient takes the whole batch's companions whatever the forward pass was cut into)
    single = p.stem_tr or _uncut(desc) or desc.Cin > 16
    p.wgrad_cb = p.stem_tr or bool(x_cb and p.use_cb and single and _wgrad_reads_cb(desc))
    p.skip_dz = bool(p.use_cb and single and not (p.has_bias and need_bias) and (not need_w or p.wgrad_cb))
    p.x_fp32_bwd = bool(p.x_virtual and need_w and not p.wgrad_cb)  # the weight gradient falls back to a kernel that reads fp32
    return p


def _bn_apply(plan, desc, z, z_bound, mean, rstd, gamma, beta, residual, res_cb, res_bound, y_bound):
    """y = act(bn(z) + residual) in the group's storage form: (y or its stand-in, the companion, the ReLU bit-plane)"""
    L = lib()
    n, c, hw, dev = desc.N, desc.Cout, desc.Ho * desc.Wo, z.device
    elems, has_res, relu = n * c * hw, plan.has_res, int(plan.relu)
    if plan.half:
        y_cb = torch.empty(elems, dtype=torch.int16, device=dev)   # ONE piece: the activation
        with _timed("bn_apply_half", (0, elems * (4 + (2 if has_res else 0)))):
            check(L.mcdseg_bn_apply_half(_p(z), _p(z_bound), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(res_cb) if has_res else None,
                                         _p(res_bound) if has_res else None, _p(y_cb), _p(y_bound), n, c, hw, relu, _stream()), "bn_apply_half")
        return _virtual((n, c, desc.Ho, desc.Wo), dev, torch.bfloat16), y_cb, None
    y = _virtual(z.shape, dev) if plan.compact else torch.empty_like(z)
    if not plan.want_cb:
        with _timed("bn_apply", (0, elems * (8 + (4 if has_res else 0)))):
            check(L.mcdseg_bn_apply(_p(z), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(residual), _p(y), n, c, hw, relu, _stream()), "bn_apply")
        return y, None, None
    rmask = None
    if plan.bits and (z.data_ptr() | y.data_ptr() | residual.data_ptr()) % 16 == 0:
        nbytes = L.mcdseg_bn_relu_mask_bytes(n, c, hw)
        if nbytes > 0:
            rmask = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    plan.bits = rmask is not None
    y_cb = _cb_alloc(n, c, hw, dev)
    math, cb_bytes = MATH_ID[CONV_MATH], 2 * PIECES[CONV_MATH]
    if rmask is not None:
        with _timed("bn_apply_cb", (0, elems * (4 + 4 + cb_bytes + 4) + rmask.numel() * 8)):
            check(L.mcdseg_bn_apply_cb_mask(_p(z), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(residual), _p(y), _p(y_cb), _p(y_bound),
                                            _p(rmask), math, n, c, hw, _stream()), "bn_apply_cb_mask")
    else:
        with _timed("bn_apply_cb", (0, elems * (4 + (0 if plan.compact else 4) + cb_bytes + (4 if has_res else 0)))):
            check(L.mcdseg_bn_apply_cb(_p(z), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(residual) if res_cb is None else None,
                                       _p(res_cb), _p(res_bound) if res_cb is not None else None, None if plan.compact else _p(y),
                                       _p(y_cb), _p(y_bound), math, n, c, hw, relu, _stream()), "bn_apply_cb")
    return y, y_cb, rmask


# the arguments of ``_ConvBNAct.apply``, and so the slots of what its backward returns and of ``ctx.needs_input_grad``
_GroupGrads = collections.namedtuple("_GroupGrads", "x weight gamma beta residual conv_bias call", defaults=(None,) * 7)


class _ConvBNAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, gamma, beta, residual, conv_bias, call):
        L = lib()
        if _FWD_SYNC == "follow":
            _fwd_sync_wait(gamma)  # (ForwardFork: the leading pass is through with this layer)
        desc = conv_desc(x.shape, weight.shape, *call.geom)
        packed, training = call.packed, call.training
        wf, wd, mpf = packed.get(getattr(weight, "_mcd_param", weight), desc)
        w_bound, split_w = packed.w_bound, _is_split(wf)
        x_cb, x_bound, res_cb, res_bound = call.x_cb, call.x_bound, call.res_cb, call.res_bound
        plan = _plan_forward(desc, split_w, call.relu, training, conv_bias is not None, x_cb is not None, call.x_virtual, residual is not None,
                             call.res_virtual, res_cb is not None, call.res_half, call.compact, call.single_piece_only, call.thin_ok,
                             call.no_cb, call.half, any(ctx.needs_input_grad))
        if plan.x_fp32:
            x = materialize(x, x_cb, x_bound)
        if not plan.x_virtual:
            x = _req(x, "conv input")
        if split_w and _scaled():
            x_bound = _bound_or_measure(x, x_bound)
        f_cb = x_cb
        if plan.stem_window:  # (cached on the tensor: the same batch goes through the stem several times per MCD step)
            f_cb, x_bound = split_companion_padded(x, x_bound)
        c, z_bound = desc.Cout, None
        if plan.half:
            z, z_bound, part, rows = _conv_fprop_half(desc, x_cb, x_bound, wf, w_bound, mpf)
        else:
            z, part, rows = _conv_fprop(desc, x, wf, _req(conv_bias, "conv bias"), training, mpf, f_cb, x_bound, w_bound)
        mean = torch.empty(c, dtype=torch.float32, device=z.device)
        rstd = torch.empty(c, dtype=torch.float32, device=z.device)
        if not call.res_virtual:
            residual, res_cb = _req(residual, "residual"), None
        elif plan.res_fp32:
            residual, res_cb = materialize(residual, res_cb, res_bound), None
        y_bound = torch.empty(1, dtype=torch.float32, device=z.device) if plan.y_bound else None
        if plan.y_bound and plan.has_res:
            res_bound = _bound_or_measure(residual, res_bound)
        if training:
            track = call.running_mean is not None
            ws = _ws64(L.mcdseg_bn_stats_workspace_bytes(rows, c), z.device)
            with _timed("bn_stats_finalize", (0, 12 * rows * mpf)):  # (one launch also when it stands for BN_RUNNING_REPEAT forward passes)
                check(L.mcdseg_bn_stats_finalize(_p(part), rows, c, mpf, _p(mean), _p(rstd), _p(call.running_mean) if track else None,
                                                 _p(call.running_var) if track else None, _p(call.nbt) if track else None,
                                                 float(call.momentum), float(call.eps), _p(gamma) if y_bound is not None else None,
                                                 _p(beta) if y_bound is not None else None,
                                                 _p(res_bound) if (y_bound is not None and plan.has_res) else None, _p(y_bound),
                                                 int(BN_RUNNING_REPEAT if track else 1), _p(ws), ctypes.c_size_t(ws.numel() * 8), _stream()),
                      "bn_stats_finalize")
            if _FWD_SYNC == "lead":
                _fwd_sync_record(gamma)
        else:
            check(L.mcdseg_bn_eval_stats(_p(call.running_mean), _p(call.running_var), c, float(call.eps), _p(mean), _p(rstd), _stream()),
                  "bn_eval_stats")
        y, y_cb, rmask = _bn_apply(plan, desc, z, z_bound, mean, rstd, gamma, beta, residual, res_cb, res_bound, y_bound)
        ctx.plan, ctx.desc, ctx.wd, ctx.w_bound = plan, desc, wd, w_bound
        ctx.packed, ctx.pack_key = packed, packed.key  # the data-gradient image is shared and re-packed in place: see backward
        ctx.defer_ok = hasattr(weight, "_mcd_param")  # the weight came through a _LateGrad alias (late_weight_grads)
        ctx.w_param = getattr(weight, "_mcd_param", None)
        if ctx.w_param is None and getattr(weight, "_mcd_grad_sink", None) is not None:
            ctx.w_param = weight  # (no alias -- a second use of the module in one graph: its gradient is reported to the sink as "not early")
        ctx.in_box, ctx.res_box = call.in_box, call.res_box
        ctx.x_cb, ctx.x_bound = x_cb, x_bound  # wgrad reads the input's split companion too (an input of this node: safe to hold)
        ctx.rmask, ctx.z_bound = rmask, z_bound
        ctx.x_half = call.x_half  # the gradient owed to an activation of the 2-byte chain: bf16 units
        keep = plan.compact  # (the companion IS the activation; an fp32 group's backward reads y)
        ctx.save_for_backward(x, z, y, mean, rstd, gamma, y_cb if keep else None, y_bound if keep else None, beta)
        ctx.set_materialize_grads(False)  # no zero-filled "gradient" for the non-differentiable companions
        for t in (y_cb, y_bound):
            if t is not None:
                ctx.mark_non_differentiable(t)
        return y, y_cb, y_bound

    @staticmethod
    def backward(ctx, dy, _dcb=None, _dbound=None):
        if dy is None:
            return tuple(_GroupGrads())
        L = lib()
        plan, desc = ctx.plan, ctx.desc
        x, z, y, mean, rstd, gamma, y_cb, y_bound, beta = ctx.saved_tensors
        if ctx.packed.key != ctx.pack_key:
            # the weight was updated in place (and its packed image re-packed) between this forward and its backward: the data gradient
            # would use the NEW weights -- what torch reports for a saved tensor as "modified by an inplace operation"
            raise RuntimeError("mcdseg: a convolution weight was modified between a forward pass and its backward pass "
                               "(an optimizer stepped the generator while its graph was still alive)")
        need = _GroupGrads(*ctx.needs_input_grad)
        dy = _req(dy, "grad_output", torch.bfloat16 if plan.half else torch.float32)
        _plan_backward(plan, desc, _is_split(ctx.wd), need.x, need.weight, need.conv_bias, ctx.x_cb is not None, dy.data_ptr() % 16 == 0)
        n, c, hw = desc.N, desc.Cout, desc.Ho * desc.Wo
        x_cb, x_bound = ctx.x_cb, ctx.x_bound
        if plan.stem_tr:
            x_cb, x_bound = split_companion_padded(x)
        dz = dres = None
        if plan.half:
            # ``dy`` bf16 units -> dz as the leading companion piece, the residual's gradient as bf16 units
            mask = {MASK_NONE: 0, MASK_Z: 2, MASK_Y_CB: 4}[plan.mask]
            src = _p(y_cb) if plan.mask == MASK_Y_CB else None
            elems = n * c * hw
            ws = _ws(L.mcdseg_bn_bwd_half_workspace_bytes(n, c, hw), dy.device)
            dgamma = torch.empty(c, dtype=torch.float32, device=dy.device)
            dbeta = torch.empty(c, dtype=torch.float32, device=dy.device)
            dz_bound = torch.empty(1, dtype=torch.float32, device=dy.device)
            with _timed("bn_bwd_reduce_half", (0, elems * (4 + (2 if mask == 4 else 0)))):
                check(L.mcdseg_bn_bwd_reduce_half(_p(dy), src, _p(z), _p(ctx.z_bound), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(dgamma),
                                                  _p(dbeta), _p(dz_bound), mask, 1, n, c, hw, _p(ws), ctypes.c_size_t(ws.numel() * 4),
                                                  _stream()), "bn_bwd_reduce_half")
            dz_cb = torch.empty(elems, dtype=torch.int16, device=dy.device)
            if plan.has_res and need.residual:
                dres = torch.empty_like(dy) if plan.relu else dy
            p_dres = _p(dres) if plan.relu else None
            with _timed("bn_bwd_apply_half", (0, elems * (6 + (2 if mask == 4 else 0) + (2 if p_dres is not None else 0)))):
                check(L.mcdseg_bn_bwd_apply_half(_p(dy), src, _p(z), _p(ctx.z_bound), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(dgamma),
                                                 _p(dbeta), _p(dz_cb), _p(dz_bound), p_dres, mask, 1, n, c, hw, _stream()),
                      "bn_bwd_apply_half")
        else:
            if plan.y_fp32:
                y, y_cb = materialize(y, y_cb, y_bound), None
            y_mask = (y if y_cb is None else None) if plan.relu else None
            src = {MASK_NONE: None, MASK_Y: y_mask, MASK_Y_CB: y_cb, MASK_BITS: ctx.rmask, MASK_Z: None if plan.use_cb else y_mask}[plan.mask]
            dgamma, dbeta, dz_bound = _channel_reduce(dy, plan.mask, src, z, mean, rstd, gamma, beta, plan.want_bound, plan.training)
            if plan.has_res and need.residual:
                dres = torch.empty_like(z) if plan.relu else dy
            if not plan.skip_dz:
                dz = torch.empty_like(z)
            dz_cb = _bn_bwd_apply(dy, plan.mask, src, plan.use_cb, z, mean, rstd, gamma, beta, dgamma, dbeta, dz, dres, dz_bound, plan.training)
            if plan.x_fp32_bwd:
                x = materialize(x, ctx.x_cb, ctx.x_bound)
            if DEBUG_TAPE is not None:  # kernel development (tools/op_contention.py): what the BN backward handed to the conv backward
                DEBUG_TAPE.append(dict(dy=dy, dz=dz, dz_cb=dz_cb, dz_bound=dz_bound, dgamma=dgamma, dbeta=dbeta, dres=dres, shape=(n, c, hw),
                                       z=z, y=y_mask, mean=mean, rstd=rstd, gamma=gamma, beta=beta, zmask=plan.mask == MASK_Z))
            if dres is not None and plan.res_half:
                dres = pack_bf16_units(dres)  # (the residual is an activation of the 2-byte chain: its gradient is owed as bf16 units)
        # the gradients this group shares with another producer (GradBox): the shortcut's goes into its box -- or comes back summed when
        # this group happens to be the last -- and the data gradient takes the box's tensor into its epilogue
        if ctx.res_box is not None and dres is not None:
            other, last = ctx.res_box.arrive()
            if last:
                dres = dres if other is None else dres + other
            else:
                ctx.res_box.leave(dres if other is None else dres + other)
                dres = None
        addend, dx_last = ctx.in_box.arrive() if (ctx.in_box is not None and need.x) else (None, True)
        dx, dw = _conv_backward(desc, x, dz, ctx.wd, need.x, need.weight, dz_cb, x_cb, dz_bound, x_bound, ctx.w_bound, defer=ctx.defer_ok,
                                param=ctx.w_param, dx_addend=addend, dx16=ctx.x_half)
        if not dx_last:
            ctx.in_box.leave(dx)
            dx = None
        # a bias in front of train-mode BN has zero gradient up to rounding (BN removes the channel mean);
        # it is still formed, as autograd does in the reference (CBR, models/dilated_fcn.py:632-644)
        dbias = _channel_reduce(dz)[1] if (plan.has_bias and need.conv_bias) else None
        return tuple(_GroupGrads(x=dx, weight=dw, gamma=dgamma if need.gamma else None, beta=dbeta if need.beta else None, residual=dres,
                                 conv_bias=dbias))


def _conv_bn_act_inference(x, conv, bn, relu, residual):
    """eval-mode BN folded into the conv epilogue: one kernel, no z / bn_apply pass, nothing kept for backward"""
    L = lib()
    x = _req(materialize(x), "conv input")
    residual = _req(materialize(residual) if residual is not None else None, "residual")
    desc = conv_desc(x.shape, conv.weight.shape, conv.stride[0], conv.padding[0], conv.dilation[0])
    wf, _, _ = conv._packed.get(conv.weight, desc)
    c = desc.Cout
    scale = torch.empty(c, dtype=torch.float32, device=x.device)
    shift = torch.empty(c, dtype=torch.float32, device=x.device)
    check(L.mcdseg_bn_eval_affine(_p(bn.weight), _p(bn.bias), _p(bn.running_mean), _p(bn.running_var), _p(conv.bias), c,
                                  float(bn.eps), _p(scale), _p(shift), _stream()), "bn_eval_affine")
    y = torch.empty((desc.N, c, desc.Ho, desc.Wo), dtype=torch.float32, device=x.device)
    split = _is_split(wf)
    direct = split and bool(L.mcdseg_conv_split_direct_ok(ctypes.byref(desc)))
    x_bound = _bound_or_measure(x, None) if (split and not direct) else None
    for a, b, d in _launches(desc, _batch_pieces(desc), False):
        with _timed(gemm_kernel_name(desc.Cout, desc.Cin, False, split, False, direct), conv_work(d)):
            args = (_p(scale), _p(shift), _p(residual[a:b]) if residual is not None else None, int(relu), _p(y[a:b]), _stream())
            if split:
                check(L.mcdseg_conv_split_fprop_affine(ctypes.byref(d), MATH_ID[CONV_MATH], _p(x[a:b]), None, _p(x_bound), _p(wf),
                                                       _p(conv._packed.w_bound), *args), "conv_split_fprop_affine")
            else:
                check(L.mcdseg_conv_fprop_affine(ctypes.byref(d), _p(x[a:b]), _p(wf), *args), "conv_fprop_affine")
    return y


def conv_bn_act(x, conv, bn, relu=True, residual=None, internal=False, in_box=None, res_box=None, thin_ok=False, shortcut_only=False):
    """y = act(bn(conv(x)) + residual) with the HIP kernels; ``conv``/``bn`` are the parameter-holding modules.
    ``internal``: the caller promises that only the next fused group reads the result (see INTERNAL_SKIP_Y).
    ``shortcut_only``: the caller promises that the result is only ever read as the ``residual`` of another group (a block's 1x1
    projection shortcut): no convolution gathers it, so its pre-split companion is not written (fp32 storage; round 5).
    ``in_box`` / ``res_box``: the ``GradBox`` through which the gradient of ``x`` / of ``residual`` is summed with its other producer."""
    geom = (conv.stride[0], conv.padding[0], conv.dilation[0])
    training = bn.training
    if not training and not torch.is_grad_enabled() and bn.track_running_stats and bn.running_mean is not None:
        return _conv_bn_act_inference(x, conv, bn, relu, residual)
    track = bn.track_running_stats and bn.running_mean is not None
    if not training and not track:
        raise NotImplementedError("mcdseg: eval-mode BatchNorm needs running statistics")
    momentum = 0.1 if bn.momentum is None else bn.momentum
    x_cb, x_bound = _cb_of(x)
    x_cb = _cb_unless_biased_window(x, conv, geom, x_cb)
    if x_cb is not None and conv.in_channels <= 16 and x_cb.numel() == x.numel() and PIECES.get(CONV_MATH, 0) > 1:
        # (the thin layers' window kernels multiply BOTH pieces of their operand whatever the arithmetic; no network of the reference
        # feeds a 16-channel convolution from inside the 2-byte chain, whose groups all have more than 16 input channels)
        raise RuntimeError("mcdseg: a convolution of %d input channels cannot consume a one-piece (2-byte chain) activation" % conv.in_channels)
    res_cb, res_bound = _cb_of(residual) if residual is not None else (None, None)
    skip_y = internal and INTERNAL_SKIP_Y and BN_ZMASK and relu and residual is None and _scaled()
    grads = torch.is_grad_enabled()
    # what the Function needs beside the six tensors autograd must see (read in ``forward`` only: not kept on ``ctx``)
    call = types.SimpleNamespace(running_mean=bn.running_mean if track else None, running_var=bn.running_var if track else None,
                      nbt=bn.num_batches_tracked if track else None, packed=conv._packed, geom=geom, training=training, momentum=momentum,
                      eps=bn.eps, relu=relu, x_cb=x_cb, x_bound=x_bound, res_cb=res_cb, res_bound=res_bound, x_virtual=is_virtual(x),
                      res_virtual=is_virtual(residual), compact=_compact_now() or skip_y, single_piece_only=skip_y and not _compact_now(),
                      thin_ok=thin_ok, no_cb=bool(shortcut_only and SHORTCUT_NO_CB and not relu and residual is None and not _compact_now()),
                      half=_half_now(), x_half=is_half(x), res_half=is_half(residual),  # (x_half: on the tensor autograd knows)
                      in_box=in_box.attach() if (in_box is not None and grads and x.requires_grad) else None,
                      res_box=res_box.attach() if (res_box is not None and grads and residual is not None and residual.requires_grad) else None)
    y, y_cb, y_bound = _ConvBNAct.apply(x, _take_late(conv), bn.weight, bn.bias, residual, conv.bias, call)
    if y_cb is not None or y_bound is not None:
        # the pre-split companion (and the bound) travel with the tensor object to the next convolution; they are only valid for the values
        # y holds NOW: remember the autograd version counter and the storage
        y._mcd_cb = (y_cb, y_bound, y._version, y.data_ptr())
    if y.stride(0) == 0 and y.numel() > 1:
        y._mcd_virtual = True  # compact storage: the companion IS the activation
    return y


def _cb_unless_biased_window(x, conv, geom, x_cb):
    """``x_cb``, or None where handing it on would be refused: given a companion, the library routes a thin 3x3 convolution to the
    LDS-window kernel (csrc/conv_thin_window.hip), which has no bias epilogue.  A convolution WITH a bias at such a geometry (the
    16-channel layers of the U-Net: no DRN has one) reads the fp32 tensor instead and splits it in its K loop -- the same values."""
    if x_cb is None or conv.bias is None or is_virtual(x):
        return x_cb
    return None if _biased_window(conv, x.shape, geom) else x_cb


def _biased_window(conv, x_shape, geom):
    """a convolution with a bias at a geometry that the library, given a companion, routes to the LDS-window kernel"""
    if conv.bias is None or CONV_MATH not in MATH_ID:
        return False
    d = conv_desc(x_shape, conv.weight.shape, *geom)
    return bool(_memo(d, ("biased_window",), lambda: lib().mcdseg_conv_split_window_ok(ctypes.byref(d), MATH_ID[CONV_MATH], 1, 0)))


def conv_reads_companion(conv, x_shape):
    """Will ``conv`` (a parameter holder of models/drn.py), run through ``conv_bn_act`` or ``conv2d_bias`` on an input of this shape, read
    the pre-split companion its producer attaches?  What a producer that knows its one consumer asks before it writes one
    (``max_pool2`` / ``relu`` / ``up_join`` take the answer as ``companion=``): no for the biased thin layers above, and where the layout
    does not apply."""
    n, c = int(x_shape[0]), int(x_shape[1])
    geom = (conv.stride[0], conv.padding[0], conv.dilation[0])
    return bool(_cb_wanted(c) and _cb_grid_ok(n, c) and not _biased_window(conv, x_shape, geom))


def _cb_of(x):
    """(pre-split companion, bound scalar) attached by the producer of ``x``: (None, None) if ``x`` did not come straight from a
    fused BN group, or if anything wrote to ``x`` since (an in-place op of the caller -- ``x.add_()``, ``relu_()``, inplace
    dropout -- bumps ``x._version``; the consumer then splits the current values itself instead of reading a stale image)"""
    rec = getattr(x, "_mcd_cb", None)
    if rec is None:
        return None, None
    cb, bound, version, ptr = rec
    if x._version != version or x.data_ptr() != ptr or not (x.is_contiguous() or is_virtual(x)):
        return None, None
    if cb is not None and cb.numel() != PIECES.get(CONV_MATH, 0) * x.numel() and not (CONV_MATH == "f16x1" and cb.numel() == x.numel()):
        cb = None  # (f16x1 reads the leading piece only: a one-piece companion of the 2-byte chain serves every consumer)
    return cb, (bound if _scaled() else None)


# ------------------------------------------------------------------------------------------------ stage join (middle fusion)
def fused_join():
    """MCDSEG_FUSED_JOIN=0 (host-side, read at every call): ``stage_join`` composes its result from ``a + b`` and ``split_companion``
    with the bound ``bound_a + bound_b`` instead of the one-pass kernel -- bitwise the same; the parity test's other side and the
    timing baseline"""
    return os.environ.get("MCDSEG_FUSED_JOIN", "1") != "0"


class _StageJoin(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, a_bound, b_bound, want_cb, fused):
        n, c, h, w = a.shape
        hw = h * w
        y_bound = None
        if fused:
            y = torch.empty_like(a)
            y_cb = _cb_alloc(n, c, hw, a.device) if want_cb else None
            if a_bound is not None:
                y_bound = torch.empty(1, dtype=torch.float32, device=a.device)
            cb_bytes = 2 * PIECES[CONV_MATH] if want_cb else 0
            with _timed("stage_join", (0, n * c * hw * (12 + cb_bytes))):
                check(lib().mcdseg_stage_join(_p(a), _p(a_bound), _p(b), _p(b_bound), _p(y), _p(y_cb), _p(y_bound), MATH_ID.get(CONV_MATH, 0),
                                              n, c, hw, _stream()), "stage_join")
        else:
            y = a + b
            if a_bound is not None:
                y_bound = a_bound + b_bound
            y_cb = split_companion(y, y_bound)[0] if want_cb else None
        ctx.set_materialize_grads(False)
        for t in (y_cb, y_bound):
            if t is not None:
                ctx.mark_non_differentiable(t)
        return y, y_cb, y_bound

    @staticmethod
    def backward(ctx, dy, _dcb=None, _dbound=None):
        return dy, dy, None, None, None, None  # d(a + b): the incoming gradient, to both


def stage_join(a, b):
    """y = a + b between two stage outputs of the FuseNet-style generator (models/dilated_fcn.py FuseDRNSegBase), with what the next
    stage's convolutions read attached to ``y`` the way ``conv_bn_act`` attaches it: the pre-split companion -- exactly when
    ``_cb_wanted(C)`` and the grid fits -- and the bound ``bound_a + bound_b`` (|a + b| cannot exceed it: nothing is measured unless a
    producer supplied no bound).  The incoming gradient goes to both inputs.  Without grad mode and with inputs that carry neither a
    companion nor a bound (the folded-BN inference kernels write none, and read none) only ``y`` is written."""
    if is_virtual(a) or is_virtual(b):
        raise RuntimeError("mcdseg: stage_join takes fp32 stage outputs, not activations kept as their companions")
    if a.shape != b.shape or a.dim() != 4:
        raise ValueError("mcdseg: stage_join takes two NCHW tensors of one shape, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    a, b = _req(a, "stage_join input"), _req(b, "stage_join input")
    n, c = a.shape[0], a.shape[1]
    recs = (_cb_of(a), _cb_of(b))
    plain = not torch.is_grad_enabled() and all(cb is None and bound is None for cb, bound in recs)
    want_cb = bool(not plain and _cb_wanted(c) and _cb_grid_ok(n, c))
    a_bound = b_bound = None
    if _scaled() and not plain and (want_cb or _use_split(c)):
        a_bound, b_bound = _bound_or_measure(a, recs[0][1]), _bound_or_measure(b, recs[1][1])
    y, y_cb, y_bound = _StageJoin.apply(a, b, a_bound, b_bound, want_cb, fused_join())
    if y_cb is not None or y_bound is not None:
        y._mcd_cb = (y_cb, y_bound, y._version, y.data_ptr())
    return y


# ------------------------------------------------------------------------------------------------ U-Net: pool, up-convolution + join, ReLU
def fused_unet():
    """MCDSEG_FUSED_UNET=0 (host-side, read at every call): ``max_pool2``, ``up_join`` and ``relu`` compose their results from
    ``F.max_pool2d``, ``F.conv_transpose2d`` + ``torch.cat``, ``torch.relu`` and ``split_companion`` instead of the kernels of
    csrc/unet.hip -- the pool and the ReLU bitwise the same, the up-convolution another summation order; the parity test's other side and
    the timing baseline"""
    return os.environ.get("MCDSEG_FUSED_UNET", "1") != "0"


def _unary_plan(x, what, companion=True):
    """what ``max_pool2`` and ``relu`` decide alike, by ``stage_join``'s rules: (x, plain, want_cb, x_bound).  ``companion=False``: the
    caller knows that nothing will read a companion of the result (``conv_reads_companion``) -- none is written, and a bound is handed on
    only where ``x`` carries one already (nothing is measured for a reader that may not exist)"""
    if is_virtual(x):
        raise RuntimeError("mcdseg: %s takes an fp32 activation, not one kept as its companion" % what)
    if x.dim() != 4:
        raise ValueError("mcdseg: %s takes an NCHW tensor, got %s" % (what, tuple(x.shape)))
    x = _req(x, what + " input")
    n, c = x.shape[0], x.shape[1]
    cb, bound = _cb_of(x)
    plain = not torch.is_grad_enabled() and cb is None and bound is None
    want_cb = bool(companion and not plain and _cb_wanted(c) and _cb_grid_ok(n, c))
    x_bound = None
    if _scaled() and not plain and (want_cb or _use_split(c)):
        x_bound = _bound_or_measure(x, bound) if companion else bound
    return x, plain, want_cb, x_bound


def _attach(y, y_cb, y_bound):
    if y_cb is not None or y_bound is not None:
        y._mcd_cb = (y_cb, y_bound, y._version, y.data_ptr())
    return y


class _MaxPool2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, x_bound, want_cb):
        n, c, h, w = x.shape
        y = torch.empty((n, c, h // 2, w // 2), dtype=torch.float32, device=x.device)
        y_cb = _cb_alloc(n, c, (h // 2) * (w // 2), x.device) if want_cb else None
        y_bound = torch.empty(1, dtype=torch.float32, device=x.device) if x_bound is not None else None
        cb_bytes = 2 * PIECES[CONV_MATH] if want_cb else 0
        with _timed("maxpool2_fwd", (0, n * c * (h // 2) * (w // 2) * (20 + cb_bytes))):
            check(lib().mcdseg_maxpool2_fwd(_p(x), _p(x_bound), _p(y), _p(y_cb), _p(y_bound), MATH_ID.get(CONV_MATH, 0), n, c, h, w,
                                            _stream()), "maxpool2_fwd")
        ctx.save_for_backward(x)
        ctx.set_materialize_grads(False)
        for t in (y_cb, y_bound):
            if t is not None:
                ctx.mark_non_differentiable(t)
        return y, y_cb, y_bound

    @staticmethod
    def backward(ctx, dy, _dcb=None, _dbound=None):
        if dy is None:
            return None, None, None
        (x,) = ctx.saved_tensors
        n, c, h, w = x.shape
        dy = _req(dy, "grad_output")
        dx = torch.empty_like(x)
        with _timed("maxpool2_bwd", (0, n * c * h * w * 9)):
            check(lib().mcdseg_maxpool2_bwd(_p(x), _p(dy), _p(dx), n, c, h, w, _stream()), "maxpool2_bwd")
        return dx, None, None


def max_pool2(x, companion=True):
    """``nn.MaxPool2d(kernel_size=2)`` (models/unet.py:135-159) with what the next convolution reads attached to the result the way
    ``stage_join`` attaches it: the pre-split companion -- when ``_cb_wanted(C)`` and the grid fits -- and the bound of ``x`` (|max|
    cannot exceed it).  Ties and NaN by torch's CPU rule; the backward recomputes the arg-max from ``x``.  Without grad mode and with an
    input that carries neither a companion nor a bound only ``y`` is written.  ``companion=False``: see ``_unary_plan``."""
    if x.dim() == 4 and (x.shape[2] % 2 or x.shape[3] % 2):  # (refused before anything -- a bound's measurement included -- is launched)
        raise ValueError("mcdseg: max_pool2 takes even H and W, got %d x %d" % (x.shape[2], x.shape[3]))
    x, plain, want_cb, x_bound = _unary_plan(x, "max_pool2", companion)
    if not fused_unet():
        y = torch.nn.functional.max_pool2d(x, 2)
        return _attach(y, split_companion(y, x_bound)[0] if want_cb else None, x_bound)
    return _attach(*_MaxPool2.apply(x, x_bound, want_cb))


class _ReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, x_bound, want_cb):
        n, c, h, w = x.shape
        y = torch.empty_like(x)
        y_cb = _cb_alloc(n, c, h * w, x.device) if want_cb else None
        y_bound = torch.empty(1, dtype=torch.float32, device=x.device) if x_bound is not None else None
        cb_bytes = 2 * PIECES[CONV_MATH] if want_cb else 0
        with _timed("relu_fwd", (0, n * c * h * w * (8 + cb_bytes))):
            check(lib().mcdseg_relu_fwd(_p(x), _p(x_bound), _p(y), _p(y_cb), _p(y_bound), MATH_ID.get(CONV_MATH, 0), n, c, h * w, _stream()),
                  "relu_fwd")
        ctx.save_for_backward(y)
        ctx.set_materialize_grads(False)
        for t in (y_cb, y_bound):
            if t is not None:
                ctx.mark_non_differentiable(t)
        return y, y_cb, y_bound

    @staticmethod
    def backward(ctx, dy, _dcb=None, _dbound=None):
        if dy is None:
            return None, None, None
        (y,) = ctx.saved_tensors
        dy = _req(dy, "grad_output")
        dx = torch.empty_like(y)
        with _timed("relu_bwd", (0, y.numel() * 12)):
            check(lib().mcdseg_relu_bwd(_p(y), _p(dy), _p(dx), y.numel(), _stream()), "relu_bwd")
        return dx, None, None


def relu(x, companion=True):
    """the ``nn.ReLU`` behind a convolution without BatchNorm (``UNetConv(..., is_batchnorm=False)``, models/unet.py:18-21): a negative
    value becomes +0, anything else passes (torch's clamp), with the companion and the bound of ``x`` attached as ``max_pool2`` does
    (``companion=False``: as there).  Backward: dx = y > 0 ? dy : 0."""
    x, plain, want_cb, x_bound = _unary_plan(x, "relu", companion)
    if not fused_unet():
        y = torch.relu(x)
        return _attach(y, split_companion(y, x_bound)[0] if want_cb else None, x_bound)
    return _attach(*_ReLU.apply(x, x_bound, want_cb))


class _UpJoin(torch.autograd.Function):
    @staticmethod
    def forward(ctx, shortcut, h, weight, bias):
        L = lib()
        n, cin, hh, wh = h.shape
        cs, cout = shortcut.shape[1], weight.shape[1]
        ct, hw4 = cs + cout, 4 * hh * wh
        y = torch.empty((n, ct, 2 * hh, 2 * wh), dtype=torch.float32, device=h.device)
        if cs:
            y[:, :cs].copy_(shortcut)  # the copy torch.cat makes
        with _timed("deconv2x2_fwd", (2 * n * hw4 * cin * cout, 4 * n * hh * wh * (cin + 4 * cout))):
            check(L.mcdseg_deconv2x2_fwd(_p(h), _p(weight), _p(bias), _p(y), ct * hw4, ct, cs, n, cin, cout, hh, wh, _stream()), "deconv2x2_fwd")
        ctx.save_for_backward(h, weight)
        ctx.cs, ctx.has_bias = cs, bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        L = lib()
        h, weight = ctx.saved_tensors
        n, cin, hh, wh = h.shape
        cs, cout = ctx.cs, weight.shape[1]
        ct, hw4 = cs + cout, 4 * hh * wh
        dy = _req(dy, "grad_output")
        need_s, need_h, need_w, need_b = ctx.needs_input_grad
        ds = dy[:, :cs] if (need_s and cs) else None  # the lower slice of the incoming gradient, as torch.cat's backward hands it on
        dh = dw = db = None
        if need_h:
            dh = torch.empty_like(h)
            with _timed("deconv2x2_bwd_data", (2 * n * hw4 * cin * cout, 4 * n * hh * wh * (cin + 4 * cout))):
                check(L.mcdseg_deconv2x2_bwd_data(_p(dy), ct * hw4, ct, cs, _p(weight), _p(dh), n, cin, cout, hh, wh, _stream()),
                      "deconv2x2_bwd_data")
        if need_w or (need_b and ctx.has_bias):
            dw = torch.empty_like(weight)
            db = torch.empty(cout, dtype=torch.float32, device=h.device) if ctx.has_bias else None
            ws = _ws64(L.mcdseg_deconv2x2_bwd_weight_workspace_bytes(n, cin, cout, hh, wh), h.device)
            with _timed("deconv2x2_bwd_weight", (2 * n * hw4 * cin * cout, 4 * n * hh * wh * (cin + 4 * cout))):
                check(L.mcdseg_deconv2x2_bwd_weight(_p(h), _p(dy), ct * hw4, ct, cs, _p(dw), _p(db), n, cin, cout, hh, wh, _p(ws),
                                                    ctypes.c_size_t(ws.numel() * 8), _stream()), "deconv2x2_bwd_weight")
        return ds, dh, dw if need_w else None, db if (need_b and ctx.has_bias) else None


def up_join(shortcut, h, up_weight, up_bias, companion=True):
    """``torch.cat([shortcut, up(h)], 1)`` with ``up = nn.ConvTranspose2d(Cin, Cout, kernel_size=2, stride=2)`` (``UNetUp.forward``,
    models/unet.py:38-43, at offset 0): one [N, Cs + Cout, 2H, 2W] buffer, ``shortcut`` copied into channels [0, Cs) and the up-convolution
    written straight into [Cs, Cs + Cout).  ``up_weight`` is torch's [Cin, Cout, 2, 2] parameter, read as it is.  The backward hands
    ``shortcut`` the lower slice of the incoming gradient and forms dh, dw, db from the upper slice in place.  The result carries a
    companion and a bound by ``stage_join``'s rules -- the bound measured: an up-convolution has no bound known in advance.
    ``companion=False`` (the caller knows that no reader of a companion follows, ``conv_reads_companion``): neither is formed."""
    for t, name in ((shortcut, "shortcut"), (h, "h")):
        if is_virtual(t):
            raise RuntimeError("mcdseg: up_join takes fp32 activations, not ones kept as their companions (%s)" % name)
    if shortcut.dim() != 4 or h.dim() != 4 or up_weight.dim() != 4 or tuple(up_weight.shape[2:]) != (2, 2) or up_weight.shape[0] != h.shape[1]:
        raise ValueError("mcdseg: up_join takes NCHW tensors and a [Cin, Cout, 2, 2] weight, got %s, %s and %s"
                         % (tuple(shortcut.shape), tuple(h.shape), tuple(up_weight.shape)))
    if shortcut.shape[0] != h.shape[0] or shortcut.shape[2] != 2 * h.shape[2] or shortcut.shape[3] != 2 * h.shape[3]:
        raise ValueError("mcdseg: up_join takes a shortcut of twice the size of h (the reference pads or crops: not built), got %s and %s"
                         % (tuple(shortcut.shape), tuple(h.shape)))
    shortcut, h = _req(shortcut, "up_join shortcut"), _req(h, "up_join input")
    up_weight, up_bias = _req(up_weight, "up_join weight"), _req(up_bias, "up_join bias")
    recs = (_cb_of(shortcut), _cb_of(h))
    plain = not torch.is_grad_enabled() and all(cb is None and bound is None for cb, bound in recs)
    if fused_unet():
        y = _UpJoin.apply(shortcut, h, up_weight, up_bias)
    else:
        y = torch.cat([shortcut, torch.nn.functional.conv_transpose2d(h, up_weight, up_bias, stride=2)], 1)
    n, c = y.shape[0], y.shape[1]
    if plain or not companion:
        return y
    if _cb_wanted(c) and _cb_grid_ok(n, c):
        return _attach(y, *split_companion(y))
    return _attach(y, None, _bound_or_measure(y, None) if _use_split(c) else None)


# ------------------------------------------------------------------------------------------------ conv (+bias)
class _Conv2dBias(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, packed, geom, x_cb, x_bound):
        x = _req(x, "conv input")
        desc = conv_desc(x.shape, weight.shape, *geom)
        wf, wd, mpf = packed.get(getattr(weight, "_mcd_param", weight), desc)
        if _is_split(wf) and _scaled():
            x_bound = _bound_or_measure(x, x_bound)
        y, _, _ = _conv_fprop(desc, x, wf, _req(bias, "conv bias"), False, mpf, x_cb, x_bound, packed.w_bound)
        ctx.desc, ctx.wd, ctx.has_bias, ctx.w_bound = desc, wd, bias is not None, packed.w_bound
        ctx.x_bound = x_bound
        ctx.packed, ctx.pack_key = packed, packed.key
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        if ctx.packed.key != ctx.pack_key:
            raise RuntimeError("mcdseg: a convolution weight was modified between a forward pass and its backward pass")
        dy = _req(dy, "grad_output")
        dx, dw = _conv_backward(ctx.desc, x, dy, ctx.wd, ctx.needs_input_grad[0], ctx.needs_input_grad[1], None, None, None, ctx.x_bound,
                                ctx.w_bound)
        db = None
        if ctx.has_bias and ctx.needs_input_grad[2]:
            _, db, _ = _channel_reduce(dy)
        return dx, dw, db, None, None, None, None


def conv2d_bias(x, conv):
    geom = (conv.stride[0], conv.padding[0], conv.dilation[0])
    if is_virtual(x):
        raise RuntimeError("mcdseg: a compact activation left its trunk (the trunk's last layer writes fp32)")
    x_cb, x_bound = _cb_of(x)
    x_cb = _cb_unless_biased_window(x, conv, geom, x_cb)
    if _FWD_SYNC == "follow" and _FWD_LEAD_DONE is not None:
        # a convolution without BatchNorm has no per-layer event: the follower of a ForwardFork runs it behind the whole leading pass
        torch.cuda.current_stream().wait_event(_FWD_LEAD_DONE)
    return _Conv2dBias.apply(x, conv.weight, conv.bias, conv._packed, geom, x_cb, x_bound)


# ------------------------------------------------------------------------------------------------ x8 up-sampler
def _up8_bwd_input(dy, w, n, c, hi, wi):
    dx = torch.empty((n, c, hi, wi), dtype=torch.float32, device=dy.device)
    with _timed("up8_bwd_input", (0, 4 * n * c * hi * wi * 65)):
        check(lib().mcdseg_up8_bwd_input(_p(dy), _p(w), _p(dx), n, c, hi, wi, _stream()), "up8_bwd_input")
    return dx


def _up8_bwd_weight(dy, x, n, c, hi, wi):
    L = lib()
    ws = _ws(L.mcdseg_up8_bwd_weight_workspace_bytes(n, c, hi, wi), dy.device)
    dw = torch.empty((c, 1, 16, 16), dtype=torch.float32, device=dy.device)
    with _timed("up8_bwd_weight", (0, 4 * n * c * hi * wi * 65)):
        check(L.mcdseg_up8_bwd_weight(_p(dy), _p(x), _p(dw), n, c, hi, wi, _p(ws), ctypes.c_size_t(ws.numel() * 4), _stream()),
              "up8_bwd_weight")
    return dw


def _up8_bwd(dy, w, x, want_dx, want_dw):
    """(dx, dw) of the up-sampler from one staged read of ``dy`` (csrc/up8.hip: up8_bwd_band_kernel); either may be skipped"""
    if not (want_dx or want_dw):
        return None, None
    L = lib()
    n, c, hi, wi = x.shape
    dx = torch.empty((n, c, hi, wi), dtype=torch.float32, device=dy.device) if want_dx else None
    dw = torch.empty((c, 1, 16, 16), dtype=torch.float32, device=dy.device) if want_dw else None
    ws = _ws(L.mcdseg_up8_bwd_workspace_bytes(n, c, hi, wi), dy.device) if want_dw else None
    name = "up8_bwd_band_kernel<%s, %s>" % ("true" if want_dx else "false", "true" if want_dw else "false")
    with _timed(name, (0, 4 * n * c * hi * wi * (64 + int(want_dx) + int(want_dw)))):
        check(L.mcdseg_up8_bwd(_p(dy), _p(w), _p(x), _p(dx), _p(dw), n, c, hi, wi, _p(ws),
                               ctypes.c_size_t(ws.numel() * 4 if ws is not None else 0), _stream()), "up8_bwd")
    return dx, dw


def _check_up(x, w):
    if x.dim() != 4 or tuple(w.shape) != (x.shape[1], 1, 16, 16):
        raise ValueError("mcdseg: up8 expects x [N,C,H,W] and w [C,1,16,16], got %s / %s" % (tuple(x.shape), tuple(w.shape)))


class _Up8(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):
        x, w = _req(x, "up8 input"), _req(w, "up8 weight")
        _check_up(x, w)
        n, c, hi, wi = x.shape
        y = torch.empty((n, c, 8 * hi, 8 * wi), dtype=torch.float32, device=x.device)
        with _timed("up8_fwd", (0, 4 * n * c * hi * wi * 65)):
            check(lib().mcdseg_up8_fwd(_p(x), _p(w), None, None, _p(y), n, c, hi, wi, _stream()), "up8_fwd")
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = _req(dy, "grad_output")
        n, c, hi, wi = x.shape
        return _up8_bwd(dy, w, x, ctx.needs_input_grad[0], ctx.needs_input_grad[1])


class _Up8Dual(torch.autograd.Function):
    """up(x1, w1) + up(x2, w2) in one pass over the full-resolution output."""

    @staticmethod
    def forward(ctx, x1, w1, x2, w2):
        x1, w1, x2, w2 = _req(x1, "up8 input"), _req(w1, "up8 weight"), _req(x2, "up8 input"), _req(w2, "up8 weight")
        _check_up(x1, w1), _check_up(x2, w2)
        if x1.shape != x2.shape:
            raise ValueError("mcdseg: up8_dual inputs differ in shape")
        n, c, hi, wi = x1.shape
        y = torch.empty((n, c, 8 * hi, 8 * wi), dtype=torch.float32, device=x1.device)
        with _timed("up8_fwd", (0, 4 * n * c * hi * wi * 66)):
            check(lib().mcdseg_up8_fwd(_p(x1), _p(w1), _p(x2), _p(w2), _p(y), n, c, hi, wi, _stream()), "up8_fwd")
        ctx.save_for_backward(x1, w1, x2, w2)
        return y

    @staticmethod
    def backward(ctx, dy):
        x1, w1, x2, w2 = ctx.saved_tensors
        dy = _req(dy, "grad_output")
        n, c, hi, wi = x1.shape
        need = ctx.needs_input_grad
        return _up8_bwd(dy, w1, x1, need[0], need[1]) + _up8_bwd(dy, w2, x2, need[2], need[3])


def up8(x, w):
    return _Up8.apply(x, w)


def up8_dual(x1, w1, x2, w2):
    return _Up8Dual.apply(x1, w1, x2, w2)


# ------------------------------------------------------------------------------------------------ multitask decoder
class _Bilinear8(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _req(x, "bilinear8 input")
        n, c, hi, wi = x.shape
        y = torch.empty((n, c, 8 * hi, 8 * wi), dtype=torch.float32, device=x.device)
        check(lib().mcdseg_bilinear8_fwd(_p(x), _p(y), n, c, hi, wi, _stream()), "bilinear8_fwd")
        ctx.shape = (n, c, hi, wi)
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _req(dy, "grad_output")
        n, c, hi, wi = ctx.shape
        dx = torch.empty((n, c, hi, wi), dtype=torch.float32, device=dy.device)
        check(lib().mcdseg_bilinear8_bwd(_p(dy), _p(dx), n, c, hi, wi, _stream()), "bilinear8_bwd")
        return dx


def bilinear8(x):
    """nn.Upsample(scale_factor=8, mode='bilinear') with align_corners=False"""
    return _Bilinear8.apply(x)


class _MSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target):
        L = lib()
        pred, target = _req(pred, "mse input"), _req(target, "mse target")
        if pred.shape != target.shape:
            raise ValueError("mcdseg: mse_loss shapes differ: %s vs %s" % (tuple(pred.shape), tuple(target.shape)))
        n = pred.numel()
        grad = torch.empty_like(pred) if ctx.needs_input_grad[0] else None
        loss = torch.empty(1, dtype=torch.float32, device=pred.device)
        ws = _ws(L.mcdseg_mse_workspace_bytes(n), pred.device)
        check(L.mcdseg_mse(_p(pred), _p(target), _p(grad), _p(loss), n, _p(ws), ctypes.c_size_t(ws.numel() * 4), _stream()), "mse")
        ctx.g = grad
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        g, ctx.g = ctx.g, None
        return _scale_(g, _req(grad_out.reshape(1), "grad_output")), None


def mse_loss(pred, target):
    return _MSE.apply(pred, target)


# ------------------------------------------------------------------------------------------------ boundary branch (seg + boundary decoder)
def _ws64(nbytes, device):
    return torch.empty(int(nbytes) // 8 + 1, dtype=torch.float64, device=device)


def _req_labels(t, name):
    """an integer label map: int64, or the uint8 ``predict_labels`` writes"""
    if t is not None and t.is_cuda and t.dtype not in (torch.int64, torch.uint8):
        raise TypeError("mcdseg: %s must be torch.int64 or torch.uint8, got %s" % (name, t.dtype))
    return _req(t, name, t.dtype if t is not None and t.is_cuda else torch.int64)


def label_boundary(labels):
    """uint8 [N,H,W]: 1 where the 3x3 dilation and the 3x3 erosion of the label map differ (``get_boundary``,
    models/dilated_fcn.py:770-774); labels int64 or uint8 [N,H,W]"""
    labels = _req_labels(labels, "labels")
    if labels.dim() != 3:
        raise ValueError("mcdseg: label_boundary takes labels [N,H,W], got %s" % (tuple(labels.shape),))
    n, h, w = labels.shape
    out = torch.empty((n, h, w), dtype=torch.uint8, device=labels.device)
    check(lib().mcdseg_label_boundary(_p(labels), int(labels.dtype == torch.uint8), _p(out), n, h, w, _stream()), "label_boundary")
    return out


def _head_maps(s1, s2, s3):
    s1, s2, s3 = _req(s1, "boundary map s1"), _req(s2, "boundary map s2"), _req(s3, "boundary map s3")
    if s3.dim() != 4 or s3.shape[1] != 1:
        raise ValueError("mcdseg: the boundary head takes 1-channel maps [N,1,h,w], got %s" % (tuple(s3.shape),))
    n, _, h8, w8 = s3.shape
    if tuple(s1.shape) != (n, 1, 4 * h8, 4 * w8) or tuple(s2.shape) != (n, 1, 2 * h8, 2 * w8):
        raise ValueError("mcdseg: the boundary head takes maps at 1/2, 1/4 and 1/8 of one resolution, got %s, %s, %s"
                         % (tuple(s1.shape), tuple(s2.shape), tuple(s3.shape)))
    return s1, s2, s3, n, 8 * h8, 8 * w8


class _BoundaryHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s1, s2, s3):
        s1, s2, s3, n, h, w = _head_maps(s1, s2, s3)
        p = torch.empty((n, 1, h, w), dtype=torch.float32, device=s1.device)
        check(lib().mcdseg_boundary_head_fwd(_p(s1), _p(s2), _p(s3), _p(p), n, h, w, _stream()), "boundary_head_fwd")
        ctx.save_for_backward(s1, s2, s3)
        return p

    @staticmethod
    def backward(ctx, dp):
        s1, s2, s3 = ctx.saved_tensors
        dp = _req(dp, "grad_output")
        n, _, h, w = dp.shape
        d1, d2, d3 = torch.empty_like(s1), torch.empty_like(s2), torch.empty_like(s3)
        check(lib().mcdseg_boundary_head_bwd(_p(s1), _p(s2), _p(s3), _p(dp), _p(d1), _p(d2), _p(d3), n, h, w, _stream()), "boundary_head_bwd")
        return d1, d2, d3


def boundary_head(s1, s2, s3):
    """(sigmoid(up2 s1) + sigmoid(up4 s2) + sigmoid(up8 s3)) / 3, bilinear with align_corners=False
    (MCDSegBDMultiTaskDecoder.boundary_forward behind its three 1x1 projections, models/dilated_fcn.py:1118-1128)"""
    return _BoundaryHead.apply(s1, s2, s3)


def _bce_target(t):
    if t is not None and t.is_cuda and t.dtype not in (torch.uint8, torch.float32):
        raise TypeError("mcdseg: bce2d target must be torch.uint8 or torch.float32, got %s" % (t.dtype,))
    return _req(t, "bce2d target", t.dtype if t is not None and t.is_cuda else torch.float32)


class _BCE2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, target):
        L = lib()
        p, target = _req(p, "bce2d input"), _bce_target(target)
        if p.numel() != target.numel():
            raise ValueError("mcdseg: bce2d shapes differ: %s vs %s" % (tuple(p.shape), tuple(target.shape)))
        n = p.numel()
        out = torch.empty(2, dtype=torch.float32, device=p.device)
        ws = _ws64(L.mcdseg_bce2d_workspace_bytes(n), p.device)
        check(L.mcdseg_bce2d(_p(p), _p(target), int(target.dtype == torch.uint8), _p(out), n, _p(ws), ctypes.c_size_t(ws.numel() * 8),
                             _stream()), "bce2d")
        ctx.save_for_backward(p, target, out)
        ctx.mark_non_differentiable(out)
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, grad_out, _):
        p, target, out = ctx.saved_tensors
        g = _req(grad_out.reshape(1), "grad_output")
        dp = torch.empty_like(p)
        check(lib().mcdseg_bce2d_bwd(_p(p), _p(target), int(target.dtype == torch.uint8), _p(out[1:]), _p(g), _p(dp), p.numel(), _stream()),
              "bce2d_bwd")
        return dp, None


def bce2d(p, target, return_beta=False):
    """class-balanced binary cross-entropy (loss.py:131-138): beta = 1 - mean(t), mean((1 - beta + (2 beta - 1) t) * bce(p, t)) in one
    pass; gradient to ``p`` only.  target: uint8 {0,1} or fp32, as many elements as p."""
    if target.requires_grad:
        raise ValueError("mcdseg: bce2d does not compute the gradient w.r.t. its target")
    loss, out = _BCE2d.apply(p, target)
    return (loss, out[1]) if return_beta else loss


class _BoundaryHeadBCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s1, s2, s3, labels):
        L = lib()
        s1, s2, s3, n, h, w = _head_maps(s1, s2, s3)
        labels = _req(labels, "labels", torch.int64)
        if tuple(labels.shape) != (n, h, w):
            raise ValueError("mcdseg: labels %s do not match the boundary maps' resolution %s" % (tuple(labels.shape), (n, h, w)))
        out = torch.empty(2, dtype=torch.float32, device=s1.device)
        ws = _ws64(L.mcdseg_bce2d_workspace_bytes(n * h * w), s1.device)
        check(L.mcdseg_boundary_head_bce_fwd(_p(s1), _p(s2), _p(s3), _p(labels), _p(out), n, h, w, _p(ws), ctypes.c_size_t(ws.numel() * 8),
                                             _stream()), "boundary_head_bce_fwd")
        ctx.save_for_backward(s1, s2, s3, labels, out)
        return out[0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        s1, s2, s3, labels, out = ctx.saved_tensors
        g = _req(grad_out.reshape(1), "grad_output")
        n, h, w = labels.shape
        d1, d2, d3 = torch.empty_like(s1), torch.empty_like(s2), torch.empty_like(s3)
        check(lib().mcdseg_boundary_head_bce_bwd(_p(s1), _p(s2), _p(s3), _p(labels), _p(out[1:]), _p(g), _p(d1), _p(d2), _p(d3), n, h, w,
                                                 _stream()), "boundary_head_bce_bwd")
        return d1, d2, d3, None


def boundary_head_bce(s1, s2, s3, labels):
    """``bce2d(boundary_head(s1, s2, s3), label_boundary(labels))`` without the two full-resolution maps, forward and backward
    (get_boundary_loss(pred_type="boundary"), models/dilated_fcn.py:743-787, 1202-1204); labels int64 [N,H,W]"""
    return _BoundaryHeadBCE.apply(s1, s2, s3, labels)


# ------------------------------------------------------------------------------------------------ boundary branch (triple decoder)
def _target_planes(t, n, h, w, name):
    """(tensor, batch stride in elements) of a boundary target: n planes [h,w] given as [n,h,w] or [n,1,h,w], uint8 or fp32.  A channel
    slice of a wider batch (planes contiguous, images a fixed distance apart) is read in place; any other non-contiguous layout is copied."""
    if t is None or not t.is_cuda:
        _req(t, name)
    if t.dtype not in (torch.uint8, torch.float32):
        raise TypeError("mcdseg: %s must be torch.uint8 or torch.float32, got %s" % (name, t.dtype))
    if tuple(t.shape) not in ((n, h, w), (n, 1, h, w)):
        raise ValueError("mcdseg: %s %s does not match the resolution %s" % (name, tuple(t.shape), (n, h, w)))
    st = t.stride()
    if st[-1] == 1 and st[-2] == w and (n == 1 or st[0] >= h * w):
        return t, (st[0] if n > 1 else h * w)
    return t.contiguous(), h * w


class _BoundaryHeadBCETarget(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s1, s2, s3, target):
        L = lib()
        s1, s2, s3, n, h, w = _head_maps(s1, s2, s3)
        target, ctx.tstride = _target_planes(target, n, h, w, "boundary target")
        out = torch.empty(2, dtype=torch.float32, device=s1.device)
        ws = _ws64(L.mcdseg_bce2d_workspace_bytes(n * h * w), s1.device)
        check(L.mcdseg_boundary_head_bce_target_fwd(_p(s1), _p(s2), _p(s3), _p(target), int(target.dtype == torch.uint8), ctx.tstride, _p(out),
                                                    n, h, w, _p(ws), ctypes.c_size_t(ws.numel() * 8), _stream()), "boundary_head_bce_target_fwd")
        ctx.save_for_backward(s1, s2, s3, target, out)
        ctx.dims = (n, h, w)
        return out[0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        s1, s2, s3, target, out = ctx.saved_tensors
        g = _req(grad_out.reshape(1), "grad_output")
        n, h, w = ctx.dims
        d1, d2, d3 = torch.empty_like(s1), torch.empty_like(s2), torch.empty_like(s3)
        check(lib().mcdseg_boundary_head_bce_target_bwd(_p(s1), _p(s2), _p(s3), _p(target), int(target.dtype == torch.uint8), ctx.tstride,
                                                        _p(out[1:]), _p(g), _p(d1), _p(d2), _p(d3), n, h, w, _stream()),
              "boundary_head_bce_target_bwd")
        return d1, d2, d3, None


def boundary_head_bce_target(s1, s2, s3, target):
    """``bce2d(boundary_head(s1, s2, s3), target)`` without the full-resolution prediction, forward and backward
    (MCDTripleMultiTaskDecoder.get_boundary_loss, models/dilated_fcn.py:1002-1004); target [N,1,H,W] or [N,H,W], uint8 or fp32, possibly
    one channel of a wider batch"""
    if target.requires_grad:
        raise ValueError("mcdseg: boundary_head_bce_target does not compute the gradient w.r.t. its target")
    return _BoundaryHeadBCETarget.apply(s1, s2, s3, target)


class _Seg2bdBCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z1, z2, weight, bias, target):
        L = lib()
        z1, z2 = _req(z1, "seg2bd logits 1"), _req(z2, "seg2bd logits 2")
        weight, bias = _req(weight, "seg2bd_conv weight"), _req(bias, "seg2bd_conv bias")
        if z1.dim() != 4 or (z2 is not None and z2.shape != z1.shape):
            raise ValueError("mcdseg: seg2bd_bce takes logits [N,C,h,w] of one shape, got %s and %s"
                             % (tuple(z1.shape), None if z2 is None else tuple(z2.shape)))
        n, c, hi, wi = z1.shape
        if tuple(weight.shape) != (1, c, 5, 5) or bias.numel() != 1:
            raise ValueError("mcdseg: seg2bd_bce takes the weight [1,%d,5,5] and bias [1] of nn.Conv2d(C, 1, 5, padding=2), got %s, %s"
                             % (c, tuple(weight.shape), tuple(bias.shape)))
        target, ctx.tstride = _target_planes(target, n, 8 * hi, 8 * wi, "seg2bd target")
        nbytes = L.mcdseg_seg2bd_bce_workspace_bytes(n, c, hi, wi)
        if nbytes == 0:
            raise ValueError("mcdseg: seg2bd_bce cannot take logits of shape %s" % (tuple(z1.shape),))
        ws = _ws64(nbytes, z1.device)
        out = torch.empty(3, dtype=torch.float32, device=z1.device)
        check(L.mcdseg_seg2bd_bce_fwd(_p(z1), _p(z2), _p(weight), _p(bias), _p(target), int(target.dtype == torch.uint8), ctx.tstride, _p(out),
                                      n, c, hi, wi, _p(ws), ctypes.c_size_t(ws.numel() * 8), _stream()), "seg2bd_bce_fwd")
        ctx.save_for_backward(z1, z2, weight, bias, target, out)
        ctx.ws = ws  # (v of the forward pass: what the backward starts from)
        ctx.mark_non_differentiable(out)
        return out[0].clone(), out[1].clone(), out

    @staticmethod
    def backward(ctx, g1, g2, _):
        z1, z2, weight, bias, target, out = ctx.saved_tensors
        n, c, hi, wi = z1.shape
        up = _req(torch.stack([g1.reshape(()), g2.reshape(())]), "grad_output")
        dz1 = torch.empty_like(z1)
        dz2 = None if z2 is None else torch.empty_like(z2)
        dw, db = torch.empty_like(weight), torch.empty_like(bias)
        ws = ctx.ws
        check(lib().mcdseg_seg2bd_bce_bwd(_p(z1), _p(z2), _p(weight), _p(bias), _p(target), int(target.dtype == torch.uint8), ctx.tstride,
                                          _p(out[2:]), _p(up), _p(dz1), _p(dz2), _p(dw), _p(db), n, c, hi, wi, _p(ws),
                                          ctypes.c_size_t(ws.numel() * 8), _stream()), "seg2bd_bce_bwd")
        return dz1, dz2, dw, db, None


def seg2bd_bce(z1, z2, weight, bias, target, return_beta=False):
    """``bce2d(sigmoid(conv2d(bilinear8(z), weight, bias, padding=2)), target)`` for the two heads' low-resolution logits z1, z2 [N,C,h,w]
    (z2 None: one head, loss2 is None) -> (loss1, loss2), from the low-resolution logits in one pass each way: no [N,C,8h,8w] tensor
    exists forward or backward (MCDTripleMultiTaskDecoder.get_boundary_loss_by_extra_conv, models/dilated_fcn.py:960-981).  Gradients go
    to z1, z2, weight [1,C,5,5] and bias [1]; target [N,1,8h,8w] or [N,8h,8w], uint8 or fp32 (soft allowed), possibly one channel of a
    wider batch, is never differentiated."""
    if target.requires_grad:
        raise ValueError("mcdseg: seg2bd_bce does not compute the gradient w.r.t. its target")
    loss1, loss2, out = _Seg2bdBCE.apply(z1, z2, weight, bias, target)
    res = (loss1, None if z2 is None else loss2)
    return res + (out[2],) if return_beta else res


# ------------------------------------------------------------------------------------------------ losses
def label_weight_sum(labels, class_weight, n_class, ignore_index=-100):
    """device scalar sum_i w[labels_i]"""
    L = lib()
    labels = _req(labels, "labels", torch.int64)
    class_weight = _req(class_weight, "class weights")
    out = torch.empty(1, dtype=torch.float32, device=labels.device)
    ws = _ws(L.mcdseg_label_weight_sum_workspace_bytes(labels.numel()), labels.device)
    check(L.mcdseg_label_weight_sum(_p(labels), _p(class_weight), int(ignore_index), int(n_class), labels.numel(), _p(out), _p(ws),
                                    ctypes.c_size_t(ws.numel() * 4), _stream()), "label_weight_sum")
    return out


def ce_normaliser(labels, class_weight, n_class, ignore_index=-100):
    """CE normaliser for this rank: None (kernel computes the local sum) for single-process runs; under data
    parallelism the all-reduced sum divided by world size, so that the optimizer's 1/world gradient average
    reproduces the reference's one global weighted mean."""
    from . import dist as mdist
    if not mdist.is_distributed():
        return None
    w = label_weight_sum(labels, class_weight, n_class, ignore_index)
    mdist.all_reduce_sum_(w)
    return w / mdist.world_size()


# The classifier discrepancies of --d_loss (loss.py:192-210) as the library's distance kinds (include/mcdseg.h MCDSEG_DIST_*): seven names,
# four functions -- Symkl2d's rows and MySymkl2d's ratio are one expression under the element mean, and SpatialJSD2d evaluates MisSymKLD's.
DIST_KINDS = {"diff": 0, "symkl": 1, "nmlsymkl": 1, "mysymkl": 1, "mis_symkl": 2, "spatial_jsd": 2, "jsd": 3}


def dist_kind(dist):
    """the library's kind (0..3) of a ``--d_loss`` name or of a kind; anything else is a ValueError (before the library is touched)"""
    if isinstance(dist, str) and dist in DIST_KINDS:
        return DIST_KINDS[dist]
    if isinstance(dist, int) and not isinstance(dist, bool) and 0 <= dist <= 3:
        return dist
    raise ValueError("mcdseg: unknown probability distance %r (one of %s, or a kind 0..3)" % (dist, ", ".join(sorted(DIST_KINDS))))


def mcd_losses(z1, z2, labels, class_weight, ignore_index=-100, ce_coef=0.0, diff_coef=0.0, want_grad=True, wsum=None, dist="diff"):
    """One fused pass.  Returns (losses[4] = CE1, CE2, Diff, sum w[y]; g1; g2) where
    g_k = ce_coef * dCE_k/dz_k + diff_coef * dDiff/dz_k (None when not requested).  ``dist``: the discrepancy, a ``--d_loss`` name or a
    kind of ``DIST_KINDS`` (anything but "diff" needs both heads)."""
    kind = dist_kind(dist)
    if kind != 0 and z2 is None:
        raise ValueError("mcdseg: the distance %r is taken between two heads" % (dist,))
    L = lib()
    z1 = _req(z1, "logits")
    z2 = _req(z2, "logits")
    if z1.dim() != 4 or (z2 is not None and z2.shape != z1.shape):
        raise ValueError("mcdseg: logits must be [N,C,H,W] and of equal shape")
    n, c, h, w = z1.shape
    if labels is not None:
        labels = _req(labels, "labels", torch.int64)
        if tuple(labels.shape) != (n, h, w):
            raise ValueError("mcdseg: labels must be [N,H,W] = %s, got %s" % ((n, h, w), tuple(labels.shape)))
    class_weight = _req(class_weight, "class weights")
    if class_weight is not None and class_weight.numel() != c:
        raise ValueError("mcdseg: class weight has %d entries for %d classes" % (class_weight.numel(), c))
    if labels is not None and ce_coef != 0.0 and wsum is None:
        wsum = ce_normaliser(labels, class_weight, c, ignore_index)
    wsum = _req(wsum, "CE normaliser")
    losses = torch.empty(4, dtype=torch.float32, device=z1.device)
    g1 = torch.empty_like(z1) if want_grad else None
    g2 = torch.empty_like(z2) if (want_grad and z2 is not None) else None
    ws = _ws(L.mcdseg_loss_workspace_bytes(n, h * w), z1.device)
    nz = (1 if z2 is None else 2) * n * c * h * w
    byts = 4 * nz * (2 if want_grad else 1) + (8 * n * h * w if labels is not None else 0)
    if kind != 0:
        with _timed("softmax_ce_dist_kernel", (0, byts)):
            check(L.mcdseg_softmax_ce_dist(_p(z1), _p(z2), _p(labels), _p(class_weight), int(ignore_index), float(ce_coef),
                                           float(diff_coef), _p(wsum), _p(g1), _p(g2), _p(losses), n, c, h * w, kind, _p(ws),
                                           ctypes.c_size_t(ws.numel() * 4), _stream()), "softmax_ce_dist")
        return losses, g1, g2
    with _timed("softmax_ce_l1_kernel<48, %s>" % ("true" if z2 is not None else "false") if c > 24 else "softmax_ce_l1_kernel", (0, byts)):
        check(L.mcdseg_softmax_ce_l1(_p(z1), _p(z2), _p(labels), _p(class_weight), int(ignore_index), float(ce_coef),
                                     float(diff_coef), _p(wsum), _p(g1), _p(g2), _p(losses), n, c, h * w, _p(ws),
                                     ctypes.c_size_t(ws.numel() * 4), _stream()), "softmax_ce_l1")
    return losses, g1, g2


def up8_loss_kernel_name(n, c, hi, wi, two, labelled, dist="diff"):
    """The kernel ``mcdseg_up8_softmax_ce_l1`` launches for this problem, as rocprofv3 prints it -- from the library's own dispatch
    (``mcdseg_up8_loss_variant``: the LDS-DMA kernel unless the option UP8_LOSS_DMA is 0 or a tensor outgrows a 32-bit buffer resource;
    the benchmark's 41 classes have an instantiation of their own).  ``labelled``: whether the call has labels, or the label tensor itself
    -- labels whose first element is not 16-byte aligned (a view into a larger tensor) run the register-staged kernel."""
    kind = dist_kind(dist)
    two = "true" if two else "false"
    if torch.is_tensor(labelled):
        labelled = 1 if labelled.data_ptr() % 16 == 0 else 2
    else:
        labelled = int(bool(labelled))
    v = lib().mcdseg_up8_loss_variant(int(n), int(c), int(hi), int(wi), labelled)
    if kind != 0:  # ``mcdseg_up8_softmax_ce_dist``: the same dispatch, kernels of their own (two heads always)
        if v > 0:
            return "up8_softmax_ce_dist_dma_kernel<%d, %s, %d>" % (v, "true" if c == v else "false", kind)
        return "up8_softmax_ce_dist_kernel<%d, %d>" % (-v, kind)
    if v > 0:
        return "up8_softmax_ce_l1_dma_kernel<%d, %s, %s>" % (v, two, "true" if c == v else "false")
    return "up8_softmax_ce_l1_kernel<%d, %s>" % (-v, two)


def up8_mcd_losses(s1, w1, s2, w2, labels, class_weight, ignore_index=-100, ce_coef=0.0, diff_coef=0.0, want_grad=True, wsum=None,
                   dist="diff"):
    """``mcd_losses(up8(s1, w1), up8(s2, w2), ...)`` without the full-resolution logits: the kernel forms each pixel's logits
    from the score maps [N,C,Hi,Wi] on the fly.  Returns (losses[4], g1, g2) with g_k [N,C,8Hi,8Wi] = the gradient w.r.t.
    the (never stored) logits of head k -- what ``_up8_bwd_input`` / ``_up8_bwd_weight`` consume."""
    kind = dist_kind(dist)
    if kind != 0 and s2 is None:
        raise ValueError("mcdseg: the distance %r is taken between two heads" % (dist,))
    L = lib()
    s1, w1, s2, w2 = _req(s1, "scores"), _req(w1, "up8 weight"), _req(s2, "scores"), _req(w2, "up8 weight")
    _check_up(s1, w1)
    if s2 is not None:
        _check_up(s2, w2)
        if s2.shape != s1.shape:
            raise ValueError("mcdseg: the two score maps differ in shape")
    n, c, hi, wi = s1.shape
    h, w = 8 * hi, 8 * wi
    if labels is not None:
        labels = _req(labels, "labels", torch.int64)
        if tuple(labels.shape) != (n, h, w):
            raise ValueError("mcdseg: labels must be [N,H,W] = %s, got %s" % ((n, h, w), tuple(labels.shape)))
    class_weight = _req(class_weight, "class weights")
    if class_weight is not None and class_weight.numel() != c:
        raise ValueError("mcdseg: class weight has %d entries for %d classes" % (class_weight.numel(), c))
    if labels is not None and ce_coef != 0.0 and wsum is None:
        wsum = ce_normaliser(labels, class_weight, c, ignore_index)
    wsum = _req(wsum, "CE normaliser")
    losses = torch.empty(4, dtype=torch.float32, device=s1.device)
    g1 = torch.empty((n, c, h, w), dtype=torch.float32, device=s1.device) if want_grad else None
    g2 = torch.empty((n, c, h, w), dtype=torch.float32, device=s1.device) if (want_grad and s2 is not None) else None
    ws = _ws(L.mcdseg_up8_loss_workspace_bytes(n, hi, wi), s1.device)
    heads = 1 if s2 is None else 2
    byts = 4 * heads * n * c * h * w * (1 if want_grad else 0) + 4 * heads * n * c * hi * wi + (8 * n * h * w if labels is not None else 0)
    if kind != 0:
        with _timed(up8_loss_kernel_name(n, c, hi, wi, True, labels, kind), (0, byts)):
            check(L.mcdseg_up8_softmax_ce_dist(_p(s1), _p(w1), _p(s2), _p(w2), _p(labels), _p(class_weight), int(ignore_index),
                                               float(ce_coef), float(diff_coef), _p(wsum), _p(g1), _p(g2), _p(losses), n, c, hi, wi, kind,
                                               _p(ws), ctypes.c_size_t(ws.numel() * 4), _stream()), "up8_softmax_ce_dist")
        return losses, g1, g2
    with _timed(up8_loss_kernel_name(n, c, hi, wi, s2 is not None, labels), (0, byts)):
        check(L.mcdseg_up8_softmax_ce_l1(_p(s1), _p(w1), _p(s2), _p(w2), _p(labels), _p(class_weight), int(ignore_index),
                                         float(ce_coef), float(diff_coef), _p(wsum), _p(g1), _p(g2), _p(losses), n, c, hi, wi,
                                         _p(ws), ctypes.c_size_t(ws.numel() * 4), _stream()), "up8_softmax_ce_l1")
    return losses, g1, g2


def up8_backward(g, s, w, want_input, want_weight):
    """(d/ds, d/dw) of the up-sampler for the logit gradient ``g`` (either may be skipped)."""
    return _up8_bwd(g, w, s, want_input, want_weight)


# ------------------------------------------------------------------------------------------------ Monte-Carlo dropout loss (uncertain model)
def _check_draws(keep, r, n, c):
    keep, r = _req(keep, "dropout keep mask", torch.uint8), _req(r, "dropout draw scalars r")
    if keep.dim() != 3 or tuple(keep.shape[1:]) != (n, c) or tuple(r.shape) != (keep.shape[0],):
        raise ValueError("mcdseg: keep must be uint8 [T,N,C] = [T,%d,%d] and r fp32 [T], got %s / %s" % (n, c, tuple(keep.shape), tuple(r.shape)))
    return keep, r


class _Up8UncertainLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, w_up, w_std, labels, class_weight, keep, r, keep_scale, lam, ignore_index, wsum):
        L = lib()
        s, w_up, w_std = _req(s, "scores"), _req(w_up, "up8 weight"), _req(w_std, "up8 weight (std)")
        _check_up(s, w_up), _check_up(s, w_std)
        n, c, hi, wi = s.shape
        labels = _req(labels, "labels", torch.int64)
        if tuple(labels.shape) != (n, 8 * hi, 8 * wi):
            raise ValueError("mcdseg: labels must be [N,H,W] = %s, got %s" % ((n, 8 * hi, 8 * wi), tuple(labels.shape)))
        class_weight = _req(class_weight, "class weights")
        if class_weight is not None and class_weight.numel() != c:
            raise ValueError("mcdseg: class weight has %d entries for %d classes" % (class_weight.numel(), c))
        keep, r = _check_draws(keep, r, n, c)
        t = keep.shape[0]
        if wsum is None:
            wsum = ce_normaliser(labels, class_weight, c, ignore_index)
        wsum = _req(wsum, "CE normaliser")
        losses = torch.empty(2 + n, dtype=torch.float32, device=s.device)
        ws = _ws(L.mcdseg_up8_uncertain_loss_workspace_bytes(n, hi, wi), s.device)
        with _timed("up8_uncertain_kernel<%s, false>" % uncertain_kernel_classes(c), (0, 8 * n * c * hi * wi + 8 * n * hi * wi * 64)):
            check(L.mcdseg_up8_uncertain_loss_fwd(_p(s), _p(w_up), _p(w_std), _p(labels), _p(class_weight), int(ignore_index), _p(keep), _p(r),
                                                  float(keep_scale), _p(wsum), float(lam), _p(losses), n, c, hi, wi, t, _p(ws),
                                                  ctypes.c_size_t(ws.numel() * 4), _stream()), "up8_uncertain_loss_fwd")
        ctx.save_for_backward(s, w_up, w_std, labels, class_weight, keep, r, losses)
        ctx.consts = (float(keep_scale), float(lam), int(ignore_index))
        return losses[0].clone(), losses[2:].clone()

    @staticmethod
    def backward(ctx, gb, gu):
        s, w_up, w_std, labels, class_weight, keep, r, losses = ctx.saved_tensors
        keep_scale, lam, ignore_index = ctx.consts
        n, c, hi, wi = s.shape
        gb, gu = _req(gb.reshape(1), "grad_output"), _req(gu.reshape(n), "grad_output")
        g_u = torch.empty((n, c, 8 * hi, 8 * wi), dtype=torch.float32, device=s.device)
        g_v = torch.empty_like(g_u)
        with _timed("up8_uncertain_kernel<%s, true>" % uncertain_kernel_classes(c), (0, 8 * n * c * hi * wi * 65 + 8 * n * hi * wi * 64)):
            check(lib().mcdseg_up8_uncertain_loss_bwd(_p(s), _p(w_up), _p(w_std), _p(labels), _p(class_weight), ignore_index, _p(keep), _p(r),
                                                      keep_scale, _p(losses[1:]), lam, _p(gb), _p(gu), _p(g_u), _p(g_v), n, c, hi, wi,
                                                      keep.shape[0], _stream()), "up8_uncertain_loss_bwd")
        need = ctx.needs_input_grad
        ds, dw_up = _up8_bwd(g_u, w_up, s, need[0], need[1])
        del g_u
        ds2, dw_std = _up8_bwd(g_v, w_std, s, need[0], need[2])
        if ds is not None:
            ds.add_(ds2)
        return (ds, dw_up, dw_std) + (None,) * 8


def uncertain_kernel_classes(c):
    """the class count of the instantiation of ``up8_uncertain_kernel`` that serves ``c`` classes (csrc/uncertain.hip: unc_ncmax)"""
    return 16 if c <= 16 else (24 if c <= 24 else (41 if c == 41 else 48))


def up8_uncertain_loss(s, w_up, w_std, labels, class_weight, keep, r, uncertain_weight=0.1, ignore_index=-100, wsum=None, keep_scale=1.25):
    """``UncertainDRNSeg.get_loss`` (models/dilated_fcn.py:169-214) behind the trunk, all T dropout draws in one pass: returns
    ``(base_loss, uncertain_loss[N])`` -- the mean over the draws of CrossEntropyLoss2d(m_t up(s)) and, per sample,
    uncertain_weight * mean_i log((1/T) sum_t softmax(m_t up(s) + m_t relu(up_std(s)) r_t)[label]) -- differentiable w.r.t.
    ``s``, ``w_up`` and ``w_std``.  ``keep``: uint8 [T,N,C], 1 where Dropout2d kept channel c of sample n in draw t (factor
    ``keep_scale`` = 1/(1-p), else 0); ``r``: fp32 [T], the reference's ``np.random.rand()`` per draw.  include/mcdseg.h has the formulas."""
    return _Up8UncertainLoss.apply(s, w_up, w_std, labels, class_weight, keep, r, keep_scale, uncertain_weight, ignore_index, wsum)


def up8_std_sum(s, w_std, n_used=None):
    """``relu(up8(s, w_std))[:, :n_used].sum(1)`` as fp32 [N,8Hi,8Wi] without the C-channel full-resolution tensor: the aleatoric
    uncertainty map of source_uncertain_tester.py:158-166"""
    s, w_std = _req(s, "scores"), _req(w_std, "up8 weight (std)")
    _check_up(s, w_std)
    n, c, hi, wi = s.shape
    n_used = c if n_used is None else int(n_used)
    out = torch.empty((n, 8 * hi, 8 * wi), dtype=torch.float32, device=s.device)
    check(lib().mcdseg_up8_std_sum(_p(s), _p(w_std), _p(out), n, c, n_used, hi, wi, _stream()), "up8_std_sum")
    return out


# ------------------------------------------------------------------------------------------------ the DANN domain classifier (csrc/dann.hip)
class _DannDown(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, groups):
        x, w1, b1, w2, b2 = _req(x, "DownConv input"), _req(w1, "conv1.weight"), _req(b1, "conv1.bias"), _req(w2, "conv2.weight"), _req(b2, "conv2.bias")
        n, cin, h, w = x.shape
        cm = w1.shape[0]
        if tuple(w1.shape) != (cm, cin, 3, 3) or tuple(w2.shape) != (cm, cm, 3, 3) or b1.numel() != cm or b2.numel() != cm:
            raise ValueError("mcdseg: DownConv weights %s / %s do not fit an input of %d channels" % (tuple(w1.shape), tuple(w2.shape), cin))
        y = torch.empty((n, cm, h // 2, w // 2), dtype=torch.float32, device=x.device)
        with _timed("dann_down_fwd_kernel<%d>" % cm, (2 * 9 * n * h * w * cm * (cin + cm), 4 * (x.numel() + y.numel()))):
            check(lib().mcdseg_dann_down_fwd(_p(x), _p(w1), _p(b1), _p(w2), _p(b2), _p(y), n, cin, cm, h, w, _stream()), "dann_down_fwd")
        ctx.save_for_backward(x, w1, b1, w2, b2)
        ctx.groups = int(groups)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w1, b1, w2, b2 = ctx.saved_tensors
        n, cin, h, w = x.shape
        cm = w1.shape[0]
        dy = _req(dy, "grad_output")
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw1, db1, dw2, db2 = torch.empty_like(w1), torch.empty_like(b1), torch.empty_like(w2), torch.empty_like(b2)
        ws = _ws(lib().mcdseg_dann_down_workspace_bytes(n, cin, cm, h, w), x.device)
        with _timed("dann_down_bwd_kernel<%d>" % cm, (2 * 9 * n * h * w * cm * (4 * cin + 3 * cm), 4 * (2 * x.numel() + dy.numel()))):
            check(lib().mcdseg_dann_down_bwd(_p(x), _p(w1), _p(b1), _p(w2), _p(b2), _p(dy), _p(dx), _p(dw1), _p(db1), _p(dw2), _p(db2), n, cin, cm,
                                             h, w, ctx.groups, _p(ws), ctypes.c_size_t(ws.numel() * 4), _stream()), "dann_down_bwd")
        _on_launch_stream(ws)
        return dx, dw1, db1, dw2, db2, None


def dann_down(x, w1, b1, w2, b2, groups=1):
    """One ``DownConv`` of the domain classifier (models/dilated_fcn.py:506-531) in one launch each way:
    ``max_pool2d(relu(conv3x3(relu(conv3x3(x, w1) + b1), w2) + b2), 2, 2)``; include/mcdseg.h has the shapes it takes.  ``groups``: the
    batch holds that many equal groups of samples (domains) whose parameter gradients are summed group by group, so that they equal
    the sum of one call per group bit for bit."""
    return _DannDown.apply(x, w1, b1, w2, b2, groups)


class _DannTail(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, w1, b1, gamma, beta, w2, b2, labels, running_mean, running_var, momentum, eps, training):
        L = lib()
        h, w1, b1, gamma, beta, w2, b2 = (_req(t, name) for t, name in ((h, "tail input"), (w1, "fc1.weight"), (b1, "fc1.bias"), (gamma, "bn1.weight"),
                                                                         (beta, "bn1.bias"), (w2, "fc2.weight"), (b2, "fc2.bias")))
        labels = _req(labels, "domain labels", torch.int32)
        rm, rv = _req(running_mean, "bn1.running_mean"), _req(running_var, "bn1.running_var")
        if rm is not running_mean or rv is not running_var:
            raise ValueError("mcdseg: the running statistics are updated in place and must be contiguous")
        groups = labels.numel()
        rows, f = h.shape
        if groups < 1 or rows % groups or tuple(w1.shape) != (10, f) or tuple(w2.shape) != (2, 10):
            raise ValueError("mcdseg: tail input %s, %d groups, fc1 %s, fc2 %s do not fit" % (tuple(h.shape), groups, tuple(w1.shape), tuple(w2.shape)))
        n = rows // groups
        loss = torch.empty(groups, dtype=torch.float32, device=h.device)
        logits = torch.empty((rows, 2), dtype=torch.float32, device=h.device)
        save = _ws64(L.mcdseg_dann_tail_save_bytes(groups, n), h.device)
        with _timed("dann_tail_fwd_kernel", (2 * rows * 10 * f, 4 * (h.numel() + w1.numel()))):
            check(L.mcdseg_dann_tail_fwd(_p(h), _p(labels), _p(w1), _p(b1), _p(gamma), _p(beta), _p(rm), _p(rv), _p(w2), _p(b2), float(momentum),
                                         float(eps), int(bool(training)), _p(loss), _p(logits), _p(save), groups, n, f, _stream()), "dann_tail_fwd")
        ctx.save_for_backward(h, w1, gamma, beta, w2, labels, logits, save)
        ctx.training = int(bool(training))
        ctx.mark_non_differentiable(logits)
        return loss, logits

    @staticmethod
    def backward(ctx, gl, _glogits):
        h, w1, gamma, beta, w2, labels, logits, save = ctx.saved_tensors
        L = lib()
        groups = labels.numel()
        rows, f = h.shape
        n = rows // groups
        up = _req(gl.reshape(groups), "grad_output")
        dh = torch.empty_like(h) if ctx.needs_input_grad[0] else None
        dw1, db1, dgamma, dbeta, dw2, db2 = (torch.empty(s, dtype=torch.float32, device=h.device) for s in ((10, f), (10,), (10,), (10,), (2, 10), (2,)))
        ws = _ws(L.mcdseg_dann_tail_workspace_bytes(groups, n), h.device)
        with _timed("dann_tail_bwd_kernel", (4 * rows * 10 * f, 4 * (3 * h.numel() + 2 * w1.numel()))):
            check(L.mcdseg_dann_tail_bwd(_p(h), _p(labels), _p(w1), _p(gamma), _p(beta), _p(w2), _p(logits), _p(save), _p(up), _p(dh), _p(dw1), _p(db1),
                                         _p(dgamma), _p(dbeta), _p(dw2), _p(db2), ctx.training, groups, n, f, _p(ws), ctypes.c_size_t(ws.numel() * 4),
                                         _stream()), "dann_tail_bwd")
        _on_launch_stream(ws)
        return (dh, dw1, db1, dgamma, dbeta, dw2, db2) + (None,) * 6


def dann_tail(h, fc1_weight, fc1_bias, bn_weight, bn_bias, fc2_weight, fc2_bias, labels, running_mean, running_var, momentum=0.1, eps=1e-5,
              training=True):
    """The domain classifier behind its two ``DownConv``s (models/dilated_fcn.py:547-551) and ``nn.CrossEntropyLoss`` against one domain label
    per group, all groups in one launch each way: ``h`` [G n, F] holds G groups of n rows, ``labels`` int32 [G] on the device.  Returns
    (loss [G], the mean cross-entropy of each group; logits [G n, 2], not differentiable).  BatchNorm1d's statistics are per group in
    training mode, and the running statistics are updated in place, group after group; include/mcdseg.h has the rest."""
    return _DannTail.apply(h, fc1_weight, fc1_bias, bn_weight, bn_bias, fc2_weight, fc2_bias, labels, running_mean, running_var, momentum, eps, training)


def predict_labels(z1, z2=None, n_used=None):
    """Inference tail of adapt_tester.py:101-124: (uint8 label map [N,H,W] = argmax over the first ``n_used`` classes
    of z1 or (z1+z2)/2, mean entropy scalar as util.calc_entropy defines it)."""
    L = lib()
    z1, z2 = _req(z1, "logits"), _req(z2, "logits")
    n, c, h, w = z1.shape
    n_used = c if n_used is None else int(n_used)
    labels = torch.empty((n, h, w), dtype=torch.uint8, device=z1.device)
    ent = torch.empty(1, dtype=torch.float32, device=z1.device)
    ws = _ws(L.mcdseg_predict_workspace_bytes(n, h * w), z1.device)
    check(L.mcdseg_predict_labels(_p(z1), _p(z2), _p(labels), _p(ent), n, c, n_used, h * w, _p(ws), ctypes.c_size_t(ws.numel() * 4),
                                  _stream()), "predict_labels")
    return labels, ent.reshape(())


def _predict_up(s, w, n_used):
    L = lib()
    s, w = _req(s, "low-resolution logits"), _req(w, "up8 weight")
    if s.dim() != 4:
        raise ValueError("mcdseg: the up-sampling predict tail takes logits [N,C,H,W], got %s" % (tuple(s.shape),))
    if w is not None:
        _check_up(s, w)
    n, c, hi, wi = s.shape
    n_used = c if n_used is None else int(n_used)
    labels = torch.empty((n, 8 * hi, 8 * wi), dtype=torch.uint8, device=s.device)
    ent = torch.empty(1, dtype=torch.float32, device=s.device)
    ws = _ws(L.mcdseg_predict_up8_workspace_bytes(n, hi), s.device)
    check(L.mcdseg_predict_labels_up8(_p(s), _p(w), _p(labels), _p(ent), n, c, n_used, hi, wi, _p(ws), ctypes.c_size_t(ws.numel() * 4),
                                      _stream()), "predict_labels_up8")
    return labels, ent.reshape(())


def predict_labels_up8(s, w, n_used=None):
    """``predict_labels(up8(s, w), None, n_used)`` without the full-resolution logits: DRNSeg's learned x8 up-sampler and the
    argmax / entropy tail in one pass (source_tester.py:119-143).  Labels are bitwise those of the two-step composition."""
    return _predict_up(s, w, n_used)


def predict_labels_bilinear8(s, n_used=None):
    """``predict_labels(bilinear8(s), None, n_used)`` in one pass, for the multitask decoder's pred_semseg1
    (adapt_multitask_tester.py:118-141)."""
    return _predict_up(s, None, n_used)


def depth_image_u8(d):
    """bilinear8(d) -> transform.unnormalize -> uint8 HWC image [N,8H,8W,3] (adapt_multitask_tester.py:148-155): numpy's float64
    arithmetic and np.uint8 cast, bit for bit (values outside [0,255] wrap as they do in the reference).  d: fp32 [N,1 or 3,H,W]."""
    d = _req(d, "depth prediction")
    if d.dim() != 4 or d.shape[1] not in (1, 3):
        raise ValueError("mcdseg: depth_image_u8 takes [N,1,H,W] or [N,3,H,W], got %s" % (tuple(d.shape),))
    n, cd, hi, wi = d.shape
    img = torch.empty((n, 8 * hi, 8 * wi, 3), dtype=torch.uint8, device=d.device)
    check(lib().mcdseg_depth_image_u8(_p(d), _p(img), n, cd, hi, wi, _stream()), "depth_image_u8")
    return img


# ------------------------------------------------------------------------------------------------ MFNet gate fusion
class _GateMix(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x1, x2, g):
        x1, x2, g = _req(x1, "x1"), _req(x2, "x2"), _req(g, "gate logits")
        if not (x1.shape == x2.shape == g.shape):
            raise ValueError("mcdseg: gate_mix needs three tensors of one shape")
        out = torch.empty_like(x1)
        check(lib().mcdseg_gate_mix_fwd(_p(x1), _p(x2), _p(g), _p(out), x1.numel(), _stream()), "gate_mix_fwd")
        ctx.save_for_backward(x1, x2, g)
        return out

    @staticmethod
    def backward(ctx, dy):
        x1, x2, g = ctx.saved_tensors
        dy = _req(dy, "grad_output")
        d1, d2, dg = torch.empty_like(x1), torch.empty_like(x1), torch.empty_like(x1)
        check(lib().mcdseg_gate_mix_bwd(_p(dy), _p(x1), _p(x2), _p(g), _p(d1), _p(d2), _p(dg), x1.numel(), _stream()), "gate_mix_bwd")
        return d1, d2, dg


def gate_mix(x1, x2, gate_logits):
    """x1*sigmoid(g) + x2*(1 - sigmoid(g)) (GateFusion.forward, models/fusion.py:19-22) in one pass, backward in one pass"""
    return _GateMix.apply(x1, x2, gate_logits)


class _SoftmaxCh(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _req(x, "logits")
        n, c, h, w = x.shape
        y = torch.empty_like(x)
        check(lib().mcdseg_softmax_ch_fwd(_p(x), _p(y), n, c, h * w, _stream()), "softmax_ch_fwd")
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = _req(dy, "grad_output")
        n, c, h, w = y.shape
        dx = torch.empty_like(y)
        check(lib().mcdseg_softmax_ch_bwd(_p(dy), _p(y), _p(dx), n, c, h * w, _stream()), "softmax_ch_bwd")
        return dx


def softmax_channels(x):
    """F.softmax over dim 1 of an NCHW tensor (the ScoreGateFusion pre-step, models/fusion.py:13-15)"""
    return _SoftmaxCh.apply(x)


class _ProbNLL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, labels, weight, ignore_index, size_average):
        L = lib()
        p = _req(p, "probabilities")
        labels = _req(labels, "labels", torch.int64)
        weight = _req(weight, "class weights")
        n, c, h, w = p.shape
        if tuple(labels.shape) != (n, h, w):
            raise ValueError("mcdseg: labels %s do not match probabilities %s" % (tuple(labels.shape), tuple(p.shape)))
        loss = torch.empty(3, dtype=torch.float32, device=p.device)
        grad = torch.empty_like(p) if ctx.needs_input_grad[0] else None
        ws = _ws64(L.mcdseg_prob_nll_workspace_bytes(n, h * w), p.device)
        check(L.mcdseg_prob_nll(_p(p), _p(labels), _p(weight), int(ignore_index), int(bool(size_average)), _p(grad), _p(loss), n, c,
                                h * w, _p(ws), ctypes.c_size_t(ws.numel() * 8), _stream()), "prob_nll")
        ctx.g = grad
        return loss[0].clone() if size_average else loss[1].clone()

    @staticmethod
    def backward(ctx, grad_out):
        g = ctx.g
        ctx.g = None
        return (g * grad_out if g is not None else None), None, None, None, None


def prob_cross_entropy2d(p, labels, weight=None, ignore_index=-100, size_average=True):
    """ProbCrossEntropyLoss2d (loss.py:16-30): NLLLoss2d(weight)(log(p), labels) with its gradient from the same call"""
    return _ProbNLL.apply(p, labels, weight, ignore_index, size_average)


def normalize_u8_(dst, src, mean, std, c_off=0):
    """ToTensor()+Normalize() of transform.py:302-315 on the device: ``src`` uint8 [N,H,W,Cs] (HWC, as PIL/numpy hand it
    over) is written as fp32 into channels [c_off, c_off+Cs) of ``dst`` [N,C,H,W].  mean/std: fp32 device tensors [Cs]."""
    src = _req(src, "uint8 image batch", torch.uint8)
    if src.dim() != 4:
        raise TypeError("mcdseg: normalize_u8_ takes a uint8 [N,H,W,C] tensor")
    if dst.dtype != torch.float32 or not dst.is_contiguous() or not dst.is_cuda:
        raise TypeError("mcdseg: normalize_u8_ writes into a contiguous fp32 GPU tensor")
    n, h, w, cs = src.shape
    if tuple(dst.shape[0:1] + dst.shape[2:]) != (n, h, w):
        raise ValueError("mcdseg: normalize_u8_ shape mismatch %s vs %s" % (tuple(src.shape), tuple(dst.shape)))
    mean, std = _req(mean.float(), "mean"), _req(std.float(), "std")
    check(lib().mcdseg_normalize_u8(_p(src), _p(dst), _p(mean), _p(std), n, h, w, cs, dst.shape[1], int(c_off), _stream()),
          "normalize_u8")
    return dst


def resize_u8(src, out_wh, nearest=False):
    """Scale(img_shape, Image.BILINEAR) (images, uint8 [N,H,W,C]) / Scale(img_shape, Image.NEAREST) (label maps, uint8 [N,H,W])
    of transform.py:303, 320 on the device -- Pillow's 8-bit resize arithmetic, bit for bit; ``out_wh`` = (W, H) as the reference
    passes it"""
    L = lib()
    src = _req(src, "uint8 batch", torch.uint8)
    ow, oh = int(out_wh[0]), int(out_wh[1])
    if nearest:
        if src.dim() != 3:
            raise TypeError("mcdseg: resize_u8(nearest) takes a uint8 [N,H,W] tensor")
        n, h, w = src.shape
        c = 1
    else:
        if src.dim() != 4:
            raise TypeError("mcdseg: resize_u8 takes a uint8 [N,H,W,C] tensor")
        n, h, w, c = src.shape
    if (ow, oh) == (w, h):
        return src
    ws = _ws(L.mcdseg_resize_workspace_bytes(n, h, w, c, oh, ow), src.device)
    if nearest:
        dst = torch.empty((n, oh, ow), dtype=torch.uint8, device=src.device)
        check(L.mcdseg_resize_nearest_u8(_p(src), _p(dst), n, h, w, oh, ow, _p(ws), ctypes.c_size_t(ws.numel() * 4), _stream()),
              "resize_nearest_u8")
    else:
        dst = torch.empty((n, oh, ow, c), dtype=torch.uint8, device=src.device)
        check(L.mcdseg_resize_bilinear_u8(_p(src), _p(dst), n, h, w, c, oh, ow, _p(ws), ctypes.c_size_t(ws.numel() * 4), _stream()),
              "resize_bilinear_u8")
    return dst


def relabel_u8(src, olabel, nlabel):
    """ToLabel()+ReLabel(olabel, nlabel) (transform.py:21-48): uint8 label maps -> int64 with the background id remapped"""
    src = _req(src, "uint8 label batch", torch.uint8)
    out = torch.empty(src.shape, dtype=torch.int64, device=src.device)
    check(lib().mcdseg_relabel_u8(_p(src), _p(out), src.numel(), int(olabel), int(nlabel), _stream()), "relabel_u8")
    return out


def _joint_tables(params, n, device):
    """(affine float64 [N,6], geom int32 [N,10]) on the device, from a ``mcdseg.augment.JointParams`` or a pair of tensors"""
    affine, geom = params.tables(device) if hasattr(params, "tables") else params
    affine, geom = _req(affine, "affine table", torch.float64), _req(geom, "geometry table", torch.int32)
    if tuple(affine.shape) != (n, 6) or tuple(geom.shape) != (n, 10):
        raise ValueError("mcdseg: the joint transform's tables must be [%d,6] and [%d,10], got %s and %s"
                         % (n, n, tuple(affine.shape), tuple(geom.shape)))
    return affine, geom


def _joint_out_hw(out_hw):
    oh, ow = int(out_hw[0]), int(out_hw[1])
    if oh <= 0 or ow <= 0:
        raise ValueError("mcdseg: the joint transform's output size must be positive, got %s" % (tuple(out_hw),))
    return oh, ow


def joint_augment_u8(src, params, out_hw, nearest=False):
    """RandomHorizontallyFlip + RandomRotate + RandomCrop of joint_transforms.py:248-255 on the device, one gather pass, Pillow's bytes:
    images (uint8 [N,H,W,C], ``Image.rotate(a, BILINEAR)``) -> uint8 [N,OH,OW,C]; label maps (``nearest=True``, uint8 [N,H,W],
    ``Image.rotate(a, NEAREST)``) -> uint8 [N,OH,OW].  ``params``: the per-sample tables (``mcdseg.augment.JointParams``, or a pair
    of device tensors: affine float64 [N,6], geom int32 [N,10]); ``out_hw`` = (OH, OW), the crop.  Pixels whose source lies outside
    the image are 0 -- for a label map that is class 0, not the background id, as ``mask.rotate`` of the reference fills it."""
    L = lib()
    src = _req(src, "uint8 batch", torch.uint8)
    oh, ow = _joint_out_hw(out_hw)
    if nearest:
        if src.dim() != 3:
            raise TypeError("mcdseg: joint_augment_u8(nearest) takes a uint8 [N,H,W] tensor")
        n, h, w = src.shape
        _, geom = _joint_tables(params, n, src.device)
        dst = torch.empty((n, oh, ow), dtype=torch.uint8, device=src.device)
        check(L.mcdseg_joint_augment_label_u8(_p(src), _p(dst), _p(geom), n, h, w, oh, ow, _stream()), "joint_augment_label_u8")
    else:
        if src.dim() != 4:
            raise TypeError("mcdseg: joint_augment_u8 takes a uint8 [N,H,W,C] tensor")
        n, h, w, c = src.shape
        affine, geom = _joint_tables(params, n, src.device)
        dst = torch.empty((n, oh, ow, c), dtype=torch.uint8, device=src.device)
        check(L.mcdseg_joint_augment_u8(_p(src), _p(dst), _p(affine), _p(geom), n, h, w, c, oh, ow, _stream()), "joint_augment_u8")
    return dst


def joint_augment_normalize_u8_(dst, src, params, mean, std, c_off=0):
    """``joint_augment_u8`` and ``normalize_u8_`` in one pass: ``src`` uint8 [N,H,W,Cs] is flipped, rotated and cropped to the size of
    ``dst`` [N,C,OH,OW] and written as fp32 into its channels [c_off, c_off+Cs).  A fill pixel is the normalised byte 0."""
    src = _req(src, "uint8 image batch", torch.uint8)
    if src.dim() != 4:
        raise TypeError("mcdseg: joint_augment_normalize_u8_ takes a uint8 [N,H,W,C] tensor")
    if dst.dtype != torch.float32 or not dst.is_contiguous() or not dst.is_cuda or dst.dim() != 4:
        raise TypeError("mcdseg: joint_augment_normalize_u8_ writes into a contiguous fp32 [N,C,OH,OW] GPU tensor")
    n, h, w, cs = src.shape
    if dst.shape[0] != n:
        raise ValueError("mcdseg: joint_augment_normalize_u8_ shape mismatch %s vs %s" % (tuple(src.shape), tuple(dst.shape)))
    oh, ow = _joint_out_hw(dst.shape[2:])
    affine, geom = _joint_tables(params, n, src.device)
    mean, std = _req(mean.float(), "mean"), _req(std.float(), "std")
    if mean.numel() < cs or std.numel() < cs:
        raise ValueError("mcdseg: joint_augment_normalize_u8_ needs a mean and a std per source channel")
    check(lib().mcdseg_joint_augment_normalize_u8(_p(src), _p(dst), _p(mean), _p(std), _p(affine), _p(geom), n, h, w, cs, oh, ow,
                                                  dst.shape[1], int(c_off), _stream()), "joint_augment_normalize_u8")
    return dst


def joint_augment_relabel_u8(src, params, out_hw, olabel, nlabel):
    """``joint_augment_u8(nearest=True)`` and ``relabel_u8`` in one pass: uint8 [N,H,W] label maps -> int64 [N,OH,OW].  The fill of
    the rotation is label 0 (see ``joint_augment_u8``); ``olabel`` -> ``nlabel`` is applied after it, as ReLabel follows the rotation."""
    src = _req(src, "uint8 label batch", torch.uint8)
    if src.dim() != 3:
        raise TypeError("mcdseg: joint_augment_relabel_u8 takes a uint8 [N,H,W] tensor")
    n, h, w = src.shape
    oh, ow = _joint_out_hw(out_hw)
    _, geom = _joint_tables(params, n, src.device)
    out = torch.empty((n, oh, ow), dtype=torch.int64, device=src.device)
    check(lib().mcdseg_joint_augment_relabel_u8(_p(src), _p(out), _p(geom), n, h, w, oh, ow, int(olabel), int(nlabel), _stream()),
          "joint_augment_relabel_u8")
    return out


def _req_maps(t, name, dtype):
    t = _req(t, name, dtype)
    if t.dim() != 3 or t.numel() == 0:
        raise TypeError("mcdseg: %s must be a non-empty %s [N,H,W] tensor" % (name, dtype))
    return t


def boundary_regions(boundary_u8, thre):
    """binalize_boundary.py:9-20 + bwboundaries (apply_bwboundary.m:10-12) on the device: uint8 boundary images [N,H,W] -> the
    canonical int32 region map [N,H,W].  ``boundary > thre`` is the mask; mask pixels connect 8-wise, the others 4-wise; -1 = the
    frame object (every mask component that touches the image border), else the smallest row-major index of the pixel's component."""
    b = _req_maps(boundary_u8, "boundary batch", torch.uint8)
    n, h, w = b.shape
    regions = torch.empty((n, h, w), dtype=torch.int32, device=b.device)
    with _timed("boundary_regions", (0, 5 * b.numel())):
        check(lib().mcdseg_boundary_regions(_p(b), int(thre), _p(regions), n, h, w, None, ctypes.c_size_t(0), _stream()),
              "boundary_regions")
    return regions


def refine_labels(seg_u8, regions, min_thre, max_thre):
    """refine_seg_by_bwboundary.py:34-42 on the device: every region (ids >= 0 of an int32 map [N,H,W], canonical or not) of
    ``min_thre < pixels < max_thre`` takes the most common value of ``seg_u8`` (uint8 [N,H,W]) inside it, ties to the value that occurs
    first in row-major order; everything else keeps its label.  Returns a new uint8 [N,H,W] tensor."""
    L = lib()
    seg = _req_maps(seg_u8, "label batch", torch.uint8)
    regions = _req_maps(regions, "region map", torch.int32)
    if tuple(seg.shape) != tuple(regions.shape):
        raise ValueError("mcdseg: refine_labels shape mismatch %s vs %s" % (tuple(seg.shape), tuple(regions.shape)))
    n, h, w = seg.shape
    nbytes = L.mcdseg_refine_workspace_bytes(n, h, w, int(min_thre))
    ws = _ws(nbytes, seg.device)
    out = torch.empty_like(seg)
    with _timed("refine_labels_by_regions", (0, 10 * seg.numel())):
        check(L.mcdseg_refine_labels_by_regions(_p(seg), _p(regions), _p(out), n, h, w, int(min_thre), int(max_thre), _p(ws),
                                                ctypes.c_size_t(ws.numel() * 4), _stream()), "refine_labels_by_regions")
    return out


def refine_labels_by_boundary(seg_u8, boundary_u8, thre=50, min_thre=500, max_thre=79333):
    """sample_scripts/refine_seg_by_boundary.sh:15-17 in one call (the reference's defaults): ``refine_labels`` over
    ``boundary_regions(boundary_u8, thre)``"""
    return refine_labels(seg_u8, boundary_regions(boundary_u8, thre), min_thre, max_thre)


# ------------------------------------------------------------------------------------------------ dense CRF over saved logits
CRF_DEFAULTS = {"n_iters": 10, "sxy_gaussian": (1, 1), "compat_gaussian": 4, "sxy_bilateral": (49, 49), "compat_bilateral": 5,
                "srgb_bilateral": (13, 13, 13)}  # tools/crf.py:14-21


def fused_crf():
    """MCDSEG_FUSED_CRF=0 (host-side, read at every call): ``dense_crf`` composes the same definition from torch -- row chunks of
    ``torch.exp(-0.5 * cdist ** 2) @ (n * Q)`` for both terms -- instead of the kernels of csrc/crf.hip: the parity test's other side
    and the timing baseline"""
    return os.environ.get("MCDSEG_FUSED_CRF", "1") != "0"


def _pair(v, k, name):
    v = tuple(float(a) for a in (v if isinstance(v, (tuple, list)) else (v,) * k))
    if len(v) != k:
        raise ValueError("mcdseg: dense_crf %s takes %d values, got %d" % (name, k, len(v)))
    return v


def _crf_composed(z, rgb, n_iters, params, c_used):
    """the definition of DESIGN.md section 4.12 in torch, fp32, every sum over all pixels of the image (the Gaussian term included)"""
    b, c, h, w = z.shape
    sxg, syg, wg, sxb, syb, wb, sr, sg, sb = params
    n = h * w
    ys, xs = torch.meshgrid(torch.arange(h, device=z.device, dtype=torch.float32), torch.arange(w, device=z.device, dtype=torch.float32),
                            indexing="ij")
    xs, ys = xs.reshape(n), ys.reshape(n)
    chunk = max(1, min(n, (1 << 27) // n))

    def kernel_rows(f, lo, hi):
        return torch.exp(-0.5 * torch.cdist(f[lo:hi], f, compute_mode="donot_use_mm_for_euclid_dist") ** 2)

    def norm(f):
        s = torch.cat([kernel_rows(f, lo, min(lo + chunk, n)).sum(1) for lo in range(0, n, chunk)])
        return 1.0 / torch.sqrt(s + 1e-20)

    def message(f, nrm, q):  # q [n, c]
        nq = nrm[:, None] * q
        return nrm[:, None] * torch.cat([kernel_rows(f, lo, min(lo + chunk, n)) @ nq for lo in range(0, n, chunk)])

    q_out = torch.empty((b, c, h, w), dtype=torch.float32, device=z.device)
    for k in range(b):
        u = -torch.log_softmax(z[k].reshape(c, n).t(), dim=1)
        terms = [(torch.stack([xs / sxg, ys / syg], 1), wg)]
        if rgb is not None:
            px = rgb[k].reshape(n, 3).float()
            terms.append((torch.stack([xs / sxb, ys / syb, px[:, 0] / sr, px[:, 1] / sg, px[:, 2] / sb], 1), wb))
        q = torch.softmax(-u, dim=1)
        if n_iters > 0:
            norms = [norm(f) for f, _ in terms]
        for _ in range(n_iters):
            x = -u
            for (f, wt), nrm in zip(terms, norms):
                x = x + wt * message(f, nrm, q)
            q = torch.softmax(x, dim=1)
        q_out[k] = q.t().reshape(c, h, w)
    labels = torch.empty((b, h, w), dtype=torch.uint8, device=z.device)
    top = q_out[:, :c_used].max(dim=1, keepdim=True).values
    first = (q_out[:, :c_used] == top).to(torch.uint8).argmax(dim=1)  # the first maximum, as numpy's argmax
    labels.copy_(first)
    return q_out, labels


def dense_crf(logits, rgb=None, n_iters=CRF_DEFAULTS["n_iters"], sxy_gaussian=CRF_DEFAULTS["sxy_gaussian"],
              compat_gaussian=CRF_DEFAULTS["compat_gaussian"], sxy_bilateral=CRF_DEFAULTS["sxy_bilateral"],
              compat_bilateral=CRF_DEFAULTS["compat_bilateral"], srgb_bilateral=CRF_DEFAULTS["srgb_bilateral"], c_used=None):
    """tools/crf.py:14-60 with exact pairwise sums: fp32 logits [B,C,H,W] (what ``prob/<name>.npy`` holds) and,
    for the bilateral term, a uint8 RGB batch [B,H,W,3] -> (Q^{n_iters} fp32 [B,C,H,W], labels uint8 [B,H,W] = the arg-max over the first
    ``c_used`` classes, all by default, first maximum on a tie).  Inference only.  ``sxy`` are (x, y) as in pydensecrf; a single number
    stands for both."""
    if logits.requires_grad:
        raise RuntimeError("mcdseg: dense_crf is inference only: the logits require grad")
    z = _req(logits, "logits")
    if z.dim() != 4 or z.numel() == 0:
        raise TypeError("mcdseg: dense_crf takes non-empty fp32 logits [B,C,H,W]")
    b, c, h, w = z.shape
    if rgb is not None:
        rgb = _req(rgb, "RGB batch", torch.uint8)
        if tuple(rgb.shape) != (b, h, w, 3):
            raise ValueError("mcdseg: dense_crf needs a uint8 RGB batch %s, got %s" % ((b, h, w, 3), tuple(rgb.shape)))
    c_used = c if c_used is None else int(c_used)
    params = (_pair(sxy_gaussian, 2, "sxy_gaussian") + (float(compat_gaussian),) + _pair(sxy_bilateral, 2, "sxy_bilateral") +
              (float(compat_bilateral),) + _pair(srgb_bilateral, 3, "srgb_bilateral"))
    L = lib()
    nbytes = L.mcdseg_dense_crf_workspace_bytes(b, c, h, w, int(rgb is not None))
    if not fused_crf():
        # the same refusals as the library's, from the library: nothing is launched by a call with a null output
        if not 1 <= c_used <= c or int(n_iters) < 0 or nbytes == 0 or min(params[:2]) <= 0 or (rgb is not None and min(params[3:5] + params[6:]) <= 0):
            raise RuntimeError("mcdseg: dense_crf refuses these arguments (C_used in [1, C], n_iters >= 0, positive standard deviations)")
        with torch.no_grad():
            return _crf_composed(z, rgb, int(n_iters), params, c_used)
    ws = _ws(nbytes, z.device)
    q = torch.empty((b, c, h, w), dtype=torch.float32, device=z.device)
    labels = torch.empty((b, h, w), dtype=torch.uint8, device=z.device)
    host = (ctypes.c_float * 10)(*(params + (0.0,)))
    n = h * w
    with _timed("dense_crf", (2.0 * b * n * n * c * int(n_iters) * (rgb is not None), 16 * z.numel() * max(int(n_iters), 1))):
        check(L.mcdseg_dense_crf(_p(z), _p(rgb), ctypes.cast(host, ctypes.c_void_p), _p(q), _p(labels), c_used, b, c, h, w, int(n_iters),
                                 _p(ws), ctypes.c_size_t(nbytes), _stream()), "dense_crf")
    return q, labels


# ------------------------------------------------------------------------------------------------ depth -> HHA
def _hha_cameras(camera, n):
    """one (fx, fy, cx, cy) or [N,4] -> a host array of n x 4 floats (the library reads the cameras on the host)"""
    cam = torch.as_tensor(camera, dtype=torch.float32, device="cpu").reshape(-1)
    if cam.numel() == 4:
        cam = cam.repeat(n)
    if cam.numel() != 4 * n:
        raise ValueError("mcdseg: depth_to_hha takes one camera (fx, fy, cx, cy) or [N,4] = [%d,4], got %d values" % (n, cam.numel()))
    return (ctypes.c_float * (4 * n))(*cam.tolist())


def _depth_cm(depth, unit_m, who):
    """the dense fp32 centimetre batch [N,H,W] of a depth batch: what ``depth_to_hha`` and ``fill_depth`` both read"""
    if not torch.is_tensor(depth) or depth.dim() != 3 or depth.numel() == 0:
        raise TypeError("mcdseg: %s takes a non-empty depth batch [N,H,W]" % who)
    if depth.dtype not in (torch.uint16, torch.int32, torch.float32):
        raise TypeError("mcdseg: %s takes uint16, int32 or fp32 depth, got %s" % (who, depth.dtype))
    if not depth.is_cuda:
        raise RuntimeError("mcdseg: the depth batch must live on the GPU -- the HIP kernels are the only implementation (no CPU fallback)")
    if unit_m is None:
        if depth.dtype != torch.float32:
            raise TypeError("mcdseg: %s needs unit_m (metres per unit) for %s depth" % (who, depth.dtype))
        return _req(depth, "depth batch")
    return _req(depth.float() * (100 * float(unit_m)), "depth batch")  # (a permuted batch keeps its strides through the multiply)


def depth_to_hha(depth, camera, unit_m=None, return_parts=False):
    """Depth -> HHA: ``depth`` [N,H,W] on the GPU, fp32 in centimetres (``unit_m`` None) or uint16 / int32 / fp32
    in units of ``unit_m`` metres (0.001 for NYU and Kinect PNGs), converted by ONE fp32 multiply, ``depth.float() * (100 * unit_m)``;
    a value <= 0 or not finite is missing.  ``camera``: one (fx, fy, cx, cy) in pixels for the batch, or [N,4].  Returns the uint8 batch
    [N,H,W,3] (disparity, height, angle; (0,0,0) at a missing pixel) -- a part ``DeviceInputPipeline.images`` takes as it is -- and with
    ``return_parts`` also a dict of what it was rounded from: ``normals3`` fp32 [N,H,W,3], ``gravity`` fp32 [N,3], ``height`` fp32 [N,H,W]."""
    z = _depth_cm(depth, unit_m, "depth_to_hha")
    n, h, w = z.shape
    host = _hha_cameras(camera, n)
    L = lib()
    nbytes = L.mcdseg_depth_to_hha_workspace_bytes(n, h, w)
    ws = _ws64(nbytes, z.device)
    out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=z.device)
    parts = None
    if return_parts:
        parts = {"normals3": torch.empty((n, h, w, 3), dtype=torch.float32, device=z.device),
                 "gravity": torch.empty((n, 3), dtype=torch.float32, device=z.device),
                 "height": torch.empty((n, h, w), dtype=torch.float32, device=z.device)}
    with _timed("depth_to_hha", (600.0 * z.numel(), 110 * z.numel())):
        check(L.mcdseg_depth_to_hha(_p(z), ctypes.cast(host, ctypes.c_void_p), _p(out), _p(parts and parts["normals3"]),
                                    _p(parts and parts["gravity"]), _p(parts and parts["height"]), n, h, w, _p(ws),
                                    ctypes.c_size_t(nbytes), _stream()), "depth_to_hha")
    _on_launch_stream(z, ws, out, *(parts.values() if parts else ()))
    return (out, parts) if return_parts else out


# ------------------------------------------------------------------------------------------------ depth inpainting
FILL_RUNNING, FILL_CONVERGED, FILL_EMPTY, FILL_NOT_CONVERGED, FILL_BREAKDOWN = 0, 1, 2, 3, 4  # MCDSEG_FILL_*
FILL_STATUS_NAMES = {FILL_RUNNING: "running", FILL_CONVERGED: "converged", FILL_EMPTY: "empty", FILL_NOT_CONVERGED: "not_converged",
                     FILL_BREAKDOWN: "breakdown"}


def fill_depth(rgb_u8, depth, unit_m=None, alpha=1.0, rtol=1e-10, max_iter=4000, check_every=8, max_valid_cm=None, keep_known=False,
               return_parts=False):
    """Depth inpainting by colorization (the NYU toolbox's ``fill_depth_colorization`` step): ``rgb_u8`` uint8
    [N,H,W,3] and ``depth`` [N,H,W] on the GPU, the depth as ``depth_to_hha`` takes it (fp32 centimetres, or uint16 / int32 / fp32 in
    units of ``unit_m`` metres); a value <= 0, not finite or (with ``max_valid_cm``) >= max_valid_cm is missing.  Returns the filled
    depth, fp32 centimetres [N,H,W], at EVERY pixel (``keep_known``: a known pixel keeps its measured value bit for bit).  The sparse
    system of each image is solved by BiCGSTAB on the device, ``check_every`` iterations per call; the per-image status records are read
    back after each call -- the only host synchronisation -- until no image is running or ``max_iter`` is reached.  Nothing raises on an
    image that did not converge: with ``return_parts`` the second value is a dict of ``x`` fp64 [N,H,W] (the solution in units of
    zmax), ``zmax`` fp64 [N], ``status`` int32 [N] (``FILL_CONVERGED``, ``FILL_EMPTY``: no known pixel, all zeros,
    ``FILL_NOT_CONVERGED``, ``FILL_BREAKDOWN``), ``iterations`` int32 [N], ``residual`` fp64 [N] (the true residual's 2-norm over
    |b| at the image's last check) -- these three on the CPU -- and ``weights`` fp64 [N,8,H,W]."""
    z = _depth_cm(depth, unit_m, "fill_depth")
    n, h, w = z.shape
    if not torch.is_tensor(rgb_u8) or rgb_u8.dtype != torch.uint8 or tuple(rgb_u8.shape) != (n, h, w, 3):
        raise TypeError("mcdseg: fill_depth takes a uint8 RGB batch %s beside the depth, got %s" %
                        ((n, h, w, 3), (rgb_u8.dtype, tuple(rgb_u8.shape)) if torch.is_tensor(rgb_u8) else type(rgb_u8).__name__))
    rgb = _req(rgb_u8, "RGB batch", torch.uint8)
    alpha, rtol, max_iter, check_every = float(alpha), float(rtol), int(max_iter), int(check_every)
    if not (0 < alpha < float("inf")) or not (0 < rtol < float("inf")):
        raise ValueError("mcdseg: fill_depth: alpha and rtol must be positive and finite, got %r and %r" % (alpha, rtol))
    if max_iter < 0 or check_every < 1:
        raise ValueError("mcdseg: fill_depth: max_iter >= 0 and check_every >= 1 are needed, got %d and %d" % (max_iter, check_every))
    if max_valid_cm is not None and not float(max_valid_cm) > 0:
        raise ValueError("mcdseg: fill_depth: max_valid_cm must be positive (or None), got %r" % (max_valid_cm,))
    if h * w < 2:
        raise ValueError("mcdseg: fill_depth needs images of at least 2 pixels, got %d x %d" % (h, w))
    L = lib()
    nbytes = L.mcdseg_fill_depth_workspace_bytes(n, h, w)
    ws = _ws64(nbytes, z.device)
    records = torch.empty((n, 2), dtype=torch.float64, device=z.device)  # {int32 status; int32 iterations; double residual} each
    dims, wsize = (n, h, w), ctypes.c_size_t(nbytes)
    with _timed("fill_depth", (0, 132 * z.numel())):
        check(L.mcdseg_fill_depth_setup(_p(rgb), _p(z), alpha, float(max_valid_cm or 0.0), *dims, _p(ws), wsize, _stream()), "fill_depth_setup")
        done, step = 0, 0  # the first call is the check before the first iteration
        while True:
            check(L.mcdseg_fill_depth_iterate(step, rtol, *dims, _p(ws), wsize, _p(records), _stream()), "fill_depth_iterate")
            done += step
            host = records.cpu()
            status, iterations = host.view(torch.int32)[:, 0].clone(), host.view(torch.int32)[:, 1].clone()
            step = min(check_every, max_iter - done)
            if step <= 0 or not bool((status == FILL_RUNNING).any()):
                break
        status[status == FILL_RUNNING] = FILL_NOT_CONVERGED
        out = torch.empty((n, h, w), dtype=torch.float32, device=z.device)
        parts = None
        if return_parts:
            parts = {"x": torch.empty((n, h, w), dtype=torch.float64, device=z.device),
                     "zmax": torch.empty((n,), dtype=torch.float64, device=z.device),
                     "status": status, "iterations": iterations, "residual": host[:, 1].clone(),
                     "weights": torch.empty((n, 8, h, w), dtype=torch.float64, device=z.device)}
        check(L.mcdseg_fill_depth_finish(*dims, _p(ws), wsize, _p(out), _p(parts and parts["x"]), _p(parts and parts["weights"]),
                                         _p(parts and parts["zmax"]), int(bool(keep_known)), _stream()), "fill_depth_finish")
    _on_launch_stream(z, rgb, ws, records, out, *((parts["x"], parts["zmax"], parts["weights"]) if parts else ()))
    return (out, parts) if return_parts else out


# ------------------------------------------------------------------------------------------------ ensembling saved predictions
ENSEMBLE_METHODS = {"averaging": 0, "nms": 1}  # MCDSEG_ENSEMBLE_AVERAGING / _NMS
ENSEMBLE_MAX_K = 16                            # MCDSEG_ENSEMBLE_MAX_K


def ensemble_probs(maps, method="averaging", n_used=None, want_prob=True):
    """tools/ensemble_predict_from_npy.py:21-32 on the device: ``maps`` is a list of 2..16 fp32 GPU tensors of one
    shape, [C,H,W] or [N,C,H,W] -- the saved maps of one image, or of a batch, one tensor per ensemble member, used where they lie ->
    (``sum(maps) / len(maps)`` for "averaging" or ``np.max(maps, 0)`` for "nms", bit for bit as numpy evaluates them but for a NaN's
    payload -- every NaN leaves as 0x7FC00000, an input NaN handed through by "nms" included --, or None without ``want_prob``; labels uint8 [H,W] / [N,H,W] = numpy's argmax over the first ``n_used`` classes, all by
    default)."""
    if isinstance(maps, torch.Tensor) or not isinstance(maps, (list, tuple)):
        raise TypeError("mcdseg: ensemble_probs takes a list of tensors, one per ensemble member")
    if not 2 <= len(maps) <= ENSEMBLE_MAX_K:
        raise ValueError("mcdseg: ensemble_probs takes 2..%d maps, got %d" % (ENSEMBLE_MAX_K, len(maps)))
    if method not in ENSEMBLE_METHODS:
        raise ValueError("mcdseg: ensemble_probs method must be one of %s, got %r" % (sorted(ENSEMBLE_METHODS), method))
    if any(torch.is_tensor(t) and t.requires_grad for t in maps):
        raise RuntimeError("mcdseg: ensemble_probs is inference only: a map requires grad")
    maps = [_req(t, "map %d" % k) for k, t in enumerate(maps)]
    shape = tuple(maps[0].shape)
    if len(shape) not in (3, 4) or maps[0].numel() == 0:
        raise TypeError("mcdseg: ensemble_probs takes non-empty fp32 maps [C,H,W] or [N,C,H,W], got %s" % (shape,))
    for k, t in enumerate(maps):
        if tuple(t.shape) != shape or t.device != maps[0].device:
            raise ValueError("mcdseg: ensemble_probs: map %d is %s on %s, map 0 is %s on %s" % (k, tuple(t.shape), t.device, shape, maps[0].device))
    n, c, h, w = shape if len(shape) == 4 else (1,) + shape
    n_used = c if n_used is None else int(n_used)
    if not 1 <= n_used <= min(c, 256):
        raise ValueError("mcdseg: ensemble_probs: n_used = %d outside [1, min(C = %d, 256)]" % (n_used, c))
    dev = maps[0].device
    out = torch.empty(shape, dtype=torch.float32, device=dev) if want_prob else None
    labels = torch.empty(shape[:-3] + (h, w), dtype=torch.uint8, device=dev)
    host = (ctypes.c_void_p * len(maps))(*[t.data_ptr() for t in maps])
    with _timed("ensemble_probs", ((len(maps) + 1) * maps[0].numel(), 4 * maps[0].numel() * (len(maps) + bool(want_prob)) + labels.numel())):
        check(lib().mcdseg_ensemble_probs(ctypes.cast(host, ctypes.c_void_p), len(maps), ENSEMBLE_METHODS[method], _p(out), _p(labels),
                                          n_used, n, c, h, w, _stream()), "ensemble_probs")
    _on_launch_stream(out, labels, *maps)
    return out, labels


def label_resize_colorize(labels_u8, out_wh, palette_u8, want_labels=True, want_vis=True):
    """tools/ensemble_predict_from_npy.py:33-35 and :50-56 in one gather: uint8 label maps [N,H,W] -> (``Image.resize(out_wh, NEAREST)``
    of each, uint8 [N,OH,OW]; the palette image of that, uint8 [N,OH,OW,3]); ``out_wh`` = (W, H) as the reference passes it, ``palette_u8``
    a uint8 [n_pal,3] GPU tensor of 1..256 colours: a label >= n_pal is black.  An output that is not wanted is None."""
    L = lib()
    lab = _req_maps(labels_u8, "label batch", torch.uint8)
    if not (want_labels or want_vis):
        raise ValueError("mcdseg: label_resize_colorize: no output wanted")
    pal = _req(palette_u8, "palette", torch.uint8)
    if want_vis and (pal is None or pal.dim() != 2 or pal.shape[1] != 3 or not 1 <= pal.shape[0] <= 256):
        raise TypeError("mcdseg: label_resize_colorize takes a uint8 palette [n_pal,3] of 1..256 colours")
    ow, oh = int(out_wh[0]), int(out_wh[1])
    if ow <= 0 or oh <= 0:
        raise ValueError("mcdseg: label_resize_colorize: out_wh must be positive, got %s" % ((ow, oh),))
    n, h, w = lab.shape
    nbytes = L.mcdseg_label_resize_colorize_workspace_bytes(oh, ow)
    ws = _ws(nbytes, lab.device)
    out = torch.empty((n, oh, ow), dtype=torch.uint8, device=lab.device) if want_labels else None
    vis = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=lab.device) if want_vis else None
    with _timed("label_resize_colorize", (0, n * oh * ow * (1 + bool(want_labels) + 3 * bool(want_vis)))):
        check(L.mcdseg_label_resize_colorize(_p(lab), _p(pal) if want_vis else None, pal.shape[0] if want_vis else 0, _p(out), _p(vis), n, h, w,
                                             oh, ow, _p(ws), ctypes.c_size_t(nbytes), _stream()), "label_resize_colorize")
    _on_launch_stream(lab, pal, ws, out, vis)
    return out, vis


# ------------------------------------------------------------------------------------------------ edge maps of RGB images
EDGE_KINDS = ("luma", "laplacian", "sobel", "canny_cls", "canny")


def canny_hysteresis(cls_u8):
    """Canny's hysteresis: a uint8 class map [N,H,W] (1 = weak, 2 = strong, anything else 0) -> uint8 [N,H,W],
    255 where a weak or strong pixel's 8-connected component of such pixels holds a strong one, else 0"""
    L = lib()
    c = _req_maps(cls_u8, "class map", torch.uint8)
    n, h, w = c.shape
    nbytes = L.mcdseg_canny_hysteresis_workspace_bytes(n, h, w)
    ws = _ws(nbytes, c.device)
    edges = torch.empty_like(c)
    with _timed("canny_hysteresis", (0, 14 * c.numel())):
        check(L.mcdseg_canny_hysteresis(_p(c), _p(edges), n, h, w, _p(ws), ctypes.c_size_t(nbytes), _stream()), "canny_hysteresis")
    _on_launch_stream(c, ws, edges)
    return edges


def edge_maps(rgb_u8, low=100, high=200, want=("laplacian", "sobel", "canny")):
    """tools/edge_detect.py:33-53 of the reference on the device (OpenCV's published 8-bit algorithm, all integer):
    uint8 RGB images [N,H,W,3] -> {key: uint8 [N,H,W]} for the keys of ``want`` out of "luma" (cvtColor's Y), "laplacian"
    (cv2.Laplacian + 128, clipped), "sobel" (the clipped gradient magnitude), "canny_cls" (0 / weak 1 / strong 2 after the non-maximum
    suppression at the thresholds ``low`` and ``high``) and "canny" (cv2.Canny: 0 / 255 after the hysteresis).  One launch forms
    everything but "canny", whose hysteresis follows on a class map that is not returned unless "canny_cls" is asked for too."""
    if isinstance(want, str):
        want = (want,)
    want = tuple(want)
    unknown = [k for k in want if k not in EDGE_KINDS]
    if unknown or not want:
        raise ValueError("mcdseg: edge_maps: want must name some of %s, got %r" % (EDGE_KINDS, want))
    if not torch.is_tensor(rgb_u8):
        raise TypeError("mcdseg: edge_maps takes a uint8 [N,H,W,3] tensor")
    if rgb_u8.dtype != torch.uint8:
        raise TypeError("mcdseg: RGB batch must be torch.uint8, got %s" % rgb_u8.dtype)
    if rgb_u8.dim() != 4 or rgb_u8.shape[3] != 3 or rgb_u8.numel() == 0:
        raise ValueError("mcdseg: edge_maps takes non-empty RGB images [N,H,W,3], got %s" % (tuple(rgb_u8.shape),))
    rgb = _req(rgb_u8, "RGB batch", torch.uint8)
    n, h, w, _ = rgb.shape
    new = lambda: torch.empty((n, h, w), dtype=torch.uint8, device=rgb.device)  # noqa: E731
    out = {k: new() for k in ("luma", "laplacian", "sobel") if k in want}
    cls = new() if ("canny" in want or "canny_cls" in want) else None
    with _timed("edge_maps", (0, rgb.numel() + n * h * w * (len(out) + (cls is not None)))):
        check(lib().mcdseg_edge_maps(_p(rgb), _p(out.get("luma")), _p(out.get("laplacian")), _p(out.get("sobel")), _p(cls), int(low),
                                     int(high), n, h, w, _stream()), "edge_maps")
    _on_launch_stream(rgb, cls, *out.values())
    if "canny_cls" in want:
        out["canny_cls"] = cls
    if "canny" in want:
        out["canny"] = canny_hysteresis(cls)
    return {k: out[k] for k in EDGE_KINDS if k in out}


def confusion_hist_(hist, gt, pred):
    """hist[n*gt + pred] += 1 for 0 <= gt < n (eval.py:21-23 fast_hist); ``hist`` int64 [n,n] on the GPU, accumulated.  An entry
    whose prediction lies outside [0, n) is dropped too: it is not binned into a neighbouring row, as the reference's
    bincount(n*gt + pred) would do."""
    gt, pred = _req(gt.long(), "ground truth", torch.int64), _req(pred.long(), "prediction", torch.int64)
    if gt.numel() != pred.numel():
        raise ValueError("mcdseg: confusion_hist_ needs as many predictions as labels")
    if hist.dtype != torch.int64 or not hist.is_cuda or not hist.is_contiguous() or hist.dim() != 2 or hist.shape[0] != hist.shape[1]:
        raise TypeError("mcdseg: confusion_hist_ accumulates into a contiguous int64 [n,n] GPU tensor")
    if gt.numel():
        check(lib().mcdseg_confusion_hist(_p(gt), _p(pred), gt.numel(), hist.shape[0], _p(hist), _stream()), "confusion_hist")
    return hist


def _scale_(g, s):
    check(lib().mcdseg_scale_by_device_scalar(_p(g), _p(s), g.numel(), _stream()), "scale_by_device_scalar")
    return g


class _CrossEntropy2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, labels, class_weight, ignore_index, size_average):
        losses, g, _ = mcd_losses(z, None, labels, class_weight, ignore_index, ce_coef=1.0, want_grad=ctx.needs_input_grad[0])
        ctx.g = g
        ctx.size_average = size_average
        ctx.wsum = losses[3:4]
        return losses[0].clone() if size_average else losses[0] * losses[3]

    @staticmethod
    def backward(ctx, grad_out):
        g, ctx.g = ctx.g, None
        s = _req(grad_out.reshape(1), "grad_output")
        if not ctx.size_average:
            s = s * ctx.wsum
        return _scale_(g, s), None, None, None, None


class _Diff2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z1, z2):
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        losses, g1, g2 = mcd_losses(z1, z2, None, None, diff_coef=1.0, want_grad=need)
        ctx.g = (g1, g2)
        return losses[2].clone()

    @staticmethod
    def backward(ctx, grad_out):
        (g1, g2), ctx.g = ctx.g, None
        s = _req(grad_out.reshape(1), "grad_output")
        return _scale_(g1, s), _scale_(g2, s)


class _ProbDistance(torch.autograd.Function):
    """a distance of ``DIST_KINDS`` between softmax(z1) and softmax(z2): value and both logit gradients from one kernel launch"""

    @staticmethod
    def forward(ctx, z1, z2, kind):
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        losses, g1, g2 = mcd_losses(z1, z2, None, None, diff_coef=1.0, want_grad=need, dist=kind)
        ctx.g = (g1, g2)
        return losses[2].clone()

    @staticmethod
    def backward(ctx, grad_out):
        (g1, g2), ctx.g = ctx.g, None
        s = _req(grad_out.reshape(1), "grad_output")
        return _scale_(g1, s), _scale_(g2, s), None


def cross_entropy2d(z, labels, class_weight=None, ignore_index=-100, size_average=True):
    return _CrossEntropy2d.apply(z, labels, class_weight, ignore_index, size_average)


def diff2d(z1, z2):
    return _Diff2d.apply(z1, z2)


def prob_distance(z1, z2, kind):
    """``--d_loss`` distance ``kind`` (a name or a kind of ``DIST_KINDS``) between the two heads' logits [N,C,H,W], differentiable"""
    kind = dist_kind(kind)
    if kind == 0:
        return _Diff2d.apply(z1, z2)
    return _ProbDistance.apply(z1, z2, kind)


# ------------------------------------------------------------------------------------------------ optimizer kernel
def sgd_momentum_flat_(p, g, v, lr, momentum, weight_decay, grad_scale=1.0, params=None):
    """``params``: the parameter objects living in ``p`` (their packed images go stale); None = every packed image does"""
    for t, name in ((p, "params"), (g, "grads"), (v, "momentum")):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError("mcdseg: flat SGD needs contiguous fp32 GPU buffers (%s)" % name)
    with _timed("sgd_momentum_kernel", (0, 20 * p.numel())):
        check(lib().mcdseg_sgd_momentum_flat(_p(p), _p(g), _p(v), p.numel(), float(lr), float(momentum), float(weight_decay),
                                             float(grad_scale), _stream()), "sgd_momentum_flat")
    bump_weight_epoch(params)


def adam_flat_(p, g, m, v, lr, betas, eps, weight_decay, step, grad_scale=1.0, params=None):
    """one Adam update (L2 weight decay, no amsgrad) of the flat buffers; ``step`` is the count of THIS update (1 for the first), whose
    bias corrections are formed here in double precision.  ``params`` as for ``sgd_momentum_flat_``."""
    for t, name in ((p, "params"), (g, "grads"), (m, "exp_avg"), (v, "exp_avg_sq")):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError("mcdseg: flat Adam needs contiguous fp32 GPU buffers (%s)" % name)
    b1, b2 = float(betas[0]), float(betas[1])
    step = int(step)
    if step < 1:
        raise ValueError("mcdseg: flat Adam's step count starts at 1, got %r" % (step,))
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    with _timed("adam_kernel", (0, 28 * p.numel())):
        check(lib().mcdseg_adam_flat(_p(p), _p(g), _p(m), _p(v), p.numel(), float(lr) / bc1, b1, b2, bc2 ** -0.5, float(eps),
                                     float(weight_decay), float(grad_scale), _stream()), "adam_flat")
    bump_weight_epoch(params)
