"""Segmentation wrappers around the DRN trunk (reference: models/dilated_fcn.py).

  DRNSeg                              :68-110   trunk + seg + up (source-only training, cfg1)
  UncertainDRNSeg                     :113-214  DRNSeg + ``up_std`` and the Monte-Carlo dropout loss, all draws in one kernel
  DRNSegBase                = G       :217-250  trunk + 1x1 ``seg`` (ver1) / trunk only (ver2)
  FuseDRNSegBase            = G       :253-337  middle fusion: one set of DRN-D stages on HHA, then on RGB, a join behind every stage
  DRNSegPixelClassifier     = F1/F2   :340-366  learned x8 depthwise transposed-conv up-sampler
  DownConv / DRNSegDomainClassifier = D  :494-551  the DANN baseline's domain classifier, three fused launches each way
  FusionDRNSegPixelClassifier         :431-470  fuse features, one up-sampler
  ScoreFusionDRNSegPixelClassifier    :473-491  one up-sampler per modality, fuse scores
  MultiTaskEncoder / MCDMultiTaskDecoder            :554-566, 661-739   segmentation + HHA regression (cfg4)
  MultiTaskEncoderReturningMultipleFeaturemaps / get_boundary_loss / MCDSegBDMultiTaskDecoder
                                      :569-629, 743-787, 1027-1222      segmentation + boundary ("segbd")
  MCDTripleMultiTaskDecoder           :790-1024 segmentation + HHA regression + boundary ("triple"), with the seg2bd convolution

State-dict keys follow the reference: ``base.<stage>...``, ``seg.{weight,bias}``,
``up.weight`` / ``up1.weight`` / ``up2.weight``.
"""
import math
import os

import numpy as np
import torch
import torch.nn as nn
from torch.nn import Parameter

from mcdseg import ops

from . import drn
from .drn import BatchNorm2d, Conv2d, FusedSequential, _has_hooks, run_fused
from .fusion import AddFusion, ConcatFusion, get_fusion_model


def _trunk(model_name, pretrained, input_ch):
    ctor = drn.__dict__.get(model_name)
    if ctor is None or not model_name.startswith("drn_"):
        raise NotImplementedError("unknown DRN variant %r" % (model_name,))
    model = ctor(pretrained=pretrained, num_classes=0, input_ch=input_ch)
    return Trunk(*model.trunk()), model.out_dim


class Trunk(FusedSequential):
    """The DRN stages as ``nn.Sequential(*children[:-2])`` (models/dilated_fcn.py:223); same state_dict keys.  Every stage but
    the last runs inside ``ops.trunk_internal()``: with MCDSEG_ACT_STORAGE=compact those layers keep their activations only
    as the pre-split companions (BASELINE config 5); the last stage writes fp32, so what leaves the trunk is an ordinary tensor."""

    def forward(self, x):
        mods = list(self.children())
        if not mods:
            return x
        # the fusing walk of FusedSequential, so that the DRN-C stem (conv1, bn1, relu as top-level children, models/drn.py:118-121)
        # runs as one fused group like everywhere else
        with ops.late_weight_grads(self):  # (the weight gradients of these layers may stay on the side stream, mcdseg/ops.py)
            with ops.trunk_internal():
                x = run_fused(mods[:-1], x, following=mods[-1])
            return run_fused(mods[-1:], x)


def _seg_head(cin, n_class):
    seg = Conv2d(cin, n_class, kernel_size=1, bias=True)
    n = seg.kernel_size[0] * seg.kernel_size[1] * seg.out_channels
    seg.weight.data.normal_(0, math.sqrt(2.0 / n))
    seg.bias.data.zero_()
    return seg


class Up8(nn.ConvTranspose2d):
    """ConvTranspose2d(C, C, 16, stride 8, padding 4, groups=C, bias=False) -- parameters in torch's layout and
    default initialisation (the reference leaves ``fill_up_weights`` commented out, :93), HIP kernels for the maths."""

    def __init__(self, n_class):
        super().__init__(n_class, n_class, 16, stride=8, padding=4, output_padding=0, groups=n_class, bias=False)

    def forward(self, x, output_size=None):
        return ops.up8(x, self.weight)


class Up8Pairs(nn.ConvTranspose2d):
    """ConvTranspose2d(2C, C, 16, stride 8, padding 4, groups=C, bias=False) behind ``ConcatFusion``
    (models/dilated_fcn.py:445-448): output channel g sums the up-sampled input channels 2g and 2g+1 of the stacked
    tensor, each with its own 16x16 kernel -- the two-input form of the up-sampling kernel on the even / odd channels."""

    def __init__(self, n_class):
        super().__init__(2 * n_class, n_class, 16, stride=8, padding=4, output_padding=0, groups=n_class, bias=False)

    def forward(self, x, output_size=None):
        return ops.up8_dual(x[:, 0::2].contiguous(), self.weight[0::2].contiguous(), x[:, 1::2].contiguous(),
                            self.weight[1::2].contiguous())


def _up(cin, n_class, use_torch_up=False):
    if use_torch_up:
        raise NotImplementedError("use_torch_up (bilinear) is not on the MCD hot path")
    return Up8(n_class) if cin == n_class else Up8Pairs(n_class)


class DRNSeg(nn.Module):
    def __init__(self, model_name, n_class, input_ch=3, pretrained_model=None, pretrained=True, use_torch_up=False):
        super().__init__()
        self.base, out_dim = _trunk(model_name, pretrained, input_ch)
        if pretrained_model is not None:
            self.base.load_state_dict({k.replace("module.", ""): v for k, v in pretrained_model.items()}, strict=False)
        self.seg = _seg_head(out_dim, n_class)
        self.up = _up(n_class, n_class, use_torch_up)

    def forward(self, x):
        return self.up(self.seg(self.base(x)))

    def optim_parameters(self, memo=None):
        yield from self.base.parameters()
        yield from self.seg.parameters()


def fused_uncertain():
    """MCDSEG_FUSED_UNCERTAIN=0 (host-side, read at every call): ``UncertainDRNSeg.get_loss`` runs the literal form -- T dropout
    passes through both up-samplers and torch ops -- instead of the one-pass kernel; the parity test's other side and the timing baseline"""
    return os.environ.get("MCDSEG_FUSED_UNCERTAIN", "1") != "0"


class UncertainDRNSeg(nn.Module):
    """DRNSeg with a second learned up-sampler ``up_std`` for the per-class aleatoric standard deviation and a Monte-Carlo dropout
    loss (models/dilated_fcn.py:113-214).  State-dict keys are the reference's: ``base.*``, ``seg.{weight,bias}``, ``up.weight``,
    ``up_std.weight`` (``dropout`` and ``criterion`` hold no parameters; the criterion's class weights are a buffer,
    ``criterion.nll_loss.weight``, exactly as there).

    ``get_loss`` does NOT run the network ``n_dropout_exp`` times as the reference does (:176-200).  Dropout2d acts on the scores
    behind the trunk and both up-samplers are linear and depthwise, so up(m_t s) = m_t up(s): the trunk (train-mode BatchNorm, no
    randomness of its own) yields the same scores in every pass.  One trunk pass under ``ops.bn_running_updates(T)`` -- the running
    statistics move as in T passes -- and ``ops.up8_uncertain_loss`` over all T draws give the reference's losses and, through one
    trunk backward, its gradients (DESIGN.md has the derivation and the fp64 check against the reference).

    The draws: ``keep`` [T,N,C] from torch's generator on the device (Bernoulli(1 - p) per sample and channel, what Dropout2d draws)
    and ``r`` [T] from a ``numpy.random.RandomState`` the module owns (``seed_draws``; the reference takes ``np.random.rand()``
    from numpy's global state), uploaded without a synchronisation.  Both can be passed in.  A ``dropout`` module left in eval mode
    (``--no_dropout``, ``fix_dropout_when_training``) keeps every channel with factor 1."""

    def __init__(self, model_name, n_class, input_ch=3, pretrained_model=None, pretrained=True, use_torch_up=False, criterion=None,
                 n_dropout_exp=10, uncertain_weight=0.1):
        super().__init__()
        self.base, out_dim = _trunk(model_name, pretrained, input_ch)
        if pretrained_model is not None:
            self.base.load_state_dict({k.replace("module.", ""): v for k, v in pretrained_model.items()}, strict=False)
        self.seg = _seg_head(out_dim, n_class)
        self.dropout = nn.Dropout2d(0.2)
        self.criterion = criterion
        self.n_dropout_exp = n_dropout_exp
        self.uncertain_weight = uncertain_weight
        self.up = _up(n_class, n_class, use_torch_up)
        self.up_std = _up(n_class, n_class, use_torch_up)
        self._draws = np.random.RandomState(int(torch.initial_seed()) % (2 ** 32))

    def seed_draws(self, seed):
        """reseed the stream the per-draw scalars r_t come from (the trainer: from ``--seed``)"""
        self._draws = np.random.RandomState(int(seed) % (2 ** 32))

    def forward(self, x):
        x = self.dropout(self.seg(self.base(x)))
        return ops.up8(x, self.up.weight), torch.relu(ops.up8(x, self.up_std.weight))  # (std must not be negative, :158)

    def optim_parameters(self, memo=None):
        yield from self.base.parameters()
        yield from self.seg.parameters()

    def _class_weight(self, device):
        w = getattr(self.criterion, "weight", None)
        return None if w is None else w.to(device=device, dtype=torch.float32)

    def draw(self, n, c, device):
        """(keep uint8 [T,N,C], r fp32 [T], keep_scale) of one step"""
        t, p = self.n_dropout_exp, self.dropout.p
        if self.dropout.training and p > 0.0:
            keep = (torch.rand((t, n, c), device=device) >= p).to(torch.uint8)
            scale = 1.0 / (1.0 - p)
        else:
            keep, scale = torch.ones((t, n, c), dtype=torch.uint8, device=device), 1.0
        r = torch.from_numpy(self._draws.random_sample(t).astype(np.float32))
        return keep, (r.pin_memory() if device.type == "cuda" else r).to(device, non_blocking=True), scale

    def get_loss(self, x, gt, separately_returning=False, keep=None, r=None):
        if not self.training:
            self.train()  # as the reference's get_loss does (:172); a model in train mode keeps what --no_dropout / --fix_bn fixed
        dropping = self.dropout.training
        n, c, t = gt.size(0), self.seg.out_channels, self.n_dropout_exp
        if keep is None or r is None:
            k0, r0, scale = self.draw(n, c, x.device)
            keep, r = (k0 if keep is None else keep), (r0 if r is None else r)
        else:
            scale = 1.0 / (1.0 - self.dropout.p) if dropping else 1.0
        ignore = getattr(self.criterion, "ignore_index", -100)
        weight = self._class_weight(x.device)
        if fused_uncertain():
            with ops.bn_running_updates(t):  # the running statistics and num_batches_tracked move as in T passes
                s = self.seg(self.base(x))
            base_loss, uncertain = ops.up8_uncertain_loss(s, self.up.weight, self.up_std.weight, gt, weight, keep, r, self.uncertain_weight,
                                                          ignore, keep_scale=scale)
        else:
            base_loss, uncertain = self._literal_loss(x, gt, weight, ignore, keep, r, scale)
        if separately_returning:
            return base_loss, uncertain
        return base_loss + uncertain

    def _literal_loss(self, x, gt, weight, ignore, keep, r, scale):
        """the reference's loop as written (:176-204): T passes of the whole network, the dropout factors applied to the scores,
        both full-resolution maps of every draw, torch ops for the rest.  Labels outside [0, C) (which the reference's gather cannot
        take) contribute nothing, as in the kernel."""
        t = keep.shape[0]
        n_pixel = gt.numel() / gt.size(0)
        valid = (gt != ignore) & (gt >= 0) & (gt < self.seg.out_channels)
        index = torch.where(valid, gt, torch.zeros_like(gt)).unsqueeze(1)
        criterion = self.criterion if self.criterion is not None else (lambda z, g: ops.cross_entropy2d(z, g, None, ignore, True))
        base_loss, prob_sum = 0, 0
        for i in range(t):
            m = keep[i].to(torch.float32).mul(scale)[:, :, None, None]
            s = self.seg(self.base(x)) * m
            mean = ops.up8(s, self.up.weight)
            std = torch.relu(ops.up8(s, self.up_std.weight))
            base_loss = base_loss + criterion(mean, gt)
            noisy = mean + std * r[i]
            log_partition = noisy.exp().sum(1).log()  # (bare, as the reference forms it; the kernel subtracts the maximum)
            prob_sum = prob_sum + (torch.gather(noisy, 1, index).squeeze(1) - log_partition).exp()
        base_loss = base_loss / t
        log_mean = torch.where(valid, torch.log(prob_sum / t), torch.zeros_like(prob_sum))
        return base_loss, log_mean.sum(1).sum(1) / n_pixel * self.uncertain_weight


class DRNSegBase(nn.Module):
    def __init__(self, model_name, n_class, pretrained=True, input_ch=3, ver="ver1"):
        super().__init__()
        self.base, out_dim = _trunk(model_name, pretrained, input_ch)
        self.ver = ver
        if ver == "ver1":
            self.seg = _seg_head(out_dim, n_class)
        elif ver == "ver2":
            print("ver2 will be used")

    def forward(self, x):
        x = self.base(x)
        return x if self.ver == "ver2" else self.seg(x)

    def optim_parameters(self, memo=None):
        yield from self.base.parameters()
        yield from self.seg.parameters()


def _walk_stage(stage, x):
    """one DRN stage with an ordinary fp32 output (the stage-tap walk of ``MultiTaskEncoderReturningMultipleFeaturemaps``)"""
    if type(stage) is FusedSequential and not _has_hooks(stage):
        return run_fused(list(stage.children()), x)
    return stage(x)


class FuseDRNSegBase(nn.Module):
    """G of the middle fusion (``--net drn_d_XX_fusenet``; models/dilated_fcn.py:253-337): ONE set of DRN-D stages ``main_layer0`` ..
    ``main_layer8`` runs twice per forward -- on the HHA channels first, keeping every stage output ``x_dk``, then on the RGB channels
    with ``x = main_layerk(x) + x_dk`` behind every stage (``ops.stage_join``) -- and the 1x1 ``seg`` head scores the last sum.  The
    weights are shared: each convolution's weight gradient is the sum of both uses, each train-mode BatchNorm takes its batch statistics
    per call and updates its running statistics twice, HHA then RGB (``num_batches_tracked`` grows by 2 per forward).

    ``sub_layer0`` .. ``sub_layer8`` -- a second trunk for ``input_ch - 3`` channels -- are built and never called, as in the reference:
    the state-dict keys are the reference's and its checkpoints load.  Their parameters carry ``requires_grad = False``: in the reference
    they never receive a gradient, so no optimizer touches them (weight decay included); here they enter no flat buffer either.

    Departures: ``input_ch`` must be 6 (with 4 the reference feeds one channel to the 3-channel ``main_layer0`` and raises), only DRN-D
    (the reference asserts it), no ``ver2`` (the reference has no such constructor), no ``optim_parameters`` (the reference's reads a
    ``self.base`` that does not exist).  Every stage output is needed as fp32 -- it has two readers -- so compact activation storage and
    the 2-byte chain built on it are refused."""

    def __init__(self, model_name, n_class, pretrained=True, input_ch=6, ver="ver1"):
        super().__init__()
        if input_ch != 6:
            raise ValueError("FuseDRNSegBase takes input_ch == 6 (RGB + HHA): its shared stem has 3 input channels and sees the HHA "
                             "channels too, got input_ch = %r" % (input_ch,))
        if ver != "ver1":
            raise NotImplementedError("FuseDRNSegBase has no ver2 form (the reference looks up a constructor that does not exist)")
        ctor = drn.__dict__.get(model_name)
        if ctor is None or not model_name.startswith("drn_"):
            raise NotImplementedError("unknown DRN variant %r" % (model_name,))
        if not model_name.startswith("drn_d_"):
            raise NotImplementedError("FuseDRNSegBase is built on the DRN-D trunks only (the reference asserts arch == \"D\"), got %r"
                                      % (model_name,))
        self.ver = ver
        model = ctor(pretrained=pretrained, num_classes=0, input_ch=3)
        sub_model = ctor(pretrained=pretrained, num_classes=0, input_ch=input_ch - 3)
        for prefix, trunk in (("main", model), ("sub", sub_model)):
            for k in range(9):
                stage = getattr(trunk, "layer%d" % k)
                if stage is None:
                    raise NotImplementedError("%s has no layer%d: the FuseNet-style generator needs all nine stages" % (model_name, k))
                setattr(self, "%s_layer%d" % (prefix, k), stage)
        for k in range(9):
            for p in getattr(self, "sub_layer%d" % k).parameters():
                p.requires_grad_(False)
        self.seg = _seg_head(model.out_dim, n_class)

    def forward(self, x):
        if ops.ACT_STORAGE == "compact":
            raise NotImplementedError("FuseDRNSegBase hands out the fp32 outputs of its stages: it does not "
                                      "run with MCDSEG_ACT_STORAGE=compact (nor the 2-byte chain built on it); use fp32 storage")
        rgb, depth = x[:, :3, :, :], x[:, 3:, :, :]
        stages = [getattr(self, "main_layer%d" % k) for k in range(9)]
        # (one _LateGrad alias per weight: the HHA pass, which comes first, takes it, the RGB pass hands autograd the parameter itself --
        # its weight gradient stays on the main stream and both reach p.grad by the end of the backward pass, ops._take_late)
        with ops.late_weight_grads(self):
            x_d = []
            for stage in stages:
                depth = _walk_stage(stage, depth)
                x_d.append(depth)
            x = rgb
            for stage, x_dk in zip(stages, x_d):
                x = ops.stage_join(_walk_stage(stage, x), x_dk)
        return self.seg(x)


class DRNSegPixelClassifier(nn.Module):
    def __init__(self, n_class, use_torch_up=False, dropout=False, ver="ver1"):
        super().__init__()
        self.dropout = dropout
        self.ver = ver
        if ver == "ver2":
            self.seg = _seg_head(512, n_class)
        self.up = _up(n_class, n_class, use_torch_up)

    def forward(self, x):
        if self.ver == "ver2":
            x = self.seg(x)
        return self.up(x)


def score_map_hw(trunk, h, w):
    """(rows, columns) of the score map the DRN trunk makes of an h x w image, read off the trunk itself: every stage that strides
    does so in its first strided convolution (the shortcut projection beside it strides alike), the others keep the size"""
    for stage in trunk.children():
        conv = next((m for m in stage.modules() if isinstance(m, nn.Conv2d) and m.stride[0] > 1), None)
        if conv is not None:
            k, s, p, d = conv.kernel_size[0], conv.stride[0], conv.padding[0], conv.dilation[0]
            h, w = ((v + 2 * p - d * (k - 1) - 1) // s + 1 for v in (h, w))
    return h, w


def domain_fc_in(model_g, img_shape):
    """``fc1``'s width for a domain classifier behind ``model_g`` at ``--train_img_shape``: the score map, pooled 2x2 twice with floor
    division, one channel.  1089 at 1080 x 1080, the only size the reference's hard-coded Linear(1089, 10) fits."""
    a, b = score_map_hw(model_g.base, int(img_shape[0]), int(img_shape[1]))
    return (a // 2 // 2) * (b // 2 // 2)


class _LogitsOnly(torch.autograd.Function):
    """the logits ``DRNSegDomainClassifier.forward`` returns: values only -- a backward pass through them says where the gradient is"""

    @staticmethod
    def forward(ctx, logits, anchor):
        return logits.clone()

    @staticmethod
    def backward(ctx, grad):
        raise RuntimeError("DRNSegDomainClassifier.forward(x) returns logits without a gradient: the fused kernels differentiate the "
                           "cross-entropy they compute.  Use model_d.domain_loss(x, label) for criterion_d(model_d(x), label), or "
                           "model_d.forward_pair(src_fet, tgt_fet) for both domains at once.")


class DownConv(nn.Module):
    """conv3x3+bias, ReLU, conv3x3+bias, ReLU, MaxPool2d(2, 2) (models/dilated_fcn.py:506-531) as ONE kernel each way
    (csrc/dann.hip); ``conv1`` / ``conv2`` hold the parameters in torch's layout and default initialisation."""

    def __init__(self, in_channels, out_channels, pooling=True):
        super().__init__()
        if not pooling:
            raise NotImplementedError("DownConv without pooling is not part of the domain classifier")
        self.in_channels, self.out_channels, self.pooling = in_channels, out_channels, pooling
        self.conv1 = nn.Conv2d(in_channels, out_channels, kernel_size=3, stride=1, padding=1, bias=True)
        self.conv2 = nn.Conv2d(out_channels, out_channels, kernel_size=3, stride=1, padding=1, bias=True)

    def forward(self, x, groups=1):
        return ops.dann_down(x, self.conv1.weight, self.conv1.bias, self.conv2.weight, self.conv2.bias, groups)


class DRNSegDomainClassifier(nn.Module):
    """D of the DANN baseline (models/dilated_fcn.py:534-551): DownConv(n_class, 10), DownConv(10, 1), flatten, Linear(fc_in, 10),
    BatchNorm1d(10), ReLU, Linear(10, 2) on G's 1/8-resolution score map -- two DownConv launches and one launch for everything behind
    them, the two-class cross-entropy included (``ops.dann_down``, ``ops.dann_tail``).  State-dict keys and shapes are the reference's.

    ``fc_in`` is a departure: the reference hard-codes 1089 = 33 x 33, which fits 1080 x 1080 images only ("TODO This is for 4ch");
    the trainer passes ``domain_fc_in`` of its image size, which is 1089 there.

    ``forward_pair(src_fet, tgt_fet)`` is what the trainer calls: both domains through the three launches at once, BatchNorm1d
    statistics per domain and the running statistics updated source first, as the reference's two calls would -- it returns the two
    mean cross-entropies (source against label 1, target against 0) and the logits.  ``domain_loss(x, label)`` is one domain alone.
    ``forward(x)`` keeps the reference's signature and returns the logits of one domain through the same kernels; the kernels
    differentiate the cross-entropy they compute, so these logits carry no gradient: a backward pass through them raises an error
    that names ``domain_loss`` and ``forward_pair``."""

    def __init__(self, n_class, fc_in=1089):
        super().__init__()
        self.conv1 = DownConv(n_class, 10)
        self.conv2 = DownConv(10, 1)
        self.fc1 = nn.Linear(fc_in, 10)
        self.bn1 = nn.BatchNorm1d(10)
        self.fc2 = nn.Linear(10, 2)
        self._labels = {}

    def _domain_labels(self, labels, device):
        key = (tuple(int(v) for v in labels), str(device))
        if key not in self._labels:
            self._labels[key] = torch.tensor(key[0], dtype=torch.int32, device=device)
        return self._labels[key]

    def _run(self, x, labels):
        h = self.conv2(self.conv1(x, len(labels)), len(labels))
        h = h.view(h.size(0), -1)
        if h.size(1) != self.fc1.in_features:
            raise ValueError("DRNSegDomainClassifier: a %dx%d score map pools to %d features, fc1 takes %d (build the classifier with "
                             "fc_in=%d)" % (x.size(2), x.size(3), h.size(1), self.fc1.in_features, h.size(1)))
        bn = self.bn1
        if bn.momentum is None or not bn.track_running_stats or not bn.affine:
            raise NotImplementedError("the fused tail takes BatchNorm1d as the reference builds it (affine, running statistics, a momentum)")
        loss, logits = ops.dann_tail(h, self.fc1.weight, self.fc1.bias, bn.weight, bn.bias, self.fc2.weight, self.fc2.bias,
                                     self._domain_labels(labels, x.device), bn.running_mean, bn.running_var, bn.momentum, bn.eps, bn.training)
        if bn.training:
            bn.num_batches_tracked += len(labels)  # (one module call per domain in the reference)
        return loss, logits

    def forward(self, x):
        logits = self._run(x, (0,))[1]
        if torch.is_grad_enabled() and self.fc2.weight.requires_grad:  # (so that a backward pass through them raises OUR message)
            return _LogitsOnly.apply(logits, self.fc2.weight)
        return logits

    def domain_loss(self, x, label):
        """(mean cross-entropy of ``x``'s rows against the one domain ``label``, logits)"""
        loss, logits = self._run(x, (label,))
        return loss[0], logits

    def forward_pair(self, src_fet, tgt_fet, labels=(1, 0)):
        """(loss [2]: source against labels[0], target against labels[1]; logits [2n, 2], source rows first)"""
        if src_fet.shape != tgt_fet.shape:
            raise ValueError("forward_pair: the two domains' score maps differ in shape: %s, %s" % (tuple(src_fet.shape), tuple(tgt_fet.shape)))
        return self._run(torch.cat([src_fet, tgt_fet]), labels)


class FusionDRNSegPixelClassifier(nn.Module):
    def __init__(self, fusion_type, n_class, use_torch_up=False, ver="ver1"):
        super().__init__()
        self.fusion = get_fusion_model(fusion_type, n_class if ver == "ver1" else 512)
        self.ver = ver
        self.up = _up(2 * n_class if isinstance(self.fusion, ConcatFusion) else n_class, n_class, use_torch_up)
        if ver == "ver2":
            self.seg = _seg_head(512, n_class)

    def forward(self, x1, x2):
        if isinstance(self.fusion, AddFusion) and self.ver == "ver1":
            # up(x1 + x2) = up(x1) + up(x2): the sum is never materialised, one pass over the full-resolution output
            return ops.up8_dual(x1, self.up.weight, x2, self.up.weight)
        h = self.fusion(x1, x2)
        if self.ver == "ver2":
            h = self.seg(h)
        return self.up(h)


class ScoreFusionDRNSegPixelClassifier(nn.Module):
    def __init__(self, fusion_type, n_class):
        super().__init__()
        self.fusion = get_fusion_model(fusion_type, n_class)
        self.up1 = Up8(n_class)
        self.up2 = Up8(n_class)

    def forward(self, x1, x2):
        if isinstance(self.fusion, AddFusion):
            # up1(x1) + up2(x2) in one pass over the full-resolution tensor
            return ops.up8_dual(x1, self.up1.weight, x2, self.up2.weight)
        return self.fusion(self.up1(x1), self.up2(x2))


# ------------------------------------------------------------------------------------------------ multitask (cfg4)
class MultiTaskEncoder(nn.Module):
    """DRN trunk on the RGB channels (models/dilated_fcn.py:554-566)."""

    def __init__(self, model_name, pretrained=True, input_ch=3):
        super().__init__()
        self.base, _ = _trunk(model_name, pretrained, input_ch)

    def forward(self, x):
        return self.base(x)


class CBR(nn.Module):
    """conv (with bias) - BN - ReLU as one fused HIP group (models/dilated_fcn.py:632-644)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True):
        super().__init__()
        self.conv = Conv2d(in_channels, out_channels, kernel_size, stride=stride, padding=padding, dilation=dilation,
                           groups=groups, bias=bias)
        self.bn = BatchNorm2d(out_channels)

    def forward(self, x):
        return ops.conv_bn_act(x, self.conv, self.bn, relu=True)


class ThreeLayerDecoder(nn.Module):
    def __init__(self, output_ch, input_ch=512):
        super().__init__()
        self.cbr1 = CBR(input_ch, 512, kernel_size=3, padding=1)
        self.cbr2 = CBR(512, 512, kernel_size=1)
        self.conv3 = Conv2d(512, output_ch, kernel_size=1)

    def forward(self, x):
        return self.conv3(self.cbr2(self.cbr1(x)))


class _Bilinear8(nn.Module):
    """nn.Upsample(scale_factor=8, mode='bilinear') (align_corners=False) on the HIP kernel; holds no parameters, so
    the decoder's state_dict is unchanged."""

    def forward(self, x):
        return ops.bilinear8(x)


class MCDMultiTaskDecoder(nn.Module):
    """Two segmentation heads + one HHA-regression head on 512-ch features, x8 bilinear up-sampling, learned
    log-variance task weights ``exp(-s) * L + s`` (models/dilated_fcn.py:661-739)."""

    def __init__(self, n_class, depth_ch, semseg_criterion=None, discrepancy_criterion=None):
        super().__init__()
        self.s_semsegcls = Parameter(torch.ones(1))
        self.s_deprgr = Parameter(torch.ones(1))
        self.semsegcls_dec1 = ThreeLayerDecoder(n_class)
        self.semsegcls_dec2 = ThreeLayerDecoder(n_class)
        self.deprgr_dec = ThreeLayerDecoder(depth_ch)
        self.semseg_criterion = semseg_criterion
        self.discrepancy_criterion = discrepancy_criterion
        self.upsample = _Bilinear8()

    def semseg_forward(self, x):
        return self.upsample(self.semsegcls_dec1(x)), self.upsample(self.semsegcls_dec2(x))

    def depth_forward(self, x):
        return self.upsample(self.deprgr_dec(x))

    def forward(self, x):
        pred_semseg1, pred_semseg2 = self.semseg_forward(x)
        return pred_semseg1, pred_semseg2, self.depth_forward(x)

    def get_cls_descrepancy(self, x):
        pred_semseg1, pred_semseg2 = self.semseg_forward(x)
        return self.discrepancy_criterion(pred_semseg1, pred_semseg2)

    def get_semseg_loss(self, x, gt_semseg, separately_returning=False):
        pred_semseg1, pred_semseg2 = self.semseg_forward(x)
        loss1 = self.semseg_criterion(pred_semseg1, gt_semseg)
        loss2 = self.semseg_criterion(pred_semseg2, gt_semseg)
        return (loss1, loss2) if separately_returning else loss1 + loss2

    def get_depth_loss(self, x, gt_dep):
        return ops.mse_loss(self.depth_forward(x), gt_dep)

    def get_loss(self, x, gt_semseg, gt_dep, separately_returning=False):
        loss1, loss2 = self.get_semseg_loss(x, gt_semseg, separately_returning=True)
        s = self.s_semsegcls
        semseg_loss = ((torch.exp(-s) * loss1 + s) + (torch.exp(-s) * loss2 + s)) / 2
        depreg_loss = torch.exp(-self.s_deprgr) * self.get_depth_loss(x, gt_dep) + self.s_deprgr
        return (semseg_loss, depreg_loss) if separately_returning else semseg_loss + depreg_loss

    def get_task_weights(self):
        import numpy as np
        return (np.sqrt(np.exp(2 * self.s_semsegcls.data.cpu().numpy())), np.sqrt(np.exp(2 * self.s_deprgr.data.cpu().numpy())))


# ------------------------------------------------------------------------------------------------ segmentation + boundary ("segbd")
class MultiTaskEncoderReturningMultipleFeaturemaps(nn.Module):
    """The DRN stages as ``main_layer0`` .. ``main_layer8``, returning every stage's output ``h0`` .. ``h8``
    (models/dilated_fcn.py:569-629).  The stages run as on the trunk's stage-tap path (``DRN._forward`` with ``out_middle``): each
    one writes an ordinary fp32 output, so the decoder's gradients into ``h2``, ``h3`` and ``h8`` meet the main path's in autograd.
    Compact activation storage keeps no fp32 stage outputs and is refused."""

    def __init__(self, model_name, pretrained=True, input_ch=3):
        super().__init__()
        ctor = drn.__dict__.get(model_name)
        if ctor is None or not model_name.startswith("drn_"):
            raise NotImplementedError("unknown DRN variant %r" % (model_name,))
        model = ctor(pretrained=pretrained, num_classes=0, input_ch=input_ch)
        if "drn_d" in model_name:
            self.main_layer0 = model.layer0
        else:
            self.main_layer0 = FusedSequential(model.conv1, model.bn1, model.relu)
        for k in range(1, 9):
            stage = getattr(model, "layer%d" % k)
            if stage is None:
                raise NotImplementedError("%s has no layer%d: the multi-feature-map encoder needs all nine stages" % (model_name, k))
            setattr(self, "main_layer%d" % k, stage)

    def forward(self, x):
        if ops.ACT_STORAGE == "compact":
            raise NotImplementedError("MultiTaskEncoderReturningMultipleFeaturemaps hands out the fp32 outputs of its stages: it does not "
                                      "run with MCDSEG_ACT_STORAGE=compact (nor the 2-byte chain built on it); use fp32 storage")
        out = {}
        with ops.late_weight_grads(self):
            for k in range(9):
                stage = getattr(self, "main_layer%d" % k)
                if type(stage) is FusedSequential and not _has_hooks(stage):
                    x = run_fused(list(stage.children()), x)
                else:
                    x = stage(x)
                out["h%d" % k] = x
        return out


def _get_boundary(var):
    """``get_boundary`` of models/dilated_fcn.py:770-774: 3x3 dilation != 3x3 erosion"""
    if var.is_cuda and var.dim() == 3 and var.dtype in (torch.int64, torch.uint8):
        return ops.label_boundary(var)
    v = var.float()
    v4 = v if v.dim() == 4 else v[:, None]
    dilation = nn.functional.max_pool2d(v4, kernel_size=3, stride=1, padding=1)
    erosion = -nn.functional.max_pool2d(-v4, kernel_size=3, stride=1, padding=1)
    return (dilation != erosion).reshape(v.shape)


def get_boundary_loss(pred, gt, pred_type="semseg", gt_type="semseg"):
    """models/dilated_fcn.py:743-787: class-balanced BCE between a boundary prediction and a boundary target, either of which may be
    given as a label map ("semseg": its boundary is taken) or as a boundary map ("boundary"; a target is detached)."""
    from loss import bce2d
    assert pred_type in ["semseg", "boundary"]
    assert gt_type in ["semseg", "boundary"]
    gt_boundary = _get_boundary(gt) if gt_type == "semseg" else gt.detach()
    pred_boundary = _get_boundary(pred) if pred_type == "semseg" else pred
    if gt_boundary.dtype != torch.uint8 or not gt_boundary.is_cuda:
        gt_boundary = gt_boundary.to(pred_boundary.dtype if pred_boundary.dtype.is_floating_point else torch.float32)
    return bce2d(pred_boundary.float(), gt_boundary)


class MCDSegBDMultiTaskDecoder(nn.Module):
    """Two segmentation heads on ``h8`` + a HED-style boundary head on ``h2``, ``h3``, ``h8`` (three 1-channel 1x1 projections,
    bilinear x2 / x4 / x8, mean of the three sigmoids), learned log-variance task weights (models/dilated_fcn.py:1027-1222).
    ``semseg_shortcut`` (full-resolution 512-channel decoders) and ``use_seg2bd_conv`` (a 5x5 convolution on the logits) are not
    built; ``depth_shortcut`` is accepted and ignored, as in the reference."""

    def __init__(self, n_class, depth_ch, semseg_criterion=None, discrepancy_criterion=None, semseg_shortcut=False,
                 depth_shortcut=False, add_pred_seg_boundary_loss=False, use_seg2bd_conv=False):
        super().__init__()
        if semseg_shortcut:
            raise NotImplementedError("semseg_shortcut (segmentation decoders on full-resolution 512-channel maps) is not implemented")
        if use_seg2bd_conv:
            raise NotImplementedError("use_seg2bd_conv (a 5x5 boundary convolution on the segmentation logits) is not implemented")
        self.s_semsegcls = Parameter(torch.ones(1))
        self.s_boundary = Parameter(torch.ones(1))
        self.semsegcls_dec1 = ThreeLayerDecoder(n_class)
        self.semsegcls_dec2 = ThreeLayerDecoder(n_class)
        self.semseg_criterion = semseg_criterion
        self.discrepancy_criterion = discrepancy_criterion
        self.upsample3 = _Bilinear8()
        self.conv1 = Conv2d(32, 1, kernel_size=1, stride=1, padding=0)
        self.conv2 = Conv2d(64, 1, kernel_size=1, stride=1, padding=0)
        self.conv3 = Conv2d(512, 1, kernel_size=1, stride=1, padding=0)
        self.semseg_shortcut = semseg_shortcut
        self.depth_shortcut = depth_shortcut
        self.add_pred_seg_boundary_loss = add_pred_seg_boundary_loss
        self.use_seg2bd_conv = use_seg2bd_conv
        if self.add_pred_seg_boundary_loss:
            self.s_pred_seg_boundary = Parameter(torch.ones(1))

    def semseg_forward(self, x_dic):
        return self.upsample3(self.semsegcls_dec1(x_dic["h8"])), self.upsample3(self.semsegcls_dec2(x_dic["h8"]))

    def _boundary_maps(self, x_dic):
        return self.conv1(x_dic["h2"]), self.conv2(x_dic["h3"]), self.conv3(x_dic["h8"])

    def boundary_forward(self, x_dic):
        return ops.boundary_head(*self._boundary_maps(x_dic))

    def forward(self, x_dic):
        pred_semseg1, pred_semseg2 = self.semseg_forward(x_dic)
        return pred_semseg1, pred_semseg2, self.boundary_forward(x_dic)

    def get_cls_descrepancy(self, x_dic):
        pred_semseg1, pred_semseg2 = self.semseg_forward(x_dic)
        return self.discrepancy_criterion(pred_semseg1, pred_semseg2)

    @staticmethod
    def _argmax_labels(pred_semseg):
        """``pred.max(1)[1]`` as a label map (gradient-free): uint8 from the predict kernel on the GPU"""
        pred = pred_semseg.detach()
        if pred.is_cuda and pred.dtype == torch.float32 and pred.shape[1] <= 255:
            return ops.predict_labels(pred)[0]
        return pred.max(1)[1]

    def get_semseg_loss(self, x_dic, gt_semseg, separately_returning=False):
        pred_semseg1, pred_semseg2 = self.semseg_forward(x_dic)
        loss1 = self.semseg_criterion(pred_semseg1, gt_semseg)
        loss2 = self.semseg_criterion(pred_semseg2, gt_semseg)
        # the "extra" losses (:1145-1153): the arg-max boundary of each head against the labels' -- values without a gradient
        loss1 = loss1 + get_boundary_loss(self._argmax_labels(pred_semseg1), gt_semseg)
        loss2 = loss2 + get_boundary_loss(self._argmax_labels(pred_semseg2), gt_semseg)
        return (loss1, loss2) if separately_returning else loss1 + loss2

    def get_psuedo_boundary_loss(self, x_dic, separately_returning=False):
        """:1183-1200.  The prediction is an arg-max and the target is detached, so the reference's value carries no gradient either:
        it is computed without a tape."""
        assert self.add_pred_seg_boundary_loss
        with torch.no_grad():
            psuedo_boundary = self.boundary_forward(x_dic)
            pred_semseg1, pred_semseg2 = self.semseg_forward(x_dic)
            loss1 = get_boundary_loss(pred=self._argmax_labels(pred_semseg1), gt=psuedo_boundary, gt_type="boundary")
            loss2 = get_boundary_loss(pred=self._argmax_labels(pred_semseg2), gt=psuedo_boundary, gt_type="boundary")
        return (loss1, loss2) if separately_returning else loss1 + loss2

    def get_boundary_loss(self, x_dic, gt_semseg):
        s1, s2, s3 = self._boundary_maps(x_dic)
        if s1.is_cuda and gt_semseg.is_cuda and gt_semseg.dtype == torch.int64:
            return ops.boundary_head_bce(s1, s2, s3, gt_semseg)  # the head, the target and the loss in one pass each way
        return get_boundary_loss(pred=ops.boundary_head(s1, s2, s3), gt=gt_semseg, pred_type="boundary")

    def get_loss(self, x, gt_semseg, separately_returning=False):
        loss1, loss2 = self.get_semseg_loss(x, gt_semseg, separately_returning=True)
        s = self.s_semsegcls
        semseg_loss = ((torch.exp(-s) * loss1 + s) + (torch.exp(-s) * loss2 + s)) / 2
        boundary_loss = torch.exp(-self.s_boundary) * self.get_boundary_loss(x, gt_semseg) + self.s_boundary
        return (semseg_loss, boundary_loss) if separately_returning else semseg_loss + boundary_loss

    def get_task_weights(self):
        """the reference reads ``self.s_deprgr`` here (:1221), which this decoder does not have -- the call raises there; the second
        value is the boundary task's standard deviation"""
        import numpy as np
        return (np.sqrt(np.exp(2 * self.s_semsegcls.data.cpu().numpy())), np.sqrt(np.exp(2 * self.s_boundary.data.cpu().numpy())))


# ------------------------------------------------------------------------------------------------ segmentation + depth + boundary ("triple")
class MCDTripleMultiTaskDecoder(nn.Module):
    """Two segmentation heads and an HHA-regression head on ``h8`` + the HED-style boundary head on ``h2``, ``h3``, ``h8``, three learned
    log-variance task weights (models/dilated_fcn.py:790-1024).  ``nmlrgr_dec`` is built and never used, as in the reference.  With
    ``use_seg2bd_conv`` a 5x5 convolution on the segmentation logits predicts the boundary as well (``get_boundary_loss_by_extra_conv``):
    ``seg2bd_conv`` holds its parameters, the convolution itself runs inside ``ops.seg2bd_bce`` on the decoders' 1/8-resolution outputs.
    ``semseg_shortcut`` and ``depth_shortcut`` (decoders on full-resolution 512-channel maps) are not built.

    ``logits=`` of the loss methods takes the pair ``_semseg_logits`` returned for the same features, for a caller that needs the
    segmentation decoders' outputs twice (the solver's step A); the default runs the decoders, as the reference does."""

    def __init__(self, n_class, depth_ch, semseg_criterion=None, discrepancy_criterion=None, semseg_shortcut=False,
                 depth_shortcut=False, add_pred_seg_boundary_loss=False, use_seg2bd_conv=False):
        super().__init__()
        if semseg_shortcut:
            raise NotImplementedError("semseg_shortcut (segmentation decoders on full-resolution 512-channel maps) is not implemented")
        if depth_shortcut:
            raise NotImplementedError("depth_shortcut (a depth decoder on full-resolution 512-channel maps) is not implemented")
        self.s_semsegcls = Parameter(torch.ones(1))
        self.s_deprgr = Parameter(torch.ones(1))
        self.s_boundary = Parameter(torch.ones(1))
        self.semsegcls_dec1 = ThreeLayerDecoder(n_class)
        self.semsegcls_dec2 = ThreeLayerDecoder(n_class)
        self.deprgr_dec = ThreeLayerDecoder(depth_ch)
        self.nmlrgr_dec = ThreeLayerDecoder(depth_ch)
        self.semseg_criterion = semseg_criterion
        self.discrepancy_criterion = discrepancy_criterion
        self.upsample3 = _Bilinear8()
        self.conv1 = Conv2d(32, 1, kernel_size=1, stride=1, padding=0)
        self.conv2 = Conv2d(64, 1, kernel_size=1, stride=1, padding=0)
        self.conv3 = Conv2d(512, 1, kernel_size=1, stride=1, padding=0)
        self.semseg_shortcut = semseg_shortcut
        self.depth_shortcut = depth_shortcut
        self.add_pred_seg_boundary_loss = add_pred_seg_boundary_loss
        if self.add_pred_seg_boundary_loss:
            self.s_pred_seg_boundary = Parameter(torch.ones(1))
        self.use_seg2bd_conv = use_seg2bd_conv
        if self.use_seg2bd_conv:
            self.seg2bd_conv = nn.Conv2d(n_class, 1, kernel_size=5, padding=2)  # (parameters only: ops.seg2bd_bce applies them)

    def _semseg_logits(self, x_dic):
        """the two segmentation decoders' outputs at 1/8 resolution"""
        return self.semsegcls_dec1(x_dic["h8"]), self.semsegcls_dec2(x_dic["h8"])

    def semseg_forward(self, x_dic, logits=None):
        z1, z2 = self._semseg_logits(x_dic) if logits is None else logits
        return self.upsample3(z1), self.upsample3(z2)

    def depth_forward(self, x_dic):
        return self.upsample3(self.deprgr_dec(x_dic["h8"]))

    def _boundary_maps(self, x_dic):
        return self.conv1(x_dic["h2"]), self.conv2(x_dic["h3"]), self.conv3(x_dic["h8"])

    def boundary_forward(self, x_dic):
        return ops.boundary_head(*self._boundary_maps(x_dic))

    def forward(self, x_dic):
        pred_semseg1, pred_semseg2 = self.semseg_forward(x_dic)
        return pred_semseg1, pred_semseg2, self.depth_forward(x_dic), self.boundary_forward(x_dic)

    def get_cls_descrepancy(self, x_dic):
        pred_semseg1, pred_semseg2 = self.semseg_forward(x_dic)
        return self.discrepancy_criterion(pred_semseg1, pred_semseg2)

    def get_semseg_loss(self, x_dic, gt_semseg, separately_returning=False, logits=None):
        pred_semseg1, pred_semseg2 = self.semseg_forward(x_dic, logits)
        loss1 = self.semseg_criterion(pred_semseg1, gt_semseg)
        loss2 = self.semseg_criterion(pred_semseg2, gt_semseg)
        if self.add_pred_seg_boundary_loss:
            # :941-949: the arg-max boundary of each head against the labels' -- values without a gradient (the reference's ``.cuda()``
            # on them only moves a value to the device)
            argmax = MCDSegBDMultiTaskDecoder._argmax_labels
            loss1 = loss1 + get_boundary_loss(argmax(pred_semseg1), gt_semseg)
            loss2 = loss2 + get_boundary_loss(argmax(pred_semseg2), gt_semseg)
        return (loss1, loss2) if separately_returning else loss1 + loss2

    def get_depth_loss(self, x_dic, gt_dep):
        return ops.mse_loss(self.depth_forward(x_dic), gt_dep)

    def get_boundary_loss_by_extra_conv(self, x_dic, gt_bdry=None, separately_returning=False, logits=None):
        """:960-981: bce2d(sigmoid(seg2bd_conv(pred_semseg)), target) per head, from the 1/8-resolution logits in one fused pass each
        way; ``gt_bdry`` None takes the detached ``boundary_forward`` as a soft target."""
        assert self.use_seg2bd_conv
        z1, z2 = self._semseg_logits(x_dic) if logits is None else logits
        if gt_bdry is None:
            with torch.no_grad():  # "do not compute gradients w.r.t target"
                gt_bdry = self.boundary_forward(x_dic)
        elif gt_bdry.dtype not in (torch.float32, torch.uint8):
            gt_bdry = gt_bdry.float()
        loss1, loss2 = ops.seg2bd_bce(z1, z2, self.seg2bd_conv.weight, self.seg2bd_conv.bias, gt_bdry.detach())
        return (loss1, loss2) if separately_returning else loss1 + loss2

    def get_psuedo_boundary_loss(self, x_dic, separately_returning=False):
        """:983-1000.  The reference raises TypeError here: it passes ``pred_semseg=`` to ``get_boundary_loss``, whose parameter is
        ``pred``.  Built as MCDSegBDMultiTaskDecoder's (:1183-1200), which is what the call was copied from: each head's arg-max boundary
        against the detached boundary head -- a value without a gradient, computed without a tape."""
        assert self.add_pred_seg_boundary_loss
        with torch.no_grad():
            psuedo_boundary = self.boundary_forward(x_dic)
            pred_semseg1, pred_semseg2 = self.semseg_forward(x_dic)
            argmax = MCDSegBDMultiTaskDecoder._argmax_labels
            loss1 = get_boundary_loss(pred=argmax(pred_semseg1), gt=psuedo_boundary, gt_type="boundary")
            loss2 = get_boundary_loss(pred=argmax(pred_semseg2), gt=psuedo_boundary, gt_type="boundary")
        return (loss1, loss2) if separately_returning else loss1 + loss2

    def get_boundary_loss(self, x_dic, gt_boundary):
        """:1002-1004: bce2d(boundary_forward(x), gt_boundary), the head and the loss in one pass each way"""
        if gt_boundary.dtype not in (torch.float32, torch.uint8):
            gt_boundary = gt_boundary.float()
        return ops.boundary_head_bce_target(*self._boundary_maps(x_dic), gt_boundary.detach())

    def _semseg_task_loss(self, x, gt_semseg, logits=None):
        loss1, loss2 = self.get_semseg_loss(x, gt_semseg, separately_returning=True, logits=logits)
        s = self.s_semsegcls
        return ((torch.exp(-s) * loss1 + s) + (torch.exp(-s) * loss2 + s)) / 2

    def get_loss(self, x, gt_semseg, gt_dep, gt_boundary, separately_returning=False, logits=None):
        semseg_loss = self._semseg_task_loss(x, gt_semseg, logits)
        depreg_loss = torch.exp(-self.s_deprgr) * self.get_depth_loss(x, gt_dep) + self.s_deprgr
        boundary_loss = torch.exp(-self.s_boundary) * self.get_boundary_loss(x, gt_boundary) + self.s_boundary
        if separately_returning:
            return semseg_loss, depreg_loss, boundary_loss
        return semseg_loss + depreg_loss + boundary_loss

    def get_task_weights(self):
        import numpy as np
        return (np.sqrt(np.exp(2 * self.s_semsegcls.data.cpu().numpy())), np.sqrt(np.exp(2 * self.s_deprgr.data.cpu().numpy())))
