"""Loss criteria of the MCD hot path on the fused HIP kernel (reference: loss.py).

  CrossEntropyLoss2d           loss.py:7-13    log_softmax(dim 1) + weighted NLL (mean over sum of weights)
  ProbCrossEntropyLoss2d       loss.py:16-30   weighted NLL of log(p) for probability maps (gated MFNet fusions)
  Diff2d                       loss.py:93-100  mean |softmax(o1) - softmax(o2)|
  get_prob_distance_criterion  loss.py:192-210 ("diff" is the default ``--d_loss``, argmyparse.py:131)
  bce2d                        loss.py:131-138 class-balanced binary cross-entropy (the seg + boundary multitask decoder)

All criteria are thin ``nn.Module`` shells over ``mcdseg.ops`` (forward value and d/dlogits come out of
one streaming pass).  ``DiscrepancyLoss`` is an alias of ``Diff2d`` (BASELINE.json uses that name; the
reference has no such symbol).  The other distances of the reference (JSD, Symkl2d, MySymkl2d, SpatialJSD2d,
MisSymKLD; loss.py:70-189) are three functions of the two softmaxes; each class names
its function in ``dist_kind`` (``mcdseg.ops.DIST_KINDS``) and runs ``ops.prob_distance`` -- the fused HIP
kernel -- on fp32 GPU logits.  Anything else (CPU tensors, fp64, ``size_average=False``) evaluates the torch
expression the class carries, which is also the statement of what the kernel computes.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from mcdseg import ops


class _ClassWeights(nn.Module):
    """holds the class-weight vector where the reference's ``nn.NLLLoss2d`` holds it: buffer ``weight``"""

    def __init__(self, weight):
        super().__init__()
        self.register_buffer("weight", weight)


class CrossEntropyLoss2d(nn.Module):
    def __init__(self, weight=None, size_average=True, ignore_index=-100):
        super().__init__()
        self.nll_loss = _ClassWeights(weight)  # state-dict key ``nll_loss.weight`` as in the reference (loss.py:10)
        self.size_average = size_average
        self.ignore_index = ignore_index

    @property
    def weight(self):
        return self.nll_loss.weight

    def forward(self, inputs, targets):
        w = self.weight
        if w is not None and w.device != inputs.device:
            w = w.to(inputs.device)
        return ops.cross_entropy2d(inputs, targets, w, self.ignore_index, self.size_average)


class ProbCrossEntropyLoss2d(nn.Module):
    """cross entropy between a probability map (0..1) and the labels (loss.py:16-30): the criterion the reference pairs
    with the gated MFNet fusions (adapt_mfnet_trainer.py:149)"""

    def __init__(self, weight=None, size_average=True):
        super().__init__()
        self.nll_loss = _ClassWeights(weight)
        self.size_average = size_average

    def forward(self, inputs, targets):
        w = self.nll_loss.weight
        if w is not None and w.device != inputs.device:
            w = w.to(inputs.device)
        return ops.prob_cross_entropy2d(inputs, targets, w, -100, self.size_average)


class Diff2d(nn.Module):
    dist_kind = 0

    def __init__(self, weight=None, size_average=True):
        super().__init__()
        self.weight = weight

    def forward(self, inputs1, inputs2):
        return ops.diff2d(inputs1, inputs2)


DiscrepancyLoss = Diff2d


# ---- the non-default probability distances (torch 0.4's implicit softmax dim of a 4-D tensor is 1, and
# F.kl_div(input, target, size_average=True) is the element-wise mean of target * (log(target) - input))
def _kl_mean(log_q, p, size_average=True):
    return F.kl_div(log_q, p, reduction="mean" if size_average else "sum")


def _on_kernel(inputs1, inputs2, size_average=True):
    """the HIP kernel takes this call: element mean, two fp32 GPU tensors of one 4-D shape with at most the 48 classes it keeps in registers"""
    return (size_average and inputs1.is_cuda and inputs2.is_cuda and inputs1.dtype == inputs2.dtype == torch.float32
            and inputs1.dim() == 4 and inputs1.shape == inputs2.shape and inputs1.shape[1] <= 48)


class JSD(nn.Module):
    """loss.py:78-89: 0.5 * (KL(p1 || softmax(m)) + KL(p2 || softmax(m))) with m the mean of the LOGITS"""

    dist_kind = 3  # mcdseg.ops.DIST_KINDS / MCDSEG_DIST_* of include/mcdseg.h

    def __init__(self, weight=None, size_average=True):
        super().__init__()
        self.weight, self.size_average = weight, size_average

    def forward(self, inputs1, inputs2):
        if _on_kernel(inputs1, inputs2, self.size_average):
            return ops.prob_distance(inputs1, inputs2, self.dist_kind)
        log_m = F.log_softmax(0.5 * (inputs1 + inputs2), dim=1)
        return 0.5 * (_kl_mean(log_m, F.softmax(inputs1, dim=1), self.size_average) +
                      _kl_mean(log_m, F.softmax(inputs2, dim=1), self.size_average))


class Symkl2d(nn.Module):
    """loss.py:103-118: symmetric KL over rows of ``n_target_ch`` entries (a plain ``view`` of NCHW, as the reference does)"""

    dist_kind = 1  # mcdseg.ops.DIST_KINDS / MCDSEG_DIST_* of include/mcdseg.h

    def __init__(self, weight=None, n_target_ch=None, size_average=True):
        super().__init__()
        self.weight, self.n_target_ch, self.size_average = weight, n_target_ch, size_average

    def forward(self, inputs1, inputs2):
        if _on_kernel(inputs1, inputs2, self.size_average):
            return ops.prob_distance(inputs1, inputs2, self.dist_kind)
        rows = lambda t: t.reshape(-1, self.n_target_ch)  # noqa: E731
        p1, p2 = rows(F.softmax(inputs1, dim=1)), rows(F.softmax(inputs2, dim=1))
        l1, l2 = rows(F.log_softmax(inputs1, dim=1)), rows(F.log_softmax(inputs2, dim=1))
        return 0.5 * (_kl_mean(l1, p2, self.size_average) + _kl_mean(l2, p1, self.size_average))


class MySymkl2d(nn.Module):
    """loss.py:144-154: mean over all elements of 0.5 * (p1 log(p1/p2) + p2 log(p2/p1))"""

    dist_kind = 1  # mcdseg.ops.DIST_KINDS / MCDSEG_DIST_* of include/mcdseg.h

    def __init__(self, weight=None, size_average=True):
        super().__init__()
        self.weight = weight

    def forward(self, inputs1, inputs2):
        if _on_kernel(inputs1, inputs2):
            return ops.prob_distance(inputs1, inputs2, self.dist_kind)
        p1, p2 = F.softmax(inputs1, dim=1), F.softmax(inputs2, dim=1)
        return torch.mean(0.5 * (p1 * torch.log(p1 / p2) + p2 * torch.log(p2 / p1)))


class MisSymKLD(nn.Module):
    """loss.py:66-75 (and SpatialJSD2d, loss.py:157-173, which evaluates the same expression): kl_div is handed
    PROBABILITIES where it expects log-probabilities -- 'strange but somehow works well' in the reference's words"""

    dist_kind = 2  # mcdseg.ops.DIST_KINDS / MCDSEG_DIST_* of include/mcdseg.h

    def __init__(self, weight=None, size_average=True):
        super().__init__()
        self.weight = weight

    def forward(self, inputs1, inputs2):
        if _on_kernel(inputs1, inputs2):
            return ops.prob_distance(inputs1, inputs2, self.dist_kind)
        p1, p2 = F.softmax(inputs1, dim=1), F.softmax(inputs2, dim=1)
        return 0.5 * (_kl_mean(p1, p2) + _kl_mean(p2, p1))


SpatialJSD2d = MisSymKLD


def bce2d(input, target):
    """loss.py:131-138: beta = 1 - mean(target), weights = 1 - beta + (2 beta - 1) target, the weighted mean binary cross-entropy.
    The reference hands F.binary_cross_entropy an [N,1,H,W] input with an [N,H,W] target, which the torch of its day took for
    equal element counts; both are flattened here.  fp32 GPU tensors (target fp32, or uint8 as ``ops.label_boundary`` writes
    it) run ``ops.bce2d`` -- one HIP pass forward, one backward; anything else evaluates the torch expression below, which is also
    the statement of what the kernel computes (logs clamped at -100 as today's F.binary_cross_entropy does, where the reference
    era added 1e-12 inside the log)."""
    assert not target.requires_grad, \
        "nn criterions don't compute the gradient w.r.t. targets - please mark these variables as not requiring gradients"
    if input.numel() != target.numel():
        raise ValueError("bce2d: input %s and target %s differ in size" % (tuple(input.shape), tuple(target.shape)))
    if input.is_cuda and target.is_cuda and input.dtype == torch.float32 and target.dtype in (torch.float32, torch.uint8):
        return ops.bce2d(input, target)
    target = target.reshape(input.shape).to(input.dtype)
    beta = 1 - torch.mean(target)
    weights = 1 - beta + (2 * beta - 1) * target
    return F.binary_cross_entropy(input, target, weights, reduction="mean")


def get_prob_distance_criterion(criterion_name, n_class=None):
    """loss.py:192-210; every name runs on the fused HIP kernels (``dist_kind`` of the class says which distance)"""
    if criterion_name == "diff":
        return Diff2d()
    if criterion_name == "jsd":
        return JSD()
    if criterion_name in ("symkl", "nmlsymkl"):
        return Symkl2d(n_target_ch=n_class, size_average=True)
    if criterion_name == "mysymkl":
        return MySymkl2d()
    if criterion_name == "spatial_jsd":
        return SpatialJSD2d()
    if criterion_name == "mis_symkl":
        return MisSymKLD()
    raise NotImplementedError()
