"""The plain statement of the data-parallel loss contract (not a test module; fp64 torch on the CPU, nothing of the product imported).

DESIGN section 5: a batch cut into ``world`` shards, one per rank, must train as the reference's single process trains on the whole
batch -- the cross-entropy is ONE weighted mean over every pixel of every shard,

    CE = sum_i w[y_i] (-log softmax(z_i)[y_i]) / W,      W = sum_i w[y_i]   over the valid pixels of the WHOLE batch,

(``global_ce``), so each rank divides by W / world and the optimizer's 1/world average of the ranks' gradients is d CE / dz.
``mean_of_means`` is the wrong answer that looks right: every shard normalised by its own sum of weights, the results averaged.  The two
agree exactly when all shards hold the same labels -- which is why the tests built on this module cut UNEQUAL shards (``make_labels``)
and why ``tests/test_dp_shard_ref_host.py`` first proves, on this statement alone, that the two answers lie far apart on every label
layout a GPU test uses.

A pixel is valid when its label is not ``ignore_index`` and lies in [0, C) (the kernels' rule; torch's nll_loss refuses the labels
outside the range that the kernels skip).  A valid pixel of a class of weight 0 adds nothing to either sum.
"""
import torch

# the discrepancy's element mean runs over N*C*H*W: equal-sized shards average exactly, so it has no normaliser to get wrong -- but a
# gradient check of the combined objective needs it
CE_COEF, DIFF_COEF = 1.0, -1.0


def shards(n, world):
    """[(n0, n1), ...]: ``world`` equal cuts of a batch of ``n`` images"""
    assert n % world == 0, (n, world)
    k = n // world
    return [(r * k, (r + 1) * k) for r in range(world)]


def class_weights(c, seed=0, dead=None):
    """real-valued weights in [0.5, 1.5); class ``dead`` (default: the last one, as the reference's void class) has weight 0"""
    g = torch.Generator().manual_seed(7000 + 31 * c + seed)
    cw = 0.5 + torch.rand(c, generator=g)
    if c > 1:
        cw[c - 1 if dead is None else dead] = 0.0
    return cw


def make_labels(n, h, w, c, ignore_index, world, seed=0, empty=None):
    """int64 [n, h, w].  Shard 0: about 90 % of its pixels carry no weight -- a mix of ``ignore_index``, the out-of-range labels -1, C and
    C + 1, and the weight-0 class C - 1 (``class_weights``); shard r > 0 is ordinary: 5 % + 10 % (r - 1) such pixels.  ``empty``: the
    index of a shard that holds no valid pixel at all (the same mix, everywhere)."""
    g = torch.Generator().manual_seed(9000 + 131 * n + 17 * h + 13 * w + 7 * c + 3 * world + seed)
    y = torch.randint(0, max(c - 1, 1), (n, h, w), generator=g)
    junk = torch.tensor([ignore_index, ignore_index, -1, c, c + 1, c - 1, c - 1, ignore_index])
    for r, (n0, n1) in enumerate(shards(n, world)):
        frac = 1.0 if r == empty else (0.9 if r == 0 else 0.05 + 0.1 * (r - 1))
        shape = (n1 - n0, h, w)
        out = torch.rand(shape, generator=g) < frac
        pick = junk[torch.randint(0, junk.numel(), shape, generator=g)]
        y[n0:n1] = torch.where(out, pick, y[n0:n1])
    return y


def valid_mask(y, c, ignore_index):
    return (y != ignore_index) & (y >= 0) & (y < c)


def weight_sum(y, cw, c, ignore_index):
    """W in fp64 (``cw`` None: weight 1)"""
    ok = valid_mask(y, c, ignore_index)
    if cw is None:
        return ok.double().sum()
    return cw.double()[y.clamp(0, c - 1)][ok].sum()


def _ce_sum(z, y, cw, ignore_index):
    """(sum_i w[y_i] nll_i, W) of logits ``z`` [n, C, h, w] (fp64, may require grad)"""
    c = z.shape[1]
    ok = valid_mask(y, c, ignore_index)
    yy = y.clamp(0, c - 1)
    wy = (torch.ones(c, dtype=torch.float64) if cw is None else cw.double())[yy] * ok.double()
    nll = -torch.log_softmax(z, dim=1).gather(1, yy[:, None]).squeeze(1)
    return (wy * nll).sum(), wy.sum()


def _leaf(z):
    return z.detach().double().cpu().clone().requires_grad_()


def global_ce(z_full, y_full, cw, ignore_index):
    """(value, d value / dz) of the reference's one weighted mean over the whole batch"""
    z = _leaf(z_full)
    s, wsum = _ce_sum(z, y_full, cw, ignore_index)
    val = s / wsum
    val.backward()
    return val.detach(), z.grad


def mean_of_means(z_full, y_full, cw, ignore_index, world):
    """THE WRONG ANSWER: each shard's own weighted mean, averaged over the shards -- what a rank-local normaliser followed by the
    optimizer's 1/world computes.  (value, gradient); a shard without a valid pixel makes it NaN, as torch's nll_loss would."""
    z = _leaf(z_full)
    val = 0.0
    for n0, n1 in shards(z.shape[0], world):
        s, wsum = _ce_sum(z[n0:n1], y_full[n0:n1], cw, ignore_index)
        val = val + s / wsum / world
    val.backward()
    return val.detach(), z.grad


def diff_l1(a, b):
    """Diff2d: mean |softmax(a) - softmax(b)| over every element"""
    return (torch.softmax(a, dim=1) - torch.softmax(b, dim=1)).abs().mean()


def _objective(z1_full, z2_full, y_full, cw, ignore_index, dist, world):
    """CE_COEF (CE(z1) + CE(z2)) + DIFF_COEF dist(z1, z2) -- ``world`` None: the global statement; else shard-local normalisers.
    ``dist``: a callable of two logit tensors (``diff_l1``, or a criterion of the product's ``loss.get_prob_distance_criterion``, which
    are torch expressions in fp64 on the CPU); z2_full None: the one-head cross-entropy.  Returns dict(ce1, ce2, dist, g1, g2)."""
    z1 = _leaf(z1_full)
    z2 = _leaf(z2_full) if z2_full is not None else None
    cuts = [(0, z1.shape[0])] if world is None else shards(z1.shape[0], world)
    ce1 = ce2 = d = torch.zeros((), dtype=torch.float64)
    for n0, n1 in cuts:
        s, wsum = _ce_sum(z1[n0:n1], y_full[n0:n1], cw, ignore_index)
        ce1 = ce1 + s / wsum / len(cuts)
        if z2 is not None:
            s, wsum = _ce_sum(z2[n0:n1], y_full[n0:n1], cw, ignore_index)
            ce2 = ce2 + s / wsum / len(cuts)
            d = d + dist(z1[n0:n1], z2[n0:n1]) / len(cuts)
    total = CE_COEF * (ce1 + ce2) + (DIFF_COEF * d if z2 is not None else 0.0)
    total.backward()
    return dict(ce1=ce1.detach(), ce2=ce2.detach(), dist=d.detach(), g1=z1.grad, g2=None if z2 is None else z2.grad)


def global_objective(z1_full, z2_full, y_full, cw, ignore_index, dist=diff_l1):
    return _objective(z1_full, z2_full, y_full, cw, ignore_index, dist, None)


def mean_of_means_objective(z1_full, z2_full, y_full, cw, ignore_index, world, dist=diff_l1):
    return _objective(z1_full, z2_full, y_full, cw, ignore_index, dist, world)


def separation(y_full, cw, c, ignore_index, world, seed=0):
    """max |d global_ce - d mean_of_means| / max |d global_ce| on seeded logits ``2 * randn`` of the labels' shape: how far apart the
    right and the wrong normaliser are on this label layout"""
    g = torch.Generator().manual_seed(555 + seed)
    n, h, w = y_full.shape
    z = 2 * torch.randn(n, c, h, w, generator=g, dtype=torch.float64)
    _, right = global_ce(z, y_full, cw, ignore_index)
    _, wrong = mean_of_means(z, y_full, cw, ignore_index, world)
    return float((right - wrong).abs().max() / right.abs().max())


# ---- the label layouts of tests/test_dp_shards_gpu.py (part b), shared with the host test that vouches for them
WORLDS = ((2, 4), (4, 4), (3, 3))                   # (world, N)
CLASSES = (12, 20, 41, 48)                          # the 16 / 24 / 41 / 48-class instantiations of the loss kernels
PLAIN_HW = ((9, 13), (16, 16))                      # logits' H x W
UP_HIWI = ((5, 7), (3, 20), (4, 33))                # score maps' Hi x Wi; the labels are 8 Hi x 8 Wi


def ignore_of(c):
    return 255 if c in (12, 41) else -100


def shard_layouts():
    """(world, n, c, h, w) of every sharded-call case"""
    out = []
    for world, n in WORLDS:
        for c in CLASSES:
            out += [(world, n, c, h, w) for h, w in PLAIN_HW]
            out += [(world, n, c, 8 * hi, 8 * wi) for hi, wi in UP_HIWI]
    return out


# ---- two real ranks (tests/dp_shard_worker.py): two ver2 classifier heads on a feature-map leaf, one optimizer step
# The test compares UPDATES p_after - p_before of fp32 parameters, which carry half an ulp of p whatever computed them: to see 2e-5 of
# the largest update, updates must be large against the parameters.  With logits ~ feats * seg_w * up_w held at O(1), the weight
# gradients grow as 1 / seg_w and 1 / up_w: small head weights (1/30 of the usual initialisation), a bias near zero (the product
# initialises it to zero), features 900 times a unit normal, and a learning rate of 1e-2.  Large gradients also keep Adam's first
# update, d / (|d| + eps) -- a sign function around d = 0 -- away from its jump; tests/test_dp_shard_ref_host.py checks both on the fp64
# statement.
HEAD_CASE = dict(n=4, c=5, feat=(512, 8, 12), ignore_index=255, lr=1e-2, momentum=0.9, weight_decay=2e-5, seed=5, small=30.0)


def head_problem():
    """the worker's inputs: features [4, 512, 8, 12], labels [4, 64, 96] cut for two ranks (shard 0 about 90 % without weight), real
    class weights, and the parameters of two heads (1x1 convolution 512 -> C with bias, then the x8 transposed convolution)"""
    hc = HEAD_CASE
    n, c, small = hc["n"], hc["c"], hc["small"]
    ch, h, w = hc["feat"]
    g = torch.Generator().manual_seed(hc["seed"])
    feats = small * small * torch.randn(n, ch, h, w, generator=g)
    heads = []
    for _ in range(2):
        heads.append(dict(seg_w=torch.randn(c, ch, 1, 1, generator=g) * (2.0 / ch ** 0.5) / small, seg_b=1e-5 * torch.randn(c, generator=g),
                          up_w=torch.randn(c, 1, 16, 16, generator=g) * 0.25 / small))
    y = make_labels(n, 8 * h, 8 * w, c, hc["ignore_index"], 2, seed=hc["seed"])
    return feats, y, class_weights(c, seed=hc["seed"]), heads


def head_logits(feats, heads, dtype=torch.float64):
    """[z1, z2]: the two heads' full-resolution logits"""
    x = feats.detach().to(dtype)
    out = []
    for hd in heads:
        s = torch.nn.functional.conv2d(x, hd["seg_w"].to(dtype), hd["seg_b"].to(dtype))
        out.append(torch.nn.functional.conv_transpose2d(s, hd["up_w"].to(dtype), stride=8, padding=4, groups=s.shape[1]))
    return out


def head_step(feats, y, cw, heads, opt, world=None, dtype=torch.float64):
    """fp64 statement of the step the worker takes on the concatenated batch: both heads' weighted-mean cross-entropy (``world`` None:
    the global one; else the mean of the shards' own means -- the wrong answer), backward, one step of torch's SGD / Adam as
    ``models.model_util.get_optimizer`` configures them.  Returns {name: tensor}: ``dfeat`` and the update ``d.<k>.<name>`` of every
    head parameter.  (``dtype`` torch.float32: torch's own fp32 run of the same statement, a yardstick.)"""
    hc = HEAD_CASE
    x = feats.detach().to(dtype).clone().requires_grad_()
    params, names = [], []
    for k, hd in enumerate(heads):
        for name in ("seg_w", "seg_b", "up_w"):
            params.append(torch.nn.Parameter(hd[name].detach().to(dtype).clone()))
            names.append("d.f%d.%s" % (k + 1, name))
    before = [p.detach().clone() for p in params]
    if opt == "sgd":
        o = torch.optim.SGD(params, lr=hc["lr"], momentum=hc["momentum"], weight_decay=hc["weight_decay"])
    else:
        o = torch.optim.Adam(params, lr=hc["lr"], betas=(0.5, 0.999), weight_decay=hc["weight_decay"])
    cuts = [(0, x.shape[0])] if world is None else shards(x.shape[0], world)
    total = 0.0
    for k in range(2):
        seg_w, seg_b, up_w = params[3 * k:3 * k + 3]
        s = torch.nn.functional.conv2d(x, seg_w, seg_b)
        z = torch.nn.functional.conv_transpose2d(s, up_w, stride=8, padding=4, groups=up_w.shape[0])
        for n0, n1 in cuts:
            num, wsum = _ce_sum(z[n0:n1].double(), y[n0:n1], cw, hc["ignore_index"])
            total = total + num / wsum / len(cuts)
    total.backward()
    o.step()
    out = {"dfeat": x.grad.double()}
    for name, p, b in zip(names, params, before):
        out[name] = p.detach().double() - b.double()
    return out
