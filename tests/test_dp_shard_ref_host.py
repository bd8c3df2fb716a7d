"""CPU: the conditions on the INPUTS of the unequal-shard tests (tests/test_dp_shards_gpu.py, tests/dp_shard_worker.py), checked on
the fp64 statement alone (tests/dp_shard_ref.py): on every label layout those tests use, the gradient of the one global weighted mean
and that of the mean of the shards' own means differ by at least 100 times the bar the GPU test applies -- so a kernel that normalises
by its local sum, an ignored ``wsum_in`` or a missing 1/world cannot pass there."""
import pytest
import torch

import dp_shard_ref as ref

GRAD_BAR = 5e-6     # test_dp_shards_gpu: the bar of world 3 (and the most a world-2/4 case may be relaxed to); the L1 kind's 2e-6 is tighter
CONV_BAR = 2e-5     # test_trainers_gpu: the two-rank step, per tensor


@pytest.mark.parametrize("world,n", ref.WORLDS)
def test_global_and_local_normalisers_are_far_apart_on_every_shard_layout(world, n):
    worst = None
    for (wd, nn, c, h, w) in ref.shard_layouts():
        if wd != world:
            continue
        ig = ref.ignore_of(c)
        y, cw = ref.make_labels(nn, h, w, c, ig, world), ref.class_weights(c)
        # what the layout promises: shard 0 about 90 % without weight, every shard with some valid pixel, every kind of invalid label
        cuts = ref.shards(nn, world)
        ws = [float(ref.weight_sum(y[a:b], cw, c, ig)) for a, b in cuts]
        frac0 = 1.0 - float((ref.valid_mask(y[:cuts[0][1]], c, ig) & (y[:cuts[0][1]] != c - 1)).double().mean())
        assert 0.8 < frac0 < 0.97, (world, c, h, w, frac0)
        assert min(ws) > 0 and ws[0] < 0.35 * max(ws[1:]), ws
        for v in (ig, -1, c, c + 1, c - 1):
            assert bool((y == v).any()), (world, c, h, w, v)
        sep = ref.separation(y, cw, c, ig, world)
        if worst is None or sep < worst[0]:
            worst = (sep, c, h, w)
        assert sep >= 100 * GRAD_BAR, (world, c, h, w, sep)
    print("world %d: the two normalisers' gradients differ by at least %.2e of the largest entry (C=%d, %dx%d); 100 x bar = %.1e"
          % ((world,) + worst + (100 * GRAD_BAR,)))


def test_equal_shards_hide_the_difference():
    """the reason the same-batch tests cannot see a local normaliser: with one shard's labels on every rank the two answers coincide"""
    c, ig = 12, 255
    y = ref.make_labels(1, 9, 13, c, ig, 1).repeat(2, 1, 1)
    g = torch.Generator().manual_seed(1)
    z = (2 * torch.randn(1, c, 9, 13, generator=g, dtype=torch.float64)).repeat(2, 1, 1, 1)
    cw = ref.class_weights(c)
    (v1, g1), (v2, g2) = ref.global_ce(z, y, cw, ig), ref.mean_of_means(z, y, cw, ig, 2)
    assert abs(float(v1 - v2)) <= 1e-14 * abs(float(v1)) and float((g1 - g2).abs().max()) <= 1e-14 * float(g1.abs().max())


def test_empty_shard_layout():
    """one shard without a valid pixel: the global statement is finite and gives that shard zero gradient; the shard-local mean is 0/0"""
    c, ig, world = 20, -100, 2
    for empty in (0, 1):
        y, cw = ref.make_labels(4, 9, 13, c, ig, world, empty=empty), ref.class_weights(c)
        a, b = ref.shards(4, world)[empty]
        assert float(ref.weight_sum(y[a:b], cw, c, ig)) == 0.0 and float(ref.weight_sum(y, cw, c, ig)) > 0
        assert bool((y[a:b] == c - 1).any()) and bool((y[a:b] == ig).any())      # all ignored AND weight-0 background
        g = torch.Generator().manual_seed(2)
        z = 2 * torch.randn(4, c, 9, 13, generator=g, dtype=torch.float64)
        val, grad = ref.global_ce(z, y, cw, ig)
        assert bool(torch.isfinite(val)) and float(grad[a:b].abs().max()) == 0.0 and float(grad.abs().max()) > 0
        wrong, _ = ref.mean_of_means(z, y, cw, ig, world)
        assert not bool(torch.isfinite(wrong))


def test_objective_gradient_is_ce_plus_discrepancy():
    """the combined statement: its CE part is ``global_ce`` of each head, its discrepancy part has no normaliser to get wrong -- the
    global and the shard-local objective differ by the CE terms' difference exactly"""
    c, ig, world = 12, 255, 2
    y, cw = ref.make_labels(4, 9, 13, c, ig, world), ref.class_weights(c)
    g = torch.Generator().manual_seed(3)
    z1, z2 = (2 * torch.randn(4, c, 9, 13, generator=g, dtype=torch.float64) for _ in range(2))
    right = ref.global_objective(z1, z2, y, cw, ig)
    wrong = ref.mean_of_means_objective(z1, z2, y, cw, ig, world)
    assert abs(float(right["dist"] - wrong["dist"])) <= 1e-14 * float(right["dist"])
    for k, z in ((1, z1), (2, z2)):
        v, gr = ref.global_ce(z, y, cw, ig)
        vw, gw = ref.mean_of_means(z, y, cw, ig, world)
        assert abs(float(right["ce%d" % k] - v)) <= 1e-14 * float(v) and abs(float(wrong["ce%d" % k] - vw)) <= 1e-14 * float(vw)
        d = (right["g%d" % k] - wrong["g%d" % k]) - (gr - gw)
        assert float(d.abs().max()) <= 1e-13 * float(gr.abs().max())
    one = ref.global_objective(z1, None, y, cw, ig)
    assert one["g2"] is None and float((one["g1"] - ref.global_ce(z1, y, cw, ig)[1]).abs().max()) <= 1e-15


def test_two_rank_head_step_separates_the_normalisers():
    """the inputs of tests/dp_shard_worker.py: the feature gradient and the SGD update of every head parameter under the shard-local
    normaliser lie more than 100 x the convolution bar from the global statement's, per tensor (Adam's first update is +-lr whatever
    the gradient's scale, so for Adam the feature gradient -- the same tensor as SGD's -- carries the condition)"""
    feats, y, cw, heads = ref.head_problem()
    hc = ref.HEAD_CASE
    ws = [float(ref.weight_sum(y[a:b], cw, hc["c"], hc["ignore_index"])) for a, b in ref.shards(hc["n"], 2)]
    assert 0 < ws[0] < 0.35 * ws[1], ws
    right, wrong = ref.head_step(feats, y, cw, heads, "sgd"), ref.head_step(feats, y, cw, heads, "sgd", world=2)
    assert right.keys() == wrong.keys() and len(right) == 7
    for k in right:
        sep = float((right[k] - wrong[k]).abs().max() / right[k].abs().max())
        print("%s: local vs global normaliser %.2e of the largest entry (100 x bar = %.1e)" % (k, sep, 100 * CONV_BAR))
        assert sep >= 100 * CONV_BAR, (k, sep)
    a_right, a_wrong = ref.head_step(feats, y, cw, heads, "adam"), ref.head_step(feats, y, cw, heads, "adam", world=2)
    assert torch.equal(a_right["dfeat"], right["dfeat"]) and torch.equal(a_wrong["dfeat"], wrong["dfeat"])


def test_two_rank_head_step_is_well_conditioned():
    """what the comparison of UPDATES needs of the inputs (dp_shard_ref.HEAD_CASE), on the fp64 statement: (1) half an ulp of every
    fp32 parameter is below a twentieth of the bar times its tensor's largest update, for both optimizers; (2) Adam's first update
    d / (|d| + eps), d = g + wd p, has the slope eps / (|d| + eps)^2 in d -- 1e8 at d = 0 -- so a gradient error delta moves it by
    that times delta: with delta = 1e-6 of the tensor's largest |d| (what an fp32 convolution chain leaves; a twentieth of the bar
    the gradient itself is held to) no element may move by more than a quarter of the bar.  (3) torch's own fp32 run of the statement
    is within a quarter of the bar: the bar is attainable in fp32."""
    feats, y, cw, heads = ref.head_problem()
    hc = ref.HEAD_CASE
    params = {"d.f%d.%s" % (k + 1, name): hd[name] for k, hd in enumerate(heads) for name in ("seg_w", "seg_b", "up_w")}
    for opt in ("sgd", "adam"):
        right, fp32 = ref.head_step(feats, y, cw, heads, opt), ref.head_step(feats, y, cw, heads, opt, dtype=torch.float32)
        for k, v in right.items():
            own = float((fp32[k] - v).abs().max() / v.abs().max())
            print("%s %s: fp32 torch is %.2e of the largest entry from fp64" % (opt, k, own))
            assert own <= CONV_BAR / 4, (opt, k, own)
            if k == "dfeat":
                continue
            p = params[k].abs().max() + v.abs().max()
            half_ulp = float(torch.finfo(torch.float32).eps * p / 2)
            assert half_ulp <= CONV_BAR / 20 * float(v.abs().max()), (opt, k, half_ulp, float(v.abs().max()))
            if opt == "sgd":  # the first step of SGD with momentum: p -= lr * d
                d = (v / -hc["lr"]).abs()
                moved = float((1e-8 * 1e-6 * d.max() / (d + 1e-8) ** 2).max())
                print("adam %s: an element's update moves by at most %.2e under a gradient error of 1e-6" % (k, moved))
                assert moved <= CONV_BAR / 4, (k, moved)
