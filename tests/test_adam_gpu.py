"""GPU: ``--opt adam`` -- the flat Adam kernel (csrc/adam.hip) and ``mcdseg.optim.FlatAdam`` against ``torch.optim.Adam`` as the
reference configures it (betas (0.5, 0.999), L2 weight decay), its state dict in torch's layout, the packed weight images behind
a step, one MCD step end to end, and one rank through the real collective."""
import copy
import json
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(16, 6, 7, 7), (16,), (33, 5, 3, 3), (41, 1, 16, 16), (7,), (1,)]   # sizes not divisible by 4, one below a float4
GRAD_SCALE = [1.0, 1e-4, 1e3, 1.0, 0.0, 1.0]    # 0: the tensor moves by weight decay alone, sqrt(v) near eps
HYPER = dict(lr=1e-3, betas=(0.5, 0.999), eps=1e-8, weight_decay=2e-5)
SKIP = (2, 2)                                   # (step, tensor): grad None there, so that tensor's step counter falls behind
FACTOR = 2.0                                    # x fp32 torch's own distance from the fp64 truth (module docstring of the test below)


@pytest.fixture(autouse=True)
def _no_pretrained(monkeypatch):
    monkeypatch.setenv("MCDSEG_PRETRAINED", "0")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class _Trio:
    """the same seeded parameters under three optimizers: torch.optim.Adam in fp64 on the CPU (the truth), torch.optim.Adam in fp32 on
    the CPU, one tensor at a time (the yardstick), and FlatAdam on the GPU"""

    def __init__(self, dev, seed=0):
        from mcdseg.optim import FlatAdam
        self.dev, self.gen = dev, torch.Generator().manual_seed(seed)
        start = [torch.randn(s, generator=self.gen) for s in SHAPES]
        self.p64 = [torch.nn.Parameter(t.double()) for t in start]
        self.p32 = [torch.nn.Parameter(t.clone()) for t in start]
        self.hip = [torch.nn.Parameter(t.to(dev)) for t in start]
        self.truth = torch.optim.Adam(self.p64, **HYPER)
        self.yard = torch.optim.Adam(self.p32, foreach=False, **HYPER)
        self.ours = FlatAdam(self.hip, **HYPER)
        self.steps = 0
        self.ratios = {}

    def step(self, skip=None):
        for i, s in enumerate(SHAPES):
            g = torch.randn(s, generator=self.gen) * GRAD_SCALE[i]
            none = skip is not None and skip == (self.steps, i)
            self.p64[i].grad = None if none else g.double()
            self.p32[i].grad = None if none else g.clone()
            self.hip[i].grad = None if none else g.to(self.dev)
        self.truth.step(), self.yard.step(), self.ours.step()
        self.steps += 1

    def check(self):
        """per tensor: max|hip - truth| <= FACTOR * max|fp32 - truth| for the parameters and exp_avg, and the same for exp_avg_sq
        (both sides relative to the truth's maximum, which cancels)"""
        bad = []
        for i in range(len(SHAPES)):
            st64, st32, sth = self.truth.state[self.p64[i]], self.yard.state[self.p32[i]], self.ours.state[self.hip[i]]
            for what, t64, t32, th in (("param", self.p64[i], self.p32[i], self.hip[i]),
                                       ("exp_avg", st64["exp_avg"], st32["exp_avg"], sth["exp_avg"]),
                                       ("exp_avg_sq", st64["exp_avg_sq"], st32["exp_avg_sq"], sth["exp_avg_sq"])):
                t64 = t64.detach()
                yard = float((t32.detach().double() - t64).abs().max())
                hip = float((th.detach().double().cpu() - t64).abs().max())
                scale = float(t64.abs().max()) if what == "exp_avg_sq" else 1.0
                ratio = hip / yard if yard > 0 else (0.0 if hip == 0 else float("inf"))
                self.ratios[what] = max(self.ratios.get(what, 0.0), ratio)
                print("step %d tensor %d %-10s hip %.3e  fp32 %.3e  ratio %.3f" % (self.steps, i, what, hip / scale, yard / scale, ratio))
                if not hip / scale <= FACTOR * yard / scale:
                    bad.append((self.steps, i, what, hip, yard))
        return bad


def test_adam_kernel_against_fp64_truth():
    """Six steps of FlatAdam on the GPU against torch.optim.Adam in fp64, in units of fp32 torch's own distance from it: per tensor and
    at every step, max|hip - truth| <= 2 x max|fp32 - truth| for the parameters, exp_avg and exp_avg_sq.  Margin 2: both sides are
    dominated by the one rounding of p per step; the kernel's fused multiply-adds and its order of the square root and the divide
    may land on the other side of a tie, nothing more.  One tensor has no gradient at one step (skipped as torch skips it: no
    decay, no moment update, no step count), one has a zero gradient (weight decay alone, sqrt(v) near eps)."""
    dev = _dev()
    trio = _Trio(dev)
    bad = []
    for step in range(6):
        trio.step(skip=SKIP)
        bad += trio.check()
    print("largest ratios:", trio.ratios)
    assert not bad, bad
    for a, b in zip(trio.p32, trio.hip):
        sa, sb = trio.yard.state[a]["step"], trio.ours.state[b]["step"]
        assert sb.device.type == "cpu" and sb.dtype == torch.float32 and sb.dim() == 0
        assert float(sa) == float(sb)
    assert float(trio.ours.state[trio.hip[2]]["step"]) == 5 and float(trio.ours.state[trio.hip[0]]["step"]) == 6
    fp, fg, fm, fv = trio.ours.flat_buffers()
    assert all(fp.data_ptr() <= p.data_ptr() < fp.data_ptr() + 4 * fp.numel() for p in trio.hip)
    for p in trio.hip:
        off = p.data_ptr() - fp.data_ptr()
        assert trio.ours.state[p]["exp_avg"].data_ptr() == fm.data_ptr() + off
        assert trio.ours.state[p]["exp_avg_sq"].data_ptr() == fv.data_ptr() + off


def test_adam_state_dict_is_torchs_both_directions():
    """after one step ``state_dict()`` is torch's layout: it loads into a fresh torch.optim.Adam, torch's loads into a fresh FlatAdam
    that has not stepped yet, and both pairs go on within the bound of the kernel test; a returned tensor is a copy"""
    dev = _dev()
    from mcdseg.optim import FlatAdam
    trio = _Trio(dev, seed=1)
    trio.step()
    sd = trio.ours.state_dict()
    assert sorted(sd.keys()) == ["param_groups", "state"] and sorted(sd["state"].keys()) == list(range(len(SHAPES)))
    assert all(set(st.keys()) == {"step", "exp_avg", "exp_avg_sq"} for st in sd["state"].values())
    # ours -> torch: a fresh fp32 torch.optim.Adam over CPU copies of our parameters becomes the yardstick
    trio.p32 = [torch.nn.Parameter(p.detach().cpu().clone()) for p in trio.hip]
    trio.yard = torch.optim.Adam(trio.p32, foreach=False, **HYPER)
    trio.yard.load_state_dict(sd)
    assert all(trio.yard.state[p]["exp_avg"].device.type == "cpu" and float(trio.yard.state[p]["step"]) == 1 for p in trio.p32)
    # torch -> ours: a fresh FlatAdam that has not stepped (nothing flat yet) takes torch's state dict
    tsd = trio.yard.state_dict()
    trio.hip = [torch.nn.Parameter(p.detach().clone()) for p in trio.hip]
    trio.ours = FlatAdam(trio.hip, lr=0.5, betas=(0.9, 0.9))       # (the loaded groups replace these)
    trio.ours.load_state_dict(tsd)
    assert trio.ours.param_groups[0]["lr"] == HYPER["lr"] and tuple(trio.ours.param_groups[0]["betas"]) == HYPER["betas"]
    # the truth restarts from the same fp32 state
    trio.p64 = [torch.nn.Parameter(p.detach().double()) for p in trio.p32]
    trio.truth = torch.optim.Adam(trio.p64, **HYPER)
    trio.truth.load_state_dict(copy.deepcopy(tsd))
    bad = []
    for _ in range(2):
        trio.step()
        bad += trio.check()
    assert not bad, bad
    assert all(float(trio.ours.state[p]["step"]) == 3 for p in trio.hip)
    # after a step too (flat storage in place), and a returned state tensor does not alias the flat buffers
    sd = trio.ours.state_dict()
    before = trio.ours.flat_buffers()[2].clone()
    for st in sd["state"].values():
        st["exp_avg"].add_(1.0), st["exp_avg_sq"].add_(1.0)
    assert torch.equal(trio.ours.flat_buffers()[2], before)
    trio.ours.load_state_dict(sd)
    assert torch.equal(trio.ours.state[trio.hip[0]]["exp_avg"], sd["state"][0]["exp_avg"])
    assert trio.ours.state[trio.hip[0]]["exp_avg"].data_ptr() == trio.ours.flat_buffers()[2].data_ptr()


def test_packed_weights_follow_an_adam_step():
    """a fused conv+BN group before and after ``FlatAdam.step()``: the packed GEMM images are rebuilt from the updated weight -- the
    output is bitwise that of a fresh module holding a copy of the updated parameters, and the convolution with the updated weight"""
    dev = _dev()
    from mcdseg import ops
    from mcdseg.optim import FlatAdam
    from models.drn import BatchNorm2d, Conv2d
    g = torch.Generator().manual_seed(5)
    conv, bn = Conv2d(32, 64, 3, padding=1, bias=False).to(dev), BatchNorm2d(64).to(dev)
    with torch.no_grad():
        conv.weight.copy_((torch.randn(conv.weight.shape, generator=g) * 0.05).to(dev))
    x = torch.randn(2, 32, 12, 20, generator=g).to(dev)
    gy = torch.randn(2, 64, 12, 20, generator=g).to(dev)
    opt = FlatAdam(list(conv.parameters()) + list(bn.parameters()), lr=1e-2, betas=(0.5, 0.999), weight_decay=2e-5)
    w0 = conv.weight.detach().clone()
    y0 = ops.conv_bn_act(x, conv, bn, relu=True)
    y0.backward(gy)
    opt.step()
    assert float((conv.weight.detach() - w0).abs().max()) > 5e-3           # (the first Adam step moves every element by about lr)
    y1 = ops.conv_bn_act(x, conv, bn, relu=True).detach()
    conv2, bn2 = Conv2d(32, 64, 3, padding=1, bias=False).to(dev), BatchNorm2d(64).to(dev)
    with torch.no_grad():
        conv2.weight.copy_(conv.weight), bn2.weight.copy_(bn.weight), bn2.bias.copy_(bn.bias)
    y2 = ops.conv_bn_act(x, conv2, bn2, relu=True).detach()
    assert torch.equal(y1, y2)
    assert not torch.equal(y1, y0.detach())

    def truth(w):
        z = F.conv2d(x.double().cpu(), w.double().cpu(), padding=1)
        return F.relu(F.batch_norm(z, None, None, bn.weight.detach().double().cpu(), bn.bias.detach().double().cpu(), training=True, eps=bn.eps))

    new, stale = truth(conv.weight.detach()), truth(w0)
    err = float((y1.double().cpu() - new).abs().max())
    assert err <= 3e-5 * float(new.abs().max()), err                        # (the tolerance of the group's own forward test)
    assert float((y1.double().cpu() - stale).abs().max()) > 100 * err       # ... and not the stale image's output


def test_mcd_step_with_adam_end_to_end():
    """``get_optimizer(..., 'adam')`` through two ``MCDSolver.step``s of a small DRN against the same steps with torch.optim.Adam on a
    deep copy.  Parameters within 2 lr per optimizer step taken: Adam's first steps are +-lr * sign-like, and wherever a gradient
    element is near zero its sign belongs to the convolutions' rounding, which is not under test here."""
    dev = _dev()
    from recipe import fill_state_, make_batch
    from loss import CrossEntropyLoss2d, get_prob_distance_criterion
    from mcdseg.optim import FlatAdam
    from models.model_util import get_models, get_optimizer
    from solvers.solver import MCDSolver
    nc, lr, iters = 5, 1e-3, 2
    ours = get_models("drn_d_22", input_ch=6, n_class=nc)
    for m, seed in zip(ours, (11, 12, 13)):
        fill_state_(m, seed)
        m.to(dev).train()
    theirs = copy.deepcopy(ours)
    src, lbl, tgt = (t.to(dev) for t in make_batch(7, 2, 6, 32, 48, nc))
    og = get_optimizer(ours[0].parameters(), "adam", lr, 0.9, 2e-5)
    of = get_optimizer(list(ours[1].parameters()) + list(ours[2].parameters()), "adam", lr, 0.9, 2e-5)
    assert type(og) is FlatAdam and type(of) is FlatAdam
    tg = torch.optim.Adam(theirs[0].parameters(), lr=lr, betas=(0.5, 0.999), weight_decay=2e-5)
    tf = torch.optim.Adam(list(theirs[1].parameters()) + list(theirs[2].parameters()), lr=lr, betas=(0.5, 0.999), weight_decay=2e-5)
    cw = torch.ones(nc)
    cw[nc - 1] = 0
    a = MCDSolver(ours[0], ours[1], ours[2], og, of, CrossEntropyLoss2d(cw.to(dev)), get_prob_distance_criterion("diff"), num_k=4)
    b = MCDSolver(theirs[0], theirs[1], theirs[2], tg, tf, CrossEntropyLoss2d(cw.to(dev)), get_prob_distance_criterion("diff"), num_k=4)
    for it in range(iters):
        ca, da = (float(v) for v in a.step(src, lbl, tgt))
        cb, db = (float(v) for v in b.step(src, lbl, tgt))
        print("iter %d: c_loss %.8f / %.8f   d_loss %.8f / %.8f" % (it, ca, cb, da, db))
        assert all(v == v and abs(v) != float("inf") for v in (ca, da))
        assert abs(ca - cb) <= 1e-4 * abs(cb), (it, ca, cb)
        assert abs(da - db) <= 1e-4 * abs(db), (it, da, db)
    # per iteration the generator's optimizer steps 1 + num_k times, the classifiers' twice
    for mo, mt, opt, topt, taken in ((ours[0], theirs[0], og, tg, 5 * iters), (ours[1], theirs[1], of, tf, 2 * iters),
                                     (ours[2], theirs[2], of, tf, 2 * iters)):
        counts = set()
        for (k, p), q in zip(mo.named_parameters(), mt.parameters()):
            count = float(opt.state.get(p, {}).get("step", 0))
            assert count == float(topt.state.get(q, {}).get("step", 0)), k
            counts.add(count)
            assert float((p.detach() - q.detach()).abs().max()) <= 2 * lr * taken, k
        assert max(counts) == taken


def test_adam_one_rank_through_the_real_collective(tmp_path):
    """a fresh child process that is the only rank of an RCCL ("nccl") process group with MCDSEG_DIST_FORCE=1: FlatAdam steps with
    the flat gradient buffer all-reduced in one piece (MCDSEG_DP_OVERLAP=0) and in buckets from the backward hooks (=1) are bitwise
    the non-distributed steps (tests/adam_rank_worker.py)"""
    _dev()
    here = os.path.dirname(os.path.abspath(__file__))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "adam_rank.json")
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), MCDSEG_DIST_BACKEND="nccl",
               MCDSEG_DIST_FORCE="1", MCDSEG_DP_BUCKET_MB="0.004", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4")
    r = subprocess.run([sys.executable, os.path.join(here, "adam_rank_worker.py"), out], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.load(open(out))
    assert res["backend"] == "nccl" and res["forced"] is True
    assert res["collectives"]["whole"] >= 2 and res["collectives"]["bucketed"] >= 2 and res["buckets"] >= 2
    assert res["whole"] == res["plain"], "one all-reduce of the flat gradients changed the step"
    assert res["bucketed"] == res["plain"], "the bucketed all-reduce changed the step"
