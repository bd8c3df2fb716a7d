"""CPU: ``--opt adam`` under data parallelism -- world size 2 over gloo through ``get_optimizer(..., 'adam')`` (the flat gradient
buffer all-reduced once, or in buckets during backward; 1/world folded into the update) -- and the pins of the interface.  The HIP
update kernel is replaced by a torch statement of its formula here: what is under test is the host-side logic."""
import copy
import os
import re
import socket

import pytest
import torch
import torch.multiprocessing as mp

LR, BETAS, EPS, WD = 1e-3, (0.5, 0.999), 1e-8, 2e-5


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _ref_adam_(p, g, m, v, lr, betas, eps, weight_decay, step, grad_scale=1.0, params=None):
    """include/mcdseg.h, mcdseg_adam_flat: the bias corrections in double precision on the host, the rest in the buffers' precision"""
    b1, b2 = betas
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    d = g * grad_scale + weight_decay * p
    m.add_((1.0 - b1) * (d - m))
    v.mul_(b2).add_((1.0 - b2) * d * d)
    p.sub_((lr / bc1) * m / (v.sqrt() * bc2 ** -0.5 + eps))


def _worker(rank, world, port, tmp, overlap=False):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      MCDSEG_PRETRAINED="0")
    if overlap:  # bucketed all-reduce from post-accumulate hooks: tiny buckets so that the parameters fall into several
        os.environ.update(MCDSEG_DP_OVERLAP="1", MCDSEG_DP_BUCKET_MB="0.0005")
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "multichannel-semseg-with-uda_amd"))
    from mcdseg import dist as mdist
    from mcdseg import ops
    from models.model_util import get_optimizer
    r, w, _ = mdist.init_from_env(backend="gloo")
    assert (r, w) == (rank, world) and mdist.is_distributed() and mdist.world_size() == world
    gen = torch.Generator().manual_seed(0)
    shapes = [(8, 3, 3, 3), (8,), (5, 7), (3,)]
    params = [torch.nn.Parameter(torch.randn(s, generator=gen)) for s in shapes]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in params]
    ref_opt = torch.optim.Adam(ref, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, foreach=False)
    opt = get_optimizer(params, "adam", LR, 0.9, WD)      # (the product's way to an Adam: --opt adam)
    ops.adam_flat_ = _ref_adam_
    type(opt)._require_gpu = False
    for step in range(3):
        grads_all = [[torch.randn(s, generator=torch.Generator().manual_seed(100 * step + 10 * k + i)) for i, s in enumerate(shapes)]
                     for k in range(world)]
        skipped = {1} if step == 1 else set()            # on every rank: a parameter without a gradient falls a step behind
        opt.zero_grad(), ref_opt.zero_grad()
        if overlap and step > 0:  # through autograd, so that the hooks see the gradients arrive (step 0: plain assignment -> fallback path)
            loss = sum((p * g).sum() for i, (p, g) in enumerate(zip(params, grads_all[rank])) if i not in skipped)
            loss.backward()
            fl = opt._flat   # (a bucket with a skipped parameter never completes; step() then flushes past it and reduces the run itself)
            assert len(fl["buckets"]) >= 2 and (skipped or all(b["work"] is not None for b in fl["buckets"]))
        else:
            for i, (p, g) in enumerate(zip(params, grads_all[rank])):
                if i not in skipped:
                    p.grad = g.clone()
        opt.step()
        for i in range(len(ref)):
            if i not in skipped:
                ref[i].grad = sum(grads_all[k][i] for k in range(world)) / world
        ref_opt.step()
    # the single-process Adam on the rank-averaged gradients
    for p, q in zip(params, ref):
        assert torch.allclose(p.detach(), q.detach(), rtol=1e-5, atol=1e-6), float((p.detach() - q.detach()).abs().max())
    assert [float(opt.state[p]["step"]) for p in params] == [3, 2, 3, 3]
    # every rank holds the same replica
    flat = opt.flat_buffers()[0].clone()
    assert all(flat.data_ptr() != p.data_ptr() for p in params) and flat.numel() >= sum(p.numel() for p in params)
    gathered = [torch.zeros_like(flat) for _ in range(world)]
    torch.distributed.all_gather(gathered, flat)
    assert all(torch.equal(gathered[0], t) for t in gathered)
    mdist.barrier()
    torch.distributed.destroy_process_group()
    open(os.path.join(tmp, "ok%d" % rank), "w").write("ok")


def test_flat_adam_data_parallel_gloo(tmp_path):
    """two ranks with different gradients: the parameters are those of a single-process torch.optim.Adam on the rank-averaged
    gradients, identical on both ranks.  (With an optimizer that does not sum over the ranks each replica follows its own shard.)"""
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    assert all((tmp_path / ("ok%d" % r)).exists() for r in range(world))


def test_flat_adam_bucketed_overlap_gloo(tmp_path):
    """the same with MCDSEG_DP_OVERLAP=1 and tiny buckets, gradients arriving through autograd's post-accumulate hooks"""
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), True), nprocs=world, join=True)
    assert all((tmp_path / ("ok%d" % r)).exists() for r in range(world))


def _params():
    gen = torch.Generator().manual_seed(0)
    return [torch.nn.Parameter(torch.randn(s, generator=gen)) for s in [(4, 3), (5,)]]


def test_get_optimizer_adam_is_the_flat_adam():
    from models.model_util import get_optimizer
    opt = get_optimizer(_params(), "adam", 1e-3, 0.9, 2e-5)
    assert type(opt).__name__ == "FlatAdam" and type(opt).__module__ == "mcdseg.optim"
    group = opt.param_groups[0]
    assert tuple(group["betas"]) == (0.5, 0.999) and group["lr"] == 1e-3 and group["weight_decay"] == 2e-5 and group["eps"] == 1e-8
    theirs = torch.optim.Adam(_params(), lr=1e-3, betas=(0.5, 0.999), weight_decay=2e-5).param_groups[0]
    assert set(theirs.keys()) <= set(group.keys()), set(theirs.keys()) - set(group.keys())
    assert all(group[k] == theirs[k] for k in theirs if k != "params"), [(k, group[k], theirs[k]) for k in theirs if k != "params"]
    # "adadelta" stays torch's; "sgd" stays the flat SGD
    assert type(get_optimizer(_params(), "adadelta", 1e-3, 0.9, 2e-5)) is torch.optim.Adadelta
    assert type(get_optimizer(_params(), "sgd", 1e-3, 0.9, 2e-5)).__name__ == "FlatSGD"


def test_adam_kernel_is_declared_and_registered():
    from mcdseg import _lib
    header = open(os.path.join(_lib.INCLUDE, "mcdseg.h")).read()
    m = re.search(r"\bint\s+mcdseg_adam_flat\s*\(([^)]*)\)\s*;", header)
    assert m is not None
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 13 and args[0] == "float* p" and args[1] == "const float* g" and args[-1] == "void* stream"
    res, argtypes = _lib._SIGNATURES["mcdseg_adam_flat"]
    assert res is _lib.c_int and len(argtypes) == 13
    assert argtypes[:4] == [_lib.c_void_p] * 4 and argtypes[4] is _lib.c_i64 and argtypes[5:12] == [_lib.c_float] * 7 and argtypes[12] is _lib.c_void_p
    assert "adam.hip" in _lib.NO_PACKED_F32 and os.path.exists(os.path.join(_lib.CSRC, "adam.hip"))


def test_flat_adam_refuses_what_it_does_not_implement():
    from mcdseg.optim import FlatAdam
    with pytest.raises(NotImplementedError):
        FlatAdam(_params(), amsgrad=True)
    with pytest.raises(NotImplementedError):
        FlatAdam(_params(), maximize=True)
    with pytest.raises(ValueError):
        FlatAdam(_params(), betas=(0.5, 1.0))
    assert FlatAdam(_params(), amsgrad=False, maximize=False).defaults["amsgrad"] is False
    with pytest.raises(RuntimeError, match="must be on the GPU"):   # no CPU fallback: a missing kernel is an error
        opt = FlatAdam(_params())
        opt.param_groups[0]["params"][0].grad = torch.zeros(4, 3)
        opt.step()


def test_flat_adam_host_logic(monkeypatch):
    """the state in torch's layout, a state dict loaded before and after the first step, and a skipped parameter -- with the kernel
    replaced by the formula"""
    from mcdseg import ops
    from mcdseg.optim import FlatAdam
    monkeypatch.setattr(FlatAdam, "_require_gpu", False)
    monkeypatch.setattr(ops, "adam_flat_", _ref_adam_)
    ours, theirs = _params(), _params()
    a = FlatAdam(ours, lr=LR, betas=BETAS, weight_decay=WD)
    b = torch.optim.Adam(theirs, lr=LR, betas=BETAS, weight_decay=WD, foreach=False)
    gen = torch.Generator().manual_seed(1)
    for step in range(3):
        for i, (p, q) in enumerate(zip(ours, theirs)):
            g = torch.randn(p.shape, generator=gen)
            p.grad, q.grad = (None, None) if (step, i) == (1, 1) else (g.clone(), g.clone())
        a.step(), b.step()
    for p, q in zip(ours, theirs):
        assert torch.allclose(p.detach(), q.detach(), rtol=1e-5, atol=1e-6)
        st, tt = a.state[p], b.state[q]
        assert set(st.keys()) == {"step", "exp_avg", "exp_avg_sq"}
        assert st["step"].dtype == torch.float32 and st["step"].dim() == 0 and st["step"].device.type == "cpu"
        assert float(st["step"]) == float(tt["step"])
        assert torch.allclose(st["exp_avg"], tt["exp_avg"], rtol=1e-5, atol=1e-7)
        assert torch.allclose(st["exp_avg_sq"], tt["exp_avg_sq"], rtol=1e-5, atol=1e-9)
    fp, fg, fm, fv = a.flat_buffers()
    assert all(a.state[p]["exp_avg"].data_ptr() - fm.data_ptr() == p.data_ptr() - fp.data_ptr() for p in ours)
    # torch's state dict into a FlatAdam that has not stepped, ours into torch's, ours into one of ours that has stepped
    sd, tsd = a.state_dict(), b.state_dict()
    assert all(st["exp_avg"].data_ptr() != a.state[p]["exp_avg"].data_ptr() for st, p in zip(sd["state"].values(), ours))
    fresh_p = [torch.nn.Parameter(p.detach().clone()) for p in theirs]
    fresh = FlatAdam(fresh_p)
    fresh.load_state_dict(copy.deepcopy(tsd))   # (torch's state dict holds the optimizer's live tensors, and a load keeps what needs no cast)
    torch.optim.Adam(_params()).load_state_dict(sd)
    a.load_state_dict(tsd)
    for p, q, f in zip(ours, theirs, fresh_p):
        g = torch.randn(p.shape, generator=gen)
        p.grad, q.grad, f.grad = g.clone(), g.clone(), g.clone()
    a.step(), b.step(), fresh.step()
    for p, q, f in zip(ours, theirs, fresh_p):
        assert torch.allclose(p.detach(), q.detach(), rtol=1e-5, atol=1e-6) and torch.allclose(f.detach(), q.detach(), rtol=1e-5, atol=1e-6)
        assert float(a.state[p]["step"]) == float(b.state[q]["step"]) == float(fresh.state[f]["step"])
        assert a.state[p]["exp_avg"].data_ptr() - a.flat_buffers()[2].data_ptr() == p.data_ptr() - a.flat_buffers()[0].data_ptr()


def test_flat_sgd_keeps_its_three_buffers(monkeypatch):
    from mcdseg.optim import FlatSGD
    monkeypatch.setattr(FlatSGD, "_require_gpu", False)
    opt = FlatSGD(_params(), lr=0.1, momentum=0.9)
    bufs = opt.flat_buffers()
    assert len(bufs) == 3 and all(torch.is_tensor(t) and t.shape == bufs[0].shape for t in bufs)
    assert bufs[0] is opt._flat["p"] and bufs[1] is opt._flat["g"] and bufs[2] is opt._flat["v"]
