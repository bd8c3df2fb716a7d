"""CPU, world_size 2 over gloo: the data-parallel path of the flat optimizer (one all-reduce of the flat gradient
buffer, 1/world folded into the update) and the global CE normaliser.  The HIP update kernel is replaced by a
reference formula here -- what is under test is the host-side distributed logic."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _ref_sgd_(p, g, v, lr, mu, wd, gs=1.0):
    v.mul_(mu).add_(g * gs + wd * p)
    p.sub_(lr * v)


def _worker(rank, world, port, tmp, overlap=False):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    if overlap:  # bucketed all-reduce from post-accumulate hooks: tiny buckets so that the three parameters fall into several
        os.environ.update(MCDSEG_DP_OVERLAP="1", MCDSEG_DP_BUCKET_MB="0.0005")
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "multichannel-semseg-with-uda_amd"))
    from mcdseg import dist as mdist
    from mcdseg import ops
    from mcdseg.optim import FlatSGD
    r, w, _ = mdist.init_from_env(backend="gloo")
    assert (r, w) == (rank, world) and mdist.is_distributed() and mdist.world_size() == world
    ops.sgd_momentum_flat_ = lambda p, g, v, lr, mu, wd, gs=1.0, params=None: _ref_sgd_(p, g, v, lr, mu, wd, gs)
    FlatSGD._require_gpu = False
    gen = torch.Generator().manual_seed(0)
    shapes = [(8, 3, 3, 3), (8,), (5, 7)]
    params = [torch.nn.Parameter(torch.randn(s, generator=gen)) for s in shapes]
    ref = [p.detach().clone() for p in params]
    refv = [torch.zeros_like(p) for p in ref]
    opt = FlatSGD(params, lr=0.1, momentum=0.9, weight_decay=0.01)
    for step in range(3):
        grads_all = [[torch.randn(s, generator=torch.Generator().manual_seed(100 * step + 10 * k + i)) for i, s in enumerate(shapes)]
                     for k in range(world)]
        opt.zero_grad()
        if overlap == "twice" and step > 0:
            # TWO backward passes before one step() (MCDSolver's step B) -- the second pass finds the buckets' collectives
            # started by the first; the update must use the ACCUMULATED gradient averaged over the ranks.  And before that a pass whose
            # gradients are dropped by zero_grad() without a step (the reference's literal loop): its collectives must not leak.
            junk = sum((p * 7.0).sum() for p in params)
            junk.backward()
            assert all(b["work"] is not None for b in opt._flat["buckets"])
            opt.zero_grad()
            assert all(b["work"] is None and b["arrived"] == 0 for b in opt._flat["buckets"])
            extra = [[torch.randn(s, generator=torch.Generator().manual_seed(5000 + 100 * step + 10 * k + i)) for i, s in enumerate(shapes)]
                     for k in range(world)]
            sum((p * g).sum() for p, g in zip(params, grads_all[rank])).backward()
            sum((p * g).sum() for p, g in zip(params, extra[rank])).backward()
            assert all(b["dirty"] and b["work"] is None for b in opt._flat["buckets"])
            grads_all = [[a + b for a, b in zip(grads_all[k], extra[k])] for k in range(world)]
        elif overlap == "skew" and step > 0:
            # WHEN a gradient arrives depends on rank-local state (a weight gradient deferred to the side stream arrives
            # early, one kept back by the memory guard at the end of the pass): here rank 0 sees the gradients in backward order and
            # rank 1 in forward order, one of them as an "early" side-stream delivery.  The collectives must still be issued in the
            # same (bucket) order on both ranks -- out of order, gloo pairs slices of different sizes and fails or hangs.
            fl = opt._flat
            order = list(reversed(range(len(params)))) if rank == 0 else list(range(len(params)))
            launched = []
            real_launch = opt._launch_reduce
            opt._launch_reduce = lambda b: (launched.append(b["index"]), real_launch(b))[1]
            for n_seen, i in enumerate(order):
                p = params[i]
                if rank == 1 and i == 0:
                    opt._early_grad(p, grads_all[rank][i])      # the side stream's delivery ...
                    p.grad = grads_all[rank][i].clone()
                    opt._grad_arrived(p)                         # ... reaches p.grad through its _LateGrad node later
                else:
                    p.grad = grads_all[rank][i].clone()
                    opt._grad_arrived(p)
            opt._launch_reduce = real_launch
            assert launched == sorted(launched) == list(range(len(fl["buckets"]))), launched
            assert all(b["work"] is not None and not b["dirty"] for b in fl["buckets"])
        elif overlap and step > 0:  # through autograd, so that the hooks see the gradients arrive (step 0: plain assignment -> fallback path)
            loss = sum((p * g).sum() for p, g in zip(params, grads_all[rank]))
            loss.backward()
            fl = opt._flat
            assert len(fl["buckets"]) >= 2 and all(b["work"] is not None for b in fl["buckets"])
        else:
            for p, g in zip(params, grads_all[rank]):
                p.grad = g.clone()
        opt.step()
        for i in range(len(ref)):
            gavg = sum(grads_all[k][i] for k in range(world)) / world
            _ref_sgd_(ref[i], gavg, refv[i], 0.1, 0.9, 0.01)
    for p, q in zip(params, ref):
        assert torch.allclose(p.detach(), q, rtol=1e-5, atol=1e-6), float((p.detach() - q).abs().max())
    # every rank holds the same replica
    flat = opt.flat_buffers()[0].clone()
    gathered = [torch.zeros_like(flat) for _ in range(world)]
    torch.distributed.all_gather(gathered, flat)
    assert all(torch.equal(gathered[0], t) for t in gathered)
    # global CE normaliser: sum over ranks / world
    local = torch.tensor([10.0 + rank])
    mdist.all_reduce_sum_(local)
    assert float(local) == sum(10.0 + k for k in range(world))
    mdist.barrier()
    torch.distributed.destroy_process_group()
    open(os.path.join(tmp, "ok%d" % rank), "w").write("ok")


def test_flat_sgd_data_parallel_gloo(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    assert all((tmp_path / ("ok%d" % r)).exists() for r in range(world))


def test_flat_sgd_bucketed_overlap_gloo(tmp_path):
    """MCDSEG_DP_OVERLAP=1: gradients copied into the flat buffer by post-accumulate hooks, buckets all-reduced asynchronously as they
    complete during backward -- same parameters as the reference update of the averaged gradients (and the un-hooked first step
    takes the one-collective path)"""
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), True), nprocs=world, join=True)
    assert all((tmp_path / ("ok%d" % r)).exists() for r in range(world))


def test_flat_sgd_bucketed_overlap_two_backward_passes_gloo(tmp_path):
    """MCDSEG_DP_OVERLAP=1 with two backward passes before one step() and with a zero_grad() that drops a pass: the
    accumulated gradient is averaged over the ranks, nothing of the dropped pass survives"""
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), "twice"), nprocs=world, join=True)
    assert all((tmp_path / ("ok%d" % r)).exists() for r in range(world))


def test_flat_sgd_bucketed_overlap_is_rank_invariant_in_launch_order_gloo(tmp_path):
    """MCDSEG_DP_OVERLAP=1 with the two ranks receiving their gradients in opposite orders: buckets are exchanged in bucket order on
    both, and the update is the reference update of the averaged gradients"""
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), "skew"), nprocs=world, join=True)
    assert all((tmp_path / ("ok%d" % r)).exists() for r in range(world))


def test_flat_sgd_early_copy_does_not_stand_for_a_summed_gradient():
    """a weight with TWO contributions in one backward pass, one delivered early through the sink and one not --
    ``p.grad`` then holds the sum while the flat slice holds the early part only; the bucket must be left to step()'s copy path.
    Single process: the bucket bookkeeping only (no process group needed for it)."""
    from mcdseg import optim
    from mcdseg.optim import FlatSGD
    old = (optim.DP_OVERLAP, optim.mdist.is_distributed, FlatSGD._require_gpu, optim.mdist.all_reduce_sum_async)
    optim.DP_OVERLAP, FlatSGD._require_gpu = True, False
    optim.mdist.is_distributed = lambda: True

    class _Work:
        def wait(self):
            pass

    optim.mdist.all_reduce_sum_async = lambda flat: _Work()
    try:
        for order in ("early_first", "early_second"):
            p = torch.nn.Parameter(torch.zeros(4))
            opt = FlatSGD([p], lr=0.1)
            opt._ensure_flat()
            b = opt._flat["buckets"][0]
            part = torch.ones(4)
            if order == "early_first":
                opt._early_grad(p, part)          # deferred contribution: copied, bucket ready and started
                assert b["ready"] and b["launched"] and not b["dirty"]
                opt._early_grad(p, None)          # a second contribution that does not pass through the sink
            else:
                opt._early_grad(p, None)
                opt._early_grad(p, part)          # an early copy behind a plain contribution: cannot stand for p.grad either
            assert b["dirty"] and b["work"] is None
            p.grad = 2 * part
            opt._grad_arrived(p)
            assert b["dirty"]
            assert not opt._finish_overlap([p])   # step() copies p.grad and reduces the run itself
            opt._reset_overlap()
            assert not (b["dirty"] or b["ready"] or b["launched"] or b["unsunk"] or b["early"]) and opt._flat["next"] == 0
    finally:
        optim.DP_OVERLAP, optim.mdist.is_distributed, FlatSGD._require_gpu, optim.mdist.all_reduce_sum_async = old


@pytest.mark.parametrize("opt_name", ["FlatSGD", "FlatAdam"])
def test_twice_used_weight_gives_both_ranks_one_sequence_of_collectives(opt_name, monkeypatch):
    """A weight used twice in one backward graph (MultiTaskMCDSolver's step A) under MCDSEG_DP_OVERLAP=1, on two ranks in different
    rank-local states: "rank A" has room to defer, both contributions come through ``_early_grad(p, dw)``; "rank B" is above the
    memory guard, both are reported as ``_early_grad(p, None)`` and the summed ``p.grad`` arrives through the hook.  A once-used weight
    sits in a second bucket.  What each rank then asks of the process group -- the bucket exchanges during the pass and, in step(),
    the fall-back all-reduce of the run -- must be ONE sequence (a collective only one rank issues pairs with the other's next one, or
    with nothing: wrong sums or a hang), and both updates must use the full summed gradient.  Single process, two optimizer instances,
    the two entry points of ``mcdseg.dist`` replaced by recorders that sum "two ranks holding the same gradients": nothing can hang."""
    from mcdseg import optim
    cls = getattr(optim, opt_name)
    monkeypatch.setattr(optim, "DP_OVERLAP", True)
    monkeypatch.setattr(optim, "DP_BUCKET_MB", 0.0)      # every parameter a bucket of its own
    monkeypatch.setattr(cls, "_require_gpu", False)
    monkeypatch.setattr(optim.mdist, "is_distributed", lambda: True)
    monkeypatch.setattr(optim.mdist, "world_size", lambda: 2)
    log = []

    class _Work:
        def wait(self):
            pass

    def _async(flat):
        log.append(("async", flat.numel()))
        flat.mul_(2)
        return _Work()

    def _sync(flat):
        log.append(("sync", flat.numel()))
        return flat.mul_(2)

    monkeypatch.setattr(optim.mdist, "all_reduce_sum_async", _async)
    monkeypatch.setattr(optim.mdist, "all_reduce_sum_", _sync)
    used = []

    def _plain_update(p, g, *rest, **kw):
        """p -= 0.1 * grad_scale * g in the place of either kernel; grad_scale is the last positional argument of both entries"""
        gs = rest[-1]
        used.append((g * gs).clone())
        p.sub_(0.1 * gs * g)

    monkeypatch.setattr(optim.ops, "sgd_momentum_flat_", _plain_update)
    monkeypatch.setattr(optim.ops, "adam_flat_", _plain_update)
    gen = torch.Generator().manual_seed(4)
    dw1, dw2, gq = torch.randn(6, generator=gen), torch.randn(6, generator=gen), torch.randn(3, generator=gen)
    seqs, after = {}, {}
    for rank in ("A", "B"):
        q, p = torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(6))   # q: used once; p: used twice
        opt = cls([q, p], lr=0.1)
        opt._ensure_flat()
        bs = opt._flat["buckets"]
        assert len(bs) == 2 and bs[0]["ids"] == {id(p)} and bs[1]["ids"] == {id(q)}
        del log[:], used[:]
        if rank == "A":
            opt._early_grad(p, dw1.clone())
            opt._early_grad(p, dw2.clone())
        else:
            opt._early_grad(p, None)
            opt._early_grad(p, None)
        p.grad = dw1 + dw2                      # what the ``_LateGrad`` node / the accumulation hands to AccumulateGrad at the end
        opt._grad_arrived(p)
        q.grad = gq.clone()
        opt._grad_arrived(q)
        opt.step()
        seqs[rank], after[rank] = list(log), (p.detach().clone(), q.detach().clone())
        assert len(used) == 1 and torch.equal(used[0][:3], gq) and torch.equal(used[0][64:70], dw1 + dw2), rank
        assert all(not (b["dirty"] or b["ready"] or b["launched"] or b["arrived"] or b["unsunk"] or b["early"]) for b in bs)
    print("rank A:", seqs["A"], " rank B:", seqs["B"])
    assert seqs["A"] == seqs["B"], seqs
    for rank in ("A", "B"):
        assert torch.equal(after[rank][0], -0.1 * (dw1 + dw2)) and torch.equal(after[rank][1], -0.1 * gq), rank


def test_single_process_helpers():
    from mcdseg import dist as mdist
    assert mdist.world_size() == 1 and mdist.rank() == 0 and not mdist.is_distributed()
    t = torch.ones(3)
    assert mdist.all_reduce_sum_(t) is t and float(t.sum()) == 3
    mdist.barrier()
    env = {k: os.environ.pop(k, None) for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    try:
        assert mdist.init_from_env() == (0, 1, 0)
    finally:
        for k, v in env.items():
            if v is not None:
                os.environ[k] = v
