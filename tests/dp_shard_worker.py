"""Helper of tests/test_trainers_gpu.py::test_two_ranks_with_unequal_shards_take_the_global_step (not a test module).

Started once per rank by ``torch.distributed.run`` with MCDSEG_SINGLE_DEVICE=1 MCDSEG_DIST_BACKEND=gloo, argv = [out.npz, optimizers] ("sgd,adam": one
fresh pair of heads and one step per optimizer, in one launch).
World 1 takes the whole batch of ``dp_shard_ref.head_problem``; of world 2 every rank takes its own, UNEQUAL shard (rank 0's labels
are about 90 % without weight).  No BatchNorm lies between the inputs and the loss (per-rank statistics are by design): the inputs
are a feature-map leaf, the model is the product's two ver2 ``DRNSegPixelClassifier`` heads, driven as step A drives them --
``MCDSolver._loss_backward(feats, labels, ce_coef=1.0)`` then ``optimizer_f.step()`` -- so ``ops.ce_normaliser``, the ``wsum_in`` form
of the loss kernel, the optimizer's flat all-reduce and the update kernel's ``grad_scale`` all run for real.  Rank 0 writes the update
of every head parameter and the ranks' feature gradients, concatenated and divided by world."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "multichannel-semseg-with-uda_amd"))
sys.path.insert(0, HERE)
os.environ["MCDSEG_PRETRAINED"] = "0"
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    import dp_shard_ref as ref
    from loss import CrossEntropyLoss2d, get_prob_distance_criterion
    from mcdseg import dist as mdist
    from mcdseg.optim import FlatAdam, FlatSGD
    from models.dilated_fcn import DRNSegPixelClassifier
    from models.model_util import get_optimizer
    from solvers.solver import MCDSolver
    out, opts = sys.argv[1], sys.argv[2].split(",")
    rank, world, _ = mdist.init_from_env()
    assert mdist.is_distributed() == (world > 1)
    dev = torch.device("cuda:0")
    hc = ref.HEAD_CASE
    feats, y, cw, heads = ref.head_problem()
    n0, n1 = ref.shards(hc["n"], world)[rank]
    res = {"world": np.int64(world)}
    for opt in opts:
        fs = []
        for hd in heads:
            f = DRNSegPixelClassifier(hc["c"], ver="ver2")
            with torch.no_grad():
                f.seg.weight.copy_(hd["seg_w"]), f.seg.bias.copy_(hd["seg_b"]), f.up.weight.copy_(hd["up_w"])
            fs.append(f.to(dev).train())
        named = [("d.f%d.%s" % (k + 1, name), p) for k, f in enumerate(fs)
                 for name, p in (("seg_w", f.seg.weight), ("seg_b", f.seg.bias), ("up_w", f.up.weight))]
        optimizer_f = get_optimizer(list(fs[0].parameters()) + list(fs[1].parameters()), opt, hc["lr"], hc["momentum"], hc["weight_decay"])
        assert type(optimizer_f) is (FlatSGD if opt == "sgd" else FlatAdam)
        criterion = CrossEntropyLoss2d(cw.to(dev), ignore_index=hc["ignore_index"])
        # (the generator handed to the constructor is never run)
        solver = MCDSolver(torch.nn.Identity(), fs[0], fs[1], None, optimizer_f, criterion, get_prob_distance_criterion("diff"))
        assert not solver.fused_up
        before = [p.detach().clone() for _, p in named]
        leaf = feats[n0:n1].to(dev).requires_grad_()
        optimizer_f.zero_grad()
        losses = solver._loss_backward((leaf,), y[n0:n1].to(dev), ce_coef=1.0)
        optimizer_f.step()
        torch.cuda.synchronize()
        grads = [leaf.grad.cpu()]
        vals = [losses[:2].cpu()]
        if world > 1:
            grads = [torch.zeros_like(grads[0]) for _ in range(world)]
            torch.distributed.all_gather(grads, leaf.grad.cpu())
            vals = [torch.zeros(2) for _ in range(world)]
            torch.distributed.all_gather(vals, losses[:2].cpu())
        res[opt + "/dfeat"] = (torch.cat(grads).double() / world).numpy()
        res[opt + "/ce"] = torch.stack(vals).double().mean(0).numpy()
        res[opt + "/wsum"] = np.float64(float(losses[3]))
        for (name, p), b in zip(named, before):
            res[opt + "/" + name] = (p.detach().double() - b.double()).cpu().numpy()
    if rank == 0:
        np.savez(out, **res)
    mdist.barrier()
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
