"""Child process of tests/test_adam_gpu.py::test_adam_one_rank_through_the_real_collective: the only rank of a forced process group
(MCDSEG_DIST_FORCE=1, RANK / WORLD_SIZE / MASTER_* in the environment).  Three FlatAdam steps each, from the same seeded parameters and
gradients (through autograd, so that the post-accumulate hooks see them arrive; one parameter goes without a gradient once):
"plain" with the process group ignored, "whole" with the flat gradient buffer all-reduced in one piece, "bucketed" with
MCDSEG_DP_OVERLAP's buckets reduced from the hooks.  Writes the bytes of the three flat buffers after every step, as hex digests."""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multichannel-semseg-with-uda_amd"))

SHAPES = [(16, 6, 7, 7), (16,), (33, 5, 3, 3), (7,), (41, 1, 16, 16)]


def run(dev, counted):
    from mcdseg import dist as mdist
    from mcdseg.optim import FlatAdam
    gen = torch.Generator().manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(s, generator=gen).to(dev)) for s in SHAPES]
    opt = FlatAdam(params, lr=1e-3, betas=(0.5, 0.999), weight_decay=2e-5)
    digests, buckets = [], 0
    mdist.COLLECTIVE_EVENTS = []
    for step in range(3):
        coef = [torch.randn(s, generator=gen).to(dev) for s in SHAPES]
        opt.zero_grad()
        sum((p * c).sum() for i, (p, c) in enumerate(zip(params, coef)) if (step, i) != (1, 3)).backward()
        buckets = max(buckets, len(opt._flat["buckets"]) if opt._flat is not None else 0)
        opt.step()
        torch.cuda.synchronize()
        digests.append([hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest() for t in opt.flat_buffers()[:1] + opt.flat_buffers()[2:]])
    counted.append(len(mdist.COLLECTIVE_EVENTS))
    mdist.COLLECTIVE_EVENTS = None
    assert [float(opt.state[p]["step"]) for p in params] == [3, 3, 3, 2, 3]
    return digests, buckets


def main():
    from mcdseg import dist as mdist
    from mcdseg import optim
    rank, world, local = mdist.init_from_env()
    assert (rank, world) == (0, 1) and mdist.is_distributed()
    dev = torch.device("cuda", local)
    res, counted = {"backend": torch.distributed.get_backend(), "forced": mdist.FORCE}, []
    mdist.FORCE = False              # one rank, not forced: no collective at all
    assert not mdist.is_distributed()
    res["plain"], _ = run(dev, counted)
    mdist.FORCE = True
    optim.DP_OVERLAP = False
    res["whole"], _ = run(dev, counted)
    optim.DP_OVERLAP = True
    res["bucketed"], res["buckets"] = run(dev, counted)
    assert counted[0] == 0, counted
    res["collectives"] = {"whole": counted[1], "bucketed": counted[2]}
    mdist.barrier()
    torch.distributed.destroy_process_group()
    with open(sys.argv[1], "w") as fh:
        json.dump(res, fh)


if __name__ == "__main__":
    main()
