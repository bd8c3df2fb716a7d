"""``hold``: one workload run under the stock allocator, under ``guards.guarded(interior=0xFF)`` and under ``guarded(interior=0x00)`` --
no guard byte changed, every returned tensor bit for bit the same in the three runs.  The procedure of
tests/test_memory_contract_gpu.py's helper of the same name, importable: a test file that holds its own ops to the memory contract
("The memory contract") takes it from here instead of importing another test module."""
import torch

from guards import guarded


class _Stock:
    """the first run: plain tensors from the caching allocator"""

    def __init__(self, device):
        self.device = device

    def put(self, t, requires_grad=False):
        out = t.detach().to(self.device)
        return out.requires_grad_(True) if requires_grad else out


def _bits(t):
    """the tensor as integers of its element size: NaNs compare by bit pattern"""
    t = t.detach().contiguous()
    if t.dtype.is_floating_point:
        t = t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.dtype.itemsize])
    return t


def hold(device, workload, workspace=False, family=None):
    """``workload(put)`` builds its inputs on the CPU from a seeded generator, moves them with ``put`` and returns a dict of named
    tensors.  ``workspace``: the operation has a ``*_workspace_bytes`` function, so at least one workspace must have been intercepted."""
    from mcdseg import ops
    ops._PACK_TABLES.clear()
    ref = {k: v.detach().clone() for k, v in workload(_Stock(device).put).items()}
    torch.cuda.synchronize(device)
    assert ref, "the workload returns nothing"
    seen = []
    for interior in (0xFF, 0x00):
        with guarded(device, interior=interior) as g:
            ops._PACK_TABLES.clear()  # no device table cached by an earlier run escapes the guards (nor does one of this run survive it)
            try:
                out = workload(g.put)
                found = g.check()
                got = {k: v.detach().clone() for k, v in out.items()}
            finally:
                ops._PACK_TABLES.clear()
            count, workspaces = g.count, g.workspaces
        assert found == [], "poison 0x%02X: a kernel wrote outside its memory: %s" % (interior, found)
        assert sorted(got) == sorted(ref)
        for k in ref:
            assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, k
            if not torch.equal(_bits(got[k]), _bits(ref[k])):
                diff = (_bits(got[k]) != _bits(ref[k])).flatten().nonzero().flatten()
                raise AssertionError("poison 0x%02X: %s depends on what its memory held before: %d of %d elements differ, the first at %d, "
                                     "the last at %d" % (interior, k, diff.numel(), ref[k].numel(), int(diff[0]), int(diff[-1])))
        assert count >= len(ref), "the workload allocated %d tensors through the harness for %d outputs: it bypassed it" % (count, len(ref))
        assert not workspace or workspaces >= 1, "no workspace was intercepted"
        seen.append((count, workspaces))
    assert seen[0] == seen[1], "the two guarded runs allocated differently: %s" % (seen,)
    print("memory contract [%s]: %d guarded allocations, %d workspaces" % (family or workload.__name__, seen[0][0], seen[0][1]))
    return ref
