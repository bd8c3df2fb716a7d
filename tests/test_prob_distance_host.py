"""The distances of ``--d_loss`` besides L1 on the loss kernels: what can be checked without a GPU -- the C ABI (header, exports,
bindings, argument checks that precede every launch), the criteria's kinds, the binding's own argument checks, and the contracts of
the new LDS-DMA kernels that are read off the built library's disassembly."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mcdseg_softmax_ce_dist", "mcdseg_up8_softmax_ce_dist")
# the table of the issue: seven names, three functions besides L1
KINDS = {"diff": 0, "symkl": 1, "nmlsymkl": 1, "mysymkl": 1, "mis_symkl": 2, "spatial_jsd": 2, "jsd": 3}


def test_dist_entry_points_are_declared_exported_bound_and_validate_their_arguments():
    from mcdseg import _lib
    with open(os.path.join(ROOT, "include", "mcdseg.h")) as fh:
        header = fh.read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib._SIGNATURES and name in _lib.EXPORTS
    for i, name in enumerate(("MCDSEG_DIST_L1", "MCDSEG_DIST_SYMKL", "MCDSEG_DIST_MIS_SYMKL", "MCDSEG_DIST_JSD")):
        assert re.search(r"#define %s %d\b" % (name, i), header), name
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()  # stands for every non-null pointer: the checks below all precede the first launch
    ws = ctypes.c_size_t(1 << 20)
    plain = lambda z1, z2, kind, losses=buf: L.mcdseg_softmax_ce_dist(z1, z2, None, None, -100, 0.0, 1.0, None, None, None, losses,  # noqa: E731
                                                                     1, 4, 4, kind, buf, ws, None)
    up = lambda s1, s2, w2, kind: L.mcdseg_up8_softmax_ce_dist(s1, buf, s2, w2, None, None, -100, 0.0, 1.0, None, None, None, buf,  # noqa: E731
                                                               1, 4, 1, 1, kind, buf, ws, None)
    for kind in (7, -1, 4):
        assert plain(buf, buf, kind) == -22 and b"dist_kind" in L.mcdseg_last_error()
        assert up(buf, buf, buf, kind) == -22 and b"dist_kind" in L.mcdseg_last_error()
    for kind in (0, 1, 2, 3):
        assert plain(None, buf, kind) == -22 and b"null pointer" in L.mcdseg_last_error()
        assert plain(buf, buf, kind, None) == -22 and b"null pointer" in L.mcdseg_last_error()
        assert up(None, buf, buf, kind) == -22 and b"null pointer" in L.mcdseg_last_error()
    for kind in (1, 2, 3):  # a distance needs both heads (diff_coef 0 and no g2, so that only the kind objects)
        assert L.mcdseg_softmax_ce_dist(buf, None, None, None, -100, 0.0, 0.0, None, None, None, buf, 1, 4, 4, kind, buf, ws, None) == -22
        assert b"z2" in L.mcdseg_last_error()
        assert L.mcdseg_up8_softmax_ce_dist(buf, buf, None, None, None, None, -100, 0.0, 0.0, None, None, None, buf, 1, 4, 1, 1, kind, buf, ws,
                                            None) == -22
        assert b"s2" in L.mcdseg_last_error()
    assert L.mcdseg_softmax_ce_dist(buf, buf, None, None, -100, 0.0, 1.0, None, None, None, buf, 1, 49, 4, 1, buf, ws, None) == -22
    assert b"48 classes" in L.mcdseg_last_error() and L.mcdseg_last_error().startswith(b"softmax_ce_dist:")
    assert up(None, buf, buf, 2) == -22 and L.mcdseg_last_error().startswith(b"up8_softmax_ce_dist:")
    # ... and the L1 entries still speak in their own name
    assert L.mcdseg_softmax_ce_l1(None, None, None, None, -100, 0.0, 0.0, None, None, None, buf, 1, 4, 4, buf, ws, None) == -22
    assert L.mcdseg_last_error().startswith(b"softmax_ce_l1:")
    assert L.mcdseg_up8_softmax_ce_l1(None, buf, None, None, None, None, -100, 0.0, 0.0, None, None, None, buf, 1, 4, 1, 1, buf, ws, None) == -22
    assert L.mcdseg_last_error().startswith(b"up8_softmax_ce_l1:")


def test_criteria_name_their_kind_and_the_binding_checks_its_arguments():
    from loss import get_prob_distance_criterion
    from mcdseg import ops
    assert ops.DIST_KINDS == KINDS
    for name, kind in KINDS.items():
        assert get_prob_distance_criterion(name, n_class=9).dist_kind == kind, name
    z = torch.zeros(1, 4, 2, 2)
    for bad in ("l2", "", 4, -1, None, 1.0, True):
        with pytest.raises(ValueError):
            ops.prob_distance(z, z, bad)
        with pytest.raises(ValueError):
            ops.mcd_losses(z, z, None, None, diff_coef=1.0, dist=bad)
        with pytest.raises(ValueError):
            ops.up8_mcd_losses(z, z, z, z, None, None, diff_coef=1.0, dist=bad)
        with pytest.raises(ValueError):
            ops.up8_loss_kernel_name(1, 4, 2, 2, True, False, dist=bad)
    for kind in ("jsd", "symkl", "mis_symkl", 1, 2, 3):
        with pytest.raises(RuntimeError, match="must live on the GPU"):  # as every other op refuses a CPU tensor
            ops.prob_distance(z, z, kind)
        with pytest.raises(ValueError, match="two heads"):
            ops.mcd_losses(z, None, None, None, dist=kind)
    # the criteria themselves keep their torch expression off the GPU (and in fp64 anywhere)
    a, b = torch.randn(2, 5, 3, 4, dtype=torch.float64), torch.randn(2, 5, 3, 4, dtype=torch.float64)
    for name in KINDS:
        if name != "diff":
            assert torch.isfinite(get_prob_distance_criterion(name, n_class=5)(a, b))


def test_solver_takes_the_criteria_and_refuses_anything_else():
    from loss import CrossEntropyLoss2d, JSD, get_prob_distance_criterion
    from solvers.solver import MCDSolver
    m = torch.nn.Conv2d(1, 1, 1)
    for name, kind in KINDS.items():
        s = MCDSolver(m, m, m, None, None, CrossEntropyLoss2d(), get_prob_distance_criterion(name, n_class=9))
        assert s.dist == kind
    for crit in (torch.nn.MSELoss(), JSD(size_average=False)):
        with pytest.raises(NotImplementedError):
            MCDSolver(m, m, m, None, None, CrossEntropyLoss2d(), crit)


def test_dist_dma_kernels_keep_the_contracts_of_the_counted_wait():
    """csrc/loss.hip: the `s_waitcnt vmcnt(63)` of the LDS-DMA kernel relies on a wave issuing heads x C gradient stores per item (plus
    the one store of its block partials), behind the next item's DMAs, with no compiler-made drain or M0 use in between -- for every
    instantiation of the new kernels as for the L1 ones; and none of them may use scratch memory."""
    from mcdseg import _lib
    counts = _lib.dist_dma_store_counts()
    assert sorted(counts) == [(nc, k) for nc in (16, 24, 41, 48) for k in (1, 2, 3)]
    l1 = _lib.loss_dma_store_counts()
    for (nc, kind), n in counts.items():
        assert n == 2 * nc + 1 == l1[(nc, 2)], (nc, kind, n)
    assert "up8_softmax_ce_dist_dma_kernel" in _lib.HIDDEN_DMA_KERNELS
    assert _lib.hidden_dma_hazards() == []
    assert _lib.drains_inside_store_loops() == []
    # no scratch, no spilled vector register: from the code objects' own metadata (what tools/kernel_resources.py prints)
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "softmax_ce_dist"], check=True, capture_output=True,
                         text=True).stdout
    rows = [ln.split() for ln in out.splitlines()[1:] if ln.strip()]
    assert len(rows) == 39, len(rows)  # 3 kinds x (3 plain + 3 register-staged + 7 LDS-DMA instantiations)
    for r in rows:
        agpr, vgpr, vspill, sgpr, sspill, lds, scratch = (int(v) for v in r[-7:])
        assert vspill == 0 and scratch == 0 and agpr + vgpr <= 256, r  # (8 waves per workgroup: 256 registers per lane)
