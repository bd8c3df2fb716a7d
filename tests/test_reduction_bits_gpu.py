"""GPU: every reduced scalar of the loss and head kernels, bit for bit against tests/golden/reduction_bits.json -- recorded with the
library as it was before csrc/block_reduce.h, when each block tail and finalizer was written out by hand.  The combination order of a
block's wave sums (tree or chain) and of the partial rows decides these bits; the cases and their shapes are in tests/reduction_cases.py.
A toolchain that moves the bits fails this test on purpose: the fixture names its compiler, and a mismatch is reported, not skipped."""
import numpy as np
import pytest

import reduction_cases as RC

pytestmark = pytest.mark.gpu

REGENERATE = "python tests/golden/make_reduction_bits.py   (on a GPU; see its docstring before committing the result)"


@pytest.fixture(scope="module")
def recorded(golden):
    return golden.json("reduction_bits.json")


def test_fixture_covers_the_cases(recorded):
    assert sorted(recorded["cases"]) == sorted(RC.CASES)


def test_compiler_is_the_fixtures(recorded):
    from mcdseg import _lib
    got = RC.compiler_version(_lib.LIB_PATH)
    assert got == recorded["compiler"], ("the library was built with another compiler than the fixture: %r, recorded %r; if the bits "
                                         "below moved with it, regenerate: %s" % (got, recorded["compiler"], REGENERATE))


@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_reduced_scalars_bitwise(name, recorded, device):
    from mcdseg import ops
    got = np.array(RC.CASES[name](device, ops), dtype=np.uint32)
    want = np.array(recorded["cases"][name], dtype=np.uint32)
    print("%s: got %s  recorded %s  (as fp32: %s / %s)" % (name, " ".join("%08x" % b for b in got), " ".join("%08x" % b for b in want),
                                                         got.view(np.float32), want.view(np.float32)))
    assert got.shape == want.shape and (got == want).all(), "reduced scalars differ from the recorded bits; to regenerate: " + REGENERATE
