#!/usr/bin/env python3
"""Generate tests/golden/reduction_bits.json: the bit patterns of every reduced scalar the cases of tests/reduction_cases.py produce, and
the compiler the library was built with.  Needs a GPU.

    python tests/golden/make_reduction_bits.py                      # the library of the working tree
    MCDSEG_LIB=/path/to/libmcdseg_prev.so python tests/golden/make_reduction_bits.py   # another build (tools/build_prev_lib.sh)

The committed file was recorded once with the library of the commit BEFORE csrc/block_reduce.h existed (every block tail and finalizer
still written out by hand), so tests/test_reduction_bits_gpu.py holds the shared helpers to the bits of the code they replaced.
Regenerate only for a change that is meant to move these bits (a new toolchain, a deliberate change of a summation order), and say so."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "multichannel-semseg-with-uda_amd"))
from mcdseg import _lib, ops  # noqa: E402
import reduction_cases as RC  # noqa: E402


def main():
    dev = torch.device("cuda:0")
    out = {"compiler": RC.compiler_version(_lib.LIB_PATH), "cases": {}}
    for name, run in RC.CASES.items():
        out["cases"][name] = run(dev, ops)
        print("%-48s %s" % (name, " ".join("%08x" % b for b in out["cases"][name])))
    with open(os.path.join(HERE, "reduction_bits.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
