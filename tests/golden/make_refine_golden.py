"""Writes tests/golden/refine_small.npz: the inputs and the expected ``regions`` / ``out`` of the boundary refinement for the cases of
tests/refine_ref.golden_cases(), produced by the numpy restatement (tests/refine_ref.py).  Per case: b_<name> (uint8 boundary),
s_<name> (uint8 labels), p_<name> (int32 [thre, min_thre, max_thre]), r_<name> (int32 regions), o_<name> (uint8 refined labels).

    python tests/golden/make_refine_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import refine_ref as R  # noqa: E402


def main(path=os.path.join(HERE, "refine_small.npz")):
    out = {}
    for name, b, seg, thre, lo, hi in R.golden_cases():
        reg = R.regions(b, thre)
        out["b_" + name], out["s_" + name] = b, seg
        out["p_" + name] = np.array([thre, lo, hi], np.int32)
        out["r_" + name], out["o_" + name] = reg, R.refine(seg, reg, lo, hi)
    np.savez_compressed(path, **out)
    return path


if __name__ == "__main__":
    print(main())
