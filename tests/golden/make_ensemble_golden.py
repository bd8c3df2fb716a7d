"""Writes tests/golden/ensemble_small.npz: three 20 x 12 x 16 maps and what ensembling them gives, for both methods.

The reference's own ``ensemble_predict`` (tools/ensemble_predict_from_npy.py:17-56) could NOT be run to make this file: it imports
``transform.py``, which imports torchvision, and torchvision is not installed where this fixture was made.  The outputs are therefore
those of the numpy / Pillow ORACLE, tests/ensemble_ref.py (19 of the 20 classes used, as the reference does, the VOC colours of 20 labels,
PNG size 21 x 17 so that both axes are resized by a ratio at which the naive nearest rule fails).  The file pins the oracle to numpy's and
Pillow's own arithmetic as they were when it was written (numpy 2.2.6, Pillow 12.2.0); no equality with a run of the reference is claimed.

    python tests/golden/make_ensemble_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ensemble_ref as R  # noqa: E402

N_USED, OUT_WH = 19, (21, 17)


def main():
    maps = [m[0] for m in R.make_maps("random", 3, 1, 20, 12, 16, seed=2024)]
    maps[1][3, 5, 7] = -0.0   # one element whose mean is (0 + -0.0 + ...): the sign of a zero sum
    maps[0][3, 5, 7] = -0.0
    maps[2][3, 5, 7] = -0.0
    out = {"p%d" % k: m for k, m in enumerate(maps)}
    for method in R.METHODS:
        prob, label, vis = R.ensemble_predict(maps, method, N_USED, OUT_WH)
        out["prob_" + method], out["label_" + method], out["vis_" + method] = prob, label, vis
    np.savez_compressed(os.path.join(HERE, "ensemble_small.npz"), n_used=np.int64(N_USED), out_wh=np.array(OUT_WH, dtype=np.int64), **out)
    print("wrote ensemble_small.npz: %s" % {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
