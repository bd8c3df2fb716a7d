#!/usr/bin/env python3
"""Generate tests/golden/fusenet_small.npz by running the REAL reference's ``FuseDRNSegBase`` (models/dilated_fcn.py:253-337) in memory,
the way make_golden.py does (same loader: lib2to3 on the reference's text, nothing copied), in fp32 and in fp64.

    python tests/golden/make_fusenet_golden.py            # needs the reference checkout make_golden.py loads

The class runs on a reduced DRN-D (tests/fusenet_ref.TINY: BasicBlock, one block or convolution per stage, widths
(16, 16, 24, 24, 32, 32, 32, 32)) that this script registers in the loaded reference's ``drn`` namespace as ``drn_d_tiny`` at run time --
a call of the reference's own ``DRN`` constructor with other arguments.  Batch 2 x 6 x 32 x 40, 7 classes.

Stored:
  "spec"                       tests/fusenet_ref.TINY as JSON (the widths, the seed of the initial state: tests/golden/recipe.fill_state_)
  "keys"                       the state-dict keys of the reference's FuseDRNSegBase with their shapes, as JSON
  "x", "dy"                    the input batch and the upstream gradient of the score map (fp32)
  "min_variance"               the smallest batch variance any BatchNorm sees in the train-mode forward (both calls of each), fp64: the
                               inputs are the first draw that keeps it above 1e-2
  "<case>/f64/<name>"          the fp64 truth; "<case>/unit/<name>": the fp32 reference's distance from it, max |.| relative to the
                               truth's largest magnitude -- for <name> in
                                 score                         the score map
                                 grad/<key>                    every main_layer* and seg gradient under dy (sub_layer* has none: asserted)
                                 state/<key>                   main_layer* running_mean / running_var / num_batches_tracked afterwards
                               cases: "train" (one train-mode forward and backward), "fix_bn" (the same with the BatchNorms fixed,
                               fix_batchnorm_when_training), "eval" (an eval-mode forward without grad: the score map only)
Convolution-weight gradients are stored rounded to fp32 (2^-24 of their own magnitude, far below every bound they are used with);
everything else is stored as fp64.

While generating, tests/fusenet_ref.FuseDRNSegBase is asserted against the reference in fp64 (1e-12 of each tensor's maximum)."""
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import load_reference  # noqa: E402
import fusenet_ref as R  # noqa: E402


def register_tiny(drn, spec):
    def drn_d_tiny(pretrained=False, input_ch=3, **kwargs):
        model = drn.DRN(drn.BasicBlock, list(spec["reps"]), arch="D", channels=tuple(spec["channels"]), **kwargs)
        return drn.replace_first_conv(model, input_ch=input_ch, arch="D")
    setattr(drn, spec["name"], drn_d_tiny)


def reference_model(dfcn, spec, dtype):
    m = dfcn.FuseDRNSegBase(spec["name"], spec["n_class"], pretrained=False, input_ch=6)
    return R.tiny_state(m.to(dtype), spec)


def main(path=R.GOLDEN):
    warnings.simplefilter("ignore")
    spec = R.TINY
    _, drn, dfcn, _, _ = load_reference()
    register_tiny(drn, spec)
    keys = [[k, list(v.shape)] for k, v in reference_model(dfcn, spec, torch.float32).state_dict().items()]
    mine_keys = [[k, list(v.shape)] for k, v in R.tiny_model(torch.float32, spec).state_dict().items()]
    assert keys == mine_keys, "fusenet_ref's state dict differs from the reference's"

    variances = []

    def watch(module, inputs):
        variances.append(float(inputs[0].detach().var(dim=(0, 2, 3), unbiased=False).min()))

    for attempt in range(50):  # the first draw that keeps every BatchNorm batch variance above 1e-2
        x, dy = R.tiny_inputs(spec, attempt)
        del variances[:]
        R.run_case(reference_model(dfcn, spec, torch.float64), "train", x, dy, watch=watch)
        print("draw %d: the smallest batch variance a BatchNorm sees: %.3e (%d calls)" % (attempt, min(variances), len(variances)))
        if min(variances) > 1e-2:
            break
    else:
        raise RuntimeError("no draw meets the variance condition")
    out = {"spec": np.array(json.dumps(spec)), "keys": np.array(json.dumps(keys)), "x": x, "dy": dy,
           "min_variance": np.float64(min(variances))}
    for case in R.CASES:
        r64 = R.run_case(reference_model(dfcn, spec, torch.float64), case, x, dy)
        r32 = R.run_case(reference_model(dfcn, spec, torch.float32), case, x, dy)
        mine = R.run_case(R.tiny_model(torch.float64, spec), case, x, dy)
        assert sorted(mine) == sorted(r64) == sorted(r32)
        for k, v in r64.items():
            err = R.rel_to_max(mine[k], v)
            assert err < 1e-12, (case, k, err)
            unit = R.rel_to_max(r32[k], v)
            out["%s/unit/%s" % (case, k)] = np.float64(unit)
            out["%s/f64/%s" % (case, k)] = v.astype(np.float32) if v.ndim == 4 and k.startswith("grad/") else v
        worst = max(r64, key=lambda k: out["%s/unit/%s" % (case, k)])
        print("%-7s %3d tensors; fusenet_ref vs reference fp64 below 1e-12; the fp32 reference's largest distance: %.2e (%s)"
              % (case, len(r64), out["%s/unit/%s" % (case, worst)], worst))
        if case != "eval":
            nbt = [v for k, v in r64.items() if k.endswith("num_batches_tracked")]
            assert nbt and all(int(v) == (2 if case == "train" else 0) for v in nbt)
    np.savez_compressed(path, **out)
    return path


if __name__ == "__main__":
    p = main()
    print(p, os.path.getsize(p), "bytes")
