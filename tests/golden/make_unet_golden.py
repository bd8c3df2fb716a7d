#!/usr/bin/env python3
"""Generate the U-Net fixtures by running the REAL reference's ``UNetBase`` / ``UNetClassifier`` (models/unet.py:122-199) in memory,
through the loader make_golden.py has (nothing is copied; the module itself imports unchanged under the installed Python and torch).

    python tests/golden/make_unet_golden.py            # needs the reference checkout make_golden.py loads

Written:
  unet_keys.json   {"base/<feature_scale>": [[key, shape], ...], "classifier/<feature_scale>": ...} of ``UNetBase(input_ch=6)`` and
                   ``UNetClassifier(n_classes=5)`` at feature_scale 4 and 8
  unet_small.npz   the case of tests/unet_ref.SPEC (N = 2, 6 x 32 x 48, 5 classes, feature_scale=8), train mode, through
                   tests/unet_ref.run -- the same procedure the GPU test runs on ``models.unet``:
     "spec"            tests/unet_ref.SPEC as JSON; parameters and inputs are drawn from its seeds (unet_ref.fill_models / inputs), none
                       are stored; "x_sum" / "labels_sum" are checksums of the drawn inputs
     "f64/<name>"      the fp64 result, for <name> in
                         feat/center, feat/conv1 .. feat/conv4, o1, o2        the five feature maps and both classifiers' logits
                         state/<key>                                          the BatchNorm running statistics after the forward
                         loss/ce, loss/diff                                   CE(o1) + CE(o2) (F.cross_entropy standing in for the
                                                                              removed NLLLoss2d) and mean |softmax(o1) - softmax(o2)|
                         grad_ce/<p>, grad_diff/<p>                           their gradients, <p> = x, g.<key>, f1.<key>, f2.<key>; a
                                                                              tensor above 2048 elements at the flat indices
                                                                              arange(0, numel, ceil(numel / 2048))
     "f32/<name>"      the fp32 reference's own result, for the losses and the running statistics
     "scale/grad_<loss>/g.<conv>.bias"   for the bias of each of G's convolutions -- all in front of a train-mode BatchNorm, so the
                       gradient is zero in exact arithmetic and the fp64 result is rounding noise around 1e-18: the largest per-channel
                       sum of the magnitudes of the terms whose sum it is (|gradient of the convolution's output|), fp64.  Errors of such
                       a tensor are taken relative to this scale (the rule of tests/dann_ref.rel_to_max for sums whose terms cancel)
     "units"           JSON {name: the fp32 reference's distance from the fp64 result, max |.| relative to the truth's largest magnitude
                       (to the scale above where there is one)}, for every f64/<name>, computed before anything is rounded
Everything this case produces, kept in both precisions (8 + 4 bytes per value), is 2.2 MB -- the 115 000 stored gradient values
alone are 1.4 MB -- where this fixture was to stay below 1.5 MB; it is 0.74 MB.  What is large is stored in 4 bytes: the feature maps,
the logits, the input's gradient and the weight gradients of more than 128 elements are the fp64 results ROUNDED to fp32 -- 2^-24 of their own magnitude,
0.3 % of the floor (2e-5 of the tensor's maximum) of every bound they are used with -- and of the fp32 reference's tensors only the
distance above is kept, which is all a test takes from them.  Everything else is stored as fp64."""
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF, load_reference  # noqa: E402
import unet_ref as R  # noqa: E402


def main():
    warnings.simplefilter("ignore")
    load_reference()  # puts the reference first on sys.path and loads its ``models`` package
    import models.unet as ref_unet
    assert ref_unet.__file__.startswith(REF), ref_unet.__file__
    spec = R.SPEC
    keys = {}
    for fs in (4, 8):
        keys["base/%d" % fs] = R.keys_shapes(ref_unet.UNetBase(feature_scale=fs, input_ch=spec["input_ch"]))
        keys["classifier/%d" % fs] = R.keys_shapes(ref_unet.UNetClassifier(feature_scale=fs, n_classes=spec["n_class"]))
    with open(R.KEYS, "w") as fh:  # one [key, shape] pair per line
        fh.write("{\n" + ",\n".join("%s: [\n%s\n]" % (json.dumps(name), ",\n".join(" " + json.dumps(pair) for pair in pairs))
                                    for name, pairs in keys.items()) + "\n}\n")

    def models(dtype):
        ms = [ref_unet.UNetBase(feature_scale=spec["feature_scale"], input_ch=spec["input_ch"]),
              ref_unet.UNetClassifier(feature_scale=spec["feature_scale"], n_classes=spec["n_class"]),
              ref_unet.UNetClassifier(feature_scale=spec["feature_scale"], n_classes=spec["n_class"])]
        return R.fill_models([m.to(dtype) for m in ms])

    # The network is piecewise linear around ReLUs and 2x2 maxima, and its deepest BatchNorm sees 12 values per channel: where fp32
    # and fp64 take different sides of one such decision the two results differ by per cents, and the fp32 distance stops being a unit
    # of rounding.  The inputs are the first draw (input_seed, input_seed + 1, ...) on which no tensor of the fp32 reference is farther
    # than 1e-3 from fp64.
    for attempt in range(200):
        spec = dict(R.SPEC, input_seed=R.SPEC["input_seed"] + attempt)
        x, labels = R.inputs(spec)
        r64 = R.run(*models(torch.float64), x, labels, scales=True)
        r32 = R.run(*models(torch.float32), x, labels)
        far = max(R.rel_to_max(r32[k], v, r64.get("scale/" + k)) for k, v in r64.items() if not k.startswith("scale/"))
        print("draw %d: the fp32 reference's largest distance from fp64 %.2e" % (attempt, far))
        if far < 1e-3:
            break
    else:
        raise RuntimeError("no draw keeps fp32 and fp64 on the same side of every decision")
    out = {"spec": np.array(json.dumps(spec)), "x_sum": np.float64(x.double().sum()), "labels_sum": np.int64(labels.sum())}
    for k in [k for k in r64 if k.startswith("scale/")]:
        out[k] = r64.pop(k)
    assert sorted(r64) == sorted(r32) and len([k for k in out if k.startswith("scale/")]) == 20
    units = {}
    for k, v in r64.items():
        units[k] = R.rel_to_max(r32[k], v, out.get("scale/" + k))
        wide = k.startswith("feat/") or k in ("o1", "o2") or (k.startswith("grad_") and (k.endswith("/x") or (
            k.split(".")[-1] == "weight" and v.size > 128 and not k.endswith(".1.weight"))))
        out["f64/" + k] = v.astype(np.float32) if wide else v
        if k.startswith("loss/") or k.startswith("state/"):
            out["f32/" + k] = r32[k]
    out["units"] = np.array(json.dumps(units))
    nbt = [int(v) for k, v in r64.items() if k.endswith("num_batches_tracked")]
    assert len(nbt) == 10 and set(nbt) == {1}  # (the state is recorded behind the first of the two passes)
    np.savez_compressed(R.GOLDEN, **out)
    worst = max(units, key=units.get)
    print("%d tensors; the fp32 reference's largest distance from fp64: %.2e (%s); losses %s" %
          (len(r64), units[worst], worst, {k: float(v) for k, v in r64.items() if k.startswith("loss/")}))
    for p in (R.KEYS, R.GOLDEN):
        print(p, os.path.getsize(p), "bytes")
        assert os.path.getsize(p) < 1500000


if __name__ == "__main__":
    main()
