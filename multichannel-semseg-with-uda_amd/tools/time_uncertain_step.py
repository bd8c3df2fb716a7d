#!/usr/bin/env python3
"""Step time of the uncertain source-only trainer's update in its two forms, on one GPU:

    fused     one trunk pass + ``ops.up8_uncertain_loss`` over all T dropout draws (the default)
    literal   MCDSEG_FUSED_UNCERTAIN=0: T passes of the whole network, as the reference's get_loss runs them

BASELINE config 1 geometry by default (drn_d_38, 6 channels, -b 2, 320 x 240, T = 10).  One step = zero_grad, get_loss, backward,
optimizer step on a fixed synthetic batch.  Each step is bracketed by device events after ``--warmup`` steps; the two forms alternate in
blocks so that what else runs on the machine meets both.  The kernel's own time is taken the same way around the autograd function's
forward and backward launches (``ops.LAUNCH_TIMER``).  Prints one JSON line.

    python tools/time_uncertain_step.py --steps 20 --warmup 5
"""
import argparse
import json
import os
import statistics
import sys

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, PKG)


class _KernelTimer:
    """ops.LAUNCH_TIMER: collects the event pairs of the up8_uncertain_kernel launches"""

    def __init__(self):
        self.pairs = {}

    def wants(self, name):
        return name.startswith("up8_uncertain_kernel")

    def add(self, name, work, start, stop):
        self.pairs.setdefault(name, []).append((start, stop))

    def medians_ms(self, skip):
        return {k: statistics.median(a.elapsed_time(b) for a, b in v[skip:]) for k, v in self.pairs.items() if len(v) > skip}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--net", default="drn_d_38")
    ap.add_argument("--input_ch", type=int, default=6)
    ap.add_argument("-b", "--batch_size", type=int, default=2)
    ap.add_argument("--train_img_shape", type=int, nargs=2, default=(320, 240), metavar=("W", "H"))
    ap.add_argument("--n_class", type=int, default=41)
    ap.add_argument("--n_dropout", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=2, help="the forms alternate in this many blocks of steps / blocks each")
    ap.add_argument("--seed", type=int, default=1234)
    args = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("this measurement runs on an MI355X: there is no CPU fallback")
    os.environ["MCDSEG_PRETRAINED"] = "0"
    from loss import CrossEntropyLoss2d
    from mcdseg import ops
    from models.model_util import get_full_uncertain_model, get_optimizer

    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(args.seed)
    w, h = args.train_img_shape
    imgs = torch.randn(args.batch_size, args.input_ch, h, w, device=dev)
    lbls = torch.randint(0, args.n_class, (args.batch_size, h, w), device=dev)
    weight = torch.ones(args.n_class)
    weight[-1] = 0.0

    def make():
        torch.manual_seed(args.seed)
        model = get_full_uncertain_model(args.net, "50", args.n_class, args.input_ch, CrossEntropyLoss2d(weight), is_data_parallel=False,
                                         n_dropout=args.n_dropout).to(dev).train()
        return model, get_optimizer(model.parameters(), "sgd", 1e-3, 0.9, 2e-5)

    def step(model, optimizer):
        optimizer.zero_grad()
        base, unc = model.get_loss(imgs, lbls, separately_returning=True)
        (base + unc.mean()).backward()
        optimizer.step()

    runs = {"fused": make(), "literal": make()}
    times = {"fused": [], "literal": []}
    timer = _KernelTimer()
    for form, (model, optimizer) in runs.items():
        os.environ["MCDSEG_FUSED_UNCERTAIN"] = "1" if form == "fused" else "0"
        for _ in range(args.warmup):
            step(model, optimizer)
    torch.cuda.synchronize()
    per_block = max(1, args.steps // args.blocks)
    for _ in range(args.blocks):
        for form, (model, optimizer) in runs.items():
            os.environ["MCDSEG_FUSED_UNCERTAIN"] = "1" if form == "fused" else "0"
            ops.LAUNCH_TIMER = timer if form == "fused" else None
            events = []
            for _ in range(per_block):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                step(model, optimizer)
                b.record()
                events.append((a, b))
            torch.cuda.synchronize()
            times[form] += [a.elapsed_time(b) for a, b in events]
    ops.LAUNCH_TIMER = None
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({"net": args.net, "input_ch": args.input_ch, "batch": args.batch_size, "shape_wh": [w, h], "n_class": args.n_class,
                      "n_dropout": args.n_dropout, "steps_per_form": len(times["fused"]), "warmup": args.warmup,
                      "fused_step_ms_median": round(med["fused"], 3), "literal_step_ms_median": round(med["literal"], 3),
                      "fused_step_ms_min_max": [round(min(times["fused"]), 3), round(max(times["fused"]), 3)],
                      "literal_step_ms_min_max": [round(min(times["literal"]), 3), round(max(times["literal"]), 3)],
                      "speedup": round(med["literal"] / med["fused"], 2),
                      "kernel_ms_median": {k: round(v, 4) for k, v in timer.medians_ms(0).items()}}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
