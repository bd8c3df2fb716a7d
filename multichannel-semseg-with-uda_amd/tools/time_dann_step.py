#!/usr/bin/env python3
"""Time of the DANN baseline's domain classifier in two forms, and of a whole DANN step, on one GPU:

    fused      ``DRNSegDomainClassifier.forward_pair``: two DownConv launches and one tail launch each way (csrc/dann.hip)
    composed   the same head from torch modules (Conv2d, ReLU, MaxPool2d, Linear, BatchNorm1d, cross_entropy), called once per domain
               as a trainer built on them would

Head geometry: BASELINE config 2's score maps by default -- 16 + 16 maps of 41 x 60 x 80.  One head pass = what one iteration of the
trainer asks of D: update 1 (loss = -CE -CE, backward into the score maps and D) and update 2 (detached score maps, loss = +CE +CE,
backward into D alone).  Each pass is bracketed by device events after ``--warmup`` passes; the two forms alternate in blocks so that
what else runs on the machine meets both.  ``--full_step`` adds the step of dann_trainer.py (drn_d_38, 6 channels, 480 x 640 at
``-b``) with its kernels' launch times.  Prints one JSON line.

    python tools/time_dann_step.py --steps 20 --warmup 5 --full_step
"""
import argparse
import json
import os
import statistics
import sys

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, PKG)


class _KernelTimer:
    """ops.LAUNCH_TIMER: collects the event pairs of the dann_* launches"""

    def __init__(self):
        self.pairs = {}

    def wants(self, name):
        return name.startswith("dann_")

    def add(self, name, work, start, stop):
        self.pairs.setdefault(name, []).append((start, stop))

    def medians_ms(self):
        return {k: round(statistics.median(a.elapsed_time(b) for a, b in v), 4) for k, v in self.pairs.items()}


def composed_head(n_class, fc_in):
    """the head written out in torch modules from its shapes: two (conv3x3, ReLU, conv3x3, ReLU, 2x2 max-pool) blocks of widths
    n_class -> 10 -> 1, then Linear(fc_in, 10), BatchNorm1d, ReLU, Linear(10, 2)"""
    from torch import nn

    def down(cin, cout):
        return [nn.Conv2d(cin, cout, 3, padding=1), nn.ReLU(), nn.Conv2d(cout, cout, 3, padding=1), nn.ReLU(), nn.MaxPool2d(2, 2)]
    return nn.Sequential(*down(n_class, 10), *down(10, 1), nn.Flatten(), nn.Linear(fc_in, 10), nn.BatchNorm1d(10), nn.ReLU(), nn.Linear(10, 2))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-b", "--batch_size", type=int, default=16, help="samples per domain")
    ap.add_argument("--n_class", type=int, default=41)
    ap.add_argument("--map_hw", type=int, nargs=2, default=(60, 80), metavar=("H", "W"), help="the score map (1/8 of the image)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=2, help="the forms alternate in this many blocks of steps / blocks each")
    ap.add_argument("--full_step", action="store_true", help="also time dann_trainer.py's step: --net at 8 x map_hw, --input_ch channels")
    ap.add_argument("--net", default="drn_d_38")
    ap.add_argument("--input_ch", type=int, default=6)
    ap.add_argument("--seed", type=int, default=1234)
    args = ap.parse_args(argv)

    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("this measurement runs on an MI355X: there is no CPU fallback")
    os.environ["MCDSEG_PRETRAINED"] = "0"
    from mcdseg import ops
    from models.dilated_fcn import DRNSegDomainClassifier

    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(args.seed)
    n, c, (h, w) = args.batch_size, args.n_class, args.map_hw
    fc_in = (h // 4) * (w // 4)
    src, tgt = (torch.randn(n, c, h, w, device=dev) for _ in range(2))
    ones = torch.ones(n, dtype=torch.long, device=dev)
    fused = DRNSegDomainClassifier(c, fc_in=fc_in).to(dev).train()
    composed = composed_head(c, fc_in).to(dev).train()

    def head_pass(form):
        """update 1 and update 2 as D sees them; the gradients into the score maps are formed and dropped"""
        for sign, into_maps in ((-1.0, True), (1.0, False)):
            a, b = (t.detach().requires_grad_(into_maps) for t in (src, tgt))
            if form == "fused":
                loss = fused.forward_pair(a, b)[0].sum() * sign
            else:
                loss = (F.cross_entropy(composed(a), ones) + F.cross_entropy(composed(b), 0 * ones)) * sign
            loss.backward()
        for m in (fused, composed):
            for p in m.parameters():
                p.grad = None

    def timed(fn, count):
        events = []
        for _ in range(count):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            events.append((a, b))
        torch.cuda.synchronize()
        return [a.elapsed_time(b) for a, b in events]

    times = {"fused": [], "composed": []}
    timer = _KernelTimer()
    for form in times:
        for _ in range(args.warmup):
            head_pass(form)
    torch.cuda.synchronize()
    per_block = max(1, args.steps // args.blocks)
    for _ in range(args.blocks):
        for form in times:
            ops.LAUNCH_TIMER = timer if form == "fused" else None
            times[form] += timed(lambda: head_pass(form), per_block)
    ops.LAUNCH_TIMER = None
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"head": {"samples_per_domain": n, "n_class": c, "map_hw": [h, w], "passes_per_form": len(times["fused"]), "warmup": args.warmup,
                    "fused_ms_median": round(med["fused"], 4), "composed_ms_median": round(med["composed"], 4),
                    "fused_ms_min_max": [round(min(times["fused"]), 4), round(max(times["fused"]), 4)],
                    "composed_ms_min_max": [round(min(times["composed"]), 4), round(max(times["composed"]), 4)],
                    "composed_over_fused": round(med["composed"] / med["fused"], 2), "kernel_ms_median": timer.medians_ms()}}
    if args.full_step:
        import dann_trainer
        from loss import CrossEntropyLoss2d
        from models.model_util import get_dann_models, get_optimizer
        del fused, composed
        torch.manual_seed(args.seed)
        models = [m.to(dev).train() for m in get_dann_models(args.net, args.input_ch, c, (8 * w, 8 * h))]
        opts = [get_optimizer(m.parameters(), "sgd", 1e-3, 0.9, 2e-5) for m in models]
        weight = torch.ones(c)
        weight[-1] = 0.0
        criterion = CrossEntropyLoss2d(weight.to(dev))
        imgs_s, imgs_t = (torch.randn(n, args.input_ch, 8 * h, 8 * w, device=dev) for _ in range(2))
        lbls = torch.randint(0, c, (n, 8 * h, 8 * w), device=dev)

        def step():
            dann_trainer.update_g_f(*models, opts[0], opts[1], criterion, imgs_s, lbls, imgs_t)
            dann_trainer.update_d(models[0], models[2], *opts, imgs_s, imgs_t)

        for _ in range(max(2, args.warmup // 2)):
            step()
        torch.cuda.synchronize()
        timer = _KernelTimer()
        ops.LAUNCH_TIMER = timer
        t = timed(step, max(3, args.steps // 2))
        ops.LAUNCH_TIMER = None
        out["full_step"] = {"net": args.net, "input_ch": args.input_ch, "batch": n, "image_hw": [8 * h, 8 * w], "steps": len(t),
                            "step_ms_median": round(statistics.median(t), 2), "step_ms_min_max": [round(min(t), 2), round(max(t), 2)],
                            "kernel_ms_median": timer.medians_ms()}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
