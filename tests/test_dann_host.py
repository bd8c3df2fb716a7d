"""CPU: the DANN baseline's host side -- tests/dann_ref against the golden data of the real reference, the domain classifier's
state-dict layout, the width of its fc1, the parser, the Trainer field behind --adjust_lr, and what the trainer refuses."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import dann_ref as R
from dann_ref import DOWN, TAIL, case


@pytest.fixture(scope="module")
def fx(golden):
    return golden.npz("dann_small.npz")


@pytest.mark.parametrize("name", DOWN + TAIL)
def test_ref_reproduces_golden_kernel_cases(fx, name):
    """the numpy formulas ARE the reference's modules: fp64 against fp64, 1e-12 relative to max (the stored inputs are fp32 values)"""
    d = case(fx, name)
    R.conditions(d)
    mine = R.down_case(d) if name in DOWN else R.tail_case(d, training=bool(int(d["training"])))
    seen = 0
    for k in fx.files:
        if k.startswith(name + "/f64/"):
            q = k[len(name) + 5:]
            scale = float(d["db1_scale"]) if (q == "db1" and name in TAIL and int(d["training"])) else None
            assert R.rel_to_max(mine[q], fx[k], scale) < 1e-12, (name, q)
            seen += 1
    assert seen == (6 if name in DOWN else 11)


def test_tie_cases_hold_their_integer_facts(fx):
    """what the GPU test asserts exactly, established on the golden numbers themselves"""
    d = case(fx, "down/ties")
    dx, dy = fx["down/ties/f64/dx"][0, 0], d["dy"][0, 0]
    want = np.zeros((4, 4))
    want[0, 1] = dy[0, 0]  # two equal maxima (3, 3): the first in row-major order
    want[0, 2] = dy[0, 1]  # four equal maxima: the first
    want[2, 3] = dy[1, 1]  # an ordinary window; the all-zero window (rows 2-3, columns 0-1) passes nothing
    assert np.array_equal(dx, want)
    odd = fx["down/ties_odd/f64/dx"][0, 0]
    assert np.array_equal(odd[:4, :4], want) and not odd[4].any() and not odd[:, 4].any()


def _torch_modules(fx, dtype):
    init = {k[len("step/init/"):]: torch.as_tensor(fx[k]) for k in fx.files if k.startswith("step/init/")}
    g = torch.nn.Conv2d(3, 5, 1)
    f = torch.nn.Module()
    f.up = torch.nn.ConvTranspose2d(5, 5, 16, stride=8, padding=4, groups=5, bias=False)
    f.forward = lambda x: f.up(x)
    d = R.TorchDomainClassifier(5, 24)
    for name, m in (("g", g), ("f", f), ("d", d)):
        m.load_state_dict({k[2:]: v for k, v in init.items() if k.startswith(name + ".")})
        m.to(dtype).train()
    return g, f, d


def test_ref_step_reproduces_the_golden_trajectory(fx):
    """dann_ref.step over a torch composition of the three modules in fp64 follows the reference's two iterations, update by update"""
    g, f, d = _torch_modules(fx, torch.float64)
    lr, momentum, wd = (float(v) for v in fx["step/hyper"])
    opts = [torch.optim.SGD(m.parameters(), lr=lr, momentum=momentum, weight_decay=wd) for m in (g, f, d)]
    cw = torch.as_tensor(fx["step/cw"]).double()
    src, tgt, lbl = torch.as_tensor(fx["step/src"]).double(), torch.as_tensor(fx["step/tgt"]).double(), torch.as_tensor(fx["step/lbl"]).long()
    mods = {"g": g, "f": f, "d": d}
    for it in range(2):
        def check(update, it=it):
            for name in (("g", "f") if update == 1 else ("d",)):
                for k, v in mods[name].state_dict().items():
                    want = fx["step/f64/i%du%d/%s.%s" % (it, update, name, k)]
                    assert R.rel_to_max(v.numpy(), want) < 1e-10, (it, update, name, k)
        c, dl = R.step(g, f, d, *opts, lambda p, t: torch.nn.functional.cross_entropy(p, t, weight=cw), src, lbl, tgt, after_update=check)
        assert abs(c - fx["step/f64/c_loss"][it]) < 1e-10 and abs(dl - fx["step/f64/d_loss"][it]) < 1e-10


def test_golden_step_shows_the_carried_over_gradient(fx):
    """on the golden numbers alone: D's first step is not the step on update 2's gradient -- it is far smaller, because the leftover
    gradient of update 1 is the negative of nearly the same loss"""
    w0 = fx["step/init/d.fc2.weight"].astype(np.float64)
    ref, alone = fx["step/f64/i0u2/d.fc2.weight"], fx["step/f64/d_alone/d.fc2.weight"]
    assert R.rel_to_max(ref, alone) > 1e-3
    assert np.abs(ref - w0).max() < 0.5 * np.abs(alone - w0).max()


def test_domain_classifier_state_dict_layout(fx, monkeypatch):
    monkeypatch.setenv("MCDSEG_PRETRAINED", "0")
    from models.dilated_fcn import DRNSegDomainClassifier
    mine = [[k, list(v.shape)] for k, v in DRNSegDomainClassifier(5).state_dict().items()]
    assert mine == json.loads(str(fx["keys"]))
    wide = DRNSegDomainClassifier(5, fc_in=24).state_dict()
    assert tuple(wide["fc1.weight"].shape) == (10, 24)
    # a state dict of the reference's layout loads
    DRNSegDomainClassifier(5, fc_in=24).load_state_dict({k[2:]: torch.as_tensor(fx["step/init/" + k]) for k in
                                                         (q[len("step/init/"):] for q in fx.files if q.startswith("step/init/d."))})


def test_fc_in_follows_the_trunk(monkeypatch):
    monkeypatch.setenv("MCDSEG_PRETRAINED", "0")
    from models.dilated_fcn import DRNSegBase, domain_fc_in, score_map_hw
    g = DRNSegBase("drn_d_22", 5, pretrained=False, input_ch=3)
    assert domain_fc_in(g, (1080, 1080)) == 1089
    assert domain_fc_in(g, (640, 480)) == 300
    assert score_map_hw(g.base, 96, 64) == (12, 8) and score_map_hw(g.base, 65, 63) == (9, 8)
    for other in ("drn_c_26", "drn_d_38"):
        m = DRNSegBase(other, 5, pretrained=False, input_ch=3)
        assert domain_fc_in(m, (1080, 1080)) == 1089 and score_map_hw(m.base, 65, 87) == (9, 11)


def test_factory_refuses_other_nets():
    from models.model_util import get_dann_models
    with pytest.raises(NotImplementedError, match="Only FCN, SegNet, PSPNet are supported!"):
        get_dann_models("fcn", 3, 5, (64, 48))


def test_parser_and_trainer_declaration():
    import dann_trainer
    import trainer_common
    from argmyparse import get_da_dann_training_parser
    args = get_da_dann_training_parser().parse_args(["suncg", "nyu"])
    assert args.method == "DANN" and not hasattr(args, "num_k")
    t = dann_trainer.TRAINER
    assert t.sums == ("d_loss", "c_loss") and t.lr_adjusted == ("optimizer_g", "optimizer_f")
    opts = {"optimizer_g": 1, "optimizer_f": 2, "optimizer_d": 3}
    assert trainer_common.lr_adjusted_optimizers(t, opts) == [1, 2]
    # the field defaults to every optimizer: the five earlier trainers adjust what they adjusted
    import adapt_trainer
    import source_uncertain_trainer
    for other in (adapt_trainer.TRAINER, source_uncertain_trainer.TRAINER):
        assert other.lr_adjusted is None and trainer_common.lr_adjusted_optimizers(other, opts) == [1, 2, 3]
    assert trainer_common.Trainer.__dataclass_fields__["lr_adjusted"].default is None


def test_trainer_refuses_batch_one_and_several_ranks(monkeypatch):
    """both before any GPU use: ``main`` raises before ``train`` builds its ``Run``"""
    import dann_trainer
    import trainer_common
    monkeypatch.setattr(trainer_common, "Run", lambda args: pytest.fail("the GPU was reached"))
    monkeypatch.setattr(dann_trainer, "train", lambda *a: pytest.fail("train was reached"))
    flags = ["suncg", "nyu", "--net", "drn_d_22", "--synthetic", "--no_pretrained"]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit, match="needs -b 2 or more"):
        dann_trainer.main(flags + ["-b", "1"])
    with pytest.raises(SystemExit, match="needs -b 2 or more"):
        dann_trainer.main(flags)  # the reference's default batch size is 1
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="runs in one process"):
        dann_trainer.main(flags + ["-b", "2"])
