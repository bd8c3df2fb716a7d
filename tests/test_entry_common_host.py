"""CPU: what the five trainers declare to ``trainer_common.train`` and what the testers take from ``tester_common`` -- the resume
back-fill, the output layout and the checkpoint layout, each against the strings and key lists of the reference's scripts."""
import argparse
import importlib
import os

import pytest

ADAPT = ["adapt_trainer", "adapt_mfnet_trainer", "adapt_multitask_trainer", "adapt_segbd_multitask_trainer"]


def _parser(name):
    mod = importlib.import_module(name)
    if hasattr(mod, "get_parser"):
        return mod.get_parser()
    import argmyparse
    return argmyparse.get_src_only_training_parser() if name == "source_trainer" else argmyparse.get_da_mcd_training_parser()


def _args(name, extra=()):
    import trainer_common
    datasets = ["suncg"] if name == "source_trainer" else ["suncg", "nyu"]
    return trainer_common.parse_args(_parser(name), datasets + ["--base_outdir", "out"] + list(extra))


# ------------------------------------------------------------------------------------------------ resume back-fill
@pytest.mark.parametrize("name", ADAPT + ["source_trainer"])
def test_backfill_fills_what_is_missing_and_keeps_what_is_there(name):
    import trainer_common
    trainer = importlib.import_module(name).TRAINER
    cli = _args(name, ["--resume", "out/m/pth/MCD-normal-drn_d_38-1.pth.tar", "--seed", "7", "--synthetic", "--synthetic_len", "5",
                       "--src_file_list", "s.txt", "--lr", "0.5", "--epochs", "9"])
    pickled = argparse.Namespace(savename="kept", seed=5, lr=0.25, epochs=3, no_tflog=True)
    got = trainer_common.resumed_args(trainer, pickled, cli)
    assert got is pickled
    assert (got.seed, got.lr, got.no_tflog, got.savename) == (5, 0.25, True, "kept")  # present: the checkpoint's
    assert (got.synthetic, got.synthetic_raw, got.synthetic_len, got.src_file_list, got.tgt_file_list, got.no_pretrained, got.solver) == \
        (True, False, 5, "s.txt", None, False, "fused")  # missing: the command line's (src / tgt_file_list in the mfnet trainer too)
    assert got.epochs == (9 if name == "adapt_segbd_multitask_trainer" else 3)
    assert "resume" not in vars(got) and "base_outdir" not in vars(got)  # nothing beyond the listed keys is copied


def test_backfill_extras_of_the_mfnet_and_segbd_trainers():
    import adapt_mfnet_trainer
    import adapt_segbd_multitask_trainer as segbd
    import trainer_common
    cli = _args("adapt_mfnet_trainer", ["--resume", "x", "--method_detail", "MFNet-GateFusion"])
    assert trainer_common.resumed_args(adapt_mfnet_trainer.TRAINER, argparse.Namespace(), cli).method_detail == "MFNet-GateFusion"
    kept = argparse.Namespace(method_detail="MFNet-ScoreAddFusion")
    assert trainer_common.resumed_args(adapt_mfnet_trainer.TRAINER, kept, cli).method_detail == "MFNet-ScoreAddFusion"
    cli = _args("adapt_segbd_multitask_trainer", ["--resume", "x", "--semseg_shortcut", "--use_seg2bd_conv", "--scale_bd_loss", "3",
                                                  "--boundary_loss_converging_epoch", "-1"])
    got = trainer_common.resumed_args(segbd.TRAINER, argparse.Namespace(epochs=1, depth_shortcut=True, scale_bd_loss=2), cli)
    assert (got.depth_shortcut, got.semseg_shortcut, got.add_pred_seg_boundary_loss, got.use_seg2bd_conv,
            got.boundary_loss_converging_epoch, got.scale_bd_loss, got.epochs) == (True, True, False, True, -1, 2, 40)


def test_adapt_trainer_takes_a_missing_savename_from_the_file_name():
    import adapt_trainer
    import trainer_common
    cli = _args("adapt_trainer", ["--resume", os.path.join("out", "m", "pth", "MCD-other-drn_d_38-3.pth.tar"), "--savename", "cli"])
    assert trainer_common.resumed_args(adapt_trainer.TRAINER, argparse.Namespace(), cli).savename == "MCD"  # infn.split("-")[0]
    assert trainer_common.resumed_args(adapt_trainer.TRAINER, argparse.Namespace(savename="mine"), cli).savename == "mine"
    for name in ADAPT[1:]:  # the rule is adapt_trainer's alone
        got = trainer_common.resumed_args(importlib.import_module(name).TRAINER, argparse.Namespace(), _args(name, ["--resume", "x"]))
        assert "savename" not in vars(got)


# ------------------------------------------------------------------------------------------------ output layout
LAYOUTS = [  # (script, flags, mode directory, model name at drn_d_38, model name at psp / res 101)
    ("adapt_trainer", ["--input_ch", "6"], "suncg-train2nyu-train_6ch", "MCD-normal-drn_d_38", "MCD-normal-psp-res101"),
    ("adapt_mfnet_trainer", ["--input_ch", "6", "--method_detail", "MFNet-ScoreAddFusion"], "suncg-train2nyu-train_6ch_MFNet",
     "MFNet-ScoreAddFusion-normal-drn_d_38", "MFNet-ScoreAddFusion-normal-psp-res101"),
    ("adapt_multitask_trainer", ["--input_ch", "4"], "suncg-train2nyu-train_4ch_MCDmultitask", "MCD-normal-drn_d_38",
     "MCD-normal-psp-res101"),
    ("adapt_segbd_multitask_trainer", ["--input_ch", "3"], "suncg-train2nyu-train_3ch_MCD_segbd_multitask", "MCD-normal-drn_d_38",
     "MCD-normal-psp-res101"),
    ("source_trainer", ["--input_ch", "6"], "suncg-train_only_6ch", "normal-drn_d_38", "normal-psp-res101"),
]


@pytest.mark.parametrize("name,flags,mode,plain,with_res", LAYOUTS, ids=[row[0] for row in LAYOUTS])
def test_output_layout_is_the_reference_scripts(name, flags, mode, plain, with_res):
    import trainer_common
    trainer = importlib.import_module(name).TRAINER
    for extra, model_name in (([], plain), (["--net", "psp", "--res", "101"], with_res)):
        args = _args(name, flags + extra)
        outdir = os.path.join("out", mode)
        fresh = trainer.layout(args, False)
        assert fresh == trainer_common.Layout(os.path.join(outdir, "pth"), os.path.join(outdir, "tflog", model_name),
                                              os.path.join(outdir, "param-%s.json" % model_name), model_name)
        assert trainer_common.checkpoint_fn(fresh, 1) == os.path.join(outdir, "pth", model_name + "-1.pth.tar")
        resumed = trainer.layout(args, True)  # (the source trainer's directories travel in the arguments the first run saved)
        assert resumed[:2] == fresh[:2] and trainer_common.checkpoint_fn(resumed, 40) == os.path.join(outdir, "pth", model_name + "-40.pth.tar")
        assert resumed.json_fn == os.path.join(outdir, "param_normal_resume.json" if name == "source_trainer"
                                               else "param-%s_resume.json" % model_name)


def test_layout_uses_the_splits_and_the_method_of_the_arguments():
    import adapt_mfnet_trainer
    import adapt_trainer
    args = _args("adapt_trainer", ["--src_split", "trainval", "--tgt_split", "val", "--method", "Mine", "--savename", "run7"])
    assert adapt_trainer.TRAINER.layout(args, False).json_fn == os.path.join("out", "suncg-trainval2nyu-val_3ch", "param-Mine-run7-drn_d_38.json")
    args = _args("adapt_mfnet_trainer", ["--method", "Mine"])  # named by method_detail, whatever --method says
    assert adapt_mfnet_trainer.TRAINER.layout(args, False).model_name == "MFNet-AddFusion-normal-drn_d_38"


# ------------------------------------------------------------------------------------------------ checkpoint layout
class _Stub:
    def __init__(self, tag):
        self.tag = tag

    def parameters(self):
        return []

    def state_dict(self):
        return {"tag": self.tag}


KEYS = {
    "adapt_trainer": ("get_models", 3, ["g_state_dict", "f1_state_dict", "f2_state_dict", "optimizer_g", "optimizer_f"]),
    "adapt_mfnet_trainer": ("get_models", 4, ["g_3ch_state_dict", "g_1ch_state_dict", "f1_state_dict", "f2_state_dict", "optimizer_g",
                                              "optimizer_f"]),
    "adapt_multitask_trainer": ("get_multitask_models", 2, ["enc_state_dict", "dec_state_dict", "optimizer_enc", "optimizer_dec"]),
    "adapt_segbd_multitask_trainer": ("get_segbd_multitask_models", 2, ["enc_state_dict", "dec_state_dict", "optimizer_enc", "optimizer_dec"]),
    "source_trainer": ("get_full_model", 1, ["state_dict", "optimizer"]),
}


@pytest.mark.parametrize("name,one_classifier", [(n, False) for n in sorted(KEYS)] + [(n, True) for n in ADAPT])  # (no such flag in source_trainer)
def test_checkpoint_keys_are_the_reference_scripts(name, one_classifier, monkeypatch):
    import trainer_common
    mod = importlib.import_module(name)
    factory, count, keys = KEYS[name]
    stubs = tuple(_Stub("model%d" % i) for i in range(count))
    monkeypatch.setattr(mod, factory, lambda *a, **k: stubs if count > 1 else stubs[0])
    monkeypatch.setattr(mod, "get_optimizer", lambda *a, **k: _Stub("optimizer"))
    args = _args(name, ["--input_ch", "6"] + (["--uses_one_classifier"] if one_classifier else []))
    modules, optimizers = mod.TRAINER.build(args)
    assert list(modules) + list(optimizers) == keys  # (the order in which they are loaded and their learning rates adjusted)
    dic = trainer_common.checkpoint_dict(args, 3, modules, optimizers)
    absent = {"f2_state_dict"} if one_classifier else set()  # (the two multitask trainers have no F2 to leave out)
    assert set(dic) == {"epoch", "args"} | (set(keys) - absent)
    assert dic["epoch"] == 3 and dic["args"] is args
    assert all(dic[k] == {"tag": "optimizer" if k.startswith("optimizer") else modules[k].tag} for k in set(keys) - absent)


# ------------------------------------------------------------------------------------------------ testers
def test_tester_output_directory():
    import tester_common
    ck = os.path.join("train_output", "suncg-train2nyu-train_6ch_MFNet", "pth", "MFNet-ScoreAddFusion-normal-drn_d_38-1.pth.tar")
    args = argparse.Namespace(trained_checkpoint=ck, tgt_dataset="nyu", split="val", outdir="o", use_f2=True)
    mode = "suncg-train2nyu-train_6ch_MFNet---nyu-val"
    assert tester_common.output_dir(args) == os.path.join("o", mode, "MFNet-ScoreAddFusion-normal-drn_d_38-1.tar-use_f2")  # ".tar" kept
    assert args.mode == mode
    assert tester_common.output_dir(args, strip_tar=True) == os.path.join("o", mode, "MFNet-ScoreAddFusion-normal-drn_d_38-1-use_f2")
    del args.use_f2  # the source-only tester's parser has no such flag
    assert tester_common.output_dir(args) == os.path.join("o", mode, "MFNet-ScoreAddFusion-normal-drn_d_38-1.tar")


def test_tester_epilogue_and_ground_truth_remap(tmp_path, capsys):
    import torch

    import tester_common

    class Meter:
        def __init__(self):
            self.hist, self.seen = torch.zeros(3, 3), []

        def update(self, labels, gts):
            self.seen.append(gts.tolist())
            self.hist += 1

        def summary(self):
            return {"pixAcc": 1.0, "mAcc": 2.0, "fwIoU": 3.0, "mIoU": 4.0}
    meter, labels = Meter(), torch.zeros(1, 2, 2, dtype=torch.uint8)
    assert tester_common.finish(str(tmp_path), 0.0, 0, meter) == 0.0  # no batch at all: no division by zero, no eval_result.json
    assert sorted(os.listdir(tmp_path)) == ["ave_ent_0.0.txt"]
    tester_common.update_meter(meter, labels, ["no ground truth"], 3)
    tester_common.update_meter(meter, labels, torch.zeros(1, 4, 4, dtype=torch.int64), 3)  # another shape than the labels'
    assert meter.seen == []
    tester_common.update_meter(meter, labels, torch.tensor([[[0, 1], [2, 255]]]), 3)
    assert meter.seen == [[[[0, 1], [255, 255]]]]  # n_class-1 is the training labels' background
    assert tester_common.finish(str(tmp_path), 1.5, 4, meter) == 0.375
    assert sorted(os.listdir(tmp_path)) == ["ave_ent_0.0.txt", "ave_ent_0.375.txt", "eval_result.json"]
    assert (tmp_path / "ave_ent_0.375.txt").read_text() == "0.375"
    assert "pixAcc 1.00  mAcc 2.00  fwIoU 3.00  mIoU 4.00" in capsys.readouterr().out
