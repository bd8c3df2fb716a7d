"""What the five trainers share.  ``Run`` is the process: process-group / device set-up, the optional tensorboard logger, the
device input pipeline and rank-0 writes.  ``train`` is the one skeleton every trainer runs -- resume, output layout, loader,
train mode, epoch loop, logging, checkpoint -- driven by a ``Trainer`` declaration of what one entry script does differently."""
import collections
import dataclasses
import os
import typing

import torch
import tqdm

from argmyparse import add_additional_params_to_args
from datasets import ConcatDataset, check_src_tgt_ok, get_dataset
from loss import CrossEntropyLoss2d, get_prob_distance_criterion
from mcdseg import dist as mdist
from models.model_util import fix_batchnorm_when_training, fix_dropout_when_training
from util import (adjust_learning_rate, check_if_done, emphasize_str, get_class_weight_from_file, load_checkpoint,
                  mkdir_if_not_exist, save_checkpoint, save_dic_to_json)


class Run:
    def __init__(self, args):
        self.rank, self.world, self.local = mdist.init_from_env()
        if not torch.cuda.is_available():
            raise SystemExit("this trainer runs on an MI355X: the HIP kernels are the only implementation (no CPU fallback)")
        self.device = torch.device("cuda", self.local if self.world > 1 else torch.cuda.current_device())
        torch.cuda.set_device(self.device)
        if getattr(args, "no_pretrained", False):
            os.environ["MCDSEG_PRETRAINED"] = "0"
        if getattr(args, "dtype", "f32") == "f16":  # reduced precision (BASELINE config 5 "bf16"): one fp16 term per product and, inside the
            from mcdseg import ops                   # trunk, ONE 16-bit value per activation / z / gradient element (ops.HALF_STORAGE) --
            ops.CONV_MATH = "f16x1"                  # unless MCDSEG_ACT_STORAGE says how activations are to be kept
            if "MCDSEG_ACT_STORAGE" not in os.environ:
                ops.ACT_STORAGE = "compact"
        torch.manual_seed(getattr(args, "seed", 1234))
        self._log = None
        self._pipe = None
        self._joint = None  # (crop_size, rotate_angle) of the joint transform, set by ``train`` once the namespace is final
        self._args = args

    def images(self, t):
        """batch -> device; raw uint8 HWC batches (``--synthetic_raw``) go through the device input pipeline"""
        if t.dtype == torch.uint8:
            return self._pipeline().images(t)
        return t.to(self.device, non_blocking=True)

    def labels(self, t):
        if t.dtype == torch.uint8:
            return self._pipeline().labels(t)
        return t.to(self.device, non_blocking=True)

    def pair(self, img, lbl):
        """a labelled batch -> device; raw uint8 image and label map go through the pipeline TOGETHER, so that a joint transform
        (``--crop_size``) flips, rotates and crops both under one draw per sample"""
        if img.dtype == torch.uint8 and lbl.dtype == torch.uint8:
            return self._pipeline().joint(img, lbl)
        return self.images(img), self.labels(lbl)

    def joint_transform_args(self, args, trainer=None):
        """(crop_size, rotate_angle) the pipeline is to apply.  The joint transform works on the raw uint8 batches (``--synthetic_raw``,
        ``--src_file_list`` / ``--tgt_file_list``); fp32 ``--synthetic`` batches and a source with channels of its own (the triple
        trainer's RGB+HHA+boundary, which has no raw form) keep ignoring the two flags, with one line that says so."""
        crop, angle = getattr(args, "crop_size", -1), getattr(args, "rotate_angle", 0)
        if crop <= 0:  # no joint transform at all, also with --rotate_angle set (adapt_trainer.py:101-102)
            return -1, 0
        raw = getattr(args, "synthetic_raw", False) or getattr(args, "src_file_list", None) or getattr(args, "tgt_file_list", None)
        own_source = trainer is not None and trainer.src_input_ch not in (None, args.input_ch)
        if not raw or own_source:
            if self.is_main:
                print("--crop_size %d --rotate_angle %s have no effect here: the joint transform runs on raw uint8 batches "
                      "(--synthetic_raw, --src_file_list / --tgt_file_list)%s" % (crop, angle, ", and this trainer's source has no raw form" if own_source else ""))
            return -1, 0
        return crop, angle

    def _pipeline(self):
        if self._pipe is None:
            from datasets import DeviceInputPipeline
            lists = getattr(self._args, "src_file_list", None) or getattr(self._args, "tgt_file_list", None)
            crop, angle = self._joint if self._joint is not None else (-1, 0)
            self._pipe = DeviceInputPipeline(self._args.input_ch, self._args.n_class, self.device,
                                             background_id=getattr(self._args, "background_id", 255),
                                             img_shape=self._args.train_img_shape if lists else None,  # real files: Scale on the GPU
                                             crop_size=crop, rotate_angle=angle,
                                             seed=getattr(self._args, "seed", 1234) + 101 * self.rank)  # per rank, as synthetic_spec shards
        return self._pipe

    @property
    def is_main(self):
        return self.rank == 0

    def configure_logger(self, tflog_dir, args):
        if not self.is_main:
            return
        mkdir_if_not_exist(tflog_dir)
        try:
            from tensorboard_logger import configure, log_value
            configure(tflog_dir, flush_secs=5)
            self._log = log_value
        except ImportError:
            if not getattr(args, "no_tflog", False):
                print("tensorboard_logger is not installed: scalar logs go to stdout only")

    def log_value(self, name, value, step):
        if self.is_main:
            if self._log is not None:
                self._log(name, value, step)
            print("  [%d] %s = %s" % (step, name, value))

    def save_params(self, args, json_fn):
        if self.is_main:
            check_if_done(json_fn)
            save_dic_to_json(dict(vars(args)), json_fn, verbose=False)
        mdist.barrier()

    def save(self, save_dic, filename):
        """rank 0 writes the checkpoint (its BatchNorm running statistics are the ones kept, as replica 0's are
        under nn.DataParallel)."""
        if self.is_main:
            save_checkpoint(save_dic, is_best=False, filename=filename)
            print("saved %s" % filename)
        mdist.barrier()

    def sync_replicas(self, modules):
        """identical start on every rank (same seed already gives that; the broadcast makes it unconditional)"""
        if self.world > 1:
            for m in modules:
                mdist.broadcast_([p.data for p in m.parameters()] + [b for b in m.buffers()])


def synthetic_spec(args, seed_offset, rank):
    shape = [int(x) for x in args.train_img_shape]
    return dict(length=args.synthetic_len, img_shape=shape, n_class=args.n_class, seed=args.seed + seed_offset + 101 * rank,
                raw=getattr(args, "synthetic_raw", False), background_id=getattr(args, "background_id", 255))


def make_loader(args, run, names_splits, src_input_ch=None):
    """DataLoader over one dataset or a ConcatDataset of (source, target); per-rank shard by seed.  ``src_input_ch``: the channel count
    of the first (source) dataset where it is not ``args.input_ch`` (``Trainer.src_input_ch``)."""
    sets = []
    lists = [getattr(args, "src_file_list", None), getattr(args, "tgt_file_list", None)]
    for i, (name, split) in enumerate(names_splits):
        spec = synthetic_spec(args, 7 * i, run.rank) if (args.synthetic or getattr(args, "synthetic_raw", False)) else None
        sets.append(get_dataset(dataset_name=name, split=split, img_transform=None, label_transform=None, test=False,
                                input_ch=src_input_ch if (i == 0 and src_input_ch is not None) else args.input_ch, synthetic=spec,
                                file_list=lists[i] if i < 2 else None))
    ds = sets[0] if len(sets) == 1 else ConcatDataset(*sets)
    return torch.utils.data.DataLoader(ds, batch_size=args.batch_size, shuffle=True, pin_memory=True, drop_last=True)


# ------------------------------------------------------------------------------------------------ the trainers' skeleton
@dataclasses.dataclass
class Trainer:
    """What one entry script declares.  ``modules`` / ``optimizers`` are dicts keyed by the checkpoint key each is saved under,
    in the order they are loaded and (the optimizers) have their learning rate adjusted."""
    build: typing.Callable                # args -> (modules, optimizers); everything that draws from torch's RNG happens here
    make_step: typing.Callable            # (args, run, modules, optimizers) -> step(*batch, epoch=) -> one loss per name in ``sums``
    layout: typing.Callable               # (args, resumed) -> Layout
    sums: tuple                           # names of the running sums, as logged
    report: typing.Callable               # (epoch, sums, modules): rank 0's prints at the end of an epoch
    backfill: tuple = ()                  # keys a resumed namespace may lack, beyond BACKFILL
    on_resume: typing.Callable = None     # (pickled args, command-line args): what the command line still decides on resume
    announces_resume: bool = False        # the two "=> load..." lines of adapt_trainer.py
    src_input_ch: int = None              # channels of the source batch where they are not --input_ch (None: --input_ch, as for the target)
    lr_adjusted: tuple = None             # keys of the optimizers whose learning rate --adjust_lr adjusts (None: all of them)


Layout = collections.namedtuple("Layout", "pth_dir tflog_dir json_fn model_name")

# switches of this build that a checkpoint written before they existed does not carry
BACKFILL = ("synthetic", "synthetic_raw", "synthetic_len", "src_file_list", "tgt_file_list", "seed", "no_pretrained", "solver", "no_tflog")


def parse_args(parser, argv):
    args = add_additional_params_to_args(parser.parse_args(argv))
    if "tgt_dataset" in vars(args):
        check_src_tgt_ok(args.src_dataset, args.tgt_dataset)
    return args


def resumed_args(trainer, args, cli):
    """the pickled namespace replaces the command line's (adapt_trainer.py:40-43); the command line fills in what it lacks"""
    if trainer.on_resume is not None:
        trainer.on_resume(args, cli)
    for k in trainer.backfill + BACKFILL:
        if k not in vars(args):
            setattr(args, k, getattr(cli, k))
    return args


def model_name(args, *lead):
    return "-".join(lead + (args.savename, args.net) + (("res%s" % args.res,) if args.net in ["fcn", "psp"] else ()))


def adapt_layout(args, resumed, mode_suffix="", method=None):
    mode = "%s-%s2%s-%s_%sch%s" % (args.src_dataset, args.src_split, args.tgt_dataset, args.tgt_split, args.input_ch, mode_suffix)
    name = model_name(args, method or args.method)
    outdir = os.path.join(args.base_outdir, mode)
    return Layout(os.path.join(outdir, "pth"), os.path.join(outdir, "tflog", name),
                  os.path.join(outdir, "param-%s%s.json" % (name, "_resume" if resumed else "")), name)


def checkpoint_fn(layout, epoch):
    return os.path.join(layout.pth_dir, "%s-%s.pth.tar" % (layout.model_name, epoch))


def held(args, modules):
    """the modules a checkpoint holds: all of them, but F2 where ``--uses_one_classifier`` made it F1"""
    one = getattr(args, "uses_one_classifier", False)
    return {key: m for key, m in modules.items() if not (one and key == "f2_state_dict")}


def checkpoint_dict(args, epoch, modules, optimizers):
    dic = {"epoch": epoch, "args": args}
    dic.update((key, m.state_dict()) for key, m in list(held(args, modules).items()) + list(optimizers.items()))
    return dic


def criteria(args, device=None, cross_entropy=CrossEntropyLoss2d):
    """(cross entropy under the class weights, the ``--d_loss`` discrepancy; symkl needs the row length -- the reference passes none
    and fails there)"""
    weight = get_class_weight_from_file(n_class=args.n_class, weight_filename=args.loss_weights_file, add_bg_loss=args.add_bg_loss)
    return cross_entropy(weight if device is None else weight.to(device)), get_prob_distance_criterion(args.d_loss, n_class=args.n_class)


def mcd_report(epoch, sums, modules):
    print("Epoch [%d] DLoss: %.4f CLoss: %.4f" % (epoch, sums["d_loss"], sums["c_loss"]))


def lr_adjusted_optimizers(trainer, optimizers):
    """the optimizers ``--adjust_lr`` touches, in the order they were declared"""
    keys = tuple(optimizers) if trainer.lr_adjusted is None else trainer.lr_adjusted
    return [optimizers[k] for k in keys]


def _resume_or_build(trainer, run, cli):
    if not cli.resume:
        return (cli,) + tuple(trainer.build(cli)) + (0,)
    if trainer.announces_resume:
        print("=> loading checkpoint '{}'".format(cli.resume))
    if not os.path.exists(cli.resume):
        raise OSError("%s does not exist!" % cli.resume)
    checkpoint = load_checkpoint(cli.resume)
    args = resumed_args(trainer, checkpoint["args"], cli)
    modules, optimizers = trainer.build(args)
    for key, m in held(args, modules).items():
        m.load_state_dict(checkpoint[key])
    for m in modules.values():
        m.to(run.device)
    for key, optimizer in optimizers.items():
        optimizer.load_state_dict(checkpoint[key])
    if trainer.announces_resume:
        print("=> loaded checkpoint '{}'".format(args.resume))
    return args, modules, optimizers, checkpoint["epoch"]


def train(trainer, args):
    """``args`` as ``parse_args`` returns them.  ``Run`` seeds torch, then the models are built, then the loader is made: the initial
    weights and the shuffle order depend on that order."""
    run = Run(args)
    resumed = bool(args.resume)
    args, modules, optimizers, start_epoch = _resume_or_build(trainer, run, args)
    if getattr(args, "uses_one_classifier", False) and "f2_state_dict" in modules:
        print("f1 and f2 are same!")
        modules["f2_state_dict"] = modules["f1_state_dict"]

    layout = trainer.layout(args, resumed)
    if run.is_main:
        mkdir_if_not_exist(layout.pth_dir)
    run.configure_logger(layout.tflog_dir, args)
    run.save_params(args, layout.json_fn)

    adapt = "tgt_dataset" in vars(args)  # (source, target) pairs and the per-iteration line, or one dataset
    train_loader = make_loader(args, run, [(args.src_dataset, args.src_split), (args.tgt_dataset, args.tgt_split)] if adapt
                               else [(args.src_dataset, args.split)], src_input_ch=trainer.src_input_ch)
    for m in modules.values():
        m.to(run.device)
    run.sync_replicas(list(modules.values()))
    for m in modules.values():
        m.train()
    if args.no_dropout:
        for m in modules.values():
            fix_dropout_when_training(m)
    if args.fix_bn:
        emphasize_str("BN layers are NOT trained!")
        for m in modules.values():
            fix_batchnorm_when_training(m)
    step = trainer.make_step(args, run, modules, optimizers)
    run._joint = run.joint_transform_args(args, trainer)

    for epoch in range(start_epoch, args.epochs):
        sums = dict.fromkeys(trainer.sums, 0.0)
        it = enumerate(train_loader)
        for ind, batch in (tqdm.tqdm(it) if run.is_main else it):
            source, *targets = batch if adapt else (batch,)
            losses = step(*run.pair(source[0], source[1]), *(run.images(t[0]) for t in targets), epoch=epoch)
            losses = dict(zip(trainer.sums, (float(v) for v in losses)))
            for name, value in losses.items():
                sums[name] += value
            if adapt and ind % 100 == 0 and run.is_main:
                print("iter [%d] DLoss: %.6f CLoss: %.4f" % (ind, losses["d_loss"], losses["c_loss"]))
            if ind > args.max_iter:
                break
        if run.is_main:
            trainer.report(epoch, sums, modules)
        for name in trainer.sums:
            run.log_value(name, sums[name], epoch)
        run.log_value("lr", args.lr, epoch)
        if args.adjust_lr:  # the reference passes weight_decay as the decay rate (adapt_trainer.py:228-230)
            for optimizer in lr_adjusted_optimizers(trainer, optimizers):
                args.lr = adjust_learning_rate(optimizer, args.lr, args.weight_decay, epoch, args.epochs)
        args.start_epoch = epoch + 1
        run.save(checkpoint_dict(args, epoch + 1, modules, optimizers), checkpoint_fn(layout, epoch + 1))
    return 0
