#!/usr/bin/env python3
"""MCD + depth-regression + boundary-detection multitask trainer -- the reference's ``adapt_triple_multitask_trainer.py`` (:24-330) on
the MI355X HIP kernels: stage-tap RGB encoder, two segmentation decoders, an HHA-regression decoder and a HED-style boundary head with
three learned task weights.  The SOURCE batch has 7 channels (RGB, HHA, a {0,1} boundary plane; ``input_ch=7``, :139-140), the target
``--input_ch``.  ``--use_seg2bd_conv`` adds a 5x5 convolution on the segmentation logits whose sigmoid is trained with the balanced BCE
(``ops.seg2bd_bce``: from the 1/8-resolution logits, no full-resolution C-channel tensor).  Under data parallelism each rank balances its
boundary losses with the beta of its own batch, as the reference's local loss does.

    python adapt_triple_multitask_trainer.py suncg nyu --input_ch 6 -b 8 --synthetic --no_pretrained --use_seg2bd_conv

7-channel raw uint8 batches (``--synthetic_raw``) and file lists are refused: the device input pipeline and the file-list loader have no
boundary column.
"""
from adapt_segbd_multitask_trainer import SEGBD_FLAGS, get_parser, on_resume
from models.model_util import get_optimizer, get_triple_multitask_models
from solvers.solver import TripleMultiTaskMCDSolver
from trainer_common import Trainer, adapt_layout, criteria, mcd_report, parse_args, train

SUMS = ("c_loss", "d_loss", "src_semseg_loss", "src_depth_loss", "tgt_depth_loss", "src_boundary_loss", "tgt_psuedo_boundary_loss",
        "src_extra_boundary_loss")


def build(args):
    criterion, criterion_d = criteria(args)  # built before the models, which keep them as buffers
    model_enc, model_dec = get_triple_multitask_models(net_name=args.net, input_ch=args.input_ch, n_class=args.n_class,
                                                       is_data_parallel=args.is_data_parallel, semseg_criterion=criterion,
                                                       discrepancy_criterion=criterion_d, depth_shortcut=args.depth_shortcut,
                                                       semseg_shortcut=args.semseg_shortcut,
                                                       add_pred_seg_boundary_loss=args.add_pred_seg_boundary_loss,
                                                       use_seg2bd_conv=args.use_seg2bd_conv)
    optimizer_enc = get_optimizer(model_enc.parameters(), lr=args.lr, momentum=args.momentum, opt=args.opt,
                                  weight_decay=args.weight_decay)
    optimizer_dec = get_optimizer(model_dec.parameters(), opt=args.opt, lr=args.lr, momentum=args.momentum,
                                  weight_decay=args.weight_decay)
    return ({"enc_state_dict": model_enc, "dec_state_dict": model_dec}, {"optimizer_enc": optimizer_enc, "optimizer_dec": optimizer_dec})


def make_step(args, run, modules, optimizers):
    enc, dec = (m.module if hasattr(m, "module") else m for m in modules.values())  # the solver takes the unwrapped modules
    solver = TripleMultiTaskMCDSolver(enc, dec, *optimizers.values(), num_k=args.num_k, num_multiply_d_loss=args.num_multiply_d_loss,
                                      add_pred_seg_boundary_loss=args.add_pred_seg_boundary_loss, use_seg2bd_conv=args.use_seg2bd_conv,
                                      boundary_loss_converging_epoch=args.boundary_loss_converging_epoch, scale_bd_loss=args.scale_bd_loss)

    def step(src_imgs, src_gt, tgt_imgs, epoch):
        c_loss, d_loss, parts = solver.step(src_imgs, src_gt, tgt_imgs, epoch=epoch)
        return (c_loss, d_loss) + tuple(parts)
    return step


def report(epoch, sums, modules):
    mcd_report(epoch, sums, modules)
    print("SrcSemsegLoss: %.4f, SrcDepthLoss: %.4f, TgtDepthLoss: %.4f , SrcBoundaryLoss: %.4f  SrcExtraBoundaryLoss: %.4f"
          % (sums["src_semseg_loss"], sums["src_depth_loss"], sums["tgt_depth_loss"], sums["src_boundary_loss"],
             sums["src_extra_boundary_loss"]))


def check_inputs(args):
    """what this trainer cannot be fed"""
    if getattr(args, "synthetic_raw", False):
        raise SystemExit("adapt_triple_multitask_trainer: --synthetic_raw is not available here -- the source batch carries a boundary "
                         "plane as its 7th channel, and the device input pipeline has no boundary column; use --synthetic")
    if getattr(args, "src_file_list", None) or getattr(args, "tgt_file_list", None):
        raise SystemExit("adapt_triple_multitask_trainer: --src_file_list / --tgt_file_list are not available here -- the file-list "
                         "loader has no boundary column for the 7-channel source batch; use --synthetic")
    if args.input_ch != 6 and not args.resume:  # (a resumed run takes the checkpoint's arguments, which went through here)
        raise SystemExit("adapt_triple_multitask_trainer: --input_ch must be 6 -- the target's three channels behind RGB are the target of "
                         "the 3-channel depth head")
    return args


TRAINER = Trainer(build=build, make_step=make_step, report=report, backfill=SEGBD_FLAGS, on_resume=on_resume, sums=SUMS, src_input_ch=7,
                  layout=lambda args, resumed: adapt_layout(args, resumed, "_MCD_triple_multitask"), announces_resume=True)


def main(argv=None):
    return train(TRAINER, check_inputs(parse_args(get_parser(), argv)))


if __name__ == "__main__":
    main()
