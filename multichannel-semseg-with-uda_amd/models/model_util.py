"""Model / optimizer factory with the reference's names and signatures (models/model_util.py:6-39, 160-310).

The DRN branches -- the ones the MCD hot path uses -- and ``get_models("unet", ..., method="MCD")`` (models/unet.py) are
implemented; every other network name raises ``NotImplementedError`` (the reference's message is kept).  ``get_optimizer('sgd')`` returns the
flat-buffer HIP SGD (``mcdseg.optim.FlatSGD``) and ``get_optimizer('adam')`` the flat-buffer HIP Adam
(``mcdseg.optim.FlatAdam``, betas (0.5, 0.999) as in the reference), state-dict compatible with ``torch.optim.SGD`` /
``torch.optim.Adam``; both sum their gradients over the ranks of a data-parallel run.  ``'adadelta'``, which the
command line cannot select, stays on torch and is not data-parallel.
"""
import os

import torch
from torch import nn
from torch.nn.modules.batchnorm import _BatchNorm

DRN_NAMES = ["drn_c_26", "drn_c_42", "drn_c_58", "drn_d_22", "drn_d_38", "drn_d_54", "drn_d_105"]


def _pretrained_default():
    # the reference always asks for ImageNet weights (a download); MCDSEG_PRETRAINED=0 / --no_pretrained turns it off
    return os.environ.get("MCDSEG_PRETRAINED", "1") != "0"


def _wrap(models, is_data_parallel):
    """``nn.DataParallel`` in the reference is single-process multi-GPU.  This build is one process per GPU
    (RCCL all-reduce inside the optimizer, ``mcdseg.dist``), so the wrapper only has to reproduce the
    ``module.`` prefix of DataParallel checkpoints."""
    if not is_data_parallel:
        return models
    wrap = lambda m: nn.DataParallel(m, device_ids=[torch.cuda.current_device()] if torch.cuda.is_available() else None)
    return [wrap(m) for m in models] if isinstance(models, (list, tuple)) else wrap(models)


def get_full_model(net, res, n_class, input_ch, is_data_parallel=True):
    if "drn" in net:
        from models.dilated_fcn import DRNSeg
        assert net in DRN_NAMES
        model = DRNSeg(net, n_class, input_ch=input_ch, pretrained=_pretrained_default())
    else:
        raise NotImplementedError("Only FCN, SegNet, PSPNet, DRNet, UNet are supported!")
    return _wrap(model, is_data_parallel)


def get_full_uncertain_model(net, res, n_class, input_ch, criterion, is_data_parallel=True, n_dropout=10):
    """models/model_util.py:42-54: ``UncertainDRNSeg`` (DRNSeg + ``up_std`` and the Monte-Carlo dropout loss)"""
    if "drn" in net:
        from models.dilated_fcn import UncertainDRNSeg
        assert net in DRN_NAMES
        model = UncertainDRNSeg(net, n_class, input_ch=input_ch, n_dropout_exp=n_dropout, criterion=criterion,
                                pretrained=_pretrained_default())
    else:
        raise NotImplementedError("Only FCN, SegNet, PSPNet, DRNet, UNet are supported!")
    return _wrap(model, is_data_parallel)


def get_models(net_name, input_ch, n_class, res="50", method="MCD", is_data_parallel=False):
    if net_name == "unet":
        # models/model_util.py:205-210 of the reference: the U-Net generator and two of its classifiers at the default feature_scale
        if method != "MCD":
            raise NotImplementedError("the U-Net (%s) is built for method \"MCD\" only (the MFNet U-Net, MultiUNetClassifier, is not), "
                                      "got %r" % (net_name, method))
        from models.unet import UNetBase, UNetClassifier
        return _wrap([UNetBase(input_ch=input_ch), UNetClassifier(n_classes=n_class), UNetClassifier(n_classes=n_class)], is_data_parallel)
    if "drn" not in net_name:
        raise NotImplementedError("Only FCN (Including Dilated FCN), SegNet, PSPNet UNet are supported!")
    from models.dilated_fcn import (DRNSegBase, DRNSegPixelClassifier, FuseDRNSegBase, FusionDRNSegPixelClassifier,
                                    ScoreFusionDRNSegPixelClassifier)
    ver = "ver2" if "ver2" in net_name else "ver1"
    drn_name = net_name.replace("_ver2", "")
    pre = _pretrained_default()
    if "fusenet" in net_name:
        # middle fusion (models/model_util.py:187-195): one siamese DRN-D generator on RGB and HHA, the plain classifiers
        if method != "MCD":
            raise NotImplementedError("the FuseNet-style generator (%s) is built for method \"MCD\" only, got %r" % (net_name, method))
        if ver == "ver2":
            raise NotImplementedError("%s: there is no ver2 FuseNet-style generator (the reference looks up a constructor that does "
                                      "not exist)" % net_name)
        model_g = FuseDRNSegBase(model_name=drn_name.replace("_fusenet", ""), n_class=n_class, input_ch=input_ch, pretrained=pre)
        return _wrap([model_g, DRNSegPixelClassifier(n_class=n_class), DRNSegPixelClassifier(n_class=n_class)], is_data_parallel)
    if method == "MCD":
        model_list = [DRNSegBase(model_name=drn_name, n_class=n_class, input_ch=input_ch, ver=ver, pretrained=pre),
                      DRNSegPixelClassifier(n_class=n_class, ver=ver), DRNSegPixelClassifier(n_class=n_class, ver=ver)]
    elif "MFNet" in method:
        assert input_ch in [4, 6]
        fusion_type = method.split("-")[-1]
        print("fusion type: %s" % fusion_type)
        g3 = DRNSegBase(model_name=drn_name, n_class=n_class, input_ch=3, ver=ver, pretrained=pre)
        g1 = DRNSegBase(model_name=drn_name, n_class=n_class, input_ch=input_ch - 3, ver=ver, pretrained=pre)
        if "score" in method.lower():
            print("Score Fusion!!!")
            fs = [ScoreFusionDRNSegPixelClassifier(fusion_type=fusion_type, n_class=n_class) for _ in range(2)]
        else:
            fs = [FusionDRNSegPixelClassifier(fusion_type=fusion_type, n_class=n_class, ver=ver) for _ in range(2)]
        model_list = [g3, g1] + fs
    else:
        return NotImplementedError("Sorry... Only MCD is supported!")  # returned, not raised: models/model_util.py:281
    return _wrap(model_list, is_data_parallel)


def get_dann_models(net_name, input_ch, n_class, img_shape, res="50"):
    """G, F and the domain classifier D of the DANN baseline (dann_trainer.py:132-141 of the reference); D's ``fc1`` is as wide as G's
    score map at ``img_shape`` makes it (models/dilated_fcn.domain_fc_in; 1089, the reference's constant, at 1080 x 1080)."""
    if "drn" not in net_name:
        raise NotImplementedError("Only FCN, SegNet, PSPNet are supported!")  # (the reference's text, dann_trainer.py:141)
    from models.dilated_fcn import DRNSegBase, DRNSegDomainClassifier, DRNSegPixelClassifier, domain_fc_in
    assert net_name in DRN_NAMES
    model_g = DRNSegBase(model_name=net_name, n_class=n_class, input_ch=input_ch, pretrained=_pretrained_default())
    return model_g, DRNSegPixelClassifier(n_class=n_class), DRNSegDomainClassifier(n_class=n_class, fc_in=domain_fc_in(model_g, img_shape))


def get_multitask_models(net_name, input_ch, n_class, semseg_criterion=None, discrepancy_criterion=None,
                         is_data_parallel=False, is_src_only=False):
    """RGB encoder + MCD multitask decoder (models/model_util.py:81-99); the source-only decoder variant is not on
    the hot path."""
    if "drn" not in net_name:
        raise NotImplementedError("Only FCN (Including Dilated FCN), SegNet, PSPNet UNet are supported!")
    if is_src_only:
        raise NotImplementedError("MultiTaskDecoder (source-only) is outside the MCD hot path")
    from models.dilated_fcn import MCDMultiTaskDecoder, MultiTaskEncoder
    model_enc = MultiTaskEncoder(model_name=net_name, input_ch=3, pretrained=_pretrained_default())  # RGB is 3 channel
    model_dec = MCDMultiTaskDecoder(n_class=n_class, depth_ch=input_ch - 3, semseg_criterion=semseg_criterion,
                                    discrepancy_criterion=discrepancy_criterion)
    if is_data_parallel:
        return _wrap(model_enc, True), _wrap(model_dec, True)
    return model_enc, model_dec


def get_segbd_multitask_models(net_name, input_ch, n_class, semseg_criterion=None, discrepancy_criterion=None,
                               is_data_parallel=False, semseg_shortcut=False, depth_shortcut=False,
                               add_pred_seg_boundary_loss=False, is_src_only=False, use_seg2bd_conv=False):
    """Stage-tap RGB encoder + segmentation / boundary decoder (models/model_util.py:102-127).  ``input_ch`` is ignored as in the
    reference: the encoder always takes the 3 RGB channels and the decoder has no depth head."""
    if "drn" not in net_name:
        raise NotImplementedError("Only FCN (Including Dilated FCN), SegNet, PSPNet UNet are supported!")
    if is_src_only:
        raise NotImplementedError("the source-only seg + boundary decoder is outside the MCD hot path")
    from models.dilated_fcn import MCDSegBDMultiTaskDecoder, MultiTaskEncoderReturningMultipleFeaturemaps
    model_enc = MultiTaskEncoderReturningMultipleFeaturemaps(model_name=net_name, input_ch=3, pretrained=_pretrained_default())
    model_dec = MCDSegBDMultiTaskDecoder(n_class=n_class, depth_ch=3, semseg_criterion=semseg_criterion,
                                         discrepancy_criterion=discrepancy_criterion, semseg_shortcut=semseg_shortcut,
                                         depth_shortcut=depth_shortcut, add_pred_seg_boundary_loss=add_pred_seg_boundary_loss,
                                         use_seg2bd_conv=use_seg2bd_conv)
    if is_data_parallel:
        return _wrap(model_enc, True), _wrap(model_dec, True)
    return model_enc, model_dec


def get_triple_multitask_models(net_name, input_ch, n_class, semseg_criterion=None, discrepancy_criterion=None,
                                is_data_parallel=False, semseg_shortcut=False, depth_shortcut=False,
                                add_pred_seg_boundary_loss=False, is_src_only=False, use_seg2bd_conv=False):
    """Stage-tap RGB encoder + segmentation / depth / boundary decoder (models/model_util.py:102-130).  ``input_ch`` is ignored as in
    the reference: the encoder always takes the 3 RGB channels and the depth head always regresses 3 (HHA) channels."""
    if "drn" not in net_name:
        raise NotImplementedError("Only FCN (Including Dilated FCN), SegNet, PSPNet UNet are supported!")
    if is_src_only:
        raise NotImplementedError("the source-only triple decoder (TripleMultiTaskDecoder) is outside the MCD hot path")
    from models.dilated_fcn import MCDTripleMultiTaskDecoder, MultiTaskEncoderReturningMultipleFeaturemaps
    model_enc = MultiTaskEncoderReturningMultipleFeaturemaps(model_name=net_name, input_ch=3, pretrained=_pretrained_default())
    model_dec = MCDTripleMultiTaskDecoder(n_class=n_class, depth_ch=3, semseg_criterion=semseg_criterion,
                                          discrepancy_criterion=discrepancy_criterion, semseg_shortcut=semseg_shortcut,
                                          depth_shortcut=depth_shortcut, add_pred_seg_boundary_loss=add_pred_seg_boundary_loss,
                                          use_seg2bd_conv=use_seg2bd_conv)
    if is_data_parallel:
        return _wrap(model_enc, True), _wrap(model_dec, True)
    return model_enc, model_dec


def get_optimizer(model_parameters, opt, lr, momentum, weight_decay):
    params = [p for p in model_parameters if p.requires_grad]
    if opt == "sgd":
        from mcdseg.optim import FlatSGD
        return FlatSGD(params, lr=lr, momentum=momentum, weight_decay=weight_decay)
    elif opt == "adadelta":
        return torch.optim.Adadelta(params, lr=lr, weight_decay=weight_decay)
    elif opt == "adam":
        from mcdseg.optim import FlatAdam
        return FlatAdam(params, lr=lr, betas=(0.5, 0.999), weight_decay=weight_decay)
    raise NotImplementedError("Only (Momentum) SGD, Adadelta, Adam are supported!")


def fix_batchnorm_when_training(model):
    if issubclass(type(model), _BatchNorm):
        model.training = False
    for module in model.children():
        fix_batchnorm_when_training(module)


def fix_dropout_when_training(model):
    if type(model) in [nn.Dropout, nn.Dropout2d, nn.Dropout3d, nn.AlphaDropout]:
        model.training = False
        print("Fixed one dropout layer")
    for module in model.children():
        fix_dropout_when_training(module)


def check_training(model):
    print(type(model))
    print(model.training)
    for module in model.children():
        check_training(module)
