"""U-Net generator and classifiers (``--net unet``) on the MI355X HIP kernels.

Counterpart of the reference's ``models/unet.py`` (``UNetConv`` :6-26, ``UNetUp`` :29-43, ``UNetBase`` :122-171, ``UNetClassifier``
:174-199): the module tree -- and therefore every ``state_dict`` key and shape, and torch's default initialisation -- is the
reference's; the arithmetic is not torch's:

  * a ``nn.Sequential(Conv2d, BatchNorm2d, ReLU)`` holder runs as one fused group (``mcdseg.ops.conv_bn_act(x, seq[0], seq[1])``, the
    way ``models.drn._project`` runs a projection shortcut's holder); these convolutions have a bias, unlike a DRN's;
  * ``nn.MaxPool2d(kernel_size=2)`` is ``ops.max_pool2``, which also writes what the next convolution gathers;
  * ``UNetUp`` is ``ops.up_join`` (the 2x2 stride-2 up-convolution written straight into the upper channel slice of the concatenation
    buffer), then ``ops.conv2d_bias`` + ``ops.relu`` twice.

Built for the case the trainers use.  Refused, before anything is launched: an input whose H or W is no multiple of 16 (the reference
pads or crops the shortcut by ``offset // 2``; at multiples of 16 the offset is 0), ``is_deconv=False`` (bilinear up-sampling), and
``MCDSEG_ACT_STORAGE=compact``.  The MFNet classifier (``MultiUNetClassifier``) and the one-piece ``UNet`` are not built.
"""
import torch.nn as nn

from mcdseg import ops
from models.drn import BatchNorm2d, Conv2d

__all__ = ["UNetConv", "UNetUp", "UNetBase", "UNetClassifier"]

FILTERS = (64, 128, 256, 512, 1024)


def _filters(feature_scale):
    return [int(x / feature_scale) for x in FILTERS]


def _refuse_compact(who):
    if ops.ACT_STORAGE == "compact":
        raise NotImplementedError("%s hands out the fp32 outputs of its stages: it does not run with MCDSEG_ACT_STORAGE=compact (nor "
                                  "the 2-byte chain built on it); use fp32 storage" % who)


def _need_deconv(is_deconv):
    if not is_deconv:
        raise NotImplementedError("mcdseg U-Net: is_deconv=False (nn.UpsamplingBilinear2d in UNetUp) is not built; only the learned "
                                  "2x2 stride-2 up-convolution is")


class UNetConv(nn.Module):
    def __init__(self, in_size, out_size, is_batchnorm):
        super().__init__()
        self.is_batchnorm = bool(is_batchnorm)
        if is_batchnorm:
            self.conv1 = nn.Sequential(Conv2d(in_size, out_size, 3, 1, 1), BatchNorm2d(out_size), nn.ReLU())
            self.conv2 = nn.Sequential(Conv2d(out_size, out_size, 3, 1, 1), BatchNorm2d(out_size), nn.ReLU())
        else:
            self.conv1 = nn.Sequential(Conv2d(in_size, out_size, 3, 1, 1), nn.ReLU())
            self.conv2 = nn.Sequential(Conv2d(out_size, out_size, 3, 1, 1), nn.ReLU())

    def forward(self, inputs, feeds=None):
        """``feeds``: the convolution that reads the result, if one does -- a ReLU writes the pre-split companion of its output only for
        a convolution that will read it (``ops.conv_reads_companion``)"""
        if self.is_batchnorm:  # two fused groups, each the holder's (Conv2d, BatchNorm2d) + ReLU
            h = ops.conv_bn_act(inputs, self.conv1[0], self.conv1[1], relu=True)
            return ops.conv_bn_act(h, self.conv2[0], self.conv2[1], relu=True)
        h = ops.conv2d_bias(inputs, self.conv1[0])
        h = ops.conv2d_bias(ops.relu(h, companion=ops.conv_reads_companion(self.conv2[0], h.shape)), self.conv2[0])
        return ops.relu(h, companion=feeds is not None and ops.conv_reads_companion(feeds, h.shape))


class UNetUp(nn.Module):
    def __init__(self, in_size, out_size, is_deconv):
        super().__init__()
        _need_deconv(is_deconv)
        self.conv = UNetConv(in_size, out_size, False)
        self.up = nn.ConvTranspose2d(in_size, out_size, kernel_size=2, stride=2)

    def forward(self, shortcut, h, feeds=None):
        if shortcut.shape[2] != 2 * h.shape[2] or shortcut.shape[3] != 2 * h.shape[3]:
            raise ValueError("mcdseg UNetUp: the shortcut must be twice the size of h (padding or cropping it is not built), got %s and %s"
                             % (tuple(shortcut.shape), tuple(h.shape)))
        first = self.conv.conv1[0]
        joined = (shortcut.shape[0], shortcut.shape[1] + self.up.out_channels, shortcut.shape[2], shortcut.shape[3])
        return self.conv(ops.up_join(shortcut, h, self.up.weight, self.up.bias, companion=ops.conv_reads_companion(first, joined)), feeds)


def _check_input(x, who):
    _refuse_compact(who)
    if x.dim() != 4 or x.shape[2] % 16 or x.shape[3] % 16:
        raise ValueError("%s: H and W must be multiples of 16 (four 2x2 poolings; the reference pads or crops the shortcuts otherwise, "
                         "which is not built), got %s" % (who, tuple(x.shape)))


class UNetBase(nn.Module):
    def __init__(self, feature_scale=4, is_deconv=True, input_ch=3, is_batchnorm=True):
        super().__init__()
        _need_deconv(is_deconv)
        self.is_deconv = is_deconv
        self.input_ch = input_ch
        self.is_batchnorm = is_batchnorm
        self.feature_scale = feature_scale
        filters = _filters(feature_scale)

        self.conv1 = UNetConv(self.input_ch, filters[0], self.is_batchnorm)
        self.maxpool1 = nn.MaxPool2d(kernel_size=2)
        self.conv2 = UNetConv(filters[0], filters[1], self.is_batchnorm)
        self.maxpool2 = nn.MaxPool2d(kernel_size=2)
        self.conv3 = UNetConv(filters[1], filters[2], self.is_batchnorm)
        self.maxpool3 = nn.MaxPool2d(kernel_size=2)
        self.conv4 = UNetConv(filters[2], filters[3], self.is_batchnorm)
        self.maxpool4 = nn.MaxPool2d(kernel_size=2)
        self.center = UNetConv(filters[3], filters[4], self.is_batchnorm)

    @staticmethod
    def _pool(x, block):
        """the pool in front of ``block``, whose first convolution is its one reader"""
        n, c, h, w = x.shape
        return ops.max_pool2(x, companion=ops.conv_reads_companion(block.conv1[0], (n, c, h // 2, w // 2)))

    def forward(self, inputs):
        _check_input(inputs, "UNetBase")
        # each conv_k feeds the pool AND the classifiers' joins: its gradient has two producers (per classifier), summed by autograd
        conv1 = self.conv1(inputs)
        conv2 = self.conv2(self._pool(conv1, self.conv2))
        conv3 = self.conv3(self._pool(conv2, self.conv3))
        conv4 = self.conv4(self._pool(conv3, self.conv4))
        center = self.center(self._pool(conv4, self.center))
        return {"center": center, "conv1": conv1, "conv2": conv2, "conv3": conv3, "conv4": conv4}


class UNetClassifier(nn.Module):
    def __init__(self, feature_scale=4, n_classes=21, is_deconv=True):
        super().__init__()
        _need_deconv(is_deconv)
        self.is_deconv = is_deconv
        self.feature_scale = feature_scale
        filters = _filters(feature_scale)

        self.up_concat4 = UNetUp(filters[4], filters[3], self.is_deconv)
        self.up_concat3 = UNetUp(filters[3], filters[2], self.is_deconv)
        self.up_concat2 = UNetUp(filters[2], filters[1], self.is_deconv)
        self.up_concat1 = UNetUp(filters[1], filters[0], self.is_deconv)

        self.final = Conv2d(filters[0], n_classes, 1)

    def forward(self, inputs):
        _check_input(inputs["conv1"], "UNetClassifier")
        up4 = self.up_concat4(inputs["conv4"], inputs["center"])
        up3 = self.up_concat3(inputs["conv3"], up4)
        up2 = self.up_concat2(inputs["conv2"], up3)
        up1 = self.up_concat1(inputs["conv1"], up2, feeds=self.final)  # (up4 .. up2 feed the next join, which reads fp32)
        return self.final(up1)
