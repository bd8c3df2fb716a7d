"""Dataset layer of the hot path.

The reference reads nine on-disk datasets from hard-coded lab paths (datasets.py:981-992); none of that is
on the MI355X path.  What the trainers need from it is kept with the reference's names and values --
``AVAILABLE_DATASET_LIST``, ``get_n_class`` (:1011-1024), ``get_img_shape`` (:1027-1043, W,H order),
``ConcatDataset`` (:20-28), ``check_src_tgt_ok`` (:1004-1008) -- plus ``SyntheticRGBD``, the seeded
stand-in the BASELINE configs run on: N(0,1) images in place of ImageNet-normalised
RGB+HHA (transform.py:307) and uniform labels with class n_class-1 as the zero-weight background
(transform.py:319-325 maps 255 there) -- and ``FileListRGBD``, a loader for real data: image / HHA / label files named in a list
are opened with PIL (``default_loader``, datasets.py:20-28) and handed over as raw uint8 arrays; everything the reference's
transforms then do (Scale, ToTensor, Normalize, ToLabel, ReLabel; transform.py:302-325) runs on the MI355X
(``DeviceInputPipeline``).
"""
import numpy as np
import torch
from torch.utils import data

AVAILABLE_DATASET_LIST = ["gta", "city", "test", "ir", "city16", "synthia", "2d3d", "sun", "suncg", "nyu"]

_IMG_SIZE = {  # (W, H) class constants of the reference's dataset classes
    "gta": [1280, 720], "synthia": [1280, 760], "city": [2048, 1024], "city16": [2048, 1024], "ir": [640, 480],
    "2d3d": [1080, 1080], "sun": [640, 480], "suncg": [640, 480], "nyu": [640, 480],
}


class ConcatDataset(data.Dataset):
    def __init__(self, *datasets):
        self.datasets = datasets

    def __getitem__(self, i):
        return tuple(d[i] for d in self.datasets)

    def __len__(self):
        return min(len(d) for d in self.datasets)


class SyntheticRGBD(data.Dataset):
    """(image [C,H,W] fp32, label [H,W] int64) generated from (seed, index).

    ``raw=True`` yields what a loader holds BEFORE the reference's transforms: a uint8 [H,W,C] image (RGB then HHA
    bytes) and a uint8 label map whose background pixels carry ``background_id`` -- the trainer then runs
    ToTensor/Normalize/ReLabel on the MI355X (``DeviceInputPipeline``).

    ``input_ch == 7`` is the triple multitask trainer's source (RGB, HHA, boundary): the draw is the same, then channel 6 is overwritten
    with the 0/1 boundary of the sample's own label map (3x3 dilation != 3x3 erosion), the {0,1} plane the reference's loader yields there
    (datasets.py:680-695).  There is no raw form of it."""

    def __init__(self, length, input_ch, img_shape_wh, n_class, seed, test=False, raw=False, background_id=255):
        self.length, self.ch, self.n_class, self.seed, self.test = length, input_ch, n_class, seed, test
        self.w, self.h = int(img_shape_wh[0]), int(img_shape_wh[1])
        self.raw, self.background_id = raw, background_id
        if raw and input_ch == 7:
            raise NotImplementedError("SyntheticRGBD: the 7-channel (RGB, HHA, boundary) sample has no raw uint8 form -- "
                                      "DeviceInputPipeline has no boundary column")

    def __len__(self):
        return self.length

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed * 1000003 + i)
        if self.raw:
            img = torch.randint(0, 256, (self.h, self.w, self.ch), generator=g, dtype=torch.uint8)
            lbl = torch.randint(0, self.n_class, (self.h, self.w), generator=g, dtype=torch.int64)
            lbl = torch.where(lbl == self.n_class - 1, torch.full_like(lbl, self.background_id), lbl).to(torch.uint8)
        else:
            img = torch.randn(self.ch, self.h, self.w, generator=g)
            lbl = torch.randint(0, self.n_class, (self.h, self.w), generator=g, dtype=torch.int64)
            if self.ch == 7:
                v = lbl.float()[None, None]
                pool = torch.nn.functional.max_pool2d
                img[6] = (pool(v, kernel_size=3, stride=1, padding=1) != -pool(-v, kernel_size=3, stride=1, padding=1))[0, 0].float()
        if self.test:
            return img, lbl, "synthetic_%06d.png" % i
        return img, lbl


IMAGENET_MEAN = [.485, .456, .406, .485, .485, .485]  # 6-channel RGB+HHA statistics of transform.py:307
IMAGENET_STD = [.229, .224, .225, .229, .229, .229]
CITY_MEAN = [0.290101, 0.328081, 0.286964]            # transform.py:311
CITY_STD = [0.182954, 0.186566, 0.184475]


def default_loader(path):
    """datasets.py:27-28 of the reference"""
    from PIL import Image
    return Image.open(path)


class FileListRGBD(data.Dataset):
    """Real data for the trainers: ``list_file`` has one sample per line, ``rgb_path [hha_path] label_path`` (whitespace
    separated; relative paths are taken from the list's directory).  ``__getitem__`` returns what the reference's loaders hold
    BEFORE their transforms -- a uint8 [H,W,3 or 6] image (RGB, then HHA) and a uint8 [H,W] label map straight from the PNGs
    (``default_loader``; palette / grey label PNGs are read as their index / grey values, as ``ToLabel`` sees them) -- so that
    resize, normalisation and relabelling run on the device.  All files of one list must share one size (batches are stacked)."""

    def __init__(self, list_file, input_ch=6, test=False):
        import os
        self.root = os.path.dirname(os.path.abspath(list_file))
        self.items = []
        for line in open(list_file):
            parts = line.split()
            if not parts or parts[0].startswith("#"):
                continue
            if len(parts) not in (2, 3):
                raise ValueError("FileListRGBD: expected 'rgb [hha] label' per line, got %r" % line)
            self.items.append([p if os.path.isabs(p) else os.path.join(self.root, p) for p in parts])
        if not self.items:
            raise ValueError("FileListRGBD: %s names no samples" % list_file)
        self.input_ch, self.test = input_ch, test
        if input_ch > 3 and any(len(it) != 3 for it in self.items):
            raise ValueError("FileListRGBD: input_ch=%d needs an HHA / depth file per sample" % input_ch)

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        it = self.items[i]
        rgb = np.array(default_loader(it[0]).convert("RGB"), dtype=np.uint8)
        if self.input_ch > 3:
            extra = default_loader(it[1])
            extra = np.array(extra.convert("RGB") if self.input_ch == 6 else extra.convert("L"), dtype=np.uint8)
            extra = extra.reshape(extra.shape[0], extra.shape[1], -1)[:, :, :self.input_ch - 3]
            img = np.concatenate([rgb, extra], axis=2)
        else:
            img = rgb[:, :, :self.input_ch]
        lbl = np.array(default_loader(it[-1]), dtype=np.uint8)  # mode "P" / "L": the class indices themselves
        if lbl.ndim != 2:
            raise ValueError("FileListRGBD: label image %s is not single-channel" % it[-1])
        out = (torch.from_numpy(np.ascontiguousarray(img)), torch.from_numpy(np.ascontiguousarray(lbl)))
        return out + (it[-1],) if self.test else out


class DeviceInputPipeline(object):
    """``get_img_transform`` / ``get_lbl_transform`` (transform.py:302-325) on the GPU: pinned uint8 batches go over PCIe as
    bytes (4x fewer than fp32); ``Scale`` (bilinear for images, nearest for label maps: Pillow's 8-bit arithmetic, bit for bit),
    ToTensor+Normalize (HWC->NCHW) and ToLabel+ReLabel(background_id -> n_class-1) each are one kernel.  ``img_shape`` = (W, H)
    as the reference passes it to ``Scale``; None leaves the size alone (the loader already produced it).

    ``crop_size > 0`` puts ``get_joint_transform(crop_size, rotate_angle)`` (joint_transforms.py:248-255: random flip, rotation, crop of
    image and label map together) in front, and -- ``use_crop`` of transform.py:302-325 -- drops ``Scale``.  The draw happens on the
    host (``mcdseg.augment.JointTransform``, seeded with ``seed``); flip, rotation, crop and the ToTensor+Normalize / ToLabel+ReLabel
    behind them are ONE gather kernel per tensor, whose bytes equal Pillow's.  One draw serves every image part and the label map of a
    sample (``joint``); ``images`` / ``labels`` called on their own draw afresh (a target batch: the reference transforms the source
    and the target dataset independently).  The rotation fills label maps with class 0, as the reference's ``mask.rotate`` does -- a
    real class, not the background id.  ``crop_size <= 0``: no joint transform at all, also with ``rotate_angle`` set."""

    def __init__(self, input_ch, n_class, device, normalize_way="imagenet", background_id=255, img_shape=None, crop_size=-1,
                 rotate_angle=0, seed=None):
        from mcdseg import augment, ops
        self._ops = ops
        self.input_ch, self.n_class, self.device, self.background_id = input_ch, n_class, device, background_id
        self.joint_transform = augment.get_joint_transform(crop_size, rotate_angle, seed)
        if self.joint_transform is not None:
            img_shape = None  # use_crop: no Scale
        self.img_shape = None if img_shape is None else (int(img_shape[0]), int(img_shape[1]))
        if normalize_way == "imagenet":
            mean, std = IMAGENET_MEAN[:input_ch], IMAGENET_STD[:input_ch]
        elif normalize_way == "city":
            mean, std = CITY_MEAN[:input_ch], CITY_STD[:input_ch]
        else:  # "No normalization..." (transform.py:314-315): ToTensor only
            mean, std = [0.0] * input_ch, [1.0] * input_ch
        self.mean = torch.tensor(mean, dtype=torch.float32, device=device)
        self.std = torch.tensor(std, dtype=torch.float32, device=device)

    def draw(self, n, h, w):
        """the joint transform's parameter tables for a batch of n samples of h x w pixels (None without a joint transform)"""
        return None if self.joint_transform is None else self.joint_transform.draw(n, h, w)

    def joint(self, parts, lbl_u8):
        """image parts and label map of ONE batch under one draw per sample -> (fp32 images, int64 labels)"""
        parts = parts if isinstance(parts, (list, tuple)) else [parts]
        params = self.draw(*lbl_u8.shape[:3])
        return self.images(*parts, params=params), self.labels(lbl_u8, params=params)

    def images(self, *parts, params=None):
        """one or more uint8 [N,H,W,c_i] tensors (e.g. RGB and HHA) -> fp32 [N, sum c_i, H, W] ([N, sum c_i, crop, crop] under
        the joint transform; ``params``: the draw to use, default a fresh one)"""
        parts = [p.to(self.device, non_blocking=True) for p in parts]
        if self.joint_transform is not None:
            params = params if params is not None else self.draw(*parts[0].shape[:3])
            n, c = parts[0].shape[0], sum(p.shape[3] for p in parts)
            oh, ow = params.out_hw if params.resize_to is None else (params.resize_to[1], params.resize_to[0])
            out = torch.empty((n, c, oh, ow), dtype=torch.float32, device=self.device)
            off = 0
            for p in parts:
                mean, std = self.mean[off:off + p.shape[3]], self.std[off:off + p.shape[3]]
                if params.resize_to is None:
                    self._ops.joint_augment_normalize_u8_(out, p, params, mean, std, c_off=off)
                else:  # the image is smaller than the crop: RandomCrop resizes (joint_transforms.py:38-39)
                    u8 = self._ops.resize_u8(self._ops.joint_augment_u8(p, params, params.out_hw), params.resize_to)
                    self._ops.normalize_u8_(out, u8, mean, std, c_off=off)
                off += p.shape[3]
            return out
        if self.img_shape is not None:
            parts = [self._ops.resize_u8(p, self.img_shape) for p in parts]
        n, h, w = parts[0].shape[:3]
        c = sum(p.shape[3] for p in parts)
        out = torch.empty((n, c, h, w), dtype=torch.float32, device=self.device)
        off = 0
        for p in parts:
            self._ops.normalize_u8_(out, p, self.mean[off:off + p.shape[3]], self.std[off:off + p.shape[3]], c_off=off)
            off += p.shape[3]
        return out

    def hha(self, depth, camera, unit_m=None, fill_rgb=None, **fill_kw):
        """the HHA part of a depth batch [N,H,W] (``ops.depth_to_hha``: DESIGN.md section 4.13), uint8 [N,H,W,3] on the device:
        ``images(rgb_u8, pipeline.hha(depth, camera, unit_m))`` is the whole 6-channel input path.  With ``fill_rgb`` (the uint8 RGB
        batch [N,H,W,3] of the same frames) the depth's holes are inpainted first (``ops.fill_depth``: section 4.16; ``fill_kw`` are its
        solver arguments) and the filled centimetres are encoded, all on the device."""
        depth = depth.to(self.device, non_blocking=True)
        if fill_rgb is None:
            if fill_kw:
                raise TypeError("DeviceInputPipeline.hha: %s given without fill_rgb" % sorted(fill_kw))
            return self._ops.depth_to_hha(depth, camera, unit_m)
        if fill_kw.get("return_parts"):
            raise TypeError("DeviceInputPipeline.hha returns the HHA part alone: call ops.fill_depth for the solver's parts")
        filled = self._ops.fill_depth(fill_rgb.to(self.device, non_blocking=True), depth, unit_m, **fill_kw)
        return self._ops.depth_to_hha(filled, camera)

    def labels(self, lbl_u8, params=None):
        lbl_u8 = lbl_u8.to(self.device, non_blocking=True)
        if self.joint_transform is not None:
            params = params if params is not None else self.draw(*lbl_u8.shape[:3])
            if params.resize_to is None:
                return self._ops.joint_augment_relabel_u8(lbl_u8, params, params.out_hw, self.background_id, self.n_class - 1)
            u8 = self._ops.resize_u8(self._ops.joint_augment_u8(lbl_u8, params, params.out_hw, nearest=True), params.resize_to, nearest=True)
            return self._ops.relabel_u8(u8, self.background_id, self.n_class - 1)
        if self.img_shape is not None:
            lbl_u8 = self._ops.resize_u8(lbl_u8, self.img_shape, nearest=True)
        return self._ops.relabel_u8(lbl_u8, self.background_id, self.n_class - 1)


def get_dataset(dataset_name, split, img_transform, label_transform, test, input_ch=3, joint_transform=None,
                synthetic=None, file_list=None):
    """``synthetic`` = dict(length, img_shape, n_class, seed) selects the generated data, ``file_list`` a list file of real
    samples (``FileListRGBD``); the reference's own on-disk dataset classes (hard-coded lab paths) are outside this build."""
    assert dataset_name in AVAILABLE_DATASET_LIST
    if file_list is not None:
        return FileListRGBD(file_list, input_ch=input_ch, test=test)
    if synthetic is None:
        raise NotImplementedError("on-disk dataset %r is outside the MI355X hot-path build; run with --synthetic, or "
                                  "--src_file_list / --tgt_file_list for real data" % dataset_name)
    return SyntheticRGBD(synthetic["length"], input_ch, synthetic["img_shape"], synthetic["n_class"], synthetic["seed"], test,
                         raw=synthetic.get("raw", False), background_id=synthetic.get("background_id", 255))


def check_src_tgt_ok(src_dataset_name, tgt_dataset_name):
    if src_dataset_name == "synthia" and not tgt_dataset_name == "city16":
        raise AssertionError("you must use synthia-city16 pair")
    elif src_dataset_name == "city16" and not tgt_dataset_name == "synthia":
        raise AssertionError("you must use synthia-city16 pair")


def get_n_class(src_dataset_name):
    if src_dataset_name in ["synthia", "city16"]:
        return 16
    elif src_dataset_name in ["gta", "city", "ir", "test"]:
        return 19 + 1
    elif src_dataset_name in ["2d3d", "sun"]:
        return 13 + 1
    elif src_dataset_name in ["suncg", "nyu"]:
        return 40 + 1
    raise NotImplementedError("You have to define the class of %s dataset" % src_dataset_name)


def get_img_shape(dataset, is_train):
    shape = list(_IMG_SIZE[dataset])
    if is_train and dataset in ("city", "city16"):
        shape = [s / 2 for s in shape]
    return shape
