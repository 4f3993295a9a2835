"""Folder datasets of the reference's test YAMLs (`PairedImageDataset`, `SingleImageDataset`:
HAT/ESC/basicsr/data/paired_image_dataset.py, single_image_dataset.py) read with PIL instead of OpenCV:
images become float32 RGB CHW tensors in [0, 1] (img_util.py imfrombytes float32 + img2tensor bgr2rgb)."""
from __future__ import annotations

import os

import numpy as np
import torch

_EXT = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff")


def read_image(path: str) -> torch.Tensor:
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im.convert("RGB"), dtype=np.float32) / np.float32(255.0)
    return torch.from_numpy(a).permute(2, 0, 1).contiguous()


def write_image(img_u8_rgb: np.ndarray, path: str) -> None:
    from PIL import Image
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    Image.fromarray(img_u8_rgb, "RGB").save(path)


def _scan(folder: str):
    return sorted(os.path.join(folder, f) for f in os.listdir(folder) if f.lower().endswith(_EXT))


class FolderDataset:
    """opt: {name, type: PairedImageDataset|SingleImageDataset, dataroot_lq, [dataroot_gt], [filename_tmpl]}.
    Paired: every LQ file must have a GT file of the same basename (paired_paths_from_folder semantics).
    type: ImageNetPairedDataset takes {name, dataroot_gt, scale, [gt_size]} only and makes each LQ image from its GT image."""

    def __init__(self, opt: dict):
        self.opt = opt
        self.gt_only = opt.get("type") == "ImageNetPairedDataset"
        # GT-only datasets: False leaves `lq` out of the items (no host imresize).  HATModel.nondist_validation clears it for
        # the time of a `val.lq_on_device` run, which makes the LQ image on the device from `gt`.
        self.make_lq = True
        if self.gt_only:
            self._init_gt_only(opt)
            return
        self.lq = _scan(opt["dataroot_lq"])
        self.gt = None
        if opt.get("type", "SingleImageDataset") == "PairedImageDataset" or opt.get("dataroot_gt"):
            tmpl = opt.get("filename_tmpl", "{}")
            gt = {os.path.splitext(os.path.basename(p))[0]: p for p in _scan(opt["dataroot_gt"])}
            if len(gt) != len(self.lq):
                raise AssertionError(f"{opt['name']}: lq and gt folders have different numbers of images: {len(self.lq)}, {len(gt)}.")
            self.gt = []
            for name, p in sorted(gt.items()):
                want = tmpl.format(name)
                match = [q for q in self.lq if os.path.splitext(os.path.basename(q))[0] == want]
                if not match:
                    raise AssertionError(f"{want} is not in the lq folder of {opt['name']}.")
                self.gt.append((match[0], p))
            self.lq = [m for m, _ in self.gt]
            self.gt = [g for _, g in self.gt]

    # ---- type: ImageNetPairedDataset (hat/data/imagenet_paired_dataset.py), test phase: a folder of ground-truth images
    # only; the LQ image is made from each GT image by the reference's MATLAB-style imresize (resize.py) ----
    def _init_gt_only(self, opt: dict):
        if opt.get("phase", "test") == "train":
            raise NotImplementedError("ImageNetPairedDataset: only the test-phase branch is built (no random crop, no augmentation)")
        if (opt.get("io_backend") or {}).get("type", "disk") != "disk":
            raise NotImplementedError("ImageNetPairedDataset: io_backend lmdb is not supported, only disk")
        for key, what in (("meta_info_file", "a meta_info_file"), ("mean", "mean / std normalisation"), ("std", "mean / std normalisation")):
            if opt.get(key) is not None:
                raise NotImplementedError(f"ImageNetPairedDataset: {what} is not supported")
        if opt.get("color") == "y":
            raise NotImplementedError("ImageNetPairedDataset: color: y is not supported")
        if not int(opt.get("scale", 0) or 0) > 0:
            raise ValueError(f"{opt.get('name')}: ImageNetPairedDataset needs `scale`: the LQ image is made from the GT image at 1 / scale")
        self.gt = _scan(opt["dataroot_gt"])
        self.lq = self.gt            # the outputs are named after lq_path

    def _getitem_gt_only(self, i):
        from . import resize
        s = int(self.opt["scale"])
        gt = read_image(self.gt[i]).numpy()                                   # (3,H,W) float32 RGB
        H, W = resize.mod_crop(gt.shape[1], gt.shape[2], s)                   # imagenet_paired_dataset.py:49-53
        gt_size = int(self.opt.get("gt_size", 0) or 0)
        if H < gt_size or W < gt_size:                                        # :56-58 enlarges with cv2.resize: out of scope
            raise RuntimeError(f"{self.gt[i]}: {H}x{W} after mod-crop is smaller than gt_size {gt_size}; enlarging is not supported")
        gt = np.ascontiguousarray(gt[:, :H, :W])
        d = {"gt_path": [self.gt[i]], "lq_path": [self.gt[i]]}
        if self.make_lq:
            lq = resize.imresize(gt, 1 / s)                                    # :59, float, unrounded
            d["lq"] = torch.from_numpy(lq).unsqueeze(0)
            gt = gt[:, :lq.shape[1] * s, :lq.shape[2] * s]                     # :79-80; a no-op after the mod-crop: ceil(H / s) s = H
        d["gt"] = torch.from_numpy(np.ascontiguousarray(gt)).unsqueeze(0)
        return d

    def __len__(self):
        return len(self.lq)

    def __getitem__(self, i):
        if self.gt_only:
            return self._getitem_gt_only(i)
        d = {"lq": read_image(self.lq[i]).unsqueeze(0), "lq_path": [self.lq[i]]}
        if self.gt is not None:
            gt = read_image(self.gt[i]).unsqueeze(0)
            # test phase: GT cropped to lq size x scale (paired_image_dataset.py:92-95) so that a GT whose size is not an
            # exact multiple of the LQ size is still scored, as the reference does
            s = int(self.opt.get("scale", 0) or 0)
            if s > 0 and self.opt.get("phase", "test") != "train":
                gt = gt[..., :d["lq"].shape[-2] * s, :d["lq"].shape[-1] * s]
            d["gt"] = gt
            d["gt_path"] = [self.gt[i]]
        return d

    def __iter__(self):
        return (self[i] for i in range(len(self)))
