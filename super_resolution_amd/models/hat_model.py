"""`HATModel` — the reference's test-time caller of the hot path (HAT/hat/models/hat_model.py on top of
basicsr SRModel/BaseModel): pad to a window multiple, run the network whole or tile by tile, crop, convert to uint8,
save, score.  Same option dictionary as the reference's test YAMLs (`network_g`, `path.pretrain_network_g`,
`path.param_key_g`, `path.strict_load_g`, `tile.{tile_size,tile_pad}`, `val.{save_img,suffix,metrics}`).
`val.self_ensemble: true | 2 | 4 | 8` (no counterpart in the reference's YAMLs; its SRModel.test_selfensemble is never called) runs
every forward of every validation branch as the geometric self-ensemble of that many members (`true`: 8), whole or per tile.

Deviations (documented in INTEGRATION.md): a tile that fails raises instead of being printed and skipped
(hat_model.py:89-90); images are read/written with PIL; `num_gpu: 0` (CPU) is not supported by the MI355X path.
"""
from __future__ import annotations

import os
from os import path as osp

import torch
from torch.nn import functional as F

from .. import archs  # noqa: F401  (registers 'HAT' in the arch registry, like hat/archs/__init__.py:8-11)
from .. import tile_parallel as tp
from ..data import write_image
from ..metrics import calculate_metric, tensor2img
from ..registry import build_network


class HATModel:
    def __init__(self, opt: dict, device=None):
        self.opt = opt
        self.device = torch.device(device if device is not None else "cuda")
        self.net_g = build_network(dict(opt["network_g"])).eval()
        load_path = (opt.get("path") or {}).get("pretrain_network_g")
        if load_path:
            self.load_network(self.net_g, load_path, (opt["path"].get("strict_load_g", True)),
                              opt["path"].get("param_key_g", "params"))
        self.net_g = self.model_to_device(self.net_g)
        self.scale = opt.get("scale", 1)
        self.metric_results = {}

    @staticmethod
    def self_ensemble_members(value) -> int:
        """`val.self_ensemble` -> the number of ensemble members: absent / None / false -> 1 (no ensemble), true -> 8, the
        integers 2, 4, 8 -> themselves; anything else (1, 3, "8", 8.0 ...) is a ValueError: the option is never guessed at."""
        if value is None or value is False:
            return 1
        if value is True:
            return 8
        if isinstance(value, int) and value in (2, 4, 8):
            return value
        raise ValueError(f"val.self_ensemble is true, 2, 4 or 8 (members of the geometric self-ensemble), got {value!r}")

    @property
    def ensemble(self) -> int:
        return self.self_ensemble_members((self.opt.get("val") or {}).get("self_ensemble"))

    def _forward_fn(self):
        """The callable process / tile_process hand the (padded) image or a tile to: the network, or with val.self_ensemble its
        forward_ensemble — so a tiled frame keeps the reference's tile grid and every tile is ensembled on its own.
        forward_ensemble is a method of the bare module, so with `num_gpu > 1` the ensemble does not go through the
        nn.DataParallel wrapper: it runs on this model's device.  Validation feeds one image at a time, which DataParallel
        would hand to one device anyway (model_to_device: tile_parallel / band_parallel are the multi-GPU paths)."""
        n = self.ensemble
        if n == 1:
            return self.net_g
        bare = self.get_bare_model(self.net_g)
        ens = bare.forward_ensemble if self._family() is None else bare.upscale_ensemble   # (the ESC family's name for it)
        return lambda t: ens(t, n)

    def _family(self):
        """The bare network where it is a fixed-scale network of the ESC family, whose frame paths are `upscale_*`; else None.
        Such a network takes a frame of any size as it is, but this harness pads to a window multiple first (ESRModel.test does,
        as HATModel.pre_process): its byte branches therefore build the padded planes themselves (hat_u8_to_planes / ops.imresize)
        and hand them to `upscale_to_u8` with the crop, so the bytes are those of the float branch."""
        from ..frames import fixed_scale_family
        bare = self.get_bare_model(self.net_g)
        return bare if fixed_scale_family(bare) else None

    def model_to_device(self, net):
        """basicsr BaseModel.model_to_device (base_model.py:91-104): `num_gpu > 1` wraps the network in nn.DataParallel, as the
        reference does (one device: DataParallel forwards straight to the module; several: torch replicates the module per
        call and every replica packs its own engine — it works, but tile_parallel / band_parallel are the multi-GPU paths of
        this build).  `dist: true` (DistributedDataParallel) is a training-time wrapper and not needed for the test pipeline."""
        net = net.to(self.device)
        if self.opt.get("dist"):
            raise NotImplementedError("dist: true wraps the network for training (DistributedDataParallel); the test pipeline "
                                      "of this build runs with dist: false (multi-GPU inference: tile_parallel / band_parallel)")
        if int(self.opt.get("num_gpu", 1) or 1) > 1:
            net = torch.nn.DataParallel(net)
        return net

    def get_bare_model(self, net):  # base_model.py:106-112
        return net.module if isinstance(net, (torch.nn.DataParallel, torch.nn.parallel.DistributedDataParallel)) else net

    # basicsr BaseModel.load_network (base_model.py:289-315)
    @staticmethod
    def load_network(net, load_path, strict=True, param_key="params"):
        sd = torch.load(load_path, map_location="cpu")
        if param_key is not None:
            if param_key not in sd and "params" in sd:
                param_key = "params"
            sd = sd[param_key] if param_key in sd else sd
        sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
        net.load_state_dict(sd, strict=strict)

    def feed_data(self, data: dict):
        self.lq = data["lq"].to(self.device)
        if "gt" in data:
            self.gt = data["gt"].to(self.device)

    def _window_size(self) -> int:
        """The multiple a frame is reflect-padded to: network_g.window_size, or 1 for a network without windows (SRVGGNetCompact,
        whose option files carry no such key); for RRDBNet the factor it unshuffles the frame by at scale 2 / 1 (2 / 4), as
        Real-ESRGAN's inference wrapper pads."""
        net = self.opt["network_g"]
        if net.get("type") == "RRDBNet" and net.get("scale", 4) in (1, 2):
            return 4 // net["scale"]
        return net.get("window_size", 1)

    def pre_process(self):  # hat_model.py:16-26
        window_size = self._window_size()
        self.scale = self.opt.get("scale", 1)
        _, _, h, w = self.lq.size()
        self.mod_pad_h = (window_size - h % window_size) % window_size
        self.mod_pad_w = (window_size - w % window_size) % window_size
        self.img = F.pad(self.lq, (0, self.mod_pad_w, 0, self.mod_pad_h), "reflect")

    def process(self):  # hat_model.py:28-38
        with torch.no_grad():
            self.output = self._forward_fn()(self.img)

    def tile_process(self):  # hat_model.py:40-108
        _, _, h, w = self.img.shape
        tiles = tp.reference_tiles(h, w, self.opt["tile"]["tile_size"], self.opt["tile"]["tile_pad"])
        with torch.no_grad():
            self.output = tp.tile_forward(self.img, self._forward_fn(), self.scale, tiles)

    def post_process(self):  # hat_model.py:110-112
        _, _, h, w = self.output.size()
        self.output = self.output[:, :, 0:h - self.mod_pad_h * self.scale, 0:w - self.mod_pad_w * self.scale]

    def test(self):
        self.pre_process()
        if "tile" in self.opt:
            self.tile_process()
        else:
            self.process()
        self.post_process()

    def _u8_frame(self, img: torch.Tensor, option: str, what: str) -> torch.Tensor:
        """The dataset's (1,3,h,w) float image, which must hold 8-bit values (v / 255, what data.read_image produces) -> the
        (1,h,w,3) uint8 frame on the device."""
        u8 = torch.round(img * 255.0).clamp(0, 255).to(torch.uint8)
        if not torch.equal(u8.to(torch.float32) / 255.0, img.to(torch.float32)):
            raise RuntimeError(f"{option} needs 8-bit {what} images (every value k / 255): this one is not")
        return u8.permute(0, 2, 3, 1).contiguous().to(self.device)

    def test_u8(self, lq: torch.Tensor, on_device: bool = False):
        """`val.u8_on_device`: the same result as test() + tensor2img, with the conversions on the device.  The LQ image goes up
        as uint8 and only the uint8 result comes back: without `tile`, HAT.forward_u8 pads, runs, crops and converts (a network of
        the ESC family: hat_u8_to_planes pads and `upscale_to_u8` runs, crops and converts: _family); with
        `tile`, hat_u8_to_planes builds the padded input (pre_process_u8), tile_process runs as always and hat_planes_to_u8
        crops and converts the assembled fp32 output.  lq: the
        dataset's (1,3,h,w) float image, which must hold 8-bit values (v / 255, what data.read_image produces).
        on_device (`val.metrics_on_device`): return the (h,w,3) uint8 device tensor instead of downloading it.
        `val.self_ensemble`: forward_u8(ensemble=n) without `tile`; with `tile`, tile_process ensembles every tile."""
        from .. import ops
        frame = self._u8_frame(lq, "val.u8_on_device", "input")
        fam = self._family()
        if "tile" not in self.opt and fam is None:
            with torch.no_grad():
                out = self.get_bare_model(self.net_g).forward_u8(frame, **self._ensemble_kw())
        elif "tile" not in self.opt:
            self.pre_process_u8(frame)
            _, _, h, w = self.img.shape
            with torch.no_grad():
                out = fam.upscale_to_u8(self.img, crop=((h - self.mod_pad_h) * self.scale, (w - self.mod_pad_w) * self.scale), **self._ensemble_kw())
            del self.img
        else:
            self.pre_process_u8(frame)
            self.tile_process()
            b, _, h, w = self.output.shape
            out = torch.empty(b, h - self.mod_pad_h * self.scale, w - self.mod_pad_w * self.scale, 3, dtype=torch.uint8, device=self.device)
            ops.planes_to_u8(self.output.to(torch.float32).contiguous(), out)
            del self.img, self.output
        return out[0] if on_device else out[0].cpu().numpy()

    def _ensemble_kw(self) -> dict:
        """ensemble=n for the byte forwards under val.self_ensemble; nothing without it (the call is then today's call)."""
        n = self.ensemble
        return {"ensemble": n} if n > 1 else {}

    def pre_process_u8(self, frame: torch.Tensor):
        """pre_process for a (B,h,w,3) uint8 device frame: self.img = the reflect-padded float32(v) / 255 planes, bit for bit
        what pre_process makes of data.read_image's tensor.  hat_u8_to_planes divides exactly and pads; a torch division on the
        device would not do (it multiplies by the reciprocal, which is off by an ulp for about half of the byte values)."""
        from .. import ops
        window_size = self._window_size()
        self.scale = self.opt.get("scale", 1)
        b, h, w, _ = frame.shape
        self.mod_pad_h = (window_size - h % window_size) % window_size
        self.mod_pad_w = (window_size - w % window_size) % window_size
        if self.mod_pad_h >= h or self.mod_pad_w >= w:
            raise RuntimeError(f"a {h}x{w} image cannot be reflect-padded to a multiple of window_size {window_size}")
        self.img = torch.empty(b, 3, h + self.mod_pad_h, w + self.mod_pad_w, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            ops.u8_to_planes(frame, self.img)

    def get_current_visuals(self):
        out = {"lq": self.lq.detach().cpu(), "result": self.output.detach().cpu()}
        if hasattr(self, "gt"):
            out["gt"] = self.gt.detach().cpu()
        return out

    def _test_float(self, val_data):
        self.feed_data(val_data)
        self.test()
        visuals = self.get_current_visuals()
        data = {"img": tensor2img(visuals["result"])}
        if "gt" in visuals:
            data["img2"] = tensor2img(visuals["gt"])
            del self.gt
        del self.lq, self.output
        return data

    def _test_metrics_on_device(self, val_data, metrics, save_img):
        """`val.metrics_on_device`: test_u8 leaves its result on the device, the ground truth goes up as uint8 and the metrics
        of type calculate_psnr / calculate_ssim come from hat_u8_metrics, those of type calculate_niqe from the NIQE block sums
        (metrics_device.calculate_metrics_u8).  A dataset without `gt` is scored when every entry is NIQE, which needs none.
        The result is downloaded only when it is saved or a metric of another type needs it; that metric is computed on the
        host as ever.
        Returns (data for the host side: 'img' / 'img2' where they exist there, {name: value} of the device metrics)."""
        from ..metrics_device import DEVICE_METRICS, calculate_metrics_u8
        out = self.test_u8(val_data["lq"], on_device=True)
        has_gt = "gt" in val_data
        scored = {}
        if metrics and has_gt:
            gt = self._u8_frame(val_data["gt"], "val.metrics_on_device", "ground-truth")[0]
            scored = calculate_metrics_u8(out, gt, metrics, niqe=True)
        elif self._no_reference(metrics):
            scored = calculate_metrics_u8(out, None, metrics, niqe=True)
        host_metrics = bool(metrics) and has_gt and any(m.get("type") not in DEVICE_METRICS for m in metrics.values())
        data = {}
        if save_img or host_metrics:
            data["img"] = out.cpu().numpy()
        if host_metrics:
            data["img2"] = tensor2img(val_data["gt"])
        return data, scored

    def test_gt_u8(self, gt: torch.Tensor):
        """`val.lq_on_device`: the (1,H,W,3) uint8 device ground truth -> the (h,w,3) uint8 device result of its own bicubic
        low-resolution image (resize.py's imresize at 1 / scale, made on the device: the float LQ never exists on the host).
        Without `tile`, HAT.forward_gt_u8 does it all (a network of the ESC family: ops.imresize writes the padded planes and
        `upscale_to_u8` runs, crops and converts: _family); with `tile`, ops.imresize writes the padded planes, tile_process runs
        as always and hat_planes_to_u8 crops and converts, as test_u8 does.  `val.self_ensemble`: as in test_u8."""
        from .. import ops
        fam = self._family()
        if "tile" not in self.opt and fam is None:
            with torch.no_grad():
                return self.get_bare_model(self.net_g).forward_gt_u8(gt, **self._ensemble_kw())[0]
        window_size = self._window_size()
        s = self.scale = self.opt.get("scale", 1)
        b, H, W, _ = gt.shape
        gt = gt[:, :H - H % s, :W - W % s]
        h, w = gt.shape[1] // s, gt.shape[2] // s
        self.mod_pad_h = (window_size - h % window_size) % window_size
        self.mod_pad_w = (window_size - w % window_size) % window_size
        if h < 1 or w < 1 or self.mod_pad_h >= h or self.mod_pad_w >= w:
            raise RuntimeError(f"a {h}x{w} image cannot be reflect-padded to a multiple of window_size {window_size}")
        with torch.cuda.device(self.device):
            self.img = ops.imresize(gt, 1.0 / s, pad_to=(h + self.mod_pad_h, w + self.mod_pad_w))
        if "tile" not in self.opt:   # (the ESC family, whole frame: the padded planes into bytes with the crop)
            with torch.no_grad():
                out = fam.upscale_to_u8(self.img, crop=(h * s, w * s), **self._ensemble_kw())
            del self.img
            return out[0]
        self.tile_process()
        out = torch.empty(b, h * s, w * s, 3, dtype=torch.uint8, device=self.device)
        ops.planes_to_u8(self.output.to(torch.float32).contiguous(), out)
        del self.img, self.output
        return out[0]

    def _test_lq_on_device(self, val_data, metrics, save_img, on_device_metrics):
        """`val.lq_on_device`: the ground truth goes up once as uint8, test_gt_u8 makes the LQ image and runs, and the result is
        scored against the same device buffer (its mod-cropped view).  Returns what _test_metrics_on_device returns."""
        from ..metrics_device import DEVICE_METRICS, calculate_metrics_u8
        if "gt" not in val_data:
            raise RuntimeError("val.lq_on_device makes the LQ image from the ground truth: it needs a dataset that delivers `gt` "
                               "(type: ImageNetPairedDataset or PairedImageDataset)")
        gt = self._u8_frame(val_data["gt"], "val.lq_on_device", "ground-truth")
        out = self.test_gt_u8(gt)
        gtc = gt[0, :out.shape[0], :out.shape[1]]
        scored = calculate_metrics_u8(out, gtc, metrics, niqe=True) if (metrics and on_device_metrics) else {}
        host_metrics = bool(metrics) and any(m.get("type") not in DEVICE_METRICS or not on_device_metrics for m in metrics.values())
        data = {}
        if save_img or host_metrics:
            data["img"] = out.cpu().numpy()
        if host_metrics:
            data["img2"] = gtc.cpu().numpy()
        return data, scored

    @staticmethod
    def _no_reference(metrics) -> bool:
        """Every entry scores the result alone (NIQE): such a set of metrics runs on a dataset without `gt`."""
        from ..metrics import NO_REFERENCE
        return bool(metrics) and all(m.get("type") in NO_REFERENCE for m in metrics.values())

    @staticmethod
    def _items(dataset, lq_on_device: bool):
        """The dataset's items.  Under `val.lq_on_device` a GT-only dataset is told not to make `lq` (data.FolderDataset.make_lq):
        its host imresize is the very step the device takes over, and nothing would read the result."""
        skip = lq_on_device and getattr(dataset, "gt_only", False)
        if not skip:
            yield from dataset
            return
        before, dataset.make_lq = dataset.make_lq, False
        try:
            yield from dataset
        finally:
            dataset.make_lq = before

    def nondist_validation(self, dataset, save_img: bool = True):  # hat_model.py:114-185
        dataset_name = dataset.opt["name"]
        val = self.opt.get("val") or {}
        metrics = val.get("metrics")
        self.metric_results = {m: 0.0 for m in (metrics or {})}
        self.ensemble   # a val.self_ensemble that is not true / 2 / 4 / 8 raises here, before the first image
        per_image = []
        n = 0
        on_device = bool(val.get("metrics_on_device"))   # implies u8_on_device; the known metrics are scored where the result is
        for val_data in self._items(dataset, bool(val.get("lq_on_device"))):
            img_name = osp.splitext(osp.basename(val_data["lq_path"][0]))[0]
            device_metrics = {}
            if val.get("lq_on_device"):   # implies u8_on_device; the LQ image is made on the device from the uploaded GT
                data, device_metrics = self._test_lq_on_device(val_data, metrics, save_img, on_device)
            elif on_device:
                data, device_metrics = self._test_metrics_on_device(val_data, metrics, save_img)
            elif val.get("u8_on_device"):
                data = {"img": self.test_u8(val_data["lq"])}
                if "gt" in val_data:
                    data["img2"] = tensor2img(val_data["gt"])
            else:
                data = self._test_float(val_data)
            sr_img = data.get("img")
            if save_img:
                suffix = val.get("suffix") or self.opt["name"]
                root = (self.opt.get("path") or {}).get("visualization") or osp.join("results", self.opt["name"], "visualization")
                write_image(sr_img, osp.join(root, dataset_name, f"{img_name}_{suffix}.png"))
            row = {"name": img_name}
            if metrics and ("img2" in data or device_metrics or self._no_reference(metrics)):
                for name, mopt in metrics.items():
                    v = device_metrics[name] if name in device_metrics else calculate_metric(data, mopt)
                    self.metric_results[name] += v
                    row[name] = v
            per_image.append(row)
            n += 1
        for m in self.metric_results:
            self.metric_results[m] /= max(n, 1)
        return dict(self.metric_results), per_image
