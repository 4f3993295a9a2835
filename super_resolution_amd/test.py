"""`python -m super_resolution_amd.test -opt options/test/HAT-S_SRx4.yml` — the reference's `hat/test.py` entry
(basicsr `test_pipeline`): parse the YAML, build the test datasets and the model harness of `model_type` (`HATModel`; ESC's `ESRModel` is the same harness), validate each dataset."""
from __future__ import annotations

import argparse
import json
import sys

import yaml

from .data import FolderDataset
from .frames import sync_guard
from .models import HATModel, model_class


def parse_options(path: str, u8: bool = False, metrics_on_device: bool = False, lq_on_device: bool = False, self_ensemble=None) -> dict:
    """self_ensemble (--self-ensemble [N]): set val.self_ensemble to N (2, 4 or 8);
    u8 (the --u8 flag): set val.u8_on_device; metrics_on_device (--metrics-on-device): set val.metrics_on_device and, since
    it implies it, val.u8_on_device; lq_on_device (--lq-on-device): set val.lq_on_device (and val.u8_on_device); without the
    flags the options are exactly what the YAML says."""
    with open(path) as f:
        opt = yaml.safe_load(f)
    if lq_on_device:
        opt["val"] = dict(opt.get("val") or {}, u8_on_device=True, lq_on_device=True)
    if u8:
        opt["val"] = dict(opt.get("val") or {}, u8_on_device=True)
    if metrics_on_device:
        opt["val"] = dict(opt.get("val") or {}, u8_on_device=True, metrics_on_device=True)
    if self_ensemble is not None:
        opt["val"] = dict(opt.get("val") or {}, self_ensemble=self_ensemble)
    opt["is_train"] = False
    for phase, d in (opt.get("datasets") or {}).items():
        d["phase"] = phase.split("_")[0]
        if "scale" in opt:
            d["scale"] = opt["scale"]
    return opt


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-opt", type=str, required=True, help="Path to option YAML file.")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--u8", action="store_true", help="8-bit frames on the device (sets val.u8_on_device): upload uint8, download uint8")
    ap.add_argument("--metrics-on-device", action="store_true",
                    help="PSNR / SSIM from 8-bit frames on the device (sets val.metrics_on_device and val.u8_on_device)")
    ap.add_argument("--lq-on-device", action="store_true",
                    help="make the bicubic LQ image on the device from the uploaded 8-bit ground truth (sets val.lq_on_device)")
    ap.add_argument("--self-ensemble", nargs="?", type=int, const=8, default=None, choices=[2, 4, 8], metavar="N",
                    help="geometric self-ensemble over the first N = 2, 4 or 8 (default when N is left out) flips / transposes of "
                         "every image (sets val.self_ensemble)")
    args = ap.parse_args(argv)
    opt = parse_options(args.opt, u8=args.u8, metrics_on_device=args.metrics_on_device, lq_on_device=args.lq_on_device,
                        self_ensemble=args.self_ensemble)
    model_class(opt.get("model_type"))   # KeyError for a model type that is not built; every one that is (HATModel, ESRModel) is this harness
    model = HATModel(opt, device=args.device)
    results = {}
    for _, dopt in sorted((opt.get("datasets") or {}).items()):
        ds = FolderDataset(dopt)
        print(f"Testing {dopt['name']} ({len(ds)} images)...", file=sys.stderr)
        with sync_guard(model.net_g):   # every image comes to the host: one whose FP16 stream clipped is run again on fp32 first
            mean, rows = model.nondist_validation(ds, save_img=(opt.get("val") or {}).get("save_img", True))
        results[dopt["name"]] = {"mean": mean, "images": rows}
        print(f"Validation {dopt['name']}: " + "  ".join(f"# {k}: {v:.4f}" for k, v in mean.items()), file=sys.stderr)
    print(json.dumps(results))
    return results


if __name__ == "__main__":
    main()
