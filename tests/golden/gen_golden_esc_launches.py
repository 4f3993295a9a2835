#!/usr/bin/env python3
"""tests/golden/esc_launches.json: the launches of one forward of every ESC-family network, as ops.profile() records them — the
(kernel name, tag) pairs in order, per case of tests/esc_launches.py and per compute dtype, on the MI355X.

The file pins what a change to the engines' HOST code must leave alone: which kernels run, in which order and in which
instantiation (the names carry the template arguments hat_conv_plan chose).  So it is recorded at the commit BEFORE such a change
and never from the code under test: check that commit's package out beside this tree, build the library, and run

    PYTHONPATH=<that checkout> python tests/golden/gen_golden_esc_launches.py

Data only; needs a GPU.  Only public API is used (tests/esc_launches.py), so the script runs against either tree."""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.append(os.path.dirname(os.path.dirname(HERE)))   # (behind PYTHONPATH: a checkout named there is the one that is recorded)


def main():
    import torch
    import esc_launches as L
    import super_resolution_amd
    dev = torch.device("cuda:0")
    out = {"recorded_on": torch.cuda.get_device_name(0), "cases": {}}
    for name, (typ, kw, frame) in L.CASES.items():
        ent = out["cases"][name] = {"type": typ, "kw": kw, "frame": list(frame)}
        for dtype in L.DTYPES:
            ent[dtype] = L.run_case(name, dtype, dev)[0]
        print(f"{name}: {len(ent['bf16'])} launches (bf16), {len(ent['fp32'])} (fp32)", flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "esc_launches.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"package {os.path.dirname(super_resolution_amd.__file__)} -> {path}")


if __name__ == "__main__":
    main()
