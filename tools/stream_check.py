"""One stream vs two streams per input size (GPU box).  python tools/stream_check.py"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from super_resolution_amd import synth
from super_resolution_amd.registry import build_network
import super_resolution_amd.archs  # noqa: F401

dev = torch.device("cuda:0")
net = build_network(dict(type="HAT", upscale=4, compute_dtype="bf16", **bench.MODELS["HAT-S"])).eval()
net.load_state_dict(synth.synth_state_dict(net.state_dict(), bench.W_SEED), strict=True)
net = net.to(dev)
eng = net.engine(dev)
for H, W in ((64, 64), (128, 128), (256, 256), (368, 320), (512, 512), (720, 1280)):
    x = synth.synth_input(bench.X_SEED, (1, 3, H, W)).to(dev)
    res = []
    for one in (False, True):
        for _ in range(3):
            eng.forward(x, one_stream=one)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            eng.forward(x, one_stream=one)
        torch.cuda.synchronize()
        res.append((time.perf_counter() - t0) / 10 * 1e3)
    print(f"{H}x{W}: two streams {res[0]:.3f} ms, one stream {res[1]:.3f} ms", flush=True)
