"""Bitwise fingerprint of what the fused loss hands its caller, through the C ABI (ctypes path), for a same-box comparison of
two builds of the library: run once per build (SVBRDF_HIP_LIB=tools/_build/libsvbrdf_<tag>.so) and compare the lines.

    SVBRDF_HIP_LIB=... python tools/loss_output_hashes.py [case ...]  >  hashes_<tag>.txt

One line per case: the loss's bit pattern and the sha256 of the gradient's bytes.  Inputs are seeded: the same arguments
give the same inputs in every run.  Cases: config 2 RenderingLoss / MixedLoss / forward-only, config-5 shape (B = 8, 512x512,
11 + 21 scenes), untied roughness, a device scene table, and a NaN map followed by a clean call."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("SVBRDF_NO_HOST_EXT", "1")
import numpy as np
import torch

from bench import synthetic_maps
from svbrdf_estimation_amd import _native, environment

CASES = {  # name: (B, H, random scenes, specular scenes, tied roughness, l1_weight, want_grad, device table)
    "config2": (8, 256, 3, 6, True, 0.0, True, False),
    "config2_mixed": (8, 256, 3, 6, True, 0.1, True, False),
    "config2_untied": (8, 256, 3, 6, False, 0.0, True, False),
    "config2_forward_only": (8, 256, 3, 6, True, 0.0, False, False),
    "config2_device_table": (8, 256, 3, 6, True, 0.0, True, True),
    "config5_shape": (8, 512, 11, 21, True, 0.0, True, False),
    "config5_shape_mixed": (8, 512, 11, 21, True, 0.1, True, False),
}


def line(name, loss, grad):
    bits = loss.detach().cpu().numpy().view(np.uint32)[0]
    gh = hashlib.sha256(grad.detach().cpu().numpy().tobytes()).hexdigest() if grad is not None else "-"
    print("%-24s loss 0x%08x (%.9g)  grad sha256 %s" % (name, bits, loss.item(), gh), flush=True)


dev = torch.device("cuda:0")
for name in (sys.argv[1:] or list(CASES)):
    B, H, nr, ns, tied, l1, want_grad, on_device = CASES[name]
    gen = torch.Generator().manual_seed(1234)
    inp, tgt = synthetic_maps(gen, B, H, tied=tied).to(dev), synthetic_maps(gen, B, H, tied=tied).to(dev)
    torch.manual_seed(4321)
    table = environment.BatchSceneSampler(B, nr, ns).sample().contiguous()
    if on_device:
        table = table.to(dev)
    loss, grad = _native.rendering_loss(inp, tgt, table, 0.1, want_grad=want_grad, l1_weight=l1)
    line(name, loss, grad)
    if name == "config2":       # a non-finite call, then the clean call again: nothing may stick
        bad = tgt.clone()
        bad[3, 4, 100, 7] = float("nan")
        line("config2_nan_target", *_native.rendering_loss(inp, bad, table, 0.1))
        line("config2_after_nan", *_native.rendering_loss(inp, tgt, table, 0.1))
torch.cuda.synchronize()
for ws in _native._workspace_cache.values():
    print("scratch all zero: %s" % (not ws.any().item()))
