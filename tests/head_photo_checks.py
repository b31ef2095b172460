"""Shared by tests/test_head_photo_loss_cpu.py and tests/test_gpu_head_photo_loss.py: the ORACLE's head-fused photo loss

    L = PhotoLoss(renderer, eps)(losses.decode_head(encoded9), photos, scenes)

as a composition of what exists, the photographs the cases are compared under, an independent definition in torch float64
autograd and the speed measurement.

Comparison values of one case (photo_checks.Reference with head=True):

    maps        = c_oracle.head_decode(enc)                 the float32 decode with the reference's rounding
    loss, g12   = photo_checks.oracle_photo_loss(maps, ...) float32, and f64=True on the same float32-decoded maps
    g9          = photo_checks.chain9(enc, maps, g12)       12 -> 9 channels in float64, the formulas of
                                                            head_checks.head_loss_f64_on_f32_decode
    tie map     = photo_checks.tie_map(maps, photos, scenes, delta_f64)

and the comparison is photo_checks.assert_photo_grad_close on the 9-channel gradient: tests/tolerances.py's bounds,
every use in the tolerance ledger.

Photographs: clip(c_oracle.render_fwd(<the case's target maps>, scenes), 0, 1) -- the target maps of tests/head_checks.py's
cases photographed under the case's own scenes (`raw=True`: unclipped).
"""
import ctypes

import numpy as np
import torch

import head_checks
import photo_checks
from oracle import c_oracle

EPS = photo_checks.EPS
ENTRIES = ("svbrdf_head_photo_loss_fwd_bwd", "svbrdf_head_photo_loss_fwd_bwd_host_scenes")


def photographs(target_maps, scenes, raw=False):
    ph = c_oracle.render_fwd(np.ascontiguousarray(target_maps, np.float32), np.ascontiguousarray(scenes, np.float32))
    return ph if raw else np.clip(ph, 0.0, 1.0)


def upstream_rounding_term(maps, photos, scenes, eps=EPS):
    """photo_checks.oracle_photo_loss hands the oracle's adjoint the upstream gradient sign(delta) / (N (rad + eps)) ROUNDED
    TO FLOAT32 -- c_oracle.render_bwd takes float32 -- with f64=True too: its "float64" gradient carries a 2^-24 relative
    error per term.  The adjoint is linear in the upstream gradient, so the adjoint of the rounding residue is exactly what
    is missing: -> [B,12,H,W] float64, to be ADDED to oracle_photo_loss(..., f64=True)'s gradient where a comparison needs
    the double value itself (tests/test_head_photo_loss_cpu.py against torch float64 autograd)."""
    maps = np.ascontiguousarray(maps, np.float32)
    scenes = np.ascontiguousarray(scenes, np.float32)
    a = c_oracle.render_fwd(maps, scenes, f64=True) + np.float64(np.float32(eps))
    b = np.asarray(photos, np.float32).astype(np.float64) + np.float64(np.float32(eps))
    g = np.sign(np.log(a) - np.log(b)) / (float(a.size) * a)
    residue = g - g.astype(np.float32).astype(np.float64)
    return np.asarray(c_oracle.render_bwd(maps, scenes, residue.astype(np.float32), f64=True), np.float64)


def torch_head_photo_loss(enc, photos, scenes, eps=EPS, maps_values=None):
    """An independent definition in torch float64 autograd on the CPU: losses.decode_head, then the eager restatement of
    the reference's renderer (oracle/eager_torch.render_scene), log and L1 mean, on the same float32-valued inputs: the
    pixel row with the float32 values of torch.linspace, pi and the 0.001 clamps with their float32 values, as in the
    oracle's float64 instantiation (head_checks.torch_head_loss).  `maps_values` [B,12,H,W]: the loss is evaluated AT
    these map values (the float32 decode the oracle's composition shades), the Jacobian of the decode stays autograd's.
    -> (loss: float, gradient [B,9,H,W] float64, decoded maps [B,12,H,W] float64)"""
    from oracle import eager_torch
    from svbrdf_estimation_amd import losses
    x = torch.from_numpy(np.asarray(enc, np.float32)).to(torch.float64).requires_grad_(True)
    ph = torch.from_numpy(np.asarray(photos, np.float32)).to(torch.float64)
    sc = torch.from_numpy(np.asarray(scenes, np.float32)).to(torch.float64)
    xrow = torch.linspace(-1, 1, x.shape[-1], dtype=torch.float32).to(torch.float64)
    decoded = losses.decode_head(x)
    maps = decoded
    if maps_values is not None:
        maps = decoded + (torch.from_numpy(np.asarray(maps_values, np.float64)) - decoded).detach()
    kw = dict(xrow=xrow, pi=float(np.float32(np.pi)), clamp_min=float(np.float32(0.001)))
    rendered = torch.stack([torch.cat([eager_torch.render_scene(maps[b], sc[b, s], **kw) for s in range(sc.shape[1])], dim=0)
                            for b in range(x.shape[0])], dim=0)
    e = float(np.float32(eps))
    loss = torch.nn.functional.l1_loss(torch.log(rendered + e), torch.log(ph + e))
    loss.backward()
    return float(loss.item()), x.grad.numpy(), decoded.detach().numpy()


# ------------------------------------------------------------------------------------------------ the cases

def sweep_inputs(c):
    """-> (enc, photos, scenes) of one case of head_checks.sweep_cases()"""
    enc, tgt, sc = head_checks.sweep_inputs(c)
    return enc, photographs(tgt, sc), sc


def pow2_inputs(name, raw=False):
    enc, tgt, sc = head_checks.pow2_inputs(name)
    return enc, photographs(tgt, sc, raw), sc


def alignment_inputs(H):
    enc, tgt, sc = head_checks.alignment_inputs(H)
    return enc, photographs(tgt, sc), sc


def argument_inputs():
    enc, tgt, sc = head_checks.argument_inputs()
    return enc, photographs(tgt, sc), sc


RAW_POW2 = "64_device"      # the power-of-two case that is also run with raw (unclipped) photographs


# ------------------------------------------------------------------------------------------------ the speed measurement

def measure_head_photo_loss(dev, native, sets=6, n=40, rounds=3):
    """-> dict of medians (us per step) at the configuration-2 shape, B = 8, 256 x 256, S = 9, by-value scene table, `sets`
    rotating batches (so the planes come from HBM), one process, the three legs alternating round by round:

        head_photo_us    the fused head photo loss, forward + adjoint: ONE launch
        composition_us   PhotoLoss(R)(losses.decode_head(x), photos, table) forward + backward through autograd: the
                         12-channel photo kernel plus the decode's elementwise passes and their backward
        photo12_us       the 12-channel photo kernel alone on the decoded maps (reported, not compared)"""
    from svbrdf_estimation_amd import environment, losses, renderers
    B, H, S = 8, 256, 9
    lib = native._load()
    torch.manual_seed(11)
    table = environment.BatchSceneSampler(B, 3, 6).sample().contiguous()
    gen = torch.Generator().manual_seed(5)
    encs = [(torch.rand((B, 9, H, H), generator=gen) * 1.8 - 0.9).to(dev) for _ in range(sets)]
    others = [(torch.rand((B, 9, H, H), generator=gen) * 1.8 - 0.9).to(dev) for _ in range(sets)]
    with torch.no_grad():
        maps = [losses.decode_head(e).contiguous() for e in encs]
        photos = [native.render_fwd(losses.decode_head(o).contiguous(), table).clamp_(0.0, 1.0) for o in others]
    del others
    g9 = [torch.empty_like(e) for e in encs]
    g12 = [torch.empty_like(m) for m in maps]
    leaves = [e.clone().requires_grad_(True) for e in encs]
    xr = native.xrow(dev, H)
    ws = torch.zeros(65, dtype=torch.int64, device=dev)
    loss = torch.empty(1, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    unfused = losses.PhotoLoss(renderers.LocalRenderer(), EPS)

    def head(i):
        k = i % sets
        rc = lib.svbrdf_head_photo_loss_fwd_bwd_host_scenes(encs[k].data_ptr(), photos[k].data_ptr(), table.data_ptr(),
                                                            xr.data_ptr(), ctypes.c_float(EPS), loss.data_ptr(),
                                                            g9[k].data_ptr(), ws.data_ptr(), ws.numel() * 8, B, S, H, H, st)
        assert rc == 0, lib.svbrdf_last_error()

    def photo12(i):
        k = i % sets
        rc = lib.svbrdf_photo_loss_fwd_bwd_host_scenes(maps[k].data_ptr(), photos[k].data_ptr(), table.data_ptr(),
                                                       xr.data_ptr(), ctypes.c_float(EPS), loss.data_ptr(), g12[k].data_ptr(),
                                                       ws.data_ptr(), ws.numel() * 8, B, S, H, H, st)
        assert rc == 0, lib.svbrdf_last_error()

    def composition(i):
        k = i % sets
        leaves[k].grad = None
        unfused(losses.decode_head(leaves[k]), photos[k], table).backward()

    legs = (("head_photo_us", head), ("composition_us", composition), ("photo12_us", photo12))
    out, res = photo_checks.timed_legs(legs, n, rounds, photo_checks.spinning_wave(native, dev), dev)
    out.update(rounds=res, device=torch.cuda.get_device_name(dev), steps_per_round=n, sets=sets)
    out["head_photo_frac_of_8TBps"] = (9 + 3 * S + 9) * 4 * H * H * B / (out["head_photo_us"] * 1e-6) / 8.0e12
    return out
