"""Shared by tests/test_weighted_photo_loss_cpu.py and tests/test_gpu_weighted_photo_loss.py: the weight fields and the cases
the photo losses with per-pixel confidence weights are compared at, and their speed measurement.  The oracle's composition,
its tie rule and the comparison values of one case are tests/photo_checks.py's, with `weights`.
"""
import numpy as np

import photo_checks
import synth
from oracle import c_oracle

EPS = photo_checks.EPS
ENTRIES = ("svbrdf_photo_loss_weighted_fwd_bwd", "svbrdf_photo_loss_weighted_fwd_bwd_host_scenes",
           "svbrdf_head_photo_loss_weighted_fwd_bwd", "svbrdf_head_photo_loss_weighted_fwd_bwd_host_scenes")


def weight_field(seed, B, P, H, masked_rows=True):
    """[B,P,H,W] float32 confidence: uniform in (0, 1) with about a quarter of the pixels exactly 0 and a quarter exactly 1;
    `masked_rows`: the top quarter of the rows 0 in every plane (pixels masked for every photo, in both layouts)"""
    u = synth.uniform01(seed, (B, P, H, H))
    w = np.where(u < 0.25, np.float32(0.0), np.where(u >= 0.75, np.float32(1.0), (u - np.float32(0.25)) * np.float32(2.0)))
    w = w.astype(np.float32)
    if masked_rows:
        w[:, :, :max(H // 4, 1), :] = 0.0
    assert w.min() == 0.0 and w.max() == 1.0
    return np.ascontiguousarray(w)


def encoded_input(seed, B, H):
    """[B,9,H,W] float32 in (-0.9, 0.9): a generator's post-tanh output away from saturation"""
    return (synth.uniform01(seed, (B, 9, H, H)) * np.float32(1.8) - np.float32(0.9)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the GPU cases
# (name, H, S = n_random + n_specular, seed of the scene table, tied roughness): B = 2 throughout.  Chosen as the smallest
# shapes at which the kernels take another path: one pass (S = 1) with a partial second workgroup (17 x 17 = 289 pixels),
# one full trip of the two-pass loop (S = 2), an odd exit of it (S = 3), widths that are no power of two (the division-free
# coordinate path) and one that is (the early-coordinate path of the by-value kernels), the three-lobe loop.
CASES = (
    ("17_s1", 17, (1, 0), 123, True),
    ("17_s2", 17, (1, 1), 7, True),
    ("33_s3", 33, (1, 2), 31, True),
    ("45_s9", 45, (3, 6), 11, True),
    ("64_s9", 64, (3, 6), 33, True),
    ("64_s9_untied", 64, (3, 6), 35, False),
)
LAYOUTS = ("per-photo", "shared")
B_CASES = 2


def case_inputs(name):
    """-> dict of one case: maps [2,12,H,H], enc [2,9,H,H], photos = clip(oracle.render_fwd(target), 0, 1), scenes, and the
    weight field in both layouts, {"per-photo": [2,S,H,H], "shared": [2,1,H,H]}"""
    idx = [c[0] for c in CASES].index(name)
    _, H, (nr, ns), seed, tied = CASES[idx]
    S = nr + ns
    sc = photo_checks.scene_table(B_CASES, seed, nr, ns)
    maps = synth.make_maps(6100 + 2 * idx, B_CASES, H, tiled_roughness=tied)
    target = synth.make_maps(6101 + 2 * idx, B_CASES, H, tiled_roughness=tied)
    photos = np.clip(c_oracle.render_fwd(target, sc), 0.0, 1.0)
    weights = {"per-photo": weight_field(6200 + idx, B_CASES, S, H), "shared": weight_field(6300 + idx, B_CASES, 1, H)}
    return dict(name=name, H=H, S=S, tied=tied, maps=maps, enc=encoded_input(6400 + idx, B_CASES, H), photos=photos,
                scenes=sc, weights=weights)


_REFERENCES = {}


def reference(name, layout, head):
    """the oracle's values of (case, weight layout, maps or head), computed once per session and shared"""
    key = (name, layout, bool(head))
    if key not in _REFERENCES:
        c = case_inputs(name)
        _REFERENCES[key] = (c, photo_checks.Reference(c["enc"] if head else c["maps"], c["photos"], c["scenes"], EPS,
                                                      head=head, weights=c["weights"][layout]))
    return _REFERENCES[key]


# ------------------------------------------------------------------------------------------------ the speed measurement

def measure_weighted_photo_loss(dev, native, layout="per-photo", sets=6, n=40, rounds=3):
    """-> dict of medians (us per step) at the configuration-2 shape, B = 8, 256 x 256, S = 9, by-value scene table, `sets`
    rotating batches (so the planes come from HBM), one process, the legs alternating round by round, the timing method
    of tests/test_gpu_photo_loss.py::test_photo_loss_is_no_slower_than_k3:

        weighted_us      the fused weighted photo loss, forward + adjoint: ONE launch
        unweighted_us    the unweighted photo loss on the same maps and photos
        composition_us   the unfused weighted composition, losses.composed_photo_loss(x, photos, table, eps, weights)
                         forward + backward through autograd: K1, the torch ops of the definition and their backward, K2

    `layout`: "per-photo" ([B,S,H,W] weights) or "shared" ([B,1,H,W])."""
    import ctypes
    import torch
    from bench import synthetic_maps
    from svbrdf_estimation_amd import environment, losses
    B, H, S = 8, 256, 9
    P = S if layout == "per-photo" else 1
    lib = native._load()
    gen = torch.Generator().manual_seed(5)
    torch.manual_seed(11)
    table = environment.BatchSceneSampler(B, 3, 6).sample().contiguous()
    ins = [synthetic_maps(gen, B, H, tied=True).to(dev) for _ in range(sets)]
    photos = [native.render_fwd(synthetic_maps(gen, B, H, tied=True).to(dev), table).clamp_(0.0, 1.0) for _ in range(sets)]
    u = [torch.rand((B, P, H, H), generator=gen) for _ in range(sets)]
    weights = [torch.where(t < 0.25, torch.zeros(()), torch.where(t >= 0.75, torch.ones(()), (t - 0.25) * 2.0)).to(dev) for t in u]
    grads = [torch.empty_like(a) for a in ins]
    leaves = [a.clone().requires_grad_(True) for a in ins]
    xr = native.xrow(dev, H)
    ws = torch.zeros(65, dtype=torch.int64, device=dev)
    loss = torch.empty(1, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def weighted(i):
        k = i % sets
        rc = lib.svbrdf_photo_loss_weighted_fwd_bwd_host_scenes(
            ins[k].data_ptr(), photos[k].data_ptr(), weights[k].data_ptr(), P, table.data_ptr(), xr.data_ptr(),
            ctypes.c_float(EPS), loss.data_ptr(), grads[k].data_ptr(), ws.data_ptr(), ws.numel() * 8, B, S, H, H, st)
        assert rc == 0, lib.svbrdf_last_error()

    def unweighted(i):
        k = i % sets
        rc = lib.svbrdf_photo_loss_fwd_bwd_host_scenes(ins[k].data_ptr(), photos[k].data_ptr(), table.data_ptr(), xr.data_ptr(),
                                                       ctypes.c_float(EPS), loss.data_ptr(), grads[k].data_ptr(), ws.data_ptr(),
                                                       ws.numel() * 8, B, S, H, H, st)
        assert rc == 0, lib.svbrdf_last_error()

    def composition(i):
        k = i % sets
        leaves[k].grad = None
        losses.composed_photo_loss(leaves[k], photos[k], table, EPS, weights[k]).backward()

    legs = (("weighted_us", weighted), ("unweighted_us", unweighted), ("composition_us", composition))
    out, res = photo_checks.timed_legs(legs, n, rounds, photo_checks.spinning_wave(native, dev), dev)
    out.update(rounds=res, device=torch.cuda.get_device_name(dev), steps_per_round=n, sets=sets, layout=layout, planes=P)
    out["weighted_frac_of_8TBps"] = (12 + 3 * S + P + 12) * 4 * H * H * B / (out["weighted_us"] * 1e-6) / 8.0e12
    return out
