"""Shared by tests/test_exposure_photo_loss_cpu.py and tests/test_gpu_exposure_photo_loss.py: the ORACLE of the photo losses
with a per-photo exposure (csrc/svbrdf_photo_exposure.hip), their cases and their speed measurement.  Nothing under oracle/
changes for it: with

    scenes' = scenes whose columns 6:9 (the light colour) were multiplied by e[b,s,:] in float32

the loss and the map gradient are photo_checks.Reference(x, photos, scenes', eps, head, weights) -- the kernels promise those
bit for bit on that table -- and the exposure gradient is

    rad = c_oracle.render_fwd(maps, scenes', f64=...)
    t   = w sign(delta) rad / (N (rad + eps) e)          per term (b, s, c, i, j), delta = log(rad + eps) - log(p' + eps)
    G   = sum_{i,j} t                                     per (b, s, c), once in fp32 and once in fp64

Bound per (b, s, c), the project's gradient contract summed over a plane (tolerances.assert_plane_sums_close does the same):
with A = sum |t64| and T = sum |t64| over the TIED terms (|delta64| < tolerances.TIE_LEVEL, not structural by photo_checks'
rule: a tied term's sign is rounding noise in any fp32 evaluation),

    |got - G64| <= GRAD_RTOL A + GRAD_ATOL_FRAC max(A) + 2 T.
"""
import numpy as np

import photo_checks
import synth
import tolerances
import weighted_photo_checks as wp
from oracle import c_oracle

EPS = photo_checks.EPS
ENTRIES = ("svbrdf_photo_loss_exposure_fwd_bwd", "svbrdf_head_photo_loss_exposure_fwd_bwd")
WORKSPACE_BYTES = "svbrdf_photo_exposure_workspace_bytes"
LAYOUTS = (None,) + wp.LAYOUTS         # no weights, per-photo, shared


def scaled_table(scenes, e):
    """scenes' : columns 6:9 times e, one float32 multiply each"""
    sc = np.array(scenes, np.float32, copy=True)
    sc[:, :, 6:9] = (sc[:, :, 6:9] * np.asarray(e, np.float32)).astype(np.float32)
    return sc


def exposure_terms(maps, photos, scenes, e, weights, f64, eps=EPS):
    """-> (t [B,S,3,H,W] float64, delta): the terms of d loss / d e on the 12-channel `maps`, evaluated in fp32 or fp64"""
    e = np.asarray(e, np.float32)
    sc = scaled_table(scenes, e)
    S = sc.shape[1]
    if weights is None:
        ph, w = np.asarray(photos, np.float32), 1.0
    else:
        ph = photo_checks.excused_photos(photos, weights)
        w = photo_checks.broadcast_weights(weights, S).astype(np.float64)[:, :, None]
    rad = c_oracle.render_fwd(np.ascontiguousarray(maps, np.float32), sc, f64=f64)
    if f64:
        a, b = rad + np.float64(np.float32(eps)), ph.astype(np.float64) + np.float64(np.float32(eps))
    else:
        a, b = rad + np.float32(eps), ph + np.float32(eps)
    with np.errstate(invalid="ignore", divide="ignore"):
        delta = np.log(a) - np.log(b)
    share = (rad / a).astype(np.float64) if not f64 else rad / a
    t = w * np.sign(delta).astype(np.float64) * share / float(delta.size) / e.astype(np.float64)[:, :, :, None, None]
    return t, delta


class ExposureReference:
    """the oracle's values of one case with exposure `e` [B,S,3], computed once: `ref` (photo_checks.Reference on the
    pre-scaled table: loss, map gradient, ties), G32 / G64 [B,S,3], the bound's A and T, and the two conditions on the inputs"""

    def __init__(self, x, photos, scenes, e, eps=EPS, head=False, weights=None):
        self.e = np.ascontiguousarray(e, np.float32)
        self.scaled = scaled_table(scenes, self.e)
        self.ref = photo_checks.Reference(x, photos, self.scaled, eps, head=head, weights=weights)
        t32, d32 = exposure_terms(self.ref.maps, photos, scenes, self.e, weights, False, eps)
        t64, d64 = exposure_terms(self.ref.maps, photos, scenes, self.e, weights, True, eps)
        self.t64 = t64
        self.G32, self.G64 = t32.sum(axis=(3, 4)), t64.sum(axis=(3, 4))
        self.A = np.abs(t64).sum(axis=(3, 4))
        ph = np.asarray(photos, np.float32) if weights is None else photo_checks.excused_photos(photos, weights)
        structural = (ph == 0.0) & (photo_checks.unclamped_n_dot_wi(self.ref.maps, self.scaled) < -1e-6)[:, :, None]
        if weights is not None:
            structural |= (photo_checks.broadcast_weights(weights, ph.shape[1]) == 0.0)[:, :, None]
        tied = (np.abs(d64) < tolerances.TIE_LEVEL) & ~structural
        self.tied_terms = int(tied.sum())
        self.T = np.where(tied, np.abs(t64), 0.0).sum(axis=(3, 4))
        self.sign_flips = int(((np.sign(d32) != np.sign(d64)) & ~tied & ~structural).sum())
        self.bound = tolerances.GRAD_RTOL * self.A + tolerances.GRAD_ATOL_FRAC * self.A.max() + 2.0 * self.T

    def worst(self, got):
        """-> (worst |got - G64| / bound, worst |got - G64| / A)"""
        err = np.abs(np.asarray(got, np.float64) - self.G64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return float((err / self.bound).max()), float(np.nanmax(np.where(self.A > 0, err / self.A, 0.0)))

    def assert_exposure_grad_close(self, got, what):
        got = np.asarray(got, np.float64)
        assert got.shape == self.G64.shape and np.isfinite(got).all(), what
        err = np.abs(got - self.G64)
        bad = err > self.bound
        assert not bad.any(), "%s: %d of %d exposure gradients outside the bound, worst err/bound %.3g at %s (got %.9g, f64 %.9g)" % (
            what, int(bad.sum()), bad.size, float((err / self.bound).max()), np.unravel_index(np.argmax(err / self.bound), err.shape),
            got.flat[np.argmax(err / self.bound)], self.G64.flat[np.argmax(err / self.bound)])


def exposure_of(H, S, B=wp.B_CASES):
    """the gains of a case: uniform in [0.5, 2)"""
    return (np.float32(0.5) + np.float32(1.5) * synth.uniform01(7000 + H + S, (B, S, 3))).astype(np.float32)


_REFERENCES = {}


def reference(name, layout, head):
    """(case inputs, exposure, ExposureReference) of one of weighted_photo_checks.CASES; layout None: no weights"""
    key = (name, layout, bool(head))
    if key not in _REFERENCES:
        c = wp.case_inputs(name)
        e = exposure_of(c["H"], c["S"])
        w = None if layout is None else c["weights"][layout]
        _REFERENCES[key] = (c, e, ExposureReference(c["enc"] if head else c["maps"], c["photos"], c["scenes"], e, EPS, head, w))
    return _REFERENCES[key]


# one more case: 64 x 64, S = 9, B = 5 -> 80 workgroups, more than loss_arrive's 64 slots
BIG = dict(name="64_s9_b5", H=64, S=9, B=5)


def big_case():
    if "big" not in _REFERENCES:
        B, H = BIG["B"], BIG["H"]
        sc = photo_checks.scene_table(B, 41, 3, 6)
        maps, target = synth.make_maps(6190, B, H), synth.make_maps(6191, B, H)
        photos = np.clip(c_oracle.render_fwd(target, sc), 0.0, 1.0)
        w = wp.weight_field(6290, B, 9, H)
        e = exposure_of(H, 9, B)
        c = dict(name=BIG["name"], H=H, S=9, maps=maps, photos=photos, scenes=sc, weights={"per-photo": w})
        _REFERENCES["big"] = (c, e, ExposureReference(maps, photos, sc, e, EPS, False, w))
    return _REFERENCES["big"]


# ------------------------------------------------------------------------------------------------ the speed measurement

def measure_exposure_photo_loss(dev, native, sets=6, n=40, rounds=3):
    """-> dict of medians (us per step) at the configuration-2 shape, B = 8, 256 x 256, S = 9, per-photo weights, `sets`
    rotating batches, one process, the legs alternating round by round (the method of
    weighted_photo_checks.measure_weighted_photo_loss):

        exposure_us      the exposure entry with grad_exposure: loss and both gradients, ONE launch
        weighted_us      the existing device-table weighted entry on the pre-scaled table: the same work without the
                         reduction of the exposure gradient
        composition_us   losses.composed_photo_loss with an exposure leaf, forward + backward through autograd"""
    import ctypes
    import torch
    from bench import synthetic_maps
    from svbrdf_estimation_amd import environment, losses
    B, H, S = 8, 256, 9
    lib = native._load()
    gen = torch.Generator().manual_seed(5)
    torch.manual_seed(11)
    table = environment.BatchSceneSampler(B, 3, 6).sample().contiguous().to(dev)
    e = (0.5 + 1.5 * torch.rand((B, S, 3), generator=gen)).to(dev)
    scaled = torch.cat((table[..., :6], table[..., 6:] * e), dim=-1).contiguous()
    ins = [synthetic_maps(gen, B, H, tied=True).to(dev) for _ in range(sets)]
    photos = [native.render_fwd(synthetic_maps(gen, B, H, tied=True).to(dev), table).clamp_(0.0, 1.0) for _ in range(sets)]
    u = [torch.rand((B, S, H, H), generator=gen) for _ in range(sets)]
    weights = [torch.where(t < 0.25, torch.zeros(()), torch.where(t >= 0.75, torch.ones(()), (t - 0.25) * 2.0)).to(dev) for t in u]
    grads = [torch.empty_like(a) for a in ins]
    leaves = [a.clone().requires_grad_(True) for a in ins]
    e_leaf = e.clone().requires_grad_(True)
    grad_e = torch.empty_like(e)
    xr = native.xrow(dev, H)
    ws = torch.zeros(lib.svbrdf_photo_exposure_workspace_bytes(B, S, H, H) // 8, dtype=torch.int64, device=dev)
    loss = torch.empty(1, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def exposure(i):
        k = i % sets
        rc = lib.svbrdf_photo_loss_exposure_fwd_bwd(
            ins[k].data_ptr(), photos[k].data_ptr(), weights[k].data_ptr(), S, e.data_ptr(), table.data_ptr(), xr.data_ptr(),
            ctypes.c_float(EPS), loss.data_ptr(), grads[k].data_ptr(), grad_e.data_ptr(), ws.data_ptr(), ws.numel() * 8,
            B, S, H, H, st)
        assert rc == 0, lib.svbrdf_last_error()

    def weighted(i):
        k = i % sets
        rc = lib.svbrdf_photo_loss_weighted_fwd_bwd(
            ins[k].data_ptr(), photos[k].data_ptr(), weights[k].data_ptr(), S, scaled.data_ptr(), xr.data_ptr(),
            ctypes.c_float(EPS), loss.data_ptr(), grads[k].data_ptr(), ws.data_ptr(), ws.numel() * 8, B, S, H, H, st)
        assert rc == 0, lib.svbrdf_last_error()

    def composition(i):
        k = i % sets
        leaves[k].grad = None
        e_leaf.grad = None
        losses.composed_photo_loss(leaves[k], photos[k], table, EPS, weights[k], e_leaf).backward()

    legs = (("exposure_us", exposure), ("weighted_us", weighted), ("composition_us", composition))
    out, res = photo_checks.timed_legs(legs, n, rounds, photo_checks.spinning_wave(native, dev), dev)
    out.update(rounds=res, device=torch.cuda.get_device_name(dev), steps_per_round=n, sets=sets)
    return out
