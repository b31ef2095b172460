"""Shared by tests/test_pose_photo_loss_cpu.py and tests/test_gpu_pose_photo_loss.py: the ORACLE of the photo losses with
the gradient towards the scene table (csrc/svbrdf_photo_pose.hip), their cases and their speed measurement.  Nothing under
oracle/ changes for it.  The loss and the map gradient are photo_checks.Reference(x, photos, scenes, eps, head, weights) --
the kernels promise those of the existing entries bit for bit -- and the table gradient comes from
oracle.eager_torch.render_scene, the eager restatement of the reference's renderer, with the scene row as a DUAL NUMBER
(torch.autograd.forward_ad, one tangent per column: forward mode applies the same sub-gradient conventions as autograd's
backward -- clamp(min=m) passes the tangent iff x >= m):

    rad, d rad / d row_k = render_scene(maps[b], dual(scenes[b,s], e_k))       on the float32-valued inputs
    t[b,s,k,c,i,j] = w sign(delta) (d rad_c / d row_k) / (N (rad_c + eps))     delta = log(rad + eps) - log(p' + eps)
    G[b,s,k]       = sum_{c,i,j} t                                             once in fp32 and once in fp64

Bound per (b, s, k), the project's gradient contract summed over a plane (tolerances.assert_plane_sums_close does the same):
with A = sum |t64| and T = sum |t64| over the TIED terms (|delta64| < tolerances.TIE_LEVEL, not structural by photo_checks'
rule: a tied term's sign is rounding noise in any fp32 evaluation),

    |got - G64| <= GRAD_RTOL A + GRAD_ATOL_FRAC max(A) + 2 T,

max(A) taken per column group -- positions (0:6) and colours (6:9) have different units.
"""
import hashlib
import math

import numpy as np
import torch
import torch.autograd.forward_ad as fwAD

import exposure_photo_checks as xp
import photo_checks
import synth
import tolerances
import weighted_photo_checks as wp
from oracle import c_oracle, eager_torch

EPS = photo_checks.EPS
ENTRIES = ("svbrdf_photo_loss_scene_grad_fwd_bwd", "svbrdf_head_photo_loss_scene_grad_fwd_bwd")
WORKSPACE_BYTES = "svbrdf_photo_scene_grad_workspace_bytes"
LAYOUTS = (None,) + wp.LAYOUTS         # no weights, per-photo, shared
GROUPS = (slice(0, 6), slice(6, 9))    # positions | colours


_RENDERINGS = {}


def dual_renderings(maps, scenes, f64, batched=False):
    """-> (rad [B,S,3,H,W], d rad / d row [B,S,9,3,H,W] float64) of oracle.eager_torch.render_scene with each scene row a dual
    number; they depend on the maps and the table only, so the weight layouts of a case share them (kept per session).
    `batched`: per item one torch.vmap over the rows and the nine unit tangents of torch.func.jvp of the same function
    instead of B S 9 eager renders -- for tables of hundreds of rows (tests/many_photos_checks.py); the same bits
    (tests/test_many_photos_cpu.py holds the two against each other), kept apart all the same."""
    maps, scenes = np.ascontiguousarray(maps, np.float32), np.ascontiguousarray(scenes, np.float32)
    key = (hashlib.sha1(maps.tobytes()).hexdigest(), hashlib.sha1(scenes.tobytes()).hexdigest(), bool(f64), bool(batched))
    if key in _RENDERINGS:
        return _RENDERINGS[key]
    dtype = torch.float64 if f64 else torch.float32
    maps_t, sc = torch.from_numpy(maps).to(dtype), torch.from_numpy(scenes).to(dtype)
    B, S = sc.shape[:2]
    H, W = maps_t.shape[-2:]
    xrow = torch.from_numpy(c_oracle.make_xrow(W).astype(np.float32)).to(dtype)
    args = dict(xrow=xrow, pi=float(np.float32(math.pi)), clamp_min=float(np.float32(0.001)))
    rad = np.empty((B, S, 3, H, W), np.float64 if f64 else np.float32)
    drad = np.empty((B, S, 9, 3, H, W), np.float64)
    for b in range(B):
        if batched:
            render = lambda row: eager_torch.render_scene(maps_t[b], row, **args)[0]
            one = lambda row, tangent: torch.func.jvp(render, (row,), (tangent,))
            primal, tangent = torch.vmap(torch.vmap(one, in_dims=(None, 0)), in_dims=(0, None))(sc[b], torch.eye(9, dtype=dtype))
            rad[b], drad[b] = primal[:, 8].numpy(), tangent.numpy()       # (the loop keeps the primal of its last tangent)
            continue
        for s in range(S):
            for k in range(9):
                with fwAD.dual_level():
                    row = fwAD.make_dual(sc[b, s], torch.eye(9, dtype=dtype)[k])
                    out = fwAD.unpack_dual(eager_torch.render_scene(maps_t[b], row, **args))
                    tangent = out.tangent if out.tangent is not None else torch.zeros_like(out.primal)
                    rad[b, s], drad[b, s, k] = out.primal[0].numpy(), tangent[0].numpy()
    _RENDERINGS[key] = (rad, drad)
    return rad, drad


def pose_terms(maps, photos, scenes, weights, f64, eps=EPS, batched=False):
    """-> (t [B,S,9,3,H,W] float64, delta [B,S,3,H,W]): the terms of d loss / d scenes on the 12-channel `maps`, evaluated in
    fp32 or fp64 on the same float32-valued inputs (pixel row, pi and the clamp with their float32 values, as the C
    oracle's float64 instantiation has them)"""
    S = np.shape(scenes)[1]
    if weights is None:
        ph, w = np.asarray(photos, np.float32), 1.0
    else:
        ph = photo_checks.excused_photos(photos, weights)
        w = photo_checks.broadcast_weights(weights, S).astype(np.float64)[:, :, None]
    rad, drad = dual_renderings(maps, scenes, f64, batched)
    e = np.float64(np.float32(eps)) if f64 else np.float32(eps)
    a, bb = rad + e, (ph.astype(np.float64) if f64 else ph) + e
    with np.errstate(invalid="ignore", divide="ignore"):
        delta = np.log(a) - np.log(bb)
    g = w * np.sign(delta).astype(np.float64) / (float(delta.size) * a.astype(np.float64))     # d loss / d rad
    return g[:, :, None] * drad, delta


class PoseReference:
    """the oracle's values of one case, computed once: `ref` (photo_checks.Reference: loss, map gradient, ties), G32 / G64
    [B,S,9], the bound's A and T, and the conditions on the inputs"""

    def __init__(self, x, photos, scenes, eps=EPS, head=False, weights=None, batched=False):
        self.scenes = np.ascontiguousarray(scenes, np.float32)
        self.ref = photo_checks.Reference(x, photos, self.scenes, eps, head=head, weights=weights)
        t32, d32 = pose_terms(self.ref.maps, photos, self.scenes, weights, False, eps, batched)
        t64, d64 = pose_terms(self.ref.maps, photos, self.scenes, weights, True, eps, batched)
        self.G32, self.G64 = t32.sum(axis=(3, 4, 5)), t64.sum(axis=(3, 4, 5))
        self.A = np.abs(t64).sum(axis=(3, 4, 5))
        ph = np.asarray(photos, np.float32) if weights is None else photo_checks.excused_photos(photos, weights)
        self.n_dot_wi = photo_checks.unclamped_n_dot_wi(self.ref.maps, self.scenes)
        structural = (ph == 0.0) & (self.n_dot_wi < -1e-6)[:, :, None]
        if weights is not None:
            structural |= (photo_checks.broadcast_weights(weights, ph.shape[1]) == 0.0)[:, :, None]
        tied = (np.abs(d64) < tolerances.TIE_LEVEL) & ~structural
        self.tied_terms = int(tied.sum())
        self.T = np.where(tied[:, :, None], np.abs(t64), 0.0).sum(axis=(3, 4, 5))
        self.sign_flips = int(((np.sign(d32) != np.sign(d64)) & ~tied & ~structural).sum())
        self.bound = tolerances.GRAD_RTOL * self.A + 2.0 * self.T
        for grp in GROUPS:
            self.bound[..., grp] += tolerances.GRAD_ATOL_FRAC * self.A[..., grp].max()

    def worst(self, got):
        """-> (worst |got - G64| / bound, worst |got - G64| / A)"""
        err = np.abs(np.asarray(got, np.float64) - self.G64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return float((err / self.bound).max()), float(np.nanmax(np.where(self.A > 0, err / self.A, 0.0)))

    def assert_scene_grad_close(self, got, what):
        got = np.asarray(got, np.float64)
        assert got.shape == self.G64.shape and np.isfinite(got).all(), what
        err = np.abs(got - self.G64)
        ratio = err / self.bound
        print("[pose] %-52s worst err/bound %.3e  err/A %.3e" % ((what,) + self.worst(got)))
        assert not (err > self.bound).any(), "%s: %d of %d scene gradients outside the bound, worst err/bound %.3g at %s (got %.9g, f64 %.9g)" % (
            what, int((err > self.bound).sum()), err.size, float(ratio.max()), np.unravel_index(np.argmax(ratio), err.shape),
            got.flat[np.argmax(ratio)], self.G64.flat[np.argmax(ratio)])


_REFERENCES = {}


def reference(name, layout, head):
    """(case inputs, PoseReference) of one of weighted_photo_checks.CASES; layout None: no weights"""
    key = (name, layout, bool(head))
    if key not in _REFERENCES:
        c = wp.case_inputs(name)
        w = None if layout is None else c["weights"][layout]
        _REFERENCES[key] = (c, PoseReference(c["enc"] if head else c["maps"], c["photos"], c["scenes"], EPS, head, w))
    return _REFERENCES[key]


BIG_PARAMS = [(layout, head) for layout in LAYOUTS for head in (False, True)]


def big_case(layout="per-photo", head=False):
    """the 80-workgroup shape (64 x 64, S = 9, B = 5: more workgroups than loss_arrive has slots) in every weight layout, maps
    and head: exposure_photo_checks' maps, photos, table and per-photo weights, a shared weight plane and an encoded input
    beside them -> (case inputs, PoseReference)"""
    key = ("big", layout, bool(head))
    if key not in _REFERENCES:
        if "big inputs" not in _REFERENCES:
            c = dict(xp.big_case()[0])
            B, H = xp.BIG["B"], xp.BIG["H"]
            c["enc"] = wp.encoded_input(6490, B, H)
            c["weights"] = {"per-photo": c["weights"]["per-photo"], "shared": wp.weight_field(6390, B, 1, H)}
            _REFERENCES["big inputs"] = c
        c = _REFERENCES["big inputs"]
        w = None if layout is None else c["weights"][layout]
        _REFERENCES[key] = (c, PoseReference(c["enc"] if head else c["maps"], c["photos"], c["scenes"], EPS, head, w))
    return _REFERENCES[key]


WAVE_LIMIT = 2.0 ** 19      # csrc/svbrdf_photo_pose.hip: a wave's sum of N |term| beyond this makes the loss NaN


def overflow_case():
    """17_s1 (B = 2, S = 1, no weights) with the camera of item 0 put 1e-9 above pixel (3, 5): d wo / d camera is 1 / |camera -
    P| = 1e9 there, so that pixel's finite terms carry its wave's sum of N |d term / d camera| far beyond the kernels' limit of
    2^19, while every rendering and the loss stay finite.  -> (case inputs with that table, the oracle's float64 loss, the
    largest |wave sum| of N t64 over the waves of 64 pixels and the camera columns)"""
    if "overflow" not in _REFERENCES:
        c = dict(wp.case_inputs("17_s1"))
        H = c["H"]
        xrow = c_oracle.make_xrow(H).astype(np.float32)
        sc = c["scenes"].copy()
        sc[0, 0, 0:3] = (xrow[5], -xrow[3], np.float32(1e-9))
        c["scenes"] = sc
        t64, _ = pose_terms(c["maps"], c["photos"], sc, None, True)
        loss64 = photo_checks.oracle_photo_loss(c["maps"], c["photos"], sc, EPS, f64=True, want_grad=False)[0]
        per_pixel = float(t64[..., 0, 0].size * 3) * t64.sum(axis=3).reshape(2, 1, 9, H * H)       # N t, channels summed
        pad = (-H * H) % 64
        waves = np.pad(per_pixel, ((0, 0), (0, 0), (0, 0), (0, pad))).reshape(2, 1, 9, -1, 64).sum(axis=-1)
        _REFERENCES["overflow"] = (c, loss64, float(np.abs(waves[:, :, 0:3]).max()))
    return _REFERENCES["overflow"]


def edge_case():
    """17 x 17, B = 2, S = 2 with hand-made rows: row 0 a LOW LIGHT beside the patch (n.wi < 0 on part of it: LN+ = 0 there and
    the photo is 0, both sides of the term exactly eps), row 1 a GRAZING CAMERA (n.wo below its clamp of 1e-3 on part of
    the patch).  -> (case inputs, PoseReference, pixels with LN+ = 0 under row 0, pixels with VN clamped under row 1)"""
    if "edge" not in _REFERENCES:
        B, H = 2, 17
        maps, target = synth.make_maps(6500, B, H), synth.make_maps(6501, B, H)
        row_light = [0.1, -0.2, 2.0, 1.6, 0.3, 0.04, 3.0, 2.5, 2.0]
        row_camera = [-1.7, 0.2, 0.03, 0.3, 0.4, 1.5, 2.0, 2.0, 3.0]
        sc = np.ascontiguousarray(np.broadcast_to(np.array([row_light, row_camera], np.float32), (B, 2, 9)))
        photos = np.clip(c_oracle.render_fwd(target, sc), 0.0, 1.0)
        # where the light is behind the INPUT's surface the photo is taken as dark too: the structural term of photo_checks
        dark = photo_checks.unclamped_n_dot_wi(maps, sc) < 0.0
        photos = np.where(dark[:, :, None], np.float32(0.0), photos).astype(np.float32)
        c = dict(name="17_edge", H=H, S=2, maps=maps, photos=photos, scenes=sc, weights={})
        r = PoseReference(maps, photos, sc, EPS, False, None)
        cam = sc.copy()
        cam[:, :, 3:6] = sc[:, :, 0:3]              # n . wo by the helper for n . wi, with the camera as the "light"
        n_dot_wo = photo_checks.unclamped_n_dot_wi(maps, cam)
        _REFERENCES["edge"] = (c, r, int((r.n_dot_wi[:, 0] < 0.0).sum()), int((n_dot_wo[:, 1] < 1e-3).sum()))
    return _REFERENCES["edge"]


def composed_scene_grad(maps, photos, scenes, weights, head=False, eps=EPS, device="cpu"):
    """the package's composed definition in float64 with the table as a leaf -> (loss: float, d loss / d scenes [B,S,9])"""
    from svbrdf_estimation_amd import losses
    x = torch.from_numpy(np.ascontiguousarray(maps, np.float32)).to(device, torch.float64)
    table = torch.from_numpy(np.ascontiguousarray(scenes, np.float32)).to(device).requires_grad_(True)
    ph = torch.from_numpy(np.ascontiguousarray(photos, np.float32)).to(device)
    w = None if weights is None else torch.from_numpy(np.ascontiguousarray(weights, np.float32)).to(device)
    loss = losses.composed_photo_loss(losses.decode_head(x) if head else x, ph, table, eps, w)
    loss.backward()
    return loss.item(), table.grad.cpu().numpy()


# ------------------------------------------------------------------------------------------------ the speed measurement

def measure_pose_photo_loss(dev, native, sets=6, n=40, rounds=3):
    """-> dict of medians (us per step) at the configuration-2 shape, B = 8, 256 x 256, S = 9, per-photo weights, `sets`
    rotating batches, one process, the legs alternating round by round (exposure_photo_checks' method):

        pose_us          the scene-gradient entry: loss, map gradient and table gradient, ONE launch
        weighted_us      the existing device-table weighted entry on the same table: the same work without the table gradient
        composition_us   losses.composed_photo_loss with the table as a leaf, forward + backward through autograd: the
                         stock-torch-op render (renderers.render_table), the only other way to that gradient"""
    import ctypes
    from bench import synthetic_maps
    from svbrdf_estimation_amd import environment, losses
    B, H, S = 8, 256, 9
    lib = native._load()
    gen = torch.Generator().manual_seed(5)
    torch.manual_seed(11)
    table = environment.BatchSceneSampler(B, 3, 6).sample().contiguous().to(dev)
    ins = [synthetic_maps(gen, B, H, tied=True).to(dev) for _ in range(sets)]
    photos = [native.render_fwd(synthetic_maps(gen, B, H, tied=True).to(dev), table).clamp_(0.0, 1.0) for _ in range(sets)]
    u = [torch.rand((B, S, H, H), generator=gen) for _ in range(sets)]
    weights = [torch.where(t < 0.25, torch.zeros(()), torch.where(t >= 0.75, torch.ones(()), (t - 0.25) * 2.0)).to(dev) for t in u]
    grads = [torch.empty_like(a) for a in ins]
    leaves = [a.clone().requires_grad_(True) for a in ins]
    t_leaf = table.clone().requires_grad_(True)
    grad_s = torch.empty_like(table)
    xr = native.xrow(dev, H)
    ws = torch.zeros(getattr(lib, WORKSPACE_BYTES)(B, S, H, H) // 8, dtype=torch.int64, device=dev)
    loss = torch.empty(1, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def pose(i):
        k = i % sets
        rc = lib.svbrdf_photo_loss_scene_grad_fwd_bwd(
            ins[k].data_ptr(), photos[k].data_ptr(), weights[k].data_ptr(), S, table.data_ptr(), xr.data_ptr(),
            ctypes.c_float(EPS), loss.data_ptr(), grads[k].data_ptr(), grad_s.data_ptr(), ws.data_ptr(), ws.numel() * 8,
            B, S, H, H, st)
        assert rc == 0, lib.svbrdf_last_error()

    def weighted(i):
        k = i % sets
        rc = lib.svbrdf_photo_loss_weighted_fwd_bwd(
            ins[k].data_ptr(), photos[k].data_ptr(), weights[k].data_ptr(), S, table.data_ptr(), xr.data_ptr(),
            ctypes.c_float(EPS), loss.data_ptr(), grads[k].data_ptr(), ws.data_ptr(), ws.numel() * 8, B, S, H, H, st)
        assert rc == 0, lib.svbrdf_last_error()

    def composition(i):
        k = i % sets
        leaves[k].grad = None
        t_leaf.grad = None
        losses.composed_photo_loss(leaves[k], photos[k], t_leaf, EPS, weights[k]).backward()

    legs = (("pose_us", pose), ("weighted_us", weighted), ("composition_us", composition))
    out, res = photo_checks.timed_legs(legs, n, rounds, photo_checks.spinning_wave(native, dev), dev)
    out.update(rounds=res, device=torch.cuda.get_device_name(dev), steps_per_round=n, sets=sets)
    return out
