"""Shared by tests/test_many_photos_cpu.py and tests/test_gpu_many_photos.py: the photo-loss family at MANY photos per item,
up to the limits the header documents (S <= 1706 forward-only, 1278 with exposure, 425 with the scene gradient, 383 for
the two fit steps with it, B S <= 288 for the by-value table).  The cases, their oracle values -- photo_checks.Reference,
exposure_photo_checks.ExposureReference and pose_photo_checks.PoseReference with the BATCHED dual-number renderings --, the
restatement of plan_loss's fixed-point rule, the LDS budget of the kernels that take dynamic LDS, and the direct C ABI calls
with guard words behind the per-scene gradients.

Every case is 17 x 17: 289 pixels, two workgroups, the second holding one partial wave and three waves without pixels.
Which S takes which path:

    S >= 22     second trip of `for (i = lane; i < 3 S; i += 64)`, the gain / colour check of exposure_body, pose_body, joint_body
    S >= 29     n_sums = 9 S > 256: second trip of photo_sums_finish's add loop; second trip of photo_loss_body's staging loop
    S >= 86     n_sums = 3 S > 256 for the exposure kernels
    B S = 288   the full by-value block
    S >= 330    (17 x 17, B = 2) plan_loss's fixed-point scale drops below 2^24: k = 23 at 383 and 425, 22 at 1278, 21 at
                1706 with B = 1
"""
import ctypes
import re

import numpy as np

import exposure_photo_checks as xp
import photo_checks
import photo_fit_checks as fc
import pose_photo_checks as pc
import synth
import tolerances
import weighted_photo_checks as wp
from oracle import c_oracle

EPS = photo_checks.EPS
H = 17
LAYOUTS = (None,) + wp.LAYOUTS         # no weights, per-photo, shared
MAX_TIED_TERMS = 8

# name: (S, B, n_random, n_specular, tied roughness)
CASES = {
    "s22": (22, 2, 8, 14, True),
    "s29": (29, 2, 10, 19, True),
    "s29_untied": (29, 2, 10, 19, False),
    "s86": (86, 2, 29, 57, True),
    "s144": (144, 2, 48, 96, True),
    "s383": (383, 2, 128, 255, True),
    "s425": (425, 2, 142, 283, True),
    "s1278": (1278, 2, 426, 852, True),
    "s1706_b1": (1706, 1, 569, 1137, True),
}
# the fixed-point exponent each case is chosen for (plan_loss; restated below)
EXPONENTS = {"s1707_b1": 21, "s22": 24, "s29": 24, "s29_untied": 24, "s86": 24, "s144": 24, "s383": 23, "s425": 23, "s1278": 22, "s1706_b1": 21}

_INPUTS = {}


def case_inputs(name):
    """-> dict of one case, built as weighted_photo_checks.case_inputs builds its own: maps, enc, photos = clip(oracle's
    rendering of other maps, 0, 1), scenes, the weight field in both layouts and the gains `e` [B,S,3] (the photos are taken
    without them, as exposure_photo_checks.reference has it); kept per session"""
    if name == "s1707_b1" and name not in _INPUTS:
        # one scene more than the forward-only stage holds: s1706_b1 with a 1707th row, photo and weight plane made of its own
        c = case_inputs("s1706_b1")
        more = lambda a, i, f=1.0: np.ascontiguousarray(np.concatenate((a, a[:, i:i + 1] * np.float32(f)), axis=1))
        _INPUTS[name] = dict(c, name=name, S=1707, scenes=more(c["scenes"], 3, 1.01), photos=more(c["photos"], 3),
                             weights={"per-photo": more(c["weights"]["per-photo"], 5), "shared": c["weights"]["shared"]},
                             e=xp.exposure_of(H, 1707, 1))
    if name not in _INPUTS:
        S, B, nr, ns, tied = CASES[name]
        assert nr + ns == S
        sc = photo_checks.scene_table(B, 900 + S, nr, ns)
        maps = synth.make_maps(7000 + S, B, H, tiled_roughness=tied)
        target = synth.make_maps(7001 + S, B, H, tiled_roughness=tied)
        photos = np.clip(c_oracle.render_fwd(target, sc), 0.0, 1.0)
        weights = {"per-photo": wp.weight_field(7100 + S, B, S, H), "shared": wp.weight_field(7200 + S, B, 1, H)}
        _INPUTS[name] = dict(name=name, H=H, S=S, B=B, tied=tied, maps=maps, enc=wp.encoded_input(7300 + S, B, H),
                             photos=photos, scenes=sc, weights=weights, e=xp.exposure_of(H, S, B))
    return _INPUTS[name]


def what(name, layout, head):
    return "%s %s %s" % (name, layout or "unweighted", "head" if head else "maps")


_REFERENCES = {}


def reference(kind, name, layout, head):
    """the oracle's values of (case, weight layout, maps or head), computed once per session and left unchanged.  kind
    "photo" -> (case, photo_checks.Reference); "exposure" -> (case, ExposureReference with the case's gains); "pose" -> (case,
    PoseReference on the batched dual-number renderings)"""
    key = (kind, name, layout, bool(head))
    if key not in _REFERENCES:
        c = case_inputs(name)
        x, w = (c["enc"] if head else c["maps"]), (None if layout is None else c["weights"][layout])
        if kind == "photo":
            R = photo_checks.Reference(x, c["photos"], c["scenes"], EPS, head=head, weights=w)
        elif kind == "exposure":
            R = xp.ExposureReference(x, c["photos"], c["scenes"], c["e"], EPS, head, w)
        else:
            assert kind == "pose", kind
            R = pc.PoseReference(x, c["photos"], c["scenes"], EPS, head, w, batched=True)
        _REFERENCES[key] = (c, R)
    return _REFERENCES[key]


def conditions(kind, R):
    """-> (tie pixels, elements that need the 2|ref - f64| widening, tied terms, sign flips, the fp32 oracle's own worst
    err / bound of the per-scene gradient or None) of a reference"""
    ref = R if kind == "photo" else R.ref
    own = None if kind == "photo" else R.worst(R.G32)[0]
    return (ref.n_ties(), ref.n_widened(), 0 if kind == "photo" else R.tied_terms, 0 if kind == "photo" else R.sign_flips, own)


def assert_conditions(kind, R, label):
    """THE CONDITIONS ON THE INPUTS, by the oracle alone: caps, not measurements"""
    ties, widened, tied, flips, own = conditions(kind, R)
    print("[many-photos] %-44s %-8s tie pixels %d, widened %d, tied terms %d, sign flips %d%s" % (
        label, kind, ties, widened, tied, flips, "" if own is None else ", fp32 oracle's own err/bound %.3g" % own))
    assert ties <= tolerances.MAX_TIE_PIXELS and widened <= tolerances.MAX_WIDENED_GRAD, (label, ties, widened)
    assert tied <= MAX_TIED_TERMS and flips == 0, (label, tied, flips)
    return ties, widened, tied, flips, own


# What the GPU tests compare at: (kind, case, layout, head).  The CPU test holds every one to the conditions above.
def _uses():
    out = []
    for name in ("s29", "s29_untied", "s425", "s1706_b1"):
        out += [("photo", name, l, h) for l in LAYOUTS for h in ((False, True) if CASES[name][4] else (False,))]
    out += [("photo", name, l, h) for name in ("s144", "s1707_b1") for l in (None, "per-photo") for h in (False, True)]
    for name in ("s22", "s86", "s1278"):
        out += [("exposure", name, l, h) for l in LAYOUTS for h in (False, True)]
    for name in ("s22", "s29", "s29_untied", "s425"):
        out += [("pose", name, l, h) for l in LAYOUTS for h in ((False, True) if CASES[name][4] else (False,))]
    out += [("pose", "s383", l, False) for l in (None, "per-photo")]
    return out


USES = _uses()


# ------------------------------------------------------------------------------------------------ plan_loss's rule, restated

LOSS_SLOTS, LOSS_THREADS, COUNT_SHIFT = 64, 256, 48


# The cases whose loss the kernels do NOT give within tolerances.LOSS_RTOL = 1e-6 of the oracle's, with the relative error
# measured on an MI355X (profiles/r24_many_photos.txt).  A thread adds the 3 S terms of its pixel one after the other in
# float32; sequential_sum_loss below does the same to the ORACLE's terms on the CPU and lands on these figures (1.27e-6,
# 1.48e-6, 1.95e-6 for the three unweighted ones), so the error is the sum's and not the terms'.  Every other case passes 1e-6
# and is held to it; these are held to sequential_sum_bound.  All are head cases at S >= 425: the 12-map cases stay near
# 1e-7 at every S.
LOSS_BEYOND_RTOL = {("s425", None, True): 1.21e-6, ("s1278", None, True): 1.42e-6, ("s1278", "shared", True): 1.02e-6,
                    ("s1706_b1", None, True): 1.94e-6, ("s1707_b1", None, True): 2.01e-6}


def fixed_point_exponent(B, S, H, W):
    """k of plan_loss (csrc/svbrdf_host.h): the partial sums are kept in units of 2^-k, k = 24 unless a slot's worst case
    -- |dlog| <= 32 per term: count 32 / 64 terms' worth from its workgroups and 32 * 256 * 3 S from one more -- could then
    reach 2^47"""
    count = float(B) * S * 3.0 * float(H) * W
    worst = count * 32.0 / LOSS_SLOTS + 32.0 * LOSS_THREADS * 3 * S
    k = 24
    while k > 0 and worst * 2.0 ** k >= 2.0 ** (COUNT_SHIFT - 1):
        k -= 1
    return k


def rule_in_source(text):
    """the rule as csrc/svbrdf_host.h states it -> (start exponent, the worst-case expression, the loop's condition and
    step) with the blanks squeezed out: what the restatement restates"""
    m = re.search(r"int k = (\d+);\s*const double l1_share = [^;]+;\s*const double worst_per_slot = ([^;]+);\s*"
                  r"while \(([^\n]+)\) ([^;]+);\s*out->fixed_scale = \(float\)std::ldexp\(1\.0, k\);", text)
    assert m, "plan_loss's rule is no longer where it was"
    return tuple(re.sub(r"\s+", "", g) for g in m.groups())


RULE = ("24", "(count*32.0/(double)kLossSlots+32.0*kLossThreads*3*S)*l1_share",
        "k>0&&worst_per_slot*std::ldexp(1.0,k)>=std::ldexp(1.0,kLossCountShift-1)", "--k")


# ------------------------------------------------------------------------------------------------ the LDS budget

LDS_BUDGET = 65536      # what the launchers' 60 * 1024 of dynamic LDS was chosen against
ROW_BYTES = LOSS_THREADS // 64 * 4
# unit: (kernel name prefix, spill words, sums per scene, the header's S limit)
LDS_UNITS = {
    "svbrdf_photo_pose": ("k_pose_", 9, 9, 425),
    "svbrdf_photo_exposure": ("k_exposure_", 4, 3, 1278),
    "svbrdf_photo_fit_pose": ("k_joint_fit", 9, 9, 383),
    "svbrdf_photo_fit_smooth": ("k_smooth_joint", 9, 9, 383),
}


def largest_dynamic_lds(unit):
    _, spill, per_scene, s_max = LDS_UNITS[unit]
    return ROW_BYTES * (spill + per_scene * s_max)


def static_lds(asm):
    """{kernel symbol: static LDS bytes} from a unit's device assembly (.amdhsa_group_segment_fixed_size of each kernel
    descriptor)"""
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel\s+(\S+)(.*?)\.end_amdhsa_kernel", asm, re.S):
        size = re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", m.group(2))
        assert size, m.group(1)
        out[m.group(1)] = int(size.group(1))
    return out


# ------------------------------------------------------------------------------------------------ the C ABI, guarded

SUMS_ENTRIES = {("pose", False): "svbrdf_photo_loss_scene_grad_fwd_bwd", ("pose", True): "svbrdf_head_photo_loss_scene_grad_fwd_bwd",
                ("exposure", False): "svbrdf_photo_loss_exposure_fwd_bwd", ("exposure", True): "svbrdf_head_photo_loss_exposure_fwd_bwd"}
SUMS_BYTES = {"pose": pc.WORKSPACE_BYTES, "exposure": xp.WORKSPACE_BYTES}


def abi_sums(native, dev, kind, c, layout, head, scenes=None, gains=None, ws=None, launch_status=False):
    """the scene-gradient ("pose") or exposure entry on the case through its own ctypes call: the loss, the map gradient
    and the per-scene gradient between guard words (photo_fit_checks.Guarded), a scratch of its own (`ws`: one to reuse
    without a memset) -> dict: loss [1], grad, sums ([B,S,9] or [B,S,3]), `guards_intact`, `scratch_zero` (ALL its words, the
    B S 9 / B S 3 accumulators behind the 65 included), `ws`, `rc`"""
    import torch
    lib = native._load()
    B, S = c["B"], c["S"]
    x = c["enc"] if head else c["maps"]
    d_x, d_ph = photo_checks.to_device(x, dev), photo_checks.to_device(c["photos"], dev)
    d_sc = photo_checks.to_device(c["scenes"] if scenes is None else scenes, dev)
    w = None if layout is None else photo_checks.to_device(c["weights"][layout], dev)
    n = 9 if kind == "pose" else 3
    loss, grad = fc.Guarded(np.full(1, -1.0, np.float32), dev), fc.Guarded(np.full_like(x, 7.0), dev)
    sums = fc.Guarded(np.full((B, S, n), 7.0, np.float32), dev)
    need = getattr(lib, SUMS_BYTES[kind])(B, S, H, H)
    assert need == (65 + n * B * S) * 8
    ws = torch.zeros(need // 8, dtype=torch.int64, device=dev) if ws is None else ws
    lead = (d_x.data_ptr(), d_ph.data_ptr(), None if w is None else w.data_ptr(), 0 if w is None else int(w.shape[1]))
    if kind == "exposure":
        d_e = photo_checks.to_device(c["e"] if gains is None else gains, dev)
        lead += (d_e.data_ptr(),)
    rc = getattr(lib, SUMS_ENTRIES[(kind, bool(head))])(
        *lead, d_sc.data_ptr(), native.xrow(dev, H).data_ptr(), ctypes.c_float(EPS), loss.ptr(), grad.ptr(), sums.ptr(),
        ws.data_ptr(), ws.numel() * 8, B, S, H, H, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if not launch_status:
        assert rc == 0, (rc, lib.svbrdf_last_error())
    torch.cuda.synchronize(dev)
    out = dict(rc=rc, ws=ws, scratch_zero=not ws.any().item(), guards_intact=True)
    for key, buf in (("loss", loss), ("grad", grad), ("sums", sums)):
        out[key], ok = buf.get()
        out["guards_intact"] = out["guards_intact"] and ok
    return out


def fit_case(name, layout, seed):
    """the case as photo_fit_checks' helpers take one: maps, photos, scenes, weights (a layout's, or None), t = 2 and a
    random Adam state with exact zeros in both moments (photo_fit_checks.case_inputs' rule)"""
    c = case_inputs(name)
    u = synth.uniform01(seed, (3,) + c["maps"].shape)
    m = ((u[0] - np.float32(0.5)) * np.float32(2e-3)).astype(np.float32)
    v = (u[1] * np.float32(1e-5)).astype(np.float32)
    m[u[2] < 0.1] = 0.0
    v[u[2] > 0.9] = 0.0
    return dict(name=what(name, layout, False), B=c["B"], H=H, S=c["S"], t=2, maps=c["maps"], photos=c["photos"],
                scenes=c["scenes"], weights=None if layout is None else c["weights"][layout], m=m, v=v)


def sequential_sum_bound(delta64, weights, S):
    """(3 S + 16) 2^-24 sum |term| / N: what a thread's sequential float32 sum of its 3 S terms, the wave and workgroup sums
    behind it and the terms' own roundings can move the loss by -- the bound the loss is held to where 1e-6 is missed"""
    w = 1.0 if weights is None else photo_checks.broadcast_weights(weights, S).astype(np.float64)[:, :, None]
    return (3 * S + 16) * 2.0 ** -24 * float((w * np.abs(delta64)).sum()) / float(np.asarray(delta64).size)


def sequential_sum_loss(delta32):
    """the loss from the fp32 oracle's terms `delta32` [B,S,3,H,W], summed as a thread of the kernels sums them: |log2| terms
    of one pixel added one after the other in float32, s outermost, the pixel's sum scaled by ln 2 in float32 -- and exactly
    from there on (the kernels' wave, workgroup and launch sums add 289 such values per item in float32 and fixed point:
    nothing beside 3 S sequential adds)"""
    d = np.asarray(delta32, np.float32)
    B, S = d.shape[:2]
    t = np.abs(d / np.float32(np.log(2.0))).astype(np.float32).reshape(B, 3 * S, -1)
    acc = np.zeros((B, t.shape[2]), np.float32)
    for i in range(3 * S):
        acc = (acc + t[:, i]).astype(np.float32)
    acc = (acc * np.float32(0.693147180559945309417)).astype(np.float32)
    return float(acc.astype(np.float64).sum() / d.size)
