"""Shared by tests/test_photo_grad_cpu.py and tests/test_gpu_photo_grad.py: what the gradient of the photo losses towards the
PHOTOGRAPHS (svbrdf_[head_]photo_loss_photo_grad_fwd_bwd, csrc/svbrdf_photo_grad_photos.hip) is compared with.

    d loss / d photo[b,s,c,i,j] = -(w / N) sign(delta) / (photo + eps),   delta = log(render + eps) - log(p' + eps)

Every element is +m, -m or 0.

The MAGNITUDE m is a pure function of w, N, eps and that one photo value.  The order of operations the kernel takes, restated
here in numpy float32 (`restated_magnitude`), every operation individually rounded:

    inv = fl(1 / N)              the double quotient rounded to float32 (what the launcher passes)       rounding 1
    num = fl(w inv)              one float32 multiply (w = 1: exact)                                     rounding 2
    den = fl(photo + eps)        one float32 add                                                         rounding 3
    m   = fl(num / den)          one IEEE float32 division                                               rounding 4

R = ROUNDINGS = 4.  (The kernel divides by den 2^-10 and scales the quotient by 2^-10: a power of two commutes with the
rounding.)  The device must equal the restatement bit for bit wherever the element is not 0.

The SIGN is -sign(delta) as the kernel's own log of the quotient decides it.  It is compared with the float64 oracle
(photo_checks.oracle_photo_loss(..., f64=True)) on every non-structural term with |delta64| >= tolerances.TIE_LEVEL; below
the level any of {-m, 0, +m} is right and the term's pixel counts against tolerances.MAX_TIE_PIXELS.  STRUCTURAL terms -- the
per-term rule of photo_checks.tie_map: the photo value is exactly 0 with the light behind the surface, or the weight is
exactly 0 -- are exactly 0 in every evaluation.

The cases: weighted_photo_checks.CASES in three weight layouts (none, per-photo, shared), and four tiny ones, the smallest at
which a lane, a wave or the scene loop's two-pass exit can go wrong (B = 2, photos = clip(oracle render of a target, 0, 1)).
"""
import numpy as np

import photo_checks
import synth
import tolerances
import weighted_photo_checks as wp
from oracle import c_oracle

EPS = photo_checks.EPS
ROUNDINGS = 4
ENTRIES = ("svbrdf_photo_loss_photo_grad_fwd_bwd", "svbrdf_head_photo_loss_photo_grad_fwd_bwd")
LAYOUTS = ("none", "per-photo", "shared")
B_CASES = 2

# (name, H, (n_random, n_specular), i): scenes scene_table(2, 900 + i, nr, ns), maps / target seeds 7100 + 2 i / 7101 + 2 i,
# weights all ones (i = 0) or weight_field(7200 + i, ...)
TINY = (
    ("1_s1", 1, (1, 0), 0),
    ("2_s2", 2, (1, 1), 1),
    ("3_s3", 3, (1, 2), 2),
    ("7_s5", 7, (2, 3), 3),
)
CASE_NAMES = tuple(c[0] for c in wp.CASES) + tuple(c[0] for c in TINY)
TIED = {c[0]: c[4] for c in wp.CASES}
TIED.update({c[0]: True for c in TINY})
# every (case, layout, head): maps everywhere, the head where the roughness is tied
PARAMS = [(n, l, h) for n in CASE_NAMES for l in LAYOUTS for h in ((False, True) if TIED[n] else (False,))]


def restated_magnitude(photos, weights, eps, count):
    """m [like photos] float32 by the four roundings above.  `weights`: broadcastable to the photos (float32), or None."""
    photos = np.asarray(photos, np.float32)
    inv = np.float32(1.0 / float(count))
    num = inv if weights is None else np.asarray(weights, np.float32) * inv
    with np.errstate(all="ignore"):
        den = photos + np.float32(eps)
        m = np.divide(num, den, dtype=np.float32)
    assert m.dtype == np.float32
    return np.broadcast_to(m, photos.shape)


def _tiny_weight_field(seed, P, H, masked_rows):
    """weighted_photo_checks.weight_field without its demand that so few values hold both a 0 and a 1"""
    u = synth.uniform01(seed, (B_CASES, P, H, H))
    w = np.where(u < 0.25, np.float32(0.0), np.where(u >= 0.75, np.float32(1.0), (u - np.float32(0.25)) * np.float32(2.0)))
    w = w.astype(np.float32)
    if masked_rows:
        w[:, :, :max(H // 4, 1), :] = 0.0
    return np.ascontiguousarray(w)


def case_inputs(name):
    """-> dict of one case as weighted_photo_checks.case_inputs gives it; weights {"none": None, "per-photo", "shared"}"""
    if name in [c[0] for c in wp.CASES]:
        c = dict(wp.case_inputs(name))
        c["weights"] = dict(c["weights"], none=None)
        return c
    _, H, (nr, ns), i = TINY[[c[0] for c in TINY].index(name)]
    S = nr + ns
    sc = photo_checks.scene_table(B_CASES, 900 + i, nr, ns)
    maps = synth.make_maps(7100 + 2 * i, B_CASES, H)
    target = synth.make_maps(7101 + 2 * i, B_CASES, H)
    photos = np.clip(c_oracle.render_fwd(target, sc), 0.0, 1.0)
    if i == 0:
        weights = {"per-photo": np.ones((B_CASES, S, H, H), np.float32), "shared": np.ones((B_CASES, 1, H, H), np.float32)}
    else:
        weights = {"per-photo": _tiny_weight_field(7200 + i, S, H, masked_rows=(i != 1)),
                   "shared": _tiny_weight_field(7200 + i, 1, H, masked_rows=(i != 1))}
    weights["none"] = None
    return dict(name=name, H=H, S=S, tied=True, maps=maps, enc=wp.encoded_input(7300 + i, B_CASES, H), photos=photos,
                scenes=sc, weights=weights)


class Comparison:
    """the comparison values of one (case, layout, maps or head), by the oracle alone:
    delta64 [B,S,3,H,W]; delta32 (the float32 oracle's); structural [B,S,3,H,W] bool; value64 = -w sign(delta64) / (N (p' + eps));
    m32 = the restatement (under a zero weight: 0)"""

    def __init__(self, c, layout, head):
        self.case, self.layout, self.head = c, layout, bool(head)
        x = c["enc"] if head else c["maps"]
        self.x = np.ascontiguousarray(x, np.float32)
        maps = c_oracle.head_decode(self.x) if head else self.x
        w, photos, sc = c["weights"][layout], c["photos"], c["scenes"]
        self.weights = w
        _, _, self.delta64 = photo_checks.oracle_photo_loss(maps, photos, sc, EPS, f64=True, want_grad=False, weights=w)
        self.loss32, _, self.delta32 = photo_checks.oracle_photo_loss(maps, photos, sc, EPS, want_grad=False, weights=w)
        S = photos.shape[1]
        excused = photos if w is None else photo_checks.excused_photos(photos, w)
        full = np.ones(photos.shape[:2] + photos.shape[3:], np.float32) if w is None else photo_checks.broadcast_weights(w, S)
        self.full_weights = full
        self.structural = (excused == 0.0) & (photo_checks.unclamped_n_dot_wi(maps, sc) < -1e-6)[:, :, None]
        self.structural = self.structural | np.broadcast_to((full == 0.0)[:, :, None], photos.shape)
        count = float(photos.size)
        eps64 = np.float64(np.float32(EPS))
        self.value64 = -full.astype(np.float64)[:, :, None] * np.sign(self.delta64) / (count * (excused.astype(np.float64) + eps64))
        self.m32 = restated_magnitude(photos, full[:, :, None], EPS, photos.size)
        self.tie_terms = ~self.structural & (np.abs(self.delta64) < tolerances.TIE_LEVEL)

    def tie_pixels(self):
        return int(self.tie_terms.any(axis=(1, 2)).sum())

    def smallest_delta(self):
        d = np.where(self.structural, np.inf, np.abs(self.delta64))
        return float(d.min())

    def check(self, got, what):
        """`got` [B,S,3,H,W] float32 from the device: the rules of the module's text -> the number of tie pixels"""
        got = np.asarray(got)
        assert got.dtype == np.float32 and got.shape == self.m32.shape, (what, got.dtype, got.shape)
        assert not np.isnan(got).any(), "%s: NaN elements on clean inputs" % what
        nz = got != 0.0
        same = np.abs(got)[nz].view(np.uint32) == np.ascontiguousarray(self.m32[nz]).view(np.uint32)
        assert same.all(), "%s: %d of %d non-zero magnitudes are not the restatement's bits" % (what, int((~same).sum()), int(nz.sum()))
        assert not got[self.structural].any(), "%s: a structural term is not exactly 0" % what
        decided = ~self.structural & ~self.tie_terms
        want_sign = -np.sign(self.delta64[decided])
        assert np.array_equal(np.sign(got[decided]).astype(np.float64), want_sign), \
            "%s: %d signs differ from -sign(delta64) outside ties" % (what, int((np.sign(got[decided]) != want_sign).sum()))
        n = self.tie_pixels()
        assert n <= tolerances.MAX_TIE_PIXELS, "%s: %d tie pixels" % (what, n)
        return n


_COMPARISONS = {}


def comparison(name, layout, head):
    """computed once per session and shared"""
    key = (name, layout, bool(head))
    if key not in _COMPARISONS:
        _COMPARISONS[key] = Comparison(case_inputs(name), layout, head)
    return _COMPARISONS[key]
