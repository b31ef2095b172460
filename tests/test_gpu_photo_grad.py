"""The gradient of the photo losses towards the PHOTOGRAPHS on the device (csrc/svbrdf_photo_grad_photos.hip: k_pgrad_*;
svbrdf_[head_]photo_loss_photo_grad_fwd_bwd; losses.PhotoLoss / HeadPhotoLoss(differentiable_photos=True)):

    d loss / d photo[b,s,c,i,j] = -(w / N) sign(delta) / (photo + eps)

Loss and map gradient: the twin entries' bits.  Magnitude: the numpy float32 restatement of tests/photo_grad_checks.py, bit for
bit wherever the element is not 0.  Sign: -sign(delta64) of the float64 oracle on every non-structural term at or above
tolerances.TIE_LEVEL; structural terms exactly 0; at most tolerances.MAX_TIE_PIXELS tie pixels (0 by the oracle alone:
tests/test_photo_grad_cpu.py).

Speed at the configuration-2 shape (B = 8, 256 x 256, S = 9, per-photo weights, six rotating batches, legs alternating in one
process): (a) the full form <= 87/60 x the weighted twin -- (24 + 6 S + P) / (24 + 3 S + P), the byte ratio, the most a purely
HBM-bound kernel could lose; (b) the full form <= composed_photo_loss forward + backward with maps and photos leaves; (c) the
form without the map adjoint <= the registration stage's composition (K1, clamp_, log, the weighted L1 and its backward to the
photos).  Measured figures: profiles/r26_photo_grad.txt.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import photo_checks
import photo_grad_checks as pg
import synth
import tolerances
import weighted_photo_checks as wp
from photo_checks import assert_scratch_is_zero as _scratch_is_zero, to_device as _t, to_numpy as _np

pytestmark = pytest.mark.gpu
EPS = pg.EPS


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X (select CPU tests with -m 'not gpu')"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def native():
    from svbrdf_estimation_amd import _native
    _native._load()
    return _native


def _module(head, normalize="count"):
    from svbrdf_estimation_amd import losses, renderers
    fn = (losses.HeadPhotoLoss if head else losses.PhotoLoss)(renderers.LocalRenderer(), normalize=normalize,
                                                             differentiable_photos=True)
    assert fn.uses_fused_kernel() and fn.eps == EPS
    return fn


def _entry(native, x, ph, sc, w, head, want_grad=True):
    """-> (loss: float, grad numpy or None, grad_photos numpy)"""
    loss, grad, gp = native.photo_loss(x, ph, sc, EPS, want_grad=want_grad, head=head, weights=w, want_photo_grad=True)
    assert (grad is None) == (not want_grad) and gp.shape == ph.shape and gp.dtype == torch.float32
    return loss.item(), (None if grad is None else _np(grad)), _np(gp)


def _same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _device_case(c, layout, head, dev):
    w = c["weights"][layout]
    return _t(c["enc"] if head else c["maps"], dev), _t(c["photos"], dev), _t(c["scenes"], dev), (None if w is None else _t(w, dev))


# ------------------------------------------------------------------------------------------------ 1. parity

@pytest.mark.parametrize("name,layout,head", pg.PARAMS, ids=["%s-%s-%s" % (n, l, "head" if h else "maps") for n, l, h in pg.PARAMS])
def test_parity(dev, native, name, layout, head):
    cmp_ = pg.comparison(name, layout, head)
    x, ph, sc, w = _device_case(cmp_.case, layout, head, dev)
    what = "%s %s %s" % (name, layout, "head" if head else "maps")
    for want_grad in (True, False):
        twin_loss, twin_grad = native.photo_loss(x, ph, sc, EPS, want_grad=want_grad, head=head, weights=w)
        loss, grad, gp = _entry(native, x, ph, sc, w, head, want_grad)
        assert loss == twin_loss.item(), "%s: loss %.9g, the twin entry's %.9g" % (what, loss, twin_loss.item())
        if want_grad:
            assert np.array_equal(_bits(grad), _bits(_np(twin_grad))), "%s: other map gradient bits than the twin entry" % what
        ties = cmp_.check(gp, "%s%s" % (what, "" if want_grad else ", no adjoint"))
        tolerances.assert_loss_close(loss, cmp_.loss32, what + " loss")
        print("[photo-grad] %s, map gradient %s: loss %.9g, %d of %d elements non-zero, %d tie pixels" % (
            what, want_grad, loss, int((gp != 0).sum()), gp.size, ties))
        if want_grad:
            first = gp
        else:
            assert np.array_equal(_bits(gp), _bits(first)), "%s: the two forms give other grad_photos bits" % what
    _scratch_is_zero(native)


def _big_case():
    """64 x 64, S = 9, B = 5: 80 workgroups on the 64 slots of the loss reduction (the shape of tests/pose_photo_checks.py)"""
    from oracle import c_oracle
    B, H = 5, 64
    sc = photo_checks.scene_table(B, 41, 3, 6)
    maps, target = synth.make_maps(6190, B, H), synth.make_maps(6191, B, H)
    photos = np.clip(c_oracle.render_fwd(target, sc), 0.0, 1.0)
    w = wp.weight_field(6290, B, 9, H)
    return dict(name="big", H=H, S=9, tied=True, maps=maps, enc=wp.encoded_input(6490, B, H), photos=photos, scenes=sc,
                weights={"per-photo": w, "none": None})


def test_more_workgroups_than_slots(dev, native):
    c = _big_case()
    for layout in ("per-photo", "none"):
        cmp_ = pg.Comparison(c, layout, False)
        x, ph, sc, w = _device_case(c, layout, False, dev)
        for want_grad in (True, False):
            twin_loss, twin_grad = native.photo_loss(x, ph, sc, EPS, want_grad=want_grad, weights=w)
            loss, grad, gp = _entry(native, x, ph, sc, w, False, want_grad)
            assert loss == twin_loss.item() and (grad is None or np.array_equal(_bits(grad), _bits(_np(twin_grad))))
            cmp_.check(gp, "80 workgroups, %s, map gradient %s" % (layout, want_grad))
            again = _entry(native, x, ph, sc, w, False, want_grad)
            assert again[0] == loss and np.array_equal(_bits(again[2]), _bits(gp))
    _scratch_is_zero(native)


# ------------------------------------------------------------------------------------------------ 2. weight layouts

@pytest.mark.parametrize("name", ["7_s5", "45_s9"])
@pytest.mark.parametrize("head", [False, True], ids=["maps", "head"])
def test_weight_layouts(dev, native, name, head):
    c = pg.case_inputs(name)
    x, ph, sc, _ = _device_case(c, "none", head, dev)
    B, S, H = pg.B_CASES, c["S"], c["H"]
    for want_grad in (True, False):
        plain = _entry(native, x, ph, sc, None, head, want_grad)
        for P in (S, 1):
            ones = _entry(native, x, ph, sc, torch.ones((B, P, H, H), device=dev), head, want_grad)
            assert ones[0] == plain[0] and np.array_equal(_bits(ones[2]), _bits(plain[2])), (name, head, P, "all ones")
            assert want_grad is False or np.array_equal(_bits(ones[1]), _bits(plain[1]))
        shared = c["weights"]["shared"]
        one = _entry(native, x, ph, sc, _t(shared, dev), head, want_grad)
        copies = _entry(native, x, ph, sc, _t(np.repeat(shared, S, axis=1), dev), head, want_grad)
        assert one[0] == copies[0] and np.array_equal(_bits(one[2]), _bits(copies[2])), (name, head, "shared plane")
    _scratch_is_zero(native)


# ------------------------------------------------------------------------------------------------ 3. independence, NaN rules

@pytest.mark.parametrize("head", [False, True], ids=["maps", "head"])
def test_element_independence_and_nan_rules(dev, native, head):
    c = pg.case_inputs("45_s9")
    xh, H, S = (c["enc"] if head else c["maps"]), c["H"], c["S"]
    x, ph, sc, _ = _device_case(c, "none", head, dev)
    mask = (c["weights"]["per-photo"] >= 0.5).astype(np.float32)
    assert (mask == 0).any() and (mask == 1).any()
    dead = np.broadcast_to((mask == 0)[:, :, None], c["photos"].shape)
    for want_grad in (True, False):
        clean = _entry(native, x, ph, sc, _t(mask, dev), head, want_grad)
        assert np.isfinite(clean[0]) and np.isfinite(clean[2]).all() and not clean[2][dead].any() and clean[2][~dead].any()
        # NaN, +inf and -1 under zero weights: exactly 0 there, no other bit changes
        junk = np.array([np.nan, np.inf, -1.0], np.float32)[(synth.uniform01(991, mask.shape) * 3).astype(np.int64)]
        spoiled = np.where((mask == 0)[:, :, None], junk[:, :, None], c["photos"]).astype(np.float32)
        got = _entry(native, x, _t(spoiled, dev), sc, _t(mask, dev), head, want_grad)
        assert got[0] == clean[0] and np.array_equal(_bits(np.abs(got[2])), _bits(np.abs(clean[2]))) and not got[2][dead].any()
        assert np.array_equal(_bits(got[2][~dead]), _bits(clean[2][~dead]))
        _scratch_is_zero(native)
        # one NaN under a weight of 1e-3: that element NaN, the loss NaN, every other element keeps its bits
        b, s, i, j = [int(v[-1]) for v in np.nonzero(mask)]
        almost = mask.copy()
        almost[b, s, i, j] = 1e-3
        base = _entry(native, x, ph, sc, _t(almost, dev), head, want_grad)
        bad = c["photos"].copy()
        bad[b, s, 1, i, j] = np.nan
        got = _entry(native, x, _t(bad, dev), sc, _t(almost, dev), head, want_grad)
        assert np.isnan(got[0]) and np.isnan(got[2][b, s, 1, i, j])
        other = np.ones(got[2].shape, bool)
        other[b, s, 1, i, j] = False
        assert np.array_equal(_bits(got[2][other]), _bits(base[2][other])) and np.isfinite(base[2]).all()
        _scratch_is_zero(native)
        # a photo value below -eps under w > 0 is a NaN term as well
        bad = c["photos"].copy()
        bad[b, s, 2, i, j] = -1.0
        got = _entry(native, x, _t(bad, dev), sc, _t(almost, dev), head, want_grad)
        assert np.isnan(got[0]) and np.isnan(got[2][b, s, 2, i, j]) and np.isfinite(got[2][b, s, :2, i, j]).all()
        _scratch_is_zero(native)
        # a weight of 2 or NaN: its three elements NaN, the others keep the clean run's bits
        for value in (2.0, np.nan):
            wbad = mask.copy()
            wbad[b, s, i, j] = value
            got = _entry(native, x, ph, sc, _t(wbad, dev), head, want_grad)
            assert np.isnan(got[0]) and np.isnan(got[2][b, s, :, i, j]).all(), value
            other = np.ones(got[2].shape, bool)
            other[b, s, :, i, j] = False
            assert np.array_equal(_bits(got[2][other]), _bits(clean[2][other])), value
            _scratch_is_zero(native)
        # a NaN map pixel: that pixel's elements NaN where w > 0, exactly 0 where w = 0; every other pixel keeps its bits
        xbad = xh.copy()
        xbad[b, 2 if head else 3, i, j] = np.nan          # a diffuse channel: it propagates through the arithmetic by itself
        got = _entry(native, _t(xbad, dev), ph, sc, _t(mask, dev), head, want_grad)
        live = mask[b, :, i, j] > 0
        assert live.any() and np.isnan(got[0])
        assert np.isnan(got[2][b, live, :, i, j]).all() and not got[2][b, ~live, :, i, j].any()
        other = np.ones(got[2].shape, bool)
        other[b, :, :, i, j] = False
        assert np.array_equal(_bits(got[2][other]), _bits(clean[2][other]))
        _scratch_is_zero(native)
        again = _entry(native, x, ph, sc, _t(mask, dev), head, want_grad)
        assert again[0] == clean[0] and np.array_equal(_bits(again[2]), _bits(clean[2]))        # nothing sticks


# ------------------------------------------------------------------------------------------------ 4. memory

def _raw_call(native, x, ph, sc, w, gp_view, head, want_grad):
    """the entry with grad_photos written where the caller says -> (loss, grad or None)"""
    B, S, _, H, W = ph.shape
    extra = (None, 0) if w is None else (w.data_ptr(), int(w.shape[1]))
    entry = pg.ENTRIES[1 if head else 0]
    return native._fused_loss_call(entry, x, ph, sc, (ctypes.c_float(EPS),), want_grad, B, S, H, W, extra, (gp_view.data_ptr(),))


@pytest.mark.parametrize("name", ["17_s2", "1_s1"])
@pytest.mark.parametrize("head", [False, True], ids=["maps", "head"])
def test_grad_photos_off_alignment_inside_sentinels(dev, native, name, head):
    c = pg.case_inputs(name)
    sentinel = np.float32(-7.25)
    for layout in ("per-photo", "none"):
        x, ph, sc, w = _device_case(c, layout, head, dev)
        for want_grad in (True, False):
            loss, grad, gp = _entry(native, x, ph, sc, w, head, want_grad)
            n, lead = ph.numel(), 17                            # 17 floats = 68 bytes: 4 bytes off 16-byte alignment
            flat = torch.full((lead + n + 64,), float(sentinel), dtype=torch.float32, device=dev)
            view = flat[lead:lead + n].view(ph.shape)
            assert view.data_ptr() % 16 == 4
            l2, g2 = _raw_call(native, x, ph, sc, w, view, head, want_grad)
            got = _np(flat)
            assert (got[:lead] == sentinel).all() and (got[lead + n:] == sentinel).all(), "a store outside grad_photos"
            assert l2.item() == loss and np.array_equal(_bits(got[lead:lead + n]), _bits(gp).ravel())
            assert g2 is None or np.array_equal(_bits(_np(g2)), _bits(grad))
    _scratch_is_zero(native)


def test_fresh_and_reused_scratch_give_the_same_bits(dev, native):
    c = pg.case_inputs("33_s3")
    x, ph, sc, w = _device_case(c, "per-photo", False, dev)
    torch.cuda.synchronize()
    native._workspace_cache.clear()
    first = _entry(native, x, ph, sc, w, False)
    for _ in range(2):
        again = _entry(native, x, ph, sc, w, False)
        assert again[0] == first[0] and np.array_equal(_bits(again[1]), _bits(first[1])) and np.array_equal(_bits(again[2]), _bits(first[2]))
    _scratch_is_zero(native)


# ------------------------------------------------------------------------------------------------ 5. modules

@pytest.mark.parametrize("head", [False, True], ids=["maps", "head"])
def test_modules(dev, native, head):
    from svbrdf_estimation_amd import losses
    cmp_ = pg.comparison("45_s9", "per-photo", head)
    c = cmp_.case
    x, ph, sc, w = _device_case(c, "per-photo", head, dev)
    loss, grad, gp = _entry(native, x, ph, sc, w, head)
    fn = _module(head)
    # backward(): the entry's bits, ONE launch
    leaf, pleaf = x.clone().requires_grad_(True), ph.clone().requires_grad_(True)
    n0 = native.launch_count()
    l = fn(leaf, pleaf, sc, w)
    assert isinstance(l, losses._PhotoLossTensor)
    l.backward()
    torch.cuda.synchronize()
    assert native.launch_count() - n0 == 1
    assert l.item() == loss and np.array_equal(_bits(_np(leaf.grad)), _bits(grad)) and np.array_equal(_bits(_np(pleaf.grad)), _bits(gp))
    # backward(gradient=0.5): 0.5 x the entry within one rounding
    leaf, pleaf = x.clone().requires_grad_(True), ph.clone().requires_grad_(True)
    fn(leaf, pleaf, sc, w).backward(gradient=torch.full((), 0.5, device=dev))
    for got, ref in ((_np(pleaf.grad), gp), (_np(leaf.grad), grad)):
        assert (np.abs(got.astype(np.float64) - 0.5 * ref.astype(np.float64)) <= 2.0 ** -24 * np.abs(0.5 * ref.astype(np.float64))).all()
    # a detached input: exactly one launch, of the form without the map adjoint
    fwd = _entry(native, x, ph, sc, w, head, want_grad=False)
    pleaf = ph.clone().requires_grad_(True)
    n0 = native.launch_count()
    l = fn(x, pleaf, sc, w)
    l.backward()
    torch.cuda.synchronize()
    assert native.launch_count() - n0 == 1
    assert l.item() == fwd[0] and np.array_equal(_bits(_np(pleaf.grad)), _bits(fwd[2]))
    # photos that do not require grad: the existing path and its bits; the default constructor still refuses
    leaf = x.clone().requires_grad_(True)
    l = fn(leaf, ph, sc, w)
    l.backward()
    assert l.item() == loss and np.array_equal(_bits(_np(leaf.grad)), _bits(grad))
    plain = (losses.HeadPhotoLoss if head else losses.PhotoLoss)(fn.renderer)
    with pytest.raises(RuntimeError, match="no gradient w.r.t. the photos"):
        plain(x, ph.clone().requires_grad_(True), sc, w)
    # a constant exposure is folded into the table's colour columns
    gains = 0.5 + torch.rand((pg.B_CASES, c["S"], 3), device=dev)
    folded = torch.cat((sc[..., :6], sc[..., 6:] * gains), dim=-1)
    want = _entry(native, x, ph, folded, w, head)
    leaf, pleaf = x.clone().requires_grad_(True), ph.clone().requires_grad_(True)
    l = fn(leaf, pleaf, sc, w, gains)
    l.backward()
    assert l.item() == want[0] and np.array_equal(_bits(_np(pleaf.grad)), _bits(want[2])) and np.array_equal(_bits(_np(leaf.grad)), _bits(want[1]))
    # normalize="weights" against the float64 value, (R + 3) 2^-24 relative on the decided terms: the R roundings of the
    # magnitude, the scale rounded to float32, the multiply by it, and one for the products of the factors
    full = cmp_.full_weights.astype(np.float64)
    scale = full.size / full.sum()
    pleaf = ph.clone().requires_grad_(True)
    _module(head, "weights")(x, pleaf, sc, w).backward()
    got = _np(pleaf.grad).astype(np.float64)
    decided = ~cmp_.structural & ~cmp_.tie_terms
    want64 = cmp_.value64 * scale
    rel = np.abs(got[decided] - want64[decided]) / np.abs(want64[decided])
    print("[photo-grad] normalize=weights %s: largest relative difference to float64 %.2f x 2^-24" % ("head" if head else "maps", rel.max() * 2.0 ** 24))
    assert rel.max() <= (pg.ROUNDINGS + 3) * 2.0 ** -24 and not got[cmp_.structural].any()
    # photos and the table (or an exposure) that require grad: the composed definition, differentiable in both
    leaf, pleaf, tleaf = x.clone().requires_grad_(True), ph.clone().requires_grad_(True), sc.clone().requires_grad_(True)
    fn(leaf, pleaf, tleaf, w).backward()
    assert tleaf.grad is not None and torch.isfinite(tleaf.grad).all() and pleaf.grad is not None
    got = _np(pleaf.grad).astype(np.float64)
    assert np.array_equal(np.sign(got[decided]), np.sign(cmp_.value64[decided]))
    assert (np.abs(got[decided] - cmp_.value64[decided]) <= 1e-5 * np.abs(cmp_.value64[decided])).all()
    _scratch_is_zero(native)


# ------------------------------------------------------------------------------------------------ 6. the chain

@pytest.mark.parametrize("with_lens", [False, True], ids=["pinhole", "lens"])
def test_rectify_then_loss_then_backward_is_the_two_entries_by_hand(dev, native, with_lens):
    """uint8 32 x 24 source, P = 2 (B = 1, S = 2), an 8 x 8 grid, 2 x 2 sub-samples: M.grad (and lens.grad) of the autograd
    chain are the bits of the photo-gradient entry followed by the rectification's gradient entry"""
    from svbrdf_estimation_amd import capture, losses, renderers
    Hs, Ws, H, S = 24, 32, 8, 2
    yy, xx = np.mgrid[0:Hs, 0:Ws].astype(np.float64)
    img = np.stack([np.stack([0.5 + 0.4 * np.sin(0.31 * xx + 0.2 * ch + p) * np.cos(0.27 * yy - 0.3 * ch) for ch in range(3)], -1)
                    for p in range(S)])
    src = torch.from_numpy(np.round(255 * img).astype(np.uint8)).reshape(1, S, Hs, Ws, 3).to(dev)
    corners = np.array([[[5.5, 4.25], [4.0, 19.5], [26.25, 20.0], [25.5, 3.75]],
                        [[6.25, 5.0], [5.5, 18.75], [27.0, 19.25], [24.75, 4.5]]])
    M0 = torch.from_numpy(np.stack([capture.patch_homography(k, H) for k in corners]).astype(np.float32)).reshape(1, S, 3, 3)
    lens0 = None
    if with_lens:
        f = 0.8 * Ws
        lens0 = torch.tensor([[f, f, (Ws - 1) / 2.0 + 1.0, (Hs - 1) / 2.0 - 1.0, -0.12, 0.03, 1e-3, -7e-4, 0.0]] * S,
                             dtype=torch.float32).reshape(1, S, 9)
    lut = capture.gamma_lut()
    maps = _t(synth.make_maps(7400, 1, H), dev)
    sc = _t(photo_checks.scene_table(1, 905, 1, 1), dev)
    fn = losses.PhotoLoss(renderers.LocalRenderer(), differentiable_photos=True)
    M = M0.clone().to(dev).requires_grad_(True)
    lens = None if lens0 is None else lens0.clone().to(dev).requires_grad_(True)
    rect, w = capture.rectify(src, M, H, lut=lut, samples=2, lens=lens)
    assert rect.shape == (1, S, 3, H, H) and rect.requires_grad and w.shape == (1, S, H, H) and (w > 0).any()
    loss = fn(maps, rect, sc, w)
    loss.backward()
    # by hand
    with torch.no_grad():
        rect0, w0 = capture.rectify(src, M0.to(dev), H, lut=lut, samples=2, lens=None if lens0 is None else lens0.to(dev))
    assert torch.equal(rect0, rect.detach()) and torch.equal(w0, w)
    l0, g0, gp = native.photo_loss(maps, rect0, sc, EPS, want_grad=False, weights=w0, want_photo_grad=True)
    assert l0.item() == loss.item() and g0 is None and gp.abs().max() > 0
    mats = M0.reshape(S, 9).to(dev).contiguous()
    args = (src.reshape(S, Hs, Ws, 3).contiguous(), capture.U8_INTERLEAVED, S, Hs, Ws, mats)
    tail = (H, H, 2, lut.to(dev), -float("inf"), float("inf"))
    p = rect0.clone().requires_grad_(True)
    losses.composed_photo_loss(maps, p, sc, EPS, w0).backward()
    if with_lens:
        rows = lens0.reshape(S, 9).to(dev).contiguous()
        gm, gl = native.rectify_lens_grad(*args, rows, *tail, gp.reshape(S, 3, H, H))
        assert np.array_equal(_bits(_np(lens.grad).reshape(S, 9)), _bits(_np(gl))) and gl.abs().max() > 0
        gm_t, _ = native.rectify_lens_grad(*args, rows, *tail, p.grad.reshape(S, 3, H, H).contiguous())
    else:
        gm = native.rectify_grad_matrices(*args, *tail, gp.reshape(S, 3, H, H))
        gm_t = native.rectify_grad_matrices(*args, *tail, p.grad.reshape(S, 3, H, H).contiguous())
    assert np.array_equal(_bits(_np(M.grad).reshape(S, 9)), _bits(_np(gm))) and gm.abs().max() > 0
    print("[photo-grad] chain %s: max |M.grad - M.grad with the loss in torch ops| / max |M.grad| = %.3g (printed, not asserted)" % (
        "with a lens" if with_lens else "pinhole", ((gm - gm_t).abs().max() / gm.abs().max()).item()))
    _scratch_is_zero(native)


# ------------------------------------------------------------------------------------------------ 7. speed

def measure_photo_grad(dev, native, sets=6, n=40, rounds=3):
    """-> medians (us per step) at the configuration-2 shape, B = 8, 256 x 256, S = 9, per-photo weights, device table, `sets`
    rotating batches, one process, the legs alternating round by round (photo_checks.timed_legs):
        full_us          svbrdf_photo_loss_photo_grad_fwd_bwd with the map gradient: loss and both gradients, ONE launch
        twin_us          svbrdf_photo_loss_weighted_fwd_bwd on the same operands
        composed_us      losses.composed_photo_loss forward + backward, maps and photos leaves
        no_adjoint_us    the entry with grad_input NULL: loss + grad_photos
        registration_us  the registration stage's composition: K1, clamp_, log, the weighted L1 and its backward to the photos"""
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
    gps = [torch.empty_like(p) for p in photos]
    leaves = [a.clone().requires_grad_(True) for a in ins]
    pleaves = [p.clone().requires_grad_(True) for p in photos]
    xr = native.xrow(dev, H)
    ws = torch.zeros(65, dtype=torch.int64, device=dev)
    loss = torch.empty(1, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    eps = ctypes.c_float(EPS)

    def entry(k, grad):
        rc = lib.svbrdf_photo_loss_photo_grad_fwd_bwd(ins[k].data_ptr(), photos[k].data_ptr(), weights[k].data_ptr(), S,
                                                      table.data_ptr(), xr.data_ptr(), eps, loss.data_ptr(), grad,
                                                      gps[k].data_ptr(), ws.data_ptr(), ws.numel() * 8, B, S, H, H, st)
        assert rc == 0, lib.svbrdf_last_error()

    def full(i):
        entry(i % sets, grads[i % sets].data_ptr())

    def no_adjoint(i):
        entry(i % sets, None)

    def twin(i):
        k = i % sets
        rc = lib.svbrdf_photo_loss_weighted_fwd_bwd(ins[k].data_ptr(), photos[k].data_ptr(), weights[k].data_ptr(), S,
                                                    table.data_ptr(), xr.data_ptr(), eps, loss.data_ptr(), grads[k].data_ptr(),
                                                    ws.data_ptr(), ws.numel() * 8, B, S, H, H, st)
        assert rc == 0, lib.svbrdf_last_error()

    def composed(i):
        k = i % sets
        leaves[k].grad = None
        pleaves[k].grad = None
        losses.composed_photo_loss(leaves[k], pleaves[k], table, EPS, weights[k]).backward()

    def registration(i):
        k = i % sets
        pleaves[k].grad = None
        with torch.no_grad():
            log_r = (native.render_fwd(ins[k], table).clamp_(0.0, 1.0) + EPS).log()
        w = weights[k]
        ((w.unsqueeze(2) * (log_r - (pleaves[k] + EPS).log()).abs()).sum() / (3.0 * w.sum())).backward()

    legs = (("full_us", full), ("twin_us", twin), ("composed_us", composed), ("no_adjoint_us", no_adjoint),
            ("registration_us", registration))
    out, res = photo_checks.timed_legs(legs, n, rounds, photo_checks.spinning_wave(native, dev), dev)
    out.update(rounds=res, device=torch.cuda.get_device_name(dev), steps_per_round=n, sets=sets)
    out["full_frac_of_8TBps"] = (12 + 3 * S + S + 12 + 3 * S) * 4 * H * H * B / (out["full_us"] * 1e-6) / 8.0e12
    return out


def test_speed_against_the_twin_and_the_compositions(dev, native):
    res = measure_photo_grad(dev, native)
    bound = 87.0 / 60.0
    text = ("photo loss with grad_photos %.2f us per launch, weighted twin %.2f (ratio %.3f, bound %.3f), composed_photo_loss "
            "with maps and photos leaves %.2f us per step (%.1fx); without the map adjoint %.2f us per launch, the registration "
            "stage's composition %.2f us per step (%.1fx); %.3f of 8 TB/s at the algorithmic bytes; per round %s" % (
                res["full_us"], res["twin_us"], res["full_us"] / res["twin_us"], bound, res["composed_us"],
                res["composed_us"] / res["full_us"], res["no_adjoint_us"], res["registration_us"],
                res["registration_us"] / res["no_adjoint_us"], res["full_frac_of_8TBps"], res["rounds"]))
    print("[photo-grad] config-2 shape, per-photo weights: " + text)
    out = os.environ.get("SVBRDF_RESULTS_DIR")
    with open(os.path.join(out, "photo_grad_speed.txt") if out else os.devnull, "w") as f:
        f.write("# tests/test_gpu_photo_grad.py speed test on %s\n%s\n" % (res["device"], text))
    assert res["full_us"] <= bound * res["twin_us"], res
    assert res["full_us"] <= res["composed_us"], res
    assert res["no_adjoint_us"] <= res["registration_us"], res
