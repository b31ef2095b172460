"""The photo losses with a per-photo exposure on the device (csrc/svbrdf_photo_exposure.hip: k_exposure_*; losses.PhotoLoss /
HeadPhotoLoss with `exposure`):

    L = (1/N) sum w | log(render(scene[b,s] with colour fl32(colour e[b,s]), input[b]) + eps) - log(p' + eps) |
    dL/de[b,s,c] = sum_{i,j} w sign(delta) rad_c / (N (rad_c + eps) e_c)

against the C oracle's composition (tests/exposure_photo_checks.py: nothing under oracle/ changes for it) and the reference
(tests/golden/g22_photo_exposure.npz), through the C ABI and through the modules.  Bounds: loss 1e-6 relative; map gradient
tests/tolerances.py's, through photo_checks.Reference on the pre-scaled table; exposure gradient per (b, s, c)
GRAD_RTOL A + GRAD_ATOL_FRAC max(A) + 2 T with A the sum of the terms' magnitudes and T that of the tied terms.  By the oracle
alone the cases have 0 tied terms and no sign flip (tests/test_exposure_photo_loss_cpu.py), and the fp32 oracle's own error is
below 1e-3 of the bound.

Why these shapes: 17 x 17 has a partial workgroup and a partial wave, whose missing pixels must add 0; 33 x 33 has five
workgroups per item; S = 1 / 2 / 3 cover the exits of the two-pass loop; the three-lobe loop; and 64 x 64, S = 9, B = 5 has 80
workgroups, more than the 64 slots of the loss reduction.

Speed at the configuration-2 shape (B = 8, 256 x 256, S = 9, per-photo weights): the fused exposure loss must be no slower than
the composition it fuses; its ratio to the weighted kernel on the pre-scaled table (the same work without the reduction of
the exposure gradient) is recorded, not asserted (profiles/r16_photo_exposure.txt).
"""
import os

import numpy as np
import pytest
import torch

import exposure_photo_checks as xp
import head_checks
import photo_checks
import synth
import tolerances
import weighted_photo_checks as wp
from photo_checks import assert_scratch_is_zero as _scratch_is_zero, to_device as _t, to_numpy as _np

pytestmark = pytest.mark.gpu
EPS = xp.EPS


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
    fn = (losses.HeadPhotoLoss if head else losses.PhotoLoss)(renderers.LocalRenderer(), normalize=normalize)
    assert fn.uses_fused_kernel() and fn.eps == EPS
    return fn


def _run_all_ways(native, dev, what, x, ph, w, sc, e, head, R):
    """the C ABI with grad_exposure and without, a host table (uploaded), the module through backward(): each within the
    bounds of `R` (an ExposureReference), all the same bits, scratch zeroed -> (loss, grad, grad_exposure) of the first"""
    d_x, d_ph, d_sc, d_e = _t(x, dev), _t(ph, dev), _t(sc, dev), _t(e, dev)
    d_w = None if w is None else _t(w, dev)
    results = {}
    loss, grad, ge = native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w, exposure=d_e, want_exposure_grad=True)
    results["C ABI"] = (loss.item(), _np(grad), _np(ge))
    loss, grad, ge = native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w, exposure=d_e)
    assert ge is None
    results["C ABI, grad_exposure = NULL"] = (loss.item(), _np(grad), None)
    loss, grad, ge = native.photo_loss(d_x, d_ph, torch.from_numpy(np.ascontiguousarray(sc)), EPS, head=head, weights=d_w,
                                       exposure=d_e, want_exposure_grad=True)
    results["C ABI, host table"] = (loss.item(), _np(grad), _np(ge))
    leaf, e_leaf = d_x.clone().requires_grad_(True), d_e.clone().requires_grad_(True)
    l = _module(head)(leaf, d_ph, d_sc, d_w, e_leaf)
    assert l.dim() == 0
    l.backward()
    results["module"] = (l.item(), _np(leaf.grad), _np(e_leaf.grad))
    first = results["C ABI"]
    for how, (loss, grad, ge) in results.items():
        if ge is not None:
            print("[exposure-photo] %s, %s: loss %.9g (oracle %.9g), exposure gradient worst err/bound %.3g, err/A %.3g; "
                  "%d tie pixels, %d tied terms" % ((what, how, loss, R.ref.loss) + R.worst(ge) + (R.ref.n_ties(), R.tied_terms)))
            R.assert_exposure_grad_close(ge, "%s %s" % (what, how))
            assert np.array_equal(ge, first[2]), "%s: %s: other exposure gradient bits" % (what, how)
        R.ref.assert_close(loss, grad, "%s %s" % (what, how))
        assert loss == first[0] and np.array_equal(grad, first[1]), "%s: %s: other bits than the first call" % (what, how)
    _scratch_is_zero(native)
    return first


CASE_PARAMS = [(name, layout, head) for name, _, _, _, tied in wp.CASES for layout in xp.LAYOUTS
               for head in ((False, True) if tied else (False,))]


@pytest.mark.parametrize("name,layout,head", CASE_PARAMS,
                         ids=["%s-%s-%s" % (n, l or "unweighted", "head" if h else "maps") for n, l, h in CASE_PARAMS])
def test_against_the_oracle(dev, native, name, layout, head):
    c, e, R = xp.reference(name, layout, head)
    assert R.tied_terms <= tolerances.MAX_TIE_PIXELS and R.sign_flips == 0
    x, w = (c["enc"] if head else c["maps"]), (None if layout is None else c["weights"][layout])
    what = "%s %s %s" % (name, layout or "unweighted", "head" if head else "maps")
    loss, grad, ge = _run_all_ways(native, dev, what, x, c["photos"], w, c["scenes"], e, head, R)
    assert np.isfinite(grad).all() and np.isfinite(ge).all() and ge.any()


def test_more_workgroups_than_slots(dev, native):
    c, e, R = xp.big_case()
    assert R.tied_terms <= tolerances.MAX_TIE_PIXELS and R.sign_flips == 0
    _run_all_ways(native, dev, "%s per-photo maps" % c["name"], c["maps"], c["photos"], c["weights"]["per-photo"], c["scenes"],
                  e, False, R)


@pytest.mark.parametrize("head", [False, True], ids=["maps", "head"])
def test_reference_fixture(dev, native, golden, head):
    """against the values the reference's renderer and torch autograd wrote, the gain a leaf that multiplies the rendering;
    NaN in the photos under zero weights, a fully masked row, H = 13"""
    g = golden("g22_photo_exposure.npz")
    B, H = int(g["B"]), int(g["H"])
    x = head_checks.fixture_input(int(g["enc_seed"]), B, H) if head else synth.make_maps(int(g["input_seed"]), B, H)
    assert synth.checksum(x) == str(g["enc_sha256" if head else "input_sha256"])
    R = xp.ExposureReference(x, g["photos"], g["scenes"], g["exposure"], EPS, head, g["weights"])
    loss, grad, ge = _run_all_ways(native, dev, "g22 %s vs the oracle" % ("head" if head else "maps"), x, g["photos"],
                                   g["weights"], g["scenes"], g["exposure"], head, R)
    ref_loss, ref_grad, ref_grad64 = (g["head_loss"], g["grad9"], g["grad9_f64"]) if head else \
        (g["loss"], g["grad_input"], g["grad_input_f64"])
    ref_ge64 = g["head_grad_exposure_f64"] if head else g["grad_exposure_f64"]
    tolerances.assert_loss_close(loss, ref_loss, "g22 vs the reference loss")
    photo_checks.assert_photo_grad_close(grad, ref_grad, ref_grad64, R.ref.tie, "g22 %s vs the reference" % ("head" if head else "maps"))
    err = np.abs(ge.astype(np.float64) - ref_ge64)
    print("[exposure-photo] g22 %s vs the reference's float64 exposure gradient: worst err/bound %.3g" % (
        "head" if head else "maps", float((err / R.bound).max())))
    assert (err <= R.bound).all()        # (the reference scales the rendering, the kernel the colour: inside the bound too)
    assert not grad[:, :, int(g["masked_row"]), :].any()


@pytest.mark.parametrize("name,head", [("17_s2", False), ("17_s2", True), ("64_s9", False), ("64_s9", True), ("64_s9_untied", False)],
                         ids=["17_s2-maps", "17_s2-head", "64_s9-maps", "64_s9-head", "64_s9_untied-maps"])
def test_bit_for_bit_relations(dev, native, name, head):
    """all-ones exposure: the existing entries' loss and gradient; exposure e: the existing entry on the float32 pre-scaled
    table; grad_exposure bit-identical over five launches"""
    c = wp.case_inputs(name)
    e = xp.exposure_of(c["H"], c["S"])
    d_x, d_ph, d_sc, d_e = _t(c["enc"] if head else c["maps"], dev), _t(c["photos"], dev), _t(c["scenes"], dev), _t(e, dev)
    d_scaled = torch.cat((d_sc[..., :6], d_sc[..., 6:] * d_e), dim=-1)
    assert np.array_equal(_np(d_scaled), xp.scaled_table(c["scenes"], e))          # one float32 multiply, host or device
    for layout in xp.LAYOUTS:
        d_w = None if layout is None else _t(c["weights"][layout], dev)
        plain_loss, plain_grad = native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w)
        loss, grad, ge = native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w, exposure=torch.ones_like(d_e),
                                           want_exposure_grad=True)
        assert loss.item() == plain_loss.item() and torch.equal(grad, plain_grad), (name, head, layout)
        assert torch.isfinite(ge).all()
        scaled_loss, scaled_grad = native.photo_loss(d_x, d_ph, d_scaled, EPS, head=head, weights=d_w)
        runs = [native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w, exposure=d_e, want_exposure_grad=True)
                for _ in range(5)]
        for loss, grad, ge in runs:
            assert loss.item() == scaled_loss.item() and torch.equal(grad, scaled_grad), (name, head, layout)
            assert torch.equal(ge, runs[0][2]), "grad_exposure differs between launches"
    _scratch_is_zero(native)


@pytest.mark.parametrize("head", [False, True], ids=["maps", "head"])
def test_broadcast_forms_sum_the_gradient(dev, native, head):
    """[B,S], [B,S,1] and [B,1,1] exposures: the [B,S,3] gradient of the expanded gains summed over the broadcast axes by
    torch's own reduction -- allclose at 1e-6 of the largest A"""
    c, e, R = xp.reference("33_s3", "per-photo", head)
    d_x, d_ph, d_sc, d_w = _t(c["enc"] if head else c["maps"], dev), _t(c["photos"], dev), _t(c["scenes"], dev), \
        _t(c["weights"]["per-photo"], dev)
    fn = _module(head)
    for form in (e[:, :, 0], e[:, :, :1], e[:, :1, :1]):
        small = _t(form, dev).requires_grad_(True)
        fn(d_x, d_ph, d_sc, d_w, small).backward()
        full = small.detach().reshape(form.shape if form.ndim == 3 else form.shape + (1,)).expand(2, c["S"], 3).contiguous()
        _, _, ge = native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w, exposure=full, want_exposure_grad=True)
        want = ge.sum_to_size(small.shape if small.dim() == 3 else small.shape + (1,)).reshape(small.shape)
        assert small.grad.shape == small.shape
        RF = xp.ExposureReference(c["enc"] if head else c["maps"], c["photos"], c["scenes"], _np(full), EPS, head, c["weights"]["per-photo"])
        assert torch.allclose(small.grad, want, rtol=0.0, atol=1e-6 * float(RF.A.max())), (form.shape, (small.grad - want).abs().max().item())
        RF.assert_exposure_grad_close(_np(ge), "expanded %s" % (form.shape,))
    _scratch_is_zero(native)


@pytest.mark.parametrize("head", [False, True], ids=["maps", "head"])
def test_bad_values(dev, native, head):
    """a zero-weight plane gives exactly (+-)0 for its photo; an exposure component of 0, -1, NaN or +inf, or a NaN in the
    maps, gives a NaN loss and an all-NaN grad_exposure; the scratch is zero after each and the next good call is correct"""
    c, e, R = xp.reference("33_s3", "per-photo", head)
    x = c["enc"] if head else c["maps"]
    d_x, d_ph, d_sc, d_e = _t(x, dev), _t(c["photos"], dev), _t(c["scenes"], dev), _t(e, dev)
    w = c["weights"]["per-photo"].copy()
    w[1, 2] = 0.0
    spoiled = c["photos"].copy()
    spoiled[1, 2] = np.nan                                              # excused with its plane
    loss, grad, ge = native.photo_loss(d_x, _t(spoiled, dev), d_sc, EPS, head=head, weights=_t(w, dev), exposure=d_e,
                                       want_exposure_grad=True)
    ge = _np(ge)
    assert np.isfinite(loss.item()) and np.isfinite(ge).all() and not ge[1, 2].any() and ge[1, :2].all() and ge[0].all()
    _scratch_is_zero(native)
    d_w = _t(c["weights"]["per-photo"], dev)
    good = native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w, exposure=d_e, want_exposure_grad=True)
    for value in (0.0, -1.0, np.nan, np.inf):
        for where in ((0, 0, 0), (1, 2, 1)):
            for weights in (d_w, None, torch.zeros_like(d_w)):          # a weight does not excuse a bad gain
                bad = e.copy()
                bad[where] = value
                loss, grad, ge = native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=weights, exposure=_t(bad, dev),
                                                   want_exposure_grad=True)
                assert np.isnan(loss.item()) and torch.isnan(ge).all(), (value, where)
                _scratch_is_zero(native)
    bad = x.copy()
    bad[1, 1, 5, 7] = np.nan
    loss, grad, ge = native.photo_loss(_t(bad, dev), d_ph, d_sc, EPS, head=head, weights=d_w, exposure=d_e, want_exposure_grad=True)
    assert np.isnan(loss.item()) and torch.isnan(ge).all()
    _scratch_is_zero(native)
    again = native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w, exposure=d_e, want_exposure_grad=True)
    assert again[0].item() == good[0].item() and torch.equal(again[1], good[1]) and torch.equal(again[2], good[2])     # nothing sticks
    R.assert_exposure_grad_close(_np(again[2]), "after the bad calls")


@pytest.mark.parametrize("head", [False, True], ids=["maps", "head"])
def test_module_behaviour(dev, native, head):
    from svbrdf_estimation_amd import losses
    c, e, R = xp.reference("33_s3", "per-photo", head)
    x, w = (c["enc"] if head else c["maps"]), c["weights"]["per-photo"]
    d_x, d_ph, d_sc, d_w, d_e = _t(x, dev), _t(c["photos"], dev), _t(c["scenes"], dev), _t(w, dev), _t(e, dev)
    fn = _module(head)
    ref_loss, ref_grad, ref_ge = native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w, exposure=d_e, want_exposure_grad=True)
    # ONE launch for the loss and a plain backward with both gradients
    leaf, e_leaf = d_x.clone().requires_grad_(True), d_e.clone().requires_grad_(True)
    torch.cuda.synchronize()
    n0 = native.launch_count()
    l = fn(leaf, d_ph, d_sc, d_w, e_leaf)
    assert isinstance(l, losses._PhotoLossTensor)
    l.backward()
    torch.cuda.synchronize()
    assert native.launch_count() - n0 == 1
    assert l.item() == ref_loss.item() and torch.equal(leaf.grad, ref_grad) and torch.equal(e_leaf.grad, ref_ge)
    # only the exposure wants a gradient (maps held fixed): still the exposure kernel, one launch
    e_only = d_e.clone().requires_grad_(True)
    n0 = native.launch_count()
    fn(d_x, d_ph, d_sc, d_w, e_only).backward()
    assert native.launch_count() - n0 == 1 and torch.equal(e_only.grad, ref_ge)
    # retain_graph=True: repeated backwards accumulate; without it a second backward fails like autograd's own nodes
    leaf, e_leaf = d_x.clone().requires_grad_(True), d_e.clone().requires_grad_(True)
    l = fn(leaf, d_ph, d_sc, d_w, e_leaf)
    l.backward(retain_graph=True)
    l.backward()
    assert torch.equal(leaf.grad, 2 * ref_grad) and torch.equal(e_leaf.grad, 2 * ref_ge)
    with pytest.raises(RuntimeError, match="second time"):
        l.backward()
    # an upstream gradient scales both
    leaf, e_leaf = d_x.clone().requires_grad_(True), d_e.clone().requires_grad_(True)
    (3.0 * fn(leaf, d_ph, d_sc, d_w, e_leaf)).backward()
    assert torch.equal(leaf.grad, 3 * ref_grad) and torch.equal(e_leaf.grad, 3 * ref_ge)
    # torch.no_grad() evaluation: the pre-scaled table through the forward-only kernel, the same loss bit for bit
    with torch.no_grad():
        n0 = native.launch_count()
        assert fn(d_x.clone().requires_grad_(True), d_ph, d_sc, d_w, d_e).item() == ref_loss.item()
        assert native.launch_count() - n0 == 1
    assert fn(d_x, d_ph, d_sc, d_w, d_e).item() == ref_loss.item() and not fn(d_x, d_ph, d_sc, d_w, d_e).requires_grad
    # float64 and create_graph=True take the composed definition
    x64, e64 = d_x.double().requires_grad_(True), d_e.double().requires_grad_(True)
    composed = fn(x64, d_ph, d_sc, d_w, e64)
    assert composed.dtype == torch.float64
    composed.backward()
    tolerances.assert_loss_close(ref_loss.item(), composed.item(), "fused vs float64 composed")
    photo_checks.assert_photo_grad_close(_np(ref_grad), _np(x64.grad), R.ref.grad64, R.ref.tie, "fused vs float64 composed")
    R.assert_exposure_grad_close(_np(e64.grad), "float64 composed exposure gradient")
    mixed = fn(d_x, d_ph, d_sc, d_w, d_e.double())
    assert mixed.dtype == torch.float64
    x2, e2 = d_x.clone().requires_grad_(True), d_e.clone().requires_grad_(True)
    g_x, g_e = torch.autograd.grad(fn(x2, d_ph, d_sc, d_w, e2), (x2, e2), create_graph=True)
    assert g_x.requires_grad and g_e.requires_grad and g_e.dtype == torch.float32
    R.assert_exposure_grad_close(_np(g_e), "create_graph exposure gradient")
    g_e.square().sum().backward()
    assert x2.grad is not None and e2.grad is not None and torch.isfinite(e2.grad).all() and e2.grad.abs().max() > 0
    # normalize="weights" scales both gradients
    full = photo_checks.broadcast_weights(w, c["S"]).astype(np.float64)
    scale = full.size / full.sum()
    leaf, e_leaf = d_x.clone().requires_grad_(True), d_e.clone().requires_grad_(True)
    got = _module(head, "weights")(leaf, d_ph, d_sc, d_w, e_leaf)
    got.backward()
    tolerances.assert_loss_close(got.item(), R.ref.loss64 * scale, "normalize=weights")
    assert torch.allclose(e_leaf.grad, ref_ge * scale, rtol=1e-6, atol=0.0) and torch.allclose(leaf.grad, ref_grad * scale, rtol=1e-6, atol=0.0)
    _scratch_is_zero(native)


def test_exposure_fit_lowers_the_loss(dev, native):
    """tools/fit_photos.py --fit-exposure in small: 32 x 32, B = 1, S = 4, the maps held at the truth, noise-free photographs
    taken with hidden gains in [0.5, 2]; 40 Adam steps on log e from e = 1.  A condition, not a measurement: the loss after
    the last step is lower than at step 0."""
    B, S, H = 1, 4, 32
    sc = photo_checks.scene_table(B, 77, 2, 2)
    maps = synth.make_maps(6500, B, H)
    hidden = xp.exposure_of(H, S, B)
    d_maps, d_sc = _t(maps, dev), _t(sc, dev)
    photos = native.render_fwd(d_maps, _t(xp.scaled_table(sc, hidden), dev))
    fn = _module(False)
    log_e = torch.zeros((B, S, 3), device=dev, requires_grad=True)
    opt = torch.optim.Adam([log_e], lr=0.05)
    history = []
    for _ in range(40):
        opt.zero_grad(set_to_none=True)
        loss = fn(d_maps, photos, d_sc, None, log_e.exp())
        loss.backward()
        opt.step()
        history.append(loss.item())
    with torch.no_grad():
        history.append(fn(d_maps, photos, d_sc, None, log_e.exp()).item())
        off = (log_e - torch.log(_t(hidden, dev))).abs().mean().item()
    print("[exposure-photo] fit: loss %.6g -> %.6g over 40 steps, mean |log e - log e*| %.4f -> %.4f" % (
        history[0], history[-1], float(np.abs(np.log(hidden)).mean()), off))
    assert np.isfinite(history).all() and history[-1] < history[0]
    _scratch_is_zero(native)


def test_exposure_is_no_slower_than_its_composition(dev, native):
    res = xp.measure_exposure_photo_loss(dev, native)
    text = ("exposure photo loss with grad_exposure %.2f us per launch, weighted photo loss on the pre-scaled table %.2f "
            "(ratio %.3f, recorded), unfused composition with an exposure leaf %.2f us per step (%.1fx); per round %s" % (
                res["exposure_us"], res["weighted_us"], res["exposure_us"] / res["weighted_us"], res["composition_us"],
                res["composition_us"] / res["exposure_us"], res["rounds"]))
    print("[exposure-photo] config-2 shape, per-photo weights: " + text)
    out = os.environ.get("SVBRDF_RESULTS_DIR")
    with open(os.path.join(out, "exposure_photo_loss_speed.txt") if out else os.devnull, "w") as f:
        f.write("# tests/test_gpu_exposure_photo_loss.py speed test on %s\n%s\n" % (res["device"], text))
    assert res["exposure_us"] <= res["composition_us"], res
