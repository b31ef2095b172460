"""The photo losses with the gradient towards the scene table on the device (csrc/svbrdf_photo_pose.hip: k_pose_*;
losses.PhotoLoss / HeadPhotoLoss with a ``[B,S,9]`` table that requires grad):

    L = (1/N) sum w | log(render(scene[b,s], input[b]) + eps) - log(p' + eps) |
    grad_scenes[b,s,:] = dL / d (camera xyz | light xyz | light rgb)

Loss and map gradient: BITWISE those of the existing weighted / unweighted entries on the same table.  grad_scenes: against
the eager restatement of the reference's renderer with the scene row as a dual number (tests/pose_photo_checks.py: nothing
under oracle/ changes for it), per (b, s, k) within GRAD_RTOL A + GRAD_ATOL_FRAC max(A) + 2 T with A the sum of the terms'
magnitudes and T that of the tied terms, max(A) per column group.  By the oracle alone the cases have 0 tied terms and no
sign flip (tests/test_pose_photo_loss_cpu.py).

Why these shapes (weighted_photo_checks.CASES plus the 80-workgroup case): 17 x 17 has a partial second workgroup and a wave
with dead lanes, which run whole and must add 0; S = 1 / 2 / 3 and 9; a width that is no power of two; tied roughness and the
three-lobe loop; 64 x 64, S = 9, B = 5 has 80 workgroups, more than the 64 slots of the loss reduction.  A hand-made table
covers a light behind part of the patch (LN+ = 0) and a grazing camera (VN at its clamp).

Speed at the configuration-2 shape (B = 8, 256 x 256, S = 9, per-photo weights): the fused entry must be no slower than the
composed torch-op definition forward + backward; its ratio to the weighted kernel on the same table is recorded, not
asserted (profiles/r17_photo_pose.txt).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import exposure_photo_checks as xp
import head_checks
import photo_checks
import pose_photo_checks as pc
import synth
import tolerances
import weighted_photo_checks as wp
from photo_checks import assert_scratch_is_zero as _scratch_is_zero, to_device as _t, to_numpy as _np

pytestmark = pytest.mark.gpu
EPS = pc.EPS


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


def _run_all_ways(native, dev, what, x, ph, w, sc, head, R):
    """the C ABI twice (two launches), the module with a device table and with a host table moved to the device: loss and
    map gradient the existing entry's bits, grad_scenes inside the bound of `R` (a PoseReference) and the same bits every
    way, scratch zeroed -> (loss, grad, grad_scenes)"""
    d_x, d_ph, d_sc = _t(x, dev), _t(ph, dev), _t(sc, dev)
    d_w = None if w is None else _t(w, dev)
    plain_loss, plain_grad = native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w)
    results = {}
    for how in ("C ABI", "C ABI, second launch"):
        loss, grad, gs = native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w, want_scene_grad=True)
        results[how] = (loss.item(), _np(grad), _np(gs))
    for how, table in (("module", d_sc.clone()), ("module, host table", torch.from_numpy(np.ascontiguousarray(sc)).clone())):
        leaf, t_leaf = d_x.clone().requires_grad_(True), table.requires_grad_(True)
        l = _module(head)(leaf, d_ph, t_leaf, d_w)
        assert l.dim() == 0
        l.backward()
        assert t_leaf.grad.device == t_leaf.device and t_leaf.grad.shape == t_leaf.shape
        results[how] = (l.item(), _np(leaf.grad), _np(t_leaf.grad))
    first = results["C ABI"]
    assert first[0] == plain_loss.item() and np.array_equal(first[1], _np(plain_grad)), \
        "%s: loss or map gradient differ from the entry without the scene gradient" % what
    for how, (loss, grad, gs) in results.items():
        R.assert_scene_grad_close(gs, "%s %s" % (what, how))
        assert loss == first[0] and np.array_equal(grad, first[1]) and np.array_equal(gs, first[2]), \
            "%s: %s: other bits than the first call" % (what, how)
    R.ref.assert_close(first[0], first[1], what)
    _scratch_is_zero(native)
    return first


CASE_PARAMS = [(name, layout, head) for name, _, _, _, tied in wp.CASES for layout in pc.LAYOUTS
               for head in ((False, True) if tied else (False,))]


@pytest.mark.parametrize("name,layout,head", CASE_PARAMS,
                         ids=["%s-%s-%s" % (n, l or "unweighted", "head" if h else "maps") for n, l, h in CASE_PARAMS])
def test_against_the_oracle(dev, native, name, layout, head):
    c, R = pc.reference(name, layout, head)
    assert R.tied_terms <= tolerances.MAX_TIE_PIXELS and R.sign_flips == 0
    x, w = (c["enc"] if head else c["maps"]), (None if layout is None else c["weights"][layout])
    what = "%s %s %s" % (name, layout or "unweighted", "head" if head else "maps")
    loss, grad, gs = _run_all_ways(native, dev, what, x, c["photos"], w, c["scenes"], head, R)
    assert np.isfinite(grad).all() and gs.all()


@pytest.mark.parametrize("layout,head", pc.BIG_PARAMS,
                         ids=["%s-%s" % (l or "unweighted", "head" if h else "maps") for l, h in pc.BIG_PARAMS])
def test_more_workgroups_than_slots(dev, native, layout, head):
    """80 workgroups on the 64 slots of the loss reduction, each of the four kernels: the accumulator adds of every
    workgroup must have returned before the finisher, whichever slot completes last, drains them"""
    c, R = pc.big_case(layout, head)
    assert R.tied_terms <= tolerances.MAX_TIE_PIXELS and R.sign_flips == 0
    w = None if layout is None else c["weights"][layout]
    _run_all_ways(native, dev, "%s %s %s" % (c["name"], layout or "unweighted", "head" if head else "maps"),
                  c["enc"] if head else c["maps"], c["photos"], w, c["scenes"], head, R)


def test_light_behind_the_patch_and_grazing_camera(dev, native):
    """the sub-gradient conventions at the clamps: LN+ = 0 where the light is behind the surface (the term and every
    gradient of it exactly 0), VN at its clamp of 1e-3 (no gradient through n.wo there)"""
    c, R, n_dark, n_grazing = pc.edge_case()
    assert n_dark > 50 and n_grazing > 50, (n_dark, n_grazing)
    assert R.tied_terms <= tolerances.MAX_TIE_PIXELS and R.sign_flips == 0
    _run_all_ways(native, dev, "17_edge maps", c["maps"], c["photos"], None, c["scenes"], False, R)


@pytest.mark.parametrize("head", [False, True], ids=["maps", "head"])
def test_reference_fixture(dev, native, golden, head):
    """against the values the reference's renderer wrote: loss and map gradient by its autograd, the table gradient by
    central differences of its float64 renderings; NaN in the photos under zero weights, a fully masked row, H = 13"""
    g = golden("g23_photo_pose.npz")
    B, H = int(g["B"]), int(g["H"])
    x = head_checks.fixture_input(int(g["enc_seed"]), B, H) if head else synth.make_maps(int(g["input_seed"]), B, H)
    assert synth.checksum(x) == str(g["enc_sha256" if head else "input_sha256"])
    R = pc.PoseReference(x, g["photos"], g["scenes"], EPS, head, g["weights"])
    what = "g23 %s" % ("head" if head else "maps")
    loss, grad, gs = _run_all_ways(native, dev, what + " vs the oracle", x, g["photos"], g["weights"], g["scenes"], head, R)
    ref_loss, ref_grad, ref_grad64 = (g["head_loss"], g["grad9"], g["grad9_f64"]) if head else \
        (g["loss"], g["grad_input"], g["grad_input_f64"])
    tolerances.assert_loss_close(loss, ref_loss, "g23 vs the reference loss")
    photo_checks.assert_photo_grad_close(grad, ref_grad, ref_grad64, R.ref.tie, what + " vs the reference")
    err = np.abs(gs.astype(np.float64) - g["head_grad_scenes_f64" if head else "grad_scenes_f64"])
    print("[pose] %s vs the reference's central differences: worst err/bound %.3g" % (what, float((err / R.bound).max())))
    assert (err <= R.bound).all()
    assert not grad[:, :, int(g["masked_row"]), :].any()


@pytest.mark.parametrize("head", [False, True], ids=["maps", "head"])
def test_colour_columns_agree_with_the_exposure_gradient(dev, native, head):
    """d L / d colour times the colour is d L / d gain at unit gains: the exposure entry's grad_exposure, within the bound;
    with exposure= the module's loss and map gradient are the exposure entry's bits and the gains' gradient is within
    ITS bound"""
    c, R = pc.reference("33_s3", "per-photo", head)
    _, e, XR = xp.reference("33_s3", "per-photo", head)
    x = c["enc"] if head else c["maps"]
    d_x, d_ph, d_sc, d_w, d_e = _t(x, dev), _t(c["photos"], dev), _t(c["scenes"], dev), _t(c["weights"]["per-photo"], dev), _t(e, dev)
    _, _, gs = native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w, want_scene_grad=True)
    _, _, ge = native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w, exposure=torch.ones_like(d_e), want_exposure_grad=True)
    colour = c["scenes"][:, :, 6:9].astype(np.float64)
    err = np.abs(_np(gs)[:, :, 6:9].astype(np.float64) * colour - _np(ge).astype(np.float64))
    bound = R.bound[:, :, 6:9] * colour
    print("[pose] colour columns vs grad_exposure at unit gains: worst err/bound %.3g" % float((err / bound).max()))
    assert (err <= bound).all()
    x_loss, x_grad, x_ge = native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w, exposure=d_e, want_exposure_grad=True)
    leaf, t_leaf, e_leaf = d_x.clone().requires_grad_(True), d_sc.clone().requires_grad_(True), d_e.clone().requires_grad_(True)
    n0 = native.launch_count()
    l = _module(head)(leaf, d_ph, t_leaf, d_w, e_leaf)
    l.backward()
    torch.cuda.synchronize()
    assert native.launch_count() - n0 == 1
    assert l.item() == x_loss.item() and torch.equal(leaf.grad, x_grad)
    XR.assert_exposure_grad_close(_np(e_leaf.grad), "gains through the table's colour columns")
    assert torch.isfinite(t_leaf.grad).all()
    _scratch_is_zero(native)


@pytest.mark.parametrize("head", [False, True], ids=["maps", "head"])
def test_bad_values(dev, native, head):
    """a colour of 0, -1, NaN or +inf, a bad weight or a NaN in the maps gives a NaN loss and an all-NaN grad_scenes; the
    scratch is zero after each and the next good call is correct"""
    c, R = pc.reference("33_s3", "per-photo", head)
    x = c["enc"] if head else c["maps"]
    d_x, d_ph, d_sc, d_w = _t(x, dev), _t(c["photos"], dev), _t(c["scenes"], dev), _t(c["weights"]["per-photo"], dev)
    good = native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w, want_scene_grad=True)
    for value in (0.0, -1.0, np.nan, np.inf):
        for where in ((0, 0, 6), (1, 2, 7)):
            for weights in (d_w, None, torch.zeros_like(d_w)):          # a weight does not excuse a bad colour
                bad = c["scenes"].copy()
                bad[where] = value
                loss, grad, gs = native.photo_loss(d_x, d_ph, _t(bad, dev), EPS, head=head, weights=weights, want_scene_grad=True)
                assert np.isnan(loss.item()) and torch.isnan(gs).all(), (value, where)
                _scratch_is_zero(native)
    for value in (-0.5, 1.5, np.nan):
        w = c["weights"]["per-photo"].copy()
        w[1, 1, 20, 3] = value
        loss, grad, gs = native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=_t(w, dev), want_scene_grad=True)
        assert np.isnan(loss.item()) and torch.isnan(gs).all(), value
        _scratch_is_zero(native)
    bad = x.copy()
    bad[1, 1, 5, 7] = np.nan
    loss, grad, gs = native.photo_loss(_t(bad, dev), d_ph, d_sc, EPS, head=head, weights=d_w, want_scene_grad=True)
    assert np.isnan(loss.item()) and torch.isnan(gs).all()
    _scratch_is_zero(native)
    bad = c["scenes"].copy()
    bad[0, 1, 4] = np.nan                                               # a NaN position
    loss, grad, gs = native.photo_loss(d_x, d_ph, _t(bad, dev), EPS, head=head, weights=d_w, want_scene_grad=True)
    assert np.isnan(loss.item()) and torch.isnan(gs).all()
    _scratch_is_zero(native)
    again = native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w, want_scene_grad=True)
    assert again[0].item() == good[0].item() and torch.equal(again[1], good[1]) and torch.equal(again[2], good[2])     # nothing sticks
    R.assert_scene_grad_close(_np(again[2]), "after the bad calls")


def test_wave_sum_beyond_the_fixed_point_limit_is_reported_as_nan(dev, native):
    """the overflow guard: a camera 1e-9 above one pixel makes that pixel's FINITE camera terms carry its wave's sum of
    N |term| some 200 times beyond the limit of 2^19 (by the oracle's float64 values), while the loss itself is finite --
    the existing entry reports it.  The scene-gradient entry must then report NaN for the loss and every gradient, never
    a finite (wrapped or saturated) number, leave the scratch zeroed, and the next call must be right again."""
    c, loss64, wave_sum = pc.overflow_case()
    assert np.isfinite(loss64) and wave_sum > 16 * pc.WAVE_LIMIT, (loss64, wave_sum)
    d_x, d_ph, d_sc = _t(c["maps"], dev), _t(c["photos"], dev), _t(c["scenes"], dev)
    plain_loss, plain_grad = native.photo_loss(d_x, d_ph, d_sc, EPS)
    tolerances.assert_loss_close(plain_loss.item(), loss64, "the loss itself is finite", rtol=1e-4)
    for weights in (None, torch.ones((2, 1, c["H"], c["H"]), device=dev)):
        loss, grad, gs = native.photo_loss(d_x, d_ph, d_sc, EPS, weights=weights, want_scene_grad=True)
        assert np.isnan(loss.item()) and torch.isnan(gs).all(), (loss.item(), gs)
        assert torch.equal(grad.view(torch.int32), plain_grad.view(torch.int32))     # the map gradient's bits stay what they are
        _scratch_is_zero(native)
    good, R = pc.reference("17_s1", None, False)
    loss, grad, gs = native.photo_loss(d_x, d_ph, _t(good["scenes"], dev), EPS, want_scene_grad=True)
    R.assert_scene_grad_close(_np(gs), "after the overflow report")
    _scratch_is_zero(native)


def test_pointers_off_alignment(dev, native):
    """every float pointer 4 bytes off its allocation's alignment: the aligned call's bits"""
    c, R = pc.reference("33_s3", "per-photo", False)
    arrays = [c["maps"], c["photos"], c["weights"]["per-photo"], c["scenes"]]
    d_x, d_ph, d_w, d_sc = (_t(a, dev) for a in arrays)
    good = native.photo_loss(d_x, d_ph, d_sc, EPS, weights=d_w, want_scene_grad=True)

    def shifted(a):
        buf = torch.empty(a.size + 1, dtype=torch.float32, device=dev)
        view = buf[1:].view(a.shape)
        view.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
        assert view.data_ptr() % 8 == 4 and view.is_contiguous()
        return view

    o_x, o_ph, o_w, o_sc = (shifted(a) for a in arrays)
    B, S, H = 2, c["S"], c["H"]
    lib = native._load()
    grad, gs, loss = shifted(np.zeros_like(c["maps"])), shifted(np.zeros_like(c["scenes"])), shifted(np.zeros(1, np.float32))
    ws = torch.zeros(getattr(lib, pc.WORKSPACE_BYTES)(B, S, H, H) // 8, dtype=torch.int64, device=dev)
    rc = lib.svbrdf_photo_loss_scene_grad_fwd_bwd(
        o_x.data_ptr(), o_ph.data_ptr(), o_w.data_ptr(), S, o_sc.data_ptr(), native.xrow(dev, H).data_ptr(), ctypes.c_float(EPS),
        loss.data_ptr(), grad.data_ptr(), gs.data_ptr(), ws.data_ptr(), ws.numel() * 8, B, S, H, H,
        ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0, lib.svbrdf_last_error()
    torch.cuda.synchronize()
    assert loss.item() == good[0].item() and torch.equal(grad, good[1]) and torch.equal(gs, good[2])
    assert not ws.any().item()


@pytest.mark.parametrize("head", [False, True], ids=["maps", "head"])
def test_module_behaviour(dev, native, head):
    from svbrdf_estimation_amd import losses
    c, R = pc.reference("33_s3", "per-photo", head)
    x, w = (c["enc"] if head else c["maps"]), c["weights"]["per-photo"]
    d_x, d_ph, d_sc, d_w = _t(x, dev), _t(c["photos"], dev), _t(c["scenes"], dev), _t(w, dev)
    fn = _module(head)
    ref_loss, ref_grad, ref_gs = native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w, want_scene_grad=True)
    # ONE launch for the loss and a plain backward with both gradients
    leaf, t_leaf = d_x.clone().requires_grad_(True), d_sc.clone().requires_grad_(True)
    torch.cuda.synchronize()
    n0 = native.launch_count()
    l = fn(leaf, d_ph, t_leaf, d_w)
    assert isinstance(l, losses._PhotoLossTensor)
    l.backward()
    torch.cuda.synchronize()
    assert native.launch_count() - n0 == 1
    assert l.item() == ref_loss.item() and torch.equal(leaf.grad, ref_grad) and torch.equal(t_leaf.grad, ref_gs)
    # only the table wants a gradient (maps held fixed): still the scene-gradient kernel, one launch
    t_only = d_sc.clone().requires_grad_(True)
    n0 = native.launch_count()
    fn(d_x, d_ph, t_only, d_w).backward()
    assert native.launch_count() - n0 == 1 and torch.equal(t_only.grad, ref_gs)
    # a table that does not require grad, or no_grad: exactly the existing path and its bits
    plain_loss, plain_grad = native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w)
    leaf = d_x.clone().requires_grad_(True)
    l = fn(leaf, d_ph, d_sc, d_w)
    l.backward()
    assert l.item() == plain_loss.item() and torch.equal(leaf.grad, plain_grad)
    with torch.no_grad():
        assert fn(d_x, d_ph, d_sc.clone().requires_grad_(True), d_w).item() == plain_loss.item()
    # retain_graph=True: repeated backwards accumulate; without it a second backward fails like autograd's own nodes
    leaf, t_leaf = d_x.clone().requires_grad_(True), d_sc.clone().requires_grad_(True)
    l = fn(leaf, d_ph, t_leaf, d_w)
    l.backward(retain_graph=True)
    l.backward()
    assert torch.equal(leaf.grad, 2 * ref_grad) and torch.equal(t_leaf.grad, 2 * ref_gs)
    with pytest.raises(RuntimeError, match="second time"):
        l.backward()
    # an upstream gradient scales both
    leaf, t_leaf = d_x.clone().requires_grad_(True), d_sc.clone().requires_grad_(True)
    (3.0 * fn(leaf, d_ph, t_leaf, d_w)).backward()
    assert torch.equal(leaf.grad, 3 * ref_grad) and torch.equal(t_leaf.grad, 3 * ref_gs)
    # float64 and create_graph=True take the composed definition
    x64, t64 = d_x.double().requires_grad_(True), d_sc.clone().requires_grad_(True)
    composed = fn(x64, d_ph, t64, d_w)
    assert composed.dtype == torch.float64
    composed.backward()
    tolerances.assert_loss_close(ref_loss.item(), composed.item(), "fused vs float64 composed")
    R.assert_scene_grad_close(_np(t64.grad), "float64 composed scene gradient")
    x2, t2 = d_x.clone().requires_grad_(True), d_sc.clone().requires_grad_(True)
    g_x, g_t = torch.autograd.grad(fn(x2, d_ph, t2, d_w), (x2, t2), create_graph=True)
    assert g_x.requires_grad and g_t.requires_grad and g_t.dtype == torch.float32
    R.assert_scene_grad_close(_np(g_t), "create_graph scene gradient")
    g_t.square().sum().backward()
    assert x2.grad is not None and t2.grad is not None and torch.isfinite(t2.grad).all() and t2.grad.abs().max() > 0
    # normalize="weights" scales both gradients
    full = photo_checks.broadcast_weights(w, c["S"]).astype(np.float64)
    scale = full.size / full.sum()
    leaf, t_leaf = d_x.clone().requires_grad_(True), d_sc.clone().requires_grad_(True)
    got = _module(head, "weights")(leaf, d_ph, t_leaf, d_w)
    got.backward()
    tolerances.assert_loss_close(got.item(), R.ref.loss64 * scale, "normalize=weights")
    assert torch.allclose(t_leaf.grad, ref_gs * scale, rtol=1e-6, atol=0.0) and torch.allclose(leaf.grad, ref_grad * scale, rtol=1e-6, atol=0.0)
    _scratch_is_zero(native)


def test_pose_fit_lowers_the_loss_and_the_position_error(dev, native):
    """tools/fit_photos.py --fit-pose in small: 32 x 32, B = 1, S = 4, the maps held at the truth, noise-free photographs;
    light and camera positions start a few per cent off; 40 Adam steps on the six position columns.  A condition, not a
    measurement: the loss and the mean position error after the last step are lower than at step 0."""
    B, S, H = 1, 4, 32
    sc = photo_checks.scene_table(B, 77, 2, 2)
    maps = synth.make_maps(6500, B, H)
    d_maps, d_true = _t(maps, dev), _t(sc, dev)
    photos = native.render_fwd(d_maps, d_true)
    off = (np.float32(1.0) + np.float32(0.06) * (synth.uniform01(6600, (B, S, 6)) - np.float32(0.5))).astype(np.float32)
    start = sc.copy()
    start[:, :, :6] *= off
    pos = _t(start[:, :, :6], dev).requires_grad_(True)
    colour = d_true[:, :, 6:]
    fn = _module(False)
    opt = torch.optim.Adam([pos], lr=0.004)
    history, error = [], []
    for _ in range(40):
        opt.zero_grad(set_to_none=True)
        error.append((pos.detach() - d_true[:, :, :6]).abs().mean().item())
        loss = fn(d_maps, photos, torch.cat((pos, colour), dim=-1))
        loss.backward()
        opt.step()
        history.append(loss.item())
    with torch.no_grad():
        history.append(fn(d_maps, photos, torch.cat((pos, colour), dim=-1)).item())
        error.append((pos - d_true[:, :, :6]).abs().mean().item())
    text = "loss %.6g -> %.6g over 40 steps, mean |position - truth| %.5f -> %.5f" % (history[0], history[-1], error[0], error[-1])
    print("[pose] fit: " + text)
    out = os.environ.get("SVBRDF_RESULTS_DIR")
    with open(os.path.join(out, "pose_photo_loss_fit.txt") if out else os.devnull, "w") as f:
        f.write("# tests/test_gpu_pose_photo_loss.py fit test\n%s\n" % text)
    assert np.isfinite(history).all() and history[-1] < history[0] and error[-1] < error[0]
    _scratch_is_zero(native)


def test_pose_is_no_slower_than_its_composition(dev, native):
    res = pc.measure_pose_photo_loss(dev, native)
    text = ("photo loss with grad_scenes %.2f us per launch, weighted photo loss on the same table %.2f "
            "(ratio %.3f, recorded), composed torch-op definition with a table leaf %.2f us per step (%.1fx); per round %s" % (
                res["pose_us"], res["weighted_us"], res["pose_us"] / res["weighted_us"], res["composition_us"],
                res["composition_us"] / res["pose_us"], res["rounds"]))
    print("[pose] config-2 shape, per-photo weights: " + text)
    out = os.environ.get("SVBRDF_RESULTS_DIR")
    with open(os.path.join(out, "pose_photo_loss_speed.txt") if out else os.devnull, "w") as f:
        f.write("# tests/test_gpu_pose_photo_loss.py speed test on %s\n%s\n" % (res["device"], text))
    assert res["pose_us"] <= res["composition_us"], res
