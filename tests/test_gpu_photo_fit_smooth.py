"""One step of a photo fit with the smoothness prior across pixels, on the device (csrc/svbrdf_photo_fit_smooth.hip:
k_smooth_step*, k_smooth_joint*; svbrdf_photo_fit_smooth_adam_step[_scene_grad]; fitting.PhotoFit(smooth=)).  The loss is
the twin entry's photo loss, bit for bit; the gradient is the numpy float32 restatement of the header's four lines
(photo_fit_smooth_checks.smooth_gradient: k from compares, c k, g + t) fed with the existing loss entry's photo gradient; the
update is photo_fit_checks.restatement on that gradient with the library's exported scalars.  Every comparison here is BIT
FOR BIT unless it says otherwise, and every call goes through the C ABI between canaries.

The hole fit's four values and the speed test's times are printed by the tests and recorded in
profiles/r22_photo_fit_smooth.txt.
"""
import numpy as np
import pytest
import torch

import photo_checks
import photo_fit_checks as fc
import photo_fit_pose_checks as jc
import photo_fit_smooth_checks as sm

pytestmark = pytest.mark.gpu
LAM = sm.LAMBDA


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def native():
    from svbrdf_estimation_amd import _native
    return _native


_CASES = {}


def case(native, dev, name):
    """the inputs of a case (maps quantised so that ties occur; the input condition checked on the host) and its reference
    values -- the loss entry's loss and photo gradient, the scene-gradient entry's three -- computed once and shared"""
    if name not in _CASES:
        c = sm.case_inputs(native, dev, name)
        sm.assert_exercises_every_k(c)
        c["ref_loss"], c["ref_grad"] = fc.abi_loss(native, dev, c)
        c["sg_loss"], c["sg_grad"], c["ref_grad_scenes"] = jc.abi_scene_grad(native, dev, c)
        _CASES[name] = c
    return _CASES[name]


def refs(c, joint):
    return (c["sg_loss"], c["sg_grad"]) if joint else (c["ref_loss"], c["ref_grad"])


def assert_clean(out):
    assert out["launches"] == 1 and out["scratch_zero"] and out["canaries_intact"] and out["inputs_intact"], {
        k: out[k] for k in ("launches", "scratch_zero", "canaries_intact", "inputs_intact")}


def assert_step(out, want, what):
    for key, exp in zip(("x", "m", "v"), want):
        assert fc.same_bits(out[key], exp), "%s: %s differs from the restatement in %d values" % (
            what, key, fc.count_differing(out[key], exp))


JOINT = pytest.mark.parametrize("joint", (False, True), ids=("maps", "joint"))


@JOINT
@pytest.mark.parametrize("name", sm.NAMES)
def test_step_is_the_twin_loss_and_the_restatement_bit_for_bit(native, dev, name, joint):
    """loss_out is the twin entry's; grad_out is g' of the restatement; maps_out, exp_avg', exp_avg_sq' are the restatement's
    on g'; maps_in, photos, weights and table intact; canaries intact; scratch zeroed; one launch; grad_out = NULL gives the
    same; the joint entry's grad_scenes is the scene-gradient entry's"""
    c = case(native, dev, name)
    lib = native._load()
    loss, grad = refs(c, joint)
    out = sm.abi_smooth(native, dev, c, LAM, joint=joint)
    assert_clean(out)
    assert fc.same_bits(out["loss"], loss) and np.isfinite(out["loss"]).all(), (out["loss"], loss)
    g2, *want = sm.expected_step(lib, c, grad, LAM)
    assert fc.same_bits(out["grad"], g2), "grad_out differs from g' in %d values" % fc.count_differing(out["grad"], g2)
    assert_step(out, want, name)
    if c["H"] > 1:
        assert not fc.same_bits(g2, grad)                           # the prior does act at this shape
    for ch in np.nonzero(LAM == 0)[0]:
        assert fc.same_bits(out["grad"][:, ch], grad[:, ch]), ch    # lambda = 0: g, bit for bit
    if joint:
        assert fc.same_bits(out["grad_scenes"], c["ref_grad_scenes"]) and np.isfinite(out["grad_scenes"]).all()
    quiet = sm.abi_smooth(native, dev, c, LAM, joint=joint, want_grad=False)
    assert_clean(quiet)
    assert fc.same_bits(quiet["loss"], loss)
    assert_step(quiet, want, name + " without grad_out")
    if joint:
        assert fc.same_bits(quiet["grad_scenes"], c["ref_grad_scenes"])


@pytest.mark.parametrize("name", jc.PARTIAL_WAVE_CASES)
def test_joint_last_pixel_of_a_partial_wave_is_updated_exactly_once(native, dev, name):
    """the joint flow's lanes past the item's last pixel shade that LAST pixel again: the update -- and here the neighbour
    loads -- run for the lanes that own a pixel only.  m != 0 at the last pixel, so a second update could not equal one
    (tests/test_gpu_photo_fit_pose.py has the argument)."""
    import synth
    c = case(native, dev, name)
    H = c["H"]
    assert (H * H) % 64 != 0
    d = dict(c)
    u = synth.uniform01(7400 + sm.NAMES.index(name), (2,) + c["maps"].shape)
    d["m"] = ((u[0] - np.float32(0.5)) * np.float32(2e-3)).astype(np.float32)
    d["v"] = (u[1] * np.float32(1e-5) + np.float32(1e-7)).astype(np.float32)
    d["m"][:, :, H - 1, H - 1] = np.float32(7e-4) * np.where(u[0][:, :, H - 1, H - 1] < 0.5, -1, 1).astype(np.float32)
    out = sm.abi_smooth(native, dev, d, LAM, joint=True)
    assert_clean(out)
    lib = native._load()
    g2, *once = sm.expected_step(lib, d, c["sg_grad"], LAM)
    twice = fc.restatement(once[0], once[1], once[2], g2, fc.library_scalars(lib, fc.LR, fc.BETA1, fc.BETA2, c["t"]))
    last = (slice(None), slice(None), H - 1, H - 1)
    for key, one, two in zip(("x", "m", "v"), once, twice):
        assert not fc.same_bits(one[last], two[last]), key
        assert fc.same_bits(out[key][last], one[last]), key
    assert_step(out, once, name + " random state")
    assert fc.same_bits(out["grad_scenes"], c["ref_grad_scenes"]) and fc.same_bits(out["loss"], c["sg_loss"])


@JOINT
@pytest.mark.parametrize("name", ("b3_13_s2_w", "b1_16_s5_shared_untied", "b5_64_s2_80_workgroups"))
def test_all_zero_lambda_is_the_existing_in_place_step(native, dev, name, joint):
    c = case(native, dev, name)
    twin = (jc.abi_joint if joint else fc.abi_fit)(native, dev, c, bounds=fc.BOUNDS_FIT)
    out = sm.abi_smooth(native, dev, c, np.zeros(12, np.float32), joint=joint, bounds=fc.BOUNDS_FIT)
    assert_clean(out)
    for key in ("x", "m", "v", "loss", "grad") + (("grad_scenes",) if joint else ()):
        assert fc.same_bits(out[key], twin[key]), key


@JOINT
def test_bounds_and_steps_of_adam(native, dev, joint):
    """the bounds clamp x' as in the twins, and t is Adam's: the restatement with bounds at t = 1, 2 and 1000"""
    c = case(native, dev, "b1_13_s5_w")
    lib = native._load()
    for t in (1, 2, 1000):
        out = sm.abi_smooth(native, dev, c, LAM, joint=joint, t=t, bounds=fc.BOUNDS_FIT)
        assert_clean(out)
        g2, *want = sm.expected_step(lib, c, refs(c, joint)[1], LAM, t=t, bounds=fc.BOUNDS_FIT)
        assert fc.same_bits(out["grad"], g2)
        assert_step(out, want, "t = %d" % t)
        assert out["x"][:, 3:].min() >= 0.0 and out["x"][:, 3:].max() <= 1.0


@JOINT
@pytest.mark.parametrize("name", ("b3_13_s2_w", "b1_32_s2_untied"))
def test_pointers_four_bytes_off_alignment(native, dev, name, joint):
    c = case(native, dev, name)
    out = sm.abi_smooth(native, dev, c, LAM, joint=joint, shift=1)
    assert_clean(out)
    g2, *want = sm.expected_step(native._load(), c, refs(c, joint)[1], LAM)
    assert fc.same_bits(out["loss"], refs(c, joint)[0]) and fc.same_bits(out["grad"], g2)
    assert_step(out, want, name + " misaligned")


@JOINT
def test_two_launches_from_the_same_inputs_give_the_same_bits(native, dev, joint):
    c = case(native, dev, "b5_64_s2_80_workgroups")
    a, b = (sm.abi_smooth(native, dev, c, LAM, joint=joint) for _ in range(2))
    for key in ("x", "m", "v", "loss", "grad") + (("grad_scenes",) if joint else ()):
        assert fc.same_bits(a[key], b[key]), key


@JOINT
@pytest.mark.parametrize("lam_there", (True, False), ids=("lambda", "lambda0"))
def test_nan_in_one_map_value(native, dev, joint, lam_there):
    """One NaN map value: that pixel's 36 values are NaN, as in the twins.  Its four neighbours are NaN in that channel only --
    the term of a NaN neighbour is NaN, as torch.sign(nan) --; with lambda = 0 on that channel they are updated normally.
    Everything else is the restatement on the loss entry's gradient of the same maps, bit for bit."""
    c = case(native, dev, "b1_17_s5")
    lib = native._load()
    ch, i, j = 7, 8, 9                                              # a roughness plane, an interior pixel
    lam = LAM.copy()
    assert lam[ch] != 0
    if not lam_there:
        lam[ch] = 0.0
    d = dict(c, maps=c["maps"].copy())
    d["maps"][0, ch, i, j] = np.nan
    if joint:
        ref_loss, ref_grad, _ = jc.abi_scene_grad(native, dev, d)
    else:
        ref_loss, ref_grad = fc.abi_loss(native, dev, d)
    assert np.isnan(ref_loss).all() and np.isnan(ref_grad[0, :, i, j]).all() and np.isnan(ref_grad).sum() == 12
    out = sm.abi_smooth(native, dev, d, lam, joint=joint)
    assert out["launches"] == 1 and out["scratch_zero"] and out["canaries_intact"]
    assert np.isnan(out["loss"]).all()
    around = ((i - 1, j), (i + 1, j), (i, j - 1), (i, j + 1))
    for key in ("x", "m", "v", "grad"):
        assert np.isnan(out[key][0, :, i, j]).all(), key
        for p, q in around:
            assert np.isnan(out[key][0, ch, p, q]) == lam_there, (key, p, q)
        assert np.isnan(out[key]).sum() == 12 + (4 if lam_there else 0), key
    g2, *want = sm.expected_step(lib, d, ref_grad, lam)
    assert fc.same_bits(out["grad"], g2)
    assert_step(out, want, "with a NaN value")


@pytest.mark.parametrize("name", ("b3_13_s2_w", "b1_17_s5"))
def test_photofit_step_is_the_c_abi_and_maps_is_the_users_tensor(native, dev, name):
    """PhotoFit(smooth=).step: one launch, results equal the direct call's, `maps` is the tensor the user gave, updated when
    step returns; the loss returned is the photo term"""
    from svbrdf_estimation_amd import fitting
    c = case(native, dev, name)
    lib = native._load()
    x = torch.from_numpy(c["maps"]).to(dev)
    fit = fitting.PhotoFit(x, lr=fc.LR, betas=(fc.BETA1, fc.BETA2), eps=fc.ADAM_EPS, bounds=fc.BOUNDS_FIT, loss_eps=fc.EPS, smooth=LAM)
    assert fit.uses_fused_kernel()
    fit.exp_avg, fit.exp_avg_sq = torch.from_numpy(c["m"]).to(dev), torch.from_numpy(c["v"]).to(dev)
    fit.state["step"] = c["t"] - 1
    photos, table = torch.from_numpy(c["photos"]).to(dev), torch.from_numpy(c["scenes"]).to(dev)
    weights = None if c["weights"] is None else torch.from_numpy(c["weights"]).to(dev)
    native.xrow(dev, c["H"])
    d = dict(c)
    for k in range(2):
        direct = sm.abi_smooth(native, dev, d, LAM, t=c["t"] + k, bounds=fc.BOUNDS_FIT, want_grad=False)
        before = lib.svbrdf_debug_launch_count()
        loss = fit.step(photos, table, weights)
        assert lib.svbrdf_debug_launch_count() - before == 1 and fit.state["step"] == c["t"] + k
        assert loss.dim() == 0 and not loss.requires_grad
        assert fc.same_bits(loss.cpu().numpy().reshape(1), direct["loss"])
        for got, key in ((fit.maps, "x"), (x, "x"), (fit.exp_avg, "m"), (fit.exp_avg_sq, "v")):
            assert fc.same_bits(got.cpu().numpy(), direct[key]), (k, key)
        d = dict(d, maps=direct["x"], m=direct["m"], v=direct["v"])
    assert fit.maps.data_ptr() == x.data_ptr() and fit._spare.data_ptr() != x.data_ptr()
    photo_checks.assert_scratch_is_zero(native)


def test_steps_are_single_steps_and_an_even_count_needs_no_copy(native, dev):
    """steps(5) and steps(4) equal 5 and 4 single steps -- maps, state, every loss -- in 5 and 4 launches; the result stands in
    the user's tensor either way"""
    from svbrdf_estimation_amd import fitting
    c = case(native, dev, "b3_13_s2_w")
    lib = native._load()
    photos, table, weights = (torch.from_numpy(c[k]).to(dev) for k in ("photos", "scenes", "weights"))

    def fresh():
        x = torch.from_numpy(c["maps"]).to(dev)
        return x, fitting.PhotoFit(x, lr=fc.LR, bounds=fc.BOUNDS_FIT, loss_eps=fc.EPS, smooth=LAM)
    for n in (5, 4):
        (xa, a), (xb, b) = fresh(), fresh()
        before = lib.svbrdf_debug_launch_count()
        several = a.steps(n, photos, table, weights)
        assert lib.svbrdf_debug_launch_count() - before == n and several.shape == (n,) and a.state["step"] == n
        single = torch.stack([b.step(photos, table, weights) for _ in range(n)])
        assert fc.same_bits(several.cpu().numpy(), single.cpu().numpy())
        for key in ("maps", "exp_avg", "exp_avg_sq"):
            assert fc.same_bits(getattr(a, key).cpu().numpy(), getattr(b, key).cpu().numpy()), (n, key)
        assert a.maps.data_ptr() == xa.data_ptr() and fc.same_bits(xa.cpu().numpy(), xb.cpu().numpy())
        assert not fc.same_bits(xa.cpu().numpy(), c["maps"])


def test_joint_path_returns_the_gradients_of_the_step_without_the_prior(native, dev):
    """the prior does not depend on the table or the gains: from the same maps, loss.backward() deposits the same table.grad and
    log_e.grad with and without it, the loss is the same photo term, one launch each -- and the maps differ"""
    from svbrdf_estimation_amd import fitting
    c = case(native, dev, "b3_13_s2_w")
    lib = native._load()
    photos, weights = torch.from_numpy(c["photos"]).to(dev), torch.from_numpy(c["weights"]).to(dev)
    got = []
    for lam in (None, LAM):
        table = torch.from_numpy(c["scenes"]).to(dev).requires_grad_(True)
        log_e = torch.full((c["B"], c["S"], 3), 0.1, device=dev, requires_grad=True)
        fit = fitting.PhotoFit(torch.from_numpy(c["maps"]).to(dev), lr=fc.LR, bounds=fc.BOUNDS_FIT, loss_eps=fc.EPS, smooth=lam)
        before = lib.svbrdf_debug_launch_count()
        loss = fit.step(photos, table, weights, exposure=log_e.exp())
        assert lib.svbrdf_debug_launch_count() - before == 1 and loss.requires_grad
        loss.backward()
        got.append((loss.detach(), table.grad, log_e.grad, fit.maps))
    for a, b in zip(got[0][:3], got[1][:3]):
        assert fc.same_bits(a.cpu().numpy(), b.cpu().numpy())
    assert got[0][1].abs().max() > 0 and not fc.same_bits(got[0][3].cpu().numpy(), got[1][3].cpu().numpy())


def test_hole_fit(native, dev):
    """The experiment of the feature at 32 x 32: S = 5, truth in constant 16 x 16 cells, an 8 x 8 block of zero weights in all
    photos inside one cell, start = truth + jitter, 200 steps, lr 0.01, lambda = 0.01 on d, r, s, bounds BOUNDS_FIT.
      * the fused fit's final photo loss is at most 1.01 x the composed fit's (composed_step with the same prior): the
        project's margin for a fused trajectory against the composed one;
      * the fused fit's error in the hole is strictly below the hole's error without the prior (which is the start's: those
        pixels never move).
    Measured on an MI355X (profiles/r22_photo_fit_smooth.txt): photo loss 0.1799944 fused and 0.1799944 composed (ratio
    1.00000), 0.1826839 without the prior; mean |d,r,s - truth| in the hole 0.07290 at the start and without the prior,
    0.04228 with it (fused and composed alike)."""
    from svbrdf_estimation_amd import fitting, losses, renderers
    H, S, steps, lam = 32, 5, 200, [0.0, 0.01, 0.01, 0.01]
    truth, start, weights, mask = sm.hole_problem(H, 16, (4, 12), S)
    table = torch.from_numpy(photo_checks.scene_table(1, 77, 2, 3)).to(dev)
    tt, w = torch.from_numpy(truth).to(dev), torch.from_numpy(weights).to(dev)
    photos = native.render_fwd(tt, table).clamp_(0.0, 1.0)
    fn = losses.PhotoLoss(renderers.LocalRenderer())
    ends = {}
    for name, smooth in (("plain", None), ("fused", lam)):
        fit = fitting.PhotoFit(torch.from_numpy(start.copy()).to(dev), lr=0.01, bounds=fc.BOUNDS_FIT, smooth=smooth)
        assert fit.uses_fused_kernel()
        fit.steps(steps, photos, table, w)
        ends[name] = (fn(fit.maps, photos, table, w).item(),) + sm.hole_errors(fit.maps.cpu().numpy(), truth, mask)
        if smooth is None:
            assert fc.same_bits(fit.maps.cpu().numpy()[..., mask], start[..., mask])
    x, m, v = torch.from_numpy(start.copy()).to(dev), torch.zeros(start.shape, device=dev), torch.zeros(start.shape, device=dev)
    for t in range(1, steps + 1):
        fitting.composed_step(x, m, v, t, photos, table, w, lr=0.01, bounds=fc.BOUNDS_FIT, smooth=lam)
    ends["composed"] = (fn(x, photos, table, w).item(),) + sm.hole_errors(x.cpu().numpy(), truth, mask)
    at_start = sm.hole_errors(start, truth, mask)
    print("[smooth] hole fit at 32 x 32, S = 5, 200 steps, (photo loss, mean |d,r,s - truth| in the hole, on seen pixels): "
          "start (-, %.5f, %.5f); fused without the prior (%.7f, %.5f, %.5f); fused with lambda 0.01 (%.7f, %.5f, %.5f); "
          "composed with lambda 0.01 (%.7f, %.5f, %.5f); loss ratio fused / composed %.5f" % (
              at_start + ends["plain"] + ends["fused"] + ends["composed"] + (ends["fused"][0] / ends["composed"][0],)))
    assert ends["plain"][1] == at_start[0]
    assert ends["fused"][0] <= 1.01 * ends["composed"][0], (ends["fused"][0], ends["composed"][0])
    assert ends["fused"][1] < ends["plain"][1], (ends["fused"][1], ends["plain"][1])


def test_smooth_step_speed(native, dev):
    """At the configuration-2 shape (B = 8, 256 x 256, S = 9, per-photo weights, rotating sets), one process, the legs
    alternating:
      * the smooth step through the C ABI, ping-ponging two buffers, takes at most 156 / 108 of the plain fused step: every one
        of the 48 neighbour words from HBM on top of the step's 72 + 3 S + P;
      * and at most the faster composed form (PhotoLoss forward + backward, fitting.smoothness backward, torch.optim.Adam
        stock / fused=True, clamp_); no margin: the project's rule for every fused entry.
    PhotoFit.step (launch + copy) and steps(16) (no copy) are recorded, not asserted.  Measured on an MI355X
    (profiles/r22_photo_fit_smooth.txt): smooth step 74.78 us, plain fused step 61.62 us (ratio 1.214 against the bound
    1.444), composed 680.17 us (stock Adam) / 639.43 us (fused=True); PhotoFit.step with its copy 86.44 us, steps(16)
    61.28 us per step."""
    r = sm.measure_smooth_fit(dev, native)
    print("[smooth] smooth step (C ABI, two buffers) %.2f us; plain fused step %.2f us (ratio %.3f, bound %.3f); "
          "PhotoFit.step with its copy %.2f us; steps(16) %.2f us per step; composed %.2f us (stock Adam), %.2f us (fused=True); "
          "smooth / faster composed %.3f; rounds %s" % (
              r["smooth_us"], r["plain_us"], r["smooth_over_plain"], r["bound"], r["photofit_us"], r["steps16_us"],
              r["composed_us"], r["composed_fused_us"], r["smooth_over_composed"], r["rounds"]))
    assert r["smooth_us"] <= r["bound"] * r["plain_us"], r
    assert r["smooth_us"] <= min(r["composed_us"], r["composed_fused_us"]), r
