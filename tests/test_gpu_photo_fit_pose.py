"""One step of a photo fit WITH the scene table's gradient in one launch, on the device (csrc/svbrdf_photo_fit_pose.hip:
k_joint_fit*; svbrdf_photo_fit_adam_step_scene_grad; fitting.PhotoFit.step with a table or an exposure that requires grad).
The loss, the map gradient and the table's gradient are bit for bit those of svbrdf_photo_loss_scene_grad_fwd_bwd, which g23
pins to the reference (the loss and map gradient through g18 / g21); the update is bit for bit the numpy float32 restatement
of tests/photo_fit_checks.py (held against float64 Adam in tests/test_photo_fit_cpu.py) fed with that gradient and the
library's exported scalars.  Every comparison here is BIT FOR BIT unless it says otherwise.

Measured on an MI355X (profiles/r20_photo_fit_pose.txt): the end points of the 40-step joint fits and the four times of the
speed test are printed by the tests and recorded there.
"""
import numpy as np
import pytest
import torch

import photo_checks
import photo_fit_checks as fc
import photo_fit_pose_checks as jc
import synth

pytestmark = pytest.mark.gpu
NAMES = [c[0] for c in fc.CASES]


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
    """the inputs of a case and the scene-gradient entry's loss and two gradients on them, computed once and shared"""
    if name not in _CASES:
        c = fc.case_inputs(native, dev, name)
        c["ref_loss"], c["ref_grad"], c["ref_grad_scenes"] = jc.abi_scene_grad(native, dev, c)
        _CASES[name] = c
    return _CASES[name]


def assert_step(out, want, what):
    for key, exp in zip(("x", "m", "v"), want):
        assert fc.same_bits(out[key], exp), "%s: %s differs from the restatement in %d values" % (
            what, key, fc.count_differing(out[key], exp))


def assert_clean(out):
    assert out["launches"] == 1 and out["scratch_zero"] and out["canaries_intact"] and out["inputs_intact"]


@pytest.mark.parametrize("name", NAMES)
def test_step_is_the_scene_gradient_entry_and_the_restatement_bit_for_bit(native, dev, name):
    """loss_out, grad_out and grad_scenes are the scene-gradient entry's; maps', exp_avg', exp_avg_sq' are the
    restatement's on that gradient; grad_out = NULL gives the same; inputs and canaries untouched; one launch; scratch left
    zeroed"""
    c = case(native, dev, name)
    lib = native._load()
    out = jc.abi_joint(native, dev, c)
    assert_clean(out)
    assert fc.same_bits(out["loss"], c["ref_loss"]) and np.isfinite(out["loss"]).all(), (out["loss"], c["ref_loss"])
    assert fc.same_bits(out["grad"], c["ref_grad"]), fc.count_differing(out["grad"], c["ref_grad"])
    assert fc.same_bits(out["grad_scenes"], c["ref_grad_scenes"]) and np.isfinite(out["grad_scenes"]).all()
    assert np.abs(out["grad_scenes"]).max() > 0
    want = fc.expected_step(lib, c, c["ref_grad"])
    assert_step(out, want, name)
    assert not fc.same_bits(out["x"], c["maps"])                    # and the maps did move
    quiet = jc.abi_joint(native, dev, c, want_grad=False)
    assert_clean(quiet)
    assert fc.same_bits(quiet["loss"], c["ref_loss"]) and fc.same_bits(quiet["grad_scenes"], c["ref_grad_scenes"])
    assert_step(quiet, want, name + " without grad_out")


@pytest.mark.parametrize("name", jc.PARTIAL_WAVE_CASES)
def test_last_pixel_of_a_partial_wave_is_updated_exactly_once(native, dev, name):
    """A wave that holds a pixel runs whole: its lanes past the item's last pixel shade that LAST pixel again with 1/N = 0.
    Were the update not confined to the lanes that own a pixel, several lanes would apply the momentum update to it.  The
    state is random with m != 0 there, so a second update cannot equal a single one: beta1 (beta1 m + c1 g) + c1 g differs
    from beta1 m + c1 g, and x' moves twice.  (Lanes of one wave that raced instead -- all loading the state before any
    stores it -- would leave an update made with THEIR gradient, +-0, which differs from the restatement's on the real
    gradient as well.)"""
    c = case(native, dev, name)
    H = c["H"]
    assert (H * H) % 64 != 0
    d = dict(c)
    u = synth.uniform01(7400 + NAMES.index(name), (2,) + c["maps"].shape)
    d["m"] = ((u[0] - np.float32(0.5)) * np.float32(2e-3)).astype(np.float32)
    d["v"] = (u[1] * np.float32(1e-5) + np.float32(1e-7)).astype(np.float32)
    d["m"][:, :, H - 1, H - 1] = np.float32(7e-4) * np.where(u[0][:, :, H - 1, H - 1] < 0.5, -1, 1).astype(np.float32)
    out = jc.abi_joint(native, dev, d)
    assert_clean(out)
    once = fc.expected_step(native._load(), d, c["ref_grad"])
    twice = fc.restatement(once[0], once[1], once[2], c["ref_grad"], fc.library_scalars(native._load(), fc.LR, fc.BETA1, fc.BETA2, c["t"]))
    for key, one, two in zip(("x", "m", "v"), once, twice):
        last = (slice(None), slice(None), H - 1, H - 1)
        assert not fc.same_bits(one[last], two[last]), key          # the check can tell one update from two
        assert fc.same_bits(out[key][last], one[last]), (key, out[key][last], one[last], two[last])
    assert_step(out, once, name + " random state")
    assert fc.same_bits(out["grad_scenes"], c["ref_grad_scenes"]) and fc.same_bits(out["loss"], c["ref_loss"])


def test_bounds(native, dev):
    """active at both ends, lo == hi, +-inf bounds = no bounds bit for bit; the table's gradient does not see them"""
    c = case(native, dev, "b3_13_s2_w")
    lib = native._load()
    free = jc.abi_joint(native, dev, c)
    inf = jc.abi_joint(native, dev, c, bounds=np.array([[-np.inf, np.inf]] * 12, np.float32))
    for key in ("x", "m", "v", "loss", "grad", "grad_scenes"):
        assert fc.same_bits(free[key], inf[key]), key
    # a band inside the range the updated maps cover: both ends bind in every channel
    lo, hi = np.quantile(free["x"], 0.3, axis=(0, 2, 3)), np.quantile(free["x"], 0.7, axis=(0, 2, 3))
    band = np.stack((lo, hi), axis=1).astype(np.float32)
    band[4] = (0.5, 0.5)                                             # lo == hi: the channel is pinned
    got = jc.abi_joint(native, dev, c, bounds=band)
    assert_clean(got)
    assert_step(got, fc.expected_step(lib, c, c["ref_grad"], bounds=band), "band")
    for ch in range(12):
        assert (got["x"][:, ch] == band[ch, 0]).any() and (got["x"][:, ch] == band[ch, 1]).any(), ch
        assert (got["x"][:, ch] >= band[ch, 0]).all() and (got["x"][:, ch] <= band[ch, 1]).all(), ch
    assert (got["x"][:, 4] == 0.5).all()
    assert fc.same_bits(got["m"], free["m"]) and fc.same_bits(got["v"], free["v"]) and fc.same_bits(got["grad"], free["grad"])
    assert fc.same_bits(got["grad_scenes"], c["ref_grad_scenes"]) and fc.same_bits(got["loss"], c["ref_loss"])


@pytest.mark.parametrize("name", ("b3_13_s2_w", "b1_17_s5"))
def test_nan_in_one_pixel(native, dev, name):
    """the loss and all of grad_scenes are NaN, that pixel's 36 values are NaN, every other pixel is the restatement bit for
    bit, and the scratch is left zeroed: a following clean call on the same scratch is correct"""
    c = case(native, dev, name)
    lib = native._load()
    d = dict(c)
    d["maps"] = c["maps"].copy()
    b, i, j = c["B"] - 1, 5, 3
    if c["weights"] is not None:                                    # a pixel that votes: a zero weight selects its terms away
        i, j = (int(k[0]) for k in np.nonzero(c["weights"][b].min(axis=0) > 0))
    d["maps"][b, 1, i, j] = np.nan                                  # a normal component
    ref_loss, ref_grad, ref_gs = jc.abi_scene_grad(native, dev, d)
    assert np.isnan(ref_loss).all() and np.isnan(ref_grad[b, :, i, j]).all() and np.isnan(ref_gs).all()
    ws = jc.scratch(lib, dev, c)
    out = jc.abi_joint(native, dev, d, ws=ws)
    assert_clean(out)
    assert np.isnan(out["loss"]).all() and np.isnan(out["grad_scenes"]).all()
    for key in ("x", "m", "v"):
        assert np.isnan(out[key][b, :, i, j]).all(), key
        assert np.isnan(out[key]).sum() == 12, key
    assert fc.same_bits(out["grad"], ref_grad)
    assert_step(out, fc.expected_step(lib, d, ref_grad), name + " with a NaN pixel")
    clean = jc.abi_joint(native, dev, c, ws=ws)
    assert_clean(clean)
    assert fc.same_bits(clean["loss"], c["ref_loss"]) and fc.same_bits(clean["grad_scenes"], c["ref_grad_scenes"])
    assert_step(clean, fc.expected_step(lib, c, c["ref_grad"]), name + " behind a NaN call")


@pytest.mark.parametrize("name", ("b3_13_s2_w", "b1_17_s5"))
def test_a_colour_of_zero_in_one_scene_row(native, dev, name):
    """the loss is NaN and grad_scenes is all NaN -- and the maps are updated all the same, per the restatement on the
    scene-gradient entry's grad_input: the thread that owns a pixel cannot know the launch's loss"""
    c = case(native, dev, name)
    d = dict(c)
    d["scenes"] = c["scenes"].copy()
    d["scenes"][c["B"] - 1, c["S"] - 1, 7] = 0.0
    ref_loss, ref_grad, ref_gs = jc.abi_scene_grad(native, dev, d)
    assert np.isnan(ref_loss).all() and np.isnan(ref_gs).all()
    out = jc.abi_joint(native, dev, d)
    assert_clean(out)
    assert np.isnan(out["loss"]).all() and np.isnan(out["grad_scenes"]).all() and out["grad_scenes"].shape == c["scenes"].shape
    assert fc.same_bits(out["grad"], ref_grad)
    assert_step(out, fc.expected_step(native._load(), d, ref_grad), name + " with a colour of 0")
    assert not fc.same_bits(out["x"], c["maps"])


@pytest.mark.parametrize("name", ("b3_13_s2_w", "b1_32_s2_untied"))
def test_pointers_four_bytes_off_alignment(native, dev, name):
    c = case(native, dev, name)
    out = jc.abi_joint(native, dev, c, shift=1)
    assert_clean(out)
    assert fc.same_bits(out["loss"], c["ref_loss"]) and fc.same_bits(out["grad"], c["ref_grad"])
    assert fc.same_bits(out["grad_scenes"], c["ref_grad_scenes"])
    assert_step(out, fc.expected_step(native._load(), c, c["ref_grad"]), name + " misaligned")


@pytest.mark.parametrize("name", ("b3_13_s2_w", "b1_16_s5_shared_untied", "b1_17_s5"))
def test_photofit_step_with_a_table_leaf_and_gains_is_the_c_abi(native, dev, name, monkeypatch):
    """PhotoFit.step(photos, table leaf, weights, exposure=log_e.exp()) over two steps: maps and state equal the direct call
    on the pre-multiplied table, table.grad equals its grad_scenes, log_e.grad is the chain rule of grad_scenes[..., 6:]
    through the multiply and exp in torch ops; one launch per step by the library's counter, no upload of the device table,
    the maps updated in place.  The same call under no_grad takes the entry without a table gradient and returns its bits."""
    from svbrdf_estimation_amd import fitting
    c = case(native, dev, name)
    lib = native._load()
    x = torch.from_numpy(c["maps"]).to(dev)
    fit = fitting.PhotoFit(x, lr=fc.LR, betas=(fc.BETA1, fc.BETA2), eps=fc.ADAM_EPS, bounds=fc.BOUNDS_FIT, loss_eps=fc.EPS)
    assert fit.uses_fused_kernel()
    fit.exp_avg, fit.exp_avg_sq = torch.from_numpy(c["m"]).to(dev), torch.from_numpy(c["v"]).to(dev)
    fit.state["step"] = c["t"] - 1
    photos = torch.from_numpy(c["photos"]).to(dev)
    table = torch.from_numpy(c["scenes"]).to(dev).requires_grad_(True)
    gains = 0.4 * (synth.uniform01(7500 + NAMES.index(name), (c["B"], c["S"], 3)) - np.float32(0.5))
    log_e = torch.from_numpy(gains.astype(np.float32)).to(dev).requires_grad_(True)
    weights = None if c["weights"] is None else torch.from_numpy(c["weights"]).to(dev)
    native.xrow(dev, c["H"])                                         # (cached once per width: not part of a step)
    torch.cuda.synchronize(dev)

    def no_upload(*a, **k):
        raise AssertionError("a device table must not be uploaded")
    monkeypatch.setattr(native, "upload_scene_table", no_upload)
    with torch.no_grad():
        scaled = torch.cat((table[..., :6], table[..., 6:] * log_e.exp()), dim=-1).cpu().numpy()
    d = dict(c, scenes=scaled)
    for k in range(2):
        direct = jc.abi_joint(native, dev, d, t=c["t"] + k, bounds=fc.BOUNDS_FIT, want_grad=False)
        table.grad, log_e.grad = None, None
        before = lib.svbrdf_debug_launch_count()
        loss = fit.step(photos, table, weights, exposure=log_e.exp())
        assert lib.svbrdf_debug_launch_count() - before == 1 and fit.state["step"] == c["t"] + k
        assert loss.dim() == 0 and loss.is_cuda and loss.requires_grad
        assert fc.same_bits(loss.detach().cpu().numpy().reshape(1), direct["loss"])
        for got, key in ((fit.maps, "x"), (fit.exp_avg, "m"), (fit.exp_avg_sq, "v")):
            assert fc.same_bits(got.cpu().numpy(), direct[key]), (k, key)      # updated when step returns
        before = lib.svbrdf_debug_launch_count()
        loss.backward()
        assert lib.svbrdf_debug_launch_count() == before             # backward is torch ops on [B,S,9]
        gs = torch.from_numpy(direct["grad_scenes"]).to(dev)
        with torch.no_grad():
            # d/d table: positions as they are, colours times the gain; d/d log e: colour-gradient x colour x gain
            want_table = torch.cat((gs[..., :6], gs[..., 6:] * log_e.exp()), dim=-1)
            want_log_e = (gs[..., 6:] * table[..., 6:]) * log_e.exp()
        assert fc.same_bits(table.grad.cpu().numpy(), want_table.cpu().numpy())
        assert fc.same_bits(log_e.grad.cpu().numpy(), want_log_e.cpu().numpy())
        assert fit.maps.grad is None
        d = dict(d, maps=direct["x"], m=direct["m"], v=direct["v"])
    assert fit.maps.data_ptr() == x.data_ptr()                       # in place
    # a table leaf alone, no gains: table.grad IS grad_scenes
    plain = jc.abi_joint(native, dev, dict(d, scenes=c["scenes"]), t=c["t"] + 2, bounds=fc.BOUNDS_FIT, want_grad=False)
    table.grad = None
    fit.step(photos, table, weights).backward()
    assert fc.same_bits(table.grad.cpu().numpy(), plain["grad_scenes"]) and fc.same_bits(fit.maps.cpu().numpy(), plain["x"])
    # under no_grad: the entry without a table gradient, its bits, a loss that does not require grad
    d = dict(d, maps=plain["x"], m=plain["m"], v=plain["v"])
    old = fc.abi_fit(native, dev, d, t=c["t"] + 3, bounds=fc.BOUNDS_FIT, want_grad=False)
    calls = []
    real = native.photo_fit_adam_step
    monkeypatch.setattr(native, "photo_fit_adam_step", lambda *a, **k: (calls.append(k.get("want_scene_grad", False)), real(*a, **k))[1])
    with torch.no_grad():
        before = lib.svbrdf_debug_launch_count()
        loss = fit.step(photos, table, weights, exposure=log_e.exp())
        assert lib.svbrdf_debug_launch_count() - before == 1
    assert calls == [False] and not loss.requires_grad and fc.same_bits(loss.cpu().numpy().reshape(1), old["loss"])
    for got, key in ((fit.maps, "x"), (fit.exp_avg, "m"), (fit.exp_avg_sq, "v")):
        assert fc.same_bits(got.cpu().numpy(), old[key]), key
    photo_checks.assert_scratch_is_zero(native)


def test_steps_take_the_gains_as_constants_and_composed_step_is_the_same_gradient(native, dev):
    """PhotoFit.steps(2, ..., exposure=) is two step() calls under no_grad bit for bit, and its losses never require grad;
    composed_step on the device with a table leaf -- PhotoLoss's scene-gradient launch, then torch ops -- returns the fused
    joint step's loss and table.grad bit for bit (the same kernel arithmetic) and maps within the rounding of the update"""
    from svbrdf_estimation_amd import fitting
    c = case(native, dev, "b3_13_s2_w")
    photos, weights = torch.from_numpy(c["photos"]).to(dev), torch.from_numpy(c["weights"]).to(dev)
    table = torch.from_numpy(c["scenes"]).to(dev).requires_grad_(True)
    log_e = torch.full((c["B"], c["S"], 1), 0.1, device=dev, requires_grad=True)

    def fresh():
        return fitting.PhotoFit(torch.from_numpy(c["maps"]).to(dev), lr=fc.LR, bounds=fc.BOUNDS_FIT, loss_eps=fc.EPS)
    a, b = fresh(), fresh()
    several = a.steps(2, photos, table, weights, exposure=log_e.exp())
    with torch.no_grad():
        single = torch.stack([b.step(photos, table, weights, exposure=log_e.exp()) for _ in range(2)])
    assert not several.requires_grad and fc.same_bits(several.cpu().numpy(), single.cpu().numpy())
    for key in ("maps", "exp_avg", "exp_avg_sq"):
        assert fc.same_bits(getattr(a, key).cpu().numpy(), getattr(b, key).cpu().numpy()), key
    assert a.state["step"] == b.state["step"] == 2 and table.grad is None and log_e.grad is None
    fused, spec = fresh(), fresh()
    fused.step(photos, table, weights, exposure=log_e.exp()).backward()
    got = table.grad.clone(), log_e.grad.clone()
    table.grad, log_e.grad = None, None
    loss = fitting.composed_step(spec.maps, spec.exp_avg, spec.exp_avg_sq, 1, photos, table, weights, lr=fc.LR, bounds=fc.BOUNDS_FIT,
                                 loss_eps=fc.EPS, exposure=log_e.exp())
    assert loss.requires_grad
    loss.backward()
    assert fc.same_bits(table.grad.cpu().numpy(), got[0].cpu().numpy()) and fc.same_bits(log_e.grad.cpu().numpy(), got[1].cpu().numpy())
    # the bound of test_composed_step_in_float32_is_the_restatement, 2^-20 |update| + 2^-23 |x'| (a square root within one
    # ulp and the four roundings behind it).  At t = 1 from a zero state |update| = lr |g| / (|g| + eps) < lr in real
    # arithmetic; 1.01 lr covers its float32 roundings
    err = (fused.maps - spec.maps).abs()
    assert (err <= 2.0 ** -20 * 1.01 * fc.LR + 2.0 ** -23 * fused.maps.abs()).all(), err.max().item()


def test_forty_step_joint_fit_against_the_unfused_trajectory(native, dev):
    """tools/fit_photos.py --fit-pose's start at 32 x 32, B = 2, S = 5, positions up to 3 % off, --pose-lr 0.002: 40 fused
    joint steps with Adam on the positions against the unfused loop (PhotoLoss, one Adam with two groups, clamp_) from the
    same start.  The two differ only by the rounding of the map update (torch forms m' with lerp and x' with addcdiv);
    grad_scenes is the same kernel arithmetic in both.  Conditions: the unfused end loss is below its start, the mean
    position error is below its start in both runs, and the fused end loss is at most 1.01 x the unfused one -- the margin
    of test_forty_step_fit_against_the_unfused_trajectory for the same mechanism (its measured ratio: 0.99995).  Measured
    on an MI355X (profiles/r20_photo_fit_pose.txt): start 0.1556223 / 0.012656, unfused end 0.0162110 / 0.011079, fused end
    0.0162021 / 0.011083 (loss ratio 0.99945)."""
    from svbrdf_estimation_amd import fitting, losses, renderers, synthesis
    B, H, S, steps, seed, lr, pose_lr = 2, 32, 5, 40, 1, 0.01, 0.002
    truth = torch.from_numpy(synth.make_maps(seed, B, H)).to(dev)
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)
    photos = synthesis.render_inputs(truth, S, use_augmentation=True, noise=None)
    torch.manual_seed(seed)
    table = torch.stack([synthesis.input_scene_table(S, True) for _ in range(B)], dim=0).to(dev)
    true_pos, colour = table[..., :6], table[..., 6:]
    off = 1.0 + 0.06 * (torch.from_numpy(synth.uniform01(seed + 3000, (B, S, 6))).to(dev) - 0.5)
    start = truth.clone()
    jitter = torch.from_numpy(synth.uniform01(seed + 1000, (B, 9, H, H))).to(dev) - 0.5
    start[:, 3:] = (start[:, 3:] + 0.3 * jitter).clamp_(0.02, 0.98)
    fn = losses.PhotoLoss(renderers.LocalRenderer())
    pos_error = lambda p: (p.detach() - true_pos).abs().mean().item()
    # the unfused loop
    x = start.clone().requires_grad_(True)
    pos = (true_pos * off).requires_grad_(True)
    start_error = pos_error(pos)
    opt = torch.optim.Adam([{"params": [x]}, {"params": [pos], "lr": pose_lr}], lr=lr)
    first = None
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        loss = fn(x, photos, torch.cat((pos, colour), dim=-1))
        first = loss.item() if first is None else first
        loss.backward()
        opt.step()
        with torch.no_grad():
            x[:, 3:].clamp_(0.0, 1.0)
    # the fused joint step, Adam on the positions alone
    fit = fitting.PhotoFit(start.clone(), lr=lr, bounds=fc.BOUNDS_FIT)
    fpos = (true_pos * off).requires_grad_(True)
    popt = torch.optim.Adam([fpos], lr=pose_lr)
    fused_first = None
    for _ in range(steps):
        popt.zero_grad(set_to_none=True)
        loss = fit.step(photos, torch.cat((fpos, colour), dim=-1))
        fused_first = loss.item() if fused_first is None else fused_first
        loss.backward()
        popt.step()
    with torch.no_grad():
        unfused_end = fn(x, photos, torch.cat((pos, colour), dim=-1)).item()
        fused_end = fn(fit.maps, photos, torch.cat((fpos, colour), dim=-1)).item()
    print("[joint] 40 joint steps at 32 x 32, B = 2, S = 5: start loss %.7f, mean |position - truth| %.6f; unfused end %.7f, "
          "position error %.6f; fused end %.7f, position error %.6f (loss ratio %.5f); max |maps fused - unfused| %.3g" % (
              first, start_error, unfused_end, pos_error(pos), fused_end, pos_error(fpos), fused_end / unfused_end,
              (fit.maps - x.detach()).abs().max().item()))
    assert fused_first == first and fit.state["step"] == steps
    assert unfused_end < first                                       # the fit does fit
    assert pos_error(pos) < start_error and pos_error(fpos) < start_error
    assert fused_end <= 1.01 * unfused_end, (fused_end, unfused_end)


def test_joint_step_speed(native, dev):
    """At the configuration-2 shape (B = 8, 256 x 256, S = 9, per-photo weights), one process, the legs alternating: the
    joint fused step through PhotoFit.step with a table leaf -- its backward() and the small Adam on the table included --
    takes at most the composed step (PhotoLoss with the table leaf forward + backward, Adam over maps and table, clamp_)
    with the faster of the stock default and fused=True; no margin: the project's rule for every fused entry.  The ratio to
    the scene-gradient loss launch alone is recorded, not asserted: nothing derives it.  Measured on an MI355X
    (profiles/r20_photo_fit_pose.txt): joint 113.08 us, scene-gradient launch 71.72 us (ratio 1.577), composed 246.48 us
    (stock Adam) / 155.02 us (fused=True); the joint launch alone, a direct call: 94.2 us."""
    r = jc.measure_joint_fit(dev, native)
    print("[joint] joint fused step %.2f us (step + backward + Adam on the table); scene-gradient loss launch %.2f us (ratio "
          "%.3f); composed step %.2f us (stock Adam), %.2f us (fused=True); joint / faster composed %.3f; rounds %s" % (
              r["joint_us"], r["scene_grad_us"], r["joint_over_scene_grad"], r["composed_us"], r["composed_fused_us"],
              r["joint_over_composed"], r["rounds"]))
    assert r["joint_us"] <= min(r["composed_us"], r["composed_fused_us"]), r
