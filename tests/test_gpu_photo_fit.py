"""One step of a photo fit in one launch, on the device (csrc/svbrdf_photo_fit.hip: k_fit_maps*; svbrdf_photo_fit_adam_step;
fitting.PhotoFit).  The gradient is bit for bit that of svbrdf_photo_loss[_weighted]_fwd_bwd, which g18 / g21 pin to the
reference; what is new is Adam's arithmetic, and its oracle is the numpy float32 restatement of tests/photo_fit_checks.py
(held against float64 Adam in tests/test_photo_fit_cpu.py) fed with that gradient and the library's exported scalars: every
comparison of maps and state here is BIT FOR BIT.

Measured on an MI355X (profiles/r18_photo_fit.txt): the end points of the 40-step trajectories and the four times of the
speed test are printed by the tests and recorded there.
"""
import ctypes

import numpy as np
import pytest
import torch

import photo_checks
import photo_fit_checks as fc
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
    """the inputs of a case and the loss entry's loss and gradient on them, computed once and shared"""
    if name not in _CASES:
        c = fc.case_inputs(native, dev, name)
        c["ref_loss"], c["ref_grad"] = fc.abi_loss(native, dev, c)
        _CASES[name] = c
    return _CASES[name]


def assert_step(out, want, what):
    for key, exp in zip(("x", "m", "v"), want):
        assert fc.same_bits(out[key], exp), "%s: %s differs from the restatement in %d values" % (
            what, key, fc.count_differing(out[key], exp))


@pytest.mark.parametrize("name", NAMES)
def test_step_is_the_loss_entry_and_the_restatement_bit_for_bit(native, dev, name):
    """loss_out and grad_out are the loss entry's; maps', exp_avg', exp_avg_sq' are the restatement's on that gradient;
    grad_out = NULL gives the same; inputs and canaries untouched; one launch; scratch left zeroed"""
    c = case(native, dev, name)
    lib = native._load()
    out = fc.abi_fit(native, dev, c)
    assert out["launches"] == 1 and out["scratch_zero"] and out["canaries_intact"] and out["inputs_intact"]
    assert fc.same_bits(out["loss"], c["ref_loss"]) and np.isfinite(out["loss"]).all(), (out["loss"], c["ref_loss"])
    assert fc.same_bits(out["grad"], c["ref_grad"]), fc.count_differing(out["grad"], c["ref_grad"])
    want = fc.expected_step(lib, c, c["ref_grad"])
    assert_step(out, want, name)
    assert not fc.same_bits(out["x"], c["maps"])                    # and the maps did move
    quiet = fc.abi_fit(native, dev, c, want_grad=False)
    assert quiet["launches"] == 1 and quiet["scratch_zero"] and quiet["canaries_intact"] and quiet["inputs_intact"]
    assert fc.same_bits(quiet["loss"], c["ref_loss"])
    assert_step(quiet, want, name + " without grad_out")


def test_bounds(native, dev):
    """active at both ends, lo == hi, +-inf bounds = no bounds bit for bit, a NaN x' stays NaN under finite bounds"""
    c = case(native, dev, "b3_13_s2_w")
    lib = native._load()
    free = fc.abi_fit(native, dev, c)
    inf = fc.abi_fit(native, dev, c, bounds=np.array([[-np.inf, np.inf]] * 12, np.float32))
    for key in ("x", "m", "v", "loss", "grad"):
        assert fc.same_bits(free[key], inf[key]), key
    # a band inside the range the updated maps cover: both ends bind in every channel
    lo, hi = np.quantile(free["x"], 0.3, axis=(0, 2, 3)), np.quantile(free["x"], 0.7, axis=(0, 2, 3))
    band = np.stack((lo, hi), axis=1).astype(np.float32)
    band[4] = (0.5, 0.5)                                             # lo == hi: the channel is pinned
    got = fc.abi_fit(native, dev, c, bounds=band)
    assert_step(got, fc.expected_step(lib, c, c["ref_grad"], bounds=band), "band")
    for ch in range(12):
        assert (got["x"][:, ch] == band[ch, 0]).any() and (got["x"][:, ch] == band[ch, 1]).any(), ch
        assert (got["x"][:, ch] >= band[ch, 0]).all() and (got["x"][:, ch] <= band[ch, 1]).all(), ch
    assert (got["x"][:, 4] == 0.5).all()
    assert fc.same_bits(got["m"], free["m"]) and fc.same_bits(got["v"], free["v"]) and fc.same_bits(got["grad"], free["grad"])
    # a NaN in the state makes x' NaN without touching the loss: it stays NaN under finite bounds
    d = dict(c)
    d["m"] = c["m"].copy()
    d["m"][1, 7, 3, 5] = np.nan
    nan = fc.abi_fit(native, dev, d, bounds=np.array([[0.0, 1.0]] * 12, np.float32))
    assert np.isnan(nan["x"][1, 7, 3, 5]) and np.isnan(nan["m"][1, 7, 3, 5]) and np.isnan(nan["x"]).sum() == 1
    assert fc.same_bits(nan["loss"], c["ref_loss"])
    assert_step(nan, fc.expected_step(lib, d, c["ref_grad"], bounds=np.array([[0.0, 1.0]] * 12, np.float32)), "NaN state")


@pytest.mark.parametrize("name", ("b3_13_s2_w", "b1_17_s5"))
def test_nan_in_one_pixel(native, dev, name):
    """the loss is NaN, that pixel's 36 values are NaN, every other pixel is the restatement bit for bit, and the scratch is
    left zeroed: a following clean call on the same scratch is correct"""
    c = case(native, dev, name)
    lib = native._load()
    d = dict(c)
    d["maps"] = c["maps"].copy()
    b, i, j = c["B"] - 1, 5, 3
    if c["weights"] is not None:                                    # a pixel that votes: a zero weight selects its terms away
        i, j = (int(k[0]) for k in np.nonzero(c["weights"][b].min(axis=0) > 0))
    d["maps"][b, 1, i, j] = np.nan                                  # a normal component
    ref_loss, ref_grad = fc.abi_loss(native, dev, d)
    assert np.isnan(ref_loss).all() and np.isnan(ref_grad[b, :, i, j]).all()
    ws = torch.zeros(65, dtype=torch.int64, device=dev)
    out = fc.abi_fit(native, dev, d, ws=ws)
    assert np.isnan(out["loss"]).all() and out["scratch_zero"] and out["canaries_intact"] and out["inputs_intact"]
    for key in ("x", "m", "v"):
        assert np.isnan(out[key][b, :, i, j]).all(), key
        assert np.isnan(out[key]).sum() == 12, key
    assert fc.same_bits(out["grad"], ref_grad)
    assert_step(out, fc.expected_step(lib, d, ref_grad), name + " with a NaN pixel")
    clean = fc.abi_fit(native, dev, c, ws=ws)
    assert fc.same_bits(clean["loss"], c["ref_loss"]) and clean["scratch_zero"]
    assert_step(clean, fc.expected_step(lib, c, c["ref_grad"]), name + " behind a NaN call")


def test_pixels_with_all_zero_weights_move_by_their_momentum(native, dev):
    """the weight field masks the top quarter of the rows in every plane: g = +-0 there, and the maps still move by m"""
    c = case(native, dev, "b3_13_s2_w")
    rows = max(c["H"] // 4, 1)
    assert not c["weights"][:, :, :rows].any() and not c["ref_grad"][:, :, :rows].any()
    out = fc.abi_fit(native, dev, c)
    want = fc.expected_step(native._load(), c, c["ref_grad"])
    assert_step(out, want, "zero weights")
    moved = out["x"][:, :, :rows] != c["maps"][:, :, :rows]
    # m != 0: the update step_size 0.9 m / den is above half an ulp of x unless |m| < ~1e-7 (den <= 0.06 here, step_size
    # 0.053): m is uniform in +-1e-3, so all but a fraction of 1e-4 move
    assert moved[c["m"][:, :, :rows] != 0].mean() > 0.99
    assert not moved[c["m"][:, :, :rows] == 0].any()                # m = 0 and g = 0: exactly no move


@pytest.mark.parametrize("name", ("b3_13_s2_w", "b1_32_s2_untied"))
def test_pointers_four_bytes_off_alignment(native, dev, name):
    c = case(native, dev, name)
    out = fc.abi_fit(native, dev, c, shift=1)
    assert out["canaries_intact"] and out["inputs_intact"] and out["scratch_zero"]
    assert fc.same_bits(out["loss"], c["ref_loss"]) and fc.same_bits(out["grad"], c["ref_grad"])
    assert_step(out, fc.expected_step(native._load(), c, c["ref_grad"]), name + " misaligned")


def test_error_codes_launch_nothing_and_touch_no_device_buffer(native, dev):
    c = case(native, dev, "b1_7_s1")
    lib = native._load()
    fn = getattr(lib, fc.STEP_ENTRY)
    B, S, H = c["B"], c["S"], c["H"]
    bufs = {k: fc.Guarded(c[k], dev) for k in ("maps", "m", "v", "photos", "scenes")}
    loss = torch.full((1,), -1.0, device=dev)
    ws = torch.zeros(65, dtype=torch.int64, device=dev)
    xr = native.xrow(dev, H)
    good = np.array([[0.0, 1.0]] * 12, np.float32)
    f = ctypes.c_float

    def call(maps=bufs["maps"].ptr(), bounds=good, lr=1e-2, b1=0.9, b2=0.999, ae=1e-8, step=1, planes=0, ws_bytes=65 * 8, W=H):
        barr = (ctypes.c_float * 24)(*np.asarray(bounds, np.float32).reshape(-1).tolist())
        return fn(maps, bufs["m"].ptr(), bufs["v"].ptr(), bufs["photos"].ptr(), None, planes, bufs["scenes"].ptr(), xr.data_ptr(),
                  f(photo_checks.EPS), barr, f(lr), f(b1), f(b2), f(ae), step, loss.data_ptr(), None, ws.data_ptr(), ws_bytes,
                  B, S, H, W, None)

    before = lib.svbrdf_debug_launch_count()
    nan = float("nan")
    bad_lo, bad_nan = good.copy(), good.copy()
    bad_lo[3], bad_nan[9] = (1.0, 0.0), (nan, 1.0)
    assert call(maps=None) == -1 and call(maps=bufs["maps"].ptr() + 2) == -3 and call(ws_bytes=64 * 8) == -4
    for bad in (dict(step=0), dict(lr=-1.0), dict(lr=nan), dict(ae=-1.0), dict(ae=float("inf")), dict(b1=1.0), dict(b2=-0.1),
                dict(bounds=bad_lo), dict(bounds=bad_nan), dict(planes=1), dict(W=H + 1)):
        assert call(**bad) == -2, bad
    torch.cuda.synchronize(dev)
    assert lib.svbrdf_debug_launch_count() == before
    for k, buf in bufs.items():
        got, ok = buf.get()
        assert ok and fc.same_bits(got, c[k]), k
    assert loss.item() == -1.0 and not ws.any().item()


@pytest.mark.parametrize("name", ("b3_13_s2_w", "b1_16_s5_shared_untied", "b1_17_s5"))
def test_photofit_step_is_the_c_abi(native, dev, name, monkeypatch):
    """PhotoFit.step equals the direct call bit for bit over two steps; one launch per step by the library's counter, no
    upload of the device table, and the state carries torch.optim.Adam's names"""
    from svbrdf_estimation_amd import fitting
    c = case(native, dev, name)
    lib = native._load()
    x = torch.from_numpy(c["maps"]).to(dev)
    fit = fitting.PhotoFit(x, lr=fc.LR, betas=(fc.BETA1, fc.BETA2), eps=fc.ADAM_EPS, bounds=fc.BOUNDS_FIT, loss_eps=fc.EPS)
    assert fit.uses_fused_kernel()
    fit.exp_avg, fit.exp_avg_sq = torch.from_numpy(c["m"]).to(dev), torch.from_numpy(c["v"]).to(dev)
    fit.state["step"] = c["t"] - 1
    photos, table = torch.from_numpy(c["photos"]).to(dev), torch.from_numpy(c["scenes"]).to(dev)
    weights = None if c["weights"] is None else torch.from_numpy(c["weights"]).to(dev)
    native.xrow(dev, c["H"])                                         # (cached once per width: not part of a step)
    torch.cuda.synchronize(dev)

    def no_upload(*a, **k):
        raise AssertionError("a device table must not be uploaded")
    monkeypatch.setattr(native, "upload_scene_table", no_upload)
    d = dict(c)
    for k in range(2):
        direct = fc.abi_fit(native, dev, d, t=c["t"] + k, bounds=fc.BOUNDS_FIT, want_grad=False)
        before = lib.svbrdf_debug_launch_count()
        loss = fit.step(photos, table, weights)
        assert lib.svbrdf_debug_launch_count() - before == 1 and fit.state["step"] == c["t"] + k
        assert loss.dim() == 0 and loss.is_cuda and fc.same_bits(loss.cpu().numpy().reshape(1), direct["loss"])
        for got, key in ((fit.maps, "x"), (fit.exp_avg, "m"), (fit.exp_avg_sq, "v")):
            assert fc.same_bits(got.cpu().numpy(), direct[key]), (k, key)
        d = dict(d, maps=direct["x"], m=direct["m"], v=direct["v"])
    assert fit.maps.data_ptr() == x.data_ptr()                       # in place
    photo_checks.assert_scratch_is_zero(native)


def test_forty_step_fit_against_the_unfused_trajectory(native, dev):
    """tools/fit_photos.py's start at 32 x 32, B = 2, S = 5: 40 fused steps against PhotoLoss + torch.optim.Adam + clamp_ from
    the same start.  The two differ only by the rounding of the update (torch forms m' with lerp and x' with addcdiv): the
    fused final loss must be at most 1.01 x the unfused one.  Measured on an MI355X (profiles/r18_photo_fit.txt): start
    0.1533104, unfused end 0.0162796, fused end 0.0162789 (ratio 0.99995)."""
    from svbrdf_estimation_amd import fitting, losses, renderers, synthesis
    B, H, S, steps, seed, lr = 2, 32, 5, 40, 1, 0.01
    truth = torch.from_numpy(synth.make_maps(seed, B, H)).to(dev)
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)
    photos = synthesis.render_inputs(truth, S, use_augmentation=True, noise=None)
    torch.manual_seed(seed)
    table = torch.stack([synthesis.input_scene_table(S, True) for _ in range(B)], dim=0).to(dev)
    start = truth.clone()
    jitter = torch.from_numpy(synth.uniform01(seed + 1000, (B, 9, H, H))).to(dev) - 0.5
    start[:, 3:] = (start[:, 3:] + 0.3 * jitter).clamp_(0.02, 0.98)
    fn = losses.PhotoLoss(renderers.LocalRenderer())
    x = start.clone().requires_grad_(True)
    opt = torch.optim.Adam([x], lr=lr)
    first = None
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        loss = fn(x, photos, table)
        first = loss.item() if first is None else first
        loss.backward()
        opt.step()
        with torch.no_grad():
            x[:, 3:].clamp_(0.0, 1.0)
    fit = fitting.PhotoFit(start.clone(), lr=lr, bounds=fc.BOUNDS_FIT)
    fused_first = None
    for _ in range(steps):
        loss = fit.step(photos, table)
        fused_first = loss.item() if fused_first is None else fused_first
    with torch.no_grad():
        unfused_end, fused_end = fn(x, photos, table).item(), fn(fit.maps, photos, table).item()
    print("[fit] 40 steps at 32 x 32, B = 2, S = 5: start %.7f; unfused end %.7f, fused end %.7f (ratio %.5f); "
          "max |maps fused - unfused| %.3g" % (first, unfused_end, fused_end, fused_end / unfused_end,
                                               (fit.maps - x.detach()).abs().max().item()))
    assert fused_first == first and fit.state["step"] == steps
    assert unfused_end < first                                       # the fit does fit
    assert fused_end <= 1.01 * unfused_end, (fused_end, unfused_end)


def test_fused_step_speed(native, dev):
    """At the configuration-2 shape (B = 8, 256 x 256, S = 9, per-photo weights), one process, photo_loss_bench's timing:
    (a) the fused step takes at most the composed step -- PhotoLoss forward + backward, torch.optim.Adam, clamp_ -- with the
        faster of the stock default and fused=True; no margin;
    (b) at most (72 + 3 S + P) / (24 + 3 S + P) = 1.8 x the weighted loss kernel's launch on the same data: the byte ratio.
    Measured on an MI355X (profiles/r18_photo_fit.txt): fused 59.98 us, weighted launch 41.32 us (ratio 1.452), composed
    195.46 us (stock Adam) / 115.16 us (fused=True)."""
    r = fc.measure_photo_fit(dev, native)
    print("[fit] fused step %.2f us; weighted loss launch %.2f us (ratio %.3f, byte ratio %.3f); composed step %.2f us "
          "(stock Adam), %.2f us (fused=True); fused / faster composed %.3f; %.3f of 8 TB/s; rounds %s" % (
              r["fit_us"], r["weighted_us"], r["fit_over_weighted"], r["byte_ratio"], r["composed_us"], r["composed_fused_us"],
              r["fit_over_composed"], r["fit_frac_of_8TBps"], r["rounds"]))
    assert abs(r["byte_ratio"] - 1.8) < 1e-12
    assert r["fit_us"] <= min(r["composed_us"], r["composed_fused_us"]), r
    assert r["fit_us"] <= r["byte_ratio"] * r["weighted_us"], r
