"""Shared by tests/test_photo_fit_smooth_cpu.py and tests/test_gpu_photo_fit_smooth.py: the numpy float32 restatement of
the smoothness prior's gradient (csrc/svbrdf_photo_fit_smooth.hip; svbrdf_photo_fit_smooth_adam_step[_scene_grad]), the
cases the GPU tests run, the direct C ABI calls with canaries around every buffer, the hole experiment and the speed
measurement.  Nothing under /reference is needed: the photo gradient is bitwise that of entries g18 / g21 / g23 already pin,
Adam is photo_fit_checks.restatement; what is new is four lines of the header, restated here.
"""
import ctypes

import numpy as np

import photo_checks
import photo_fit_checks as fc
import photo_fit_pose_checks as jc
import synth
import weighted_photo_checks as wp

F32 = np.float32
EPS = fc.EPS
STEP_ENTRY, JOINT_ENTRY = "svbrdf_photo_fit_smooth_adam_step", "svbrdf_photo_fit_smooth_adam_step_scene_grad"
# lambda per plane: some 0 (planes 0, 5, 9: they read no neighbour), some equal, some distinct
LAMBDA = np.array([0.0, 0.5, 0.5, 0.02, 0.3, 0.0, 0.01, 0.01, 0.01, 0.0, 0.7, 0.05], dtype=np.float32)
QUANTISED = (1, 3, 6, 7, 8, 10)     # planes whose values are multiples of 1/8 in the GPU cases: ties occur (all have a lambda)


# ------------------------------------------------------------------------------------------------ the oracle

def coefficients(lam, B, H, W):
    """c[ch] = (float)((double)lambda[ch] / ((double)B H W)): the float32 lambdas the entry takes, rounded once"""
    lam = np.asarray(lam, dtype=np.float32).astype(np.float64)
    return (lam / (float(B) * float(H) * float(W))).astype(np.float32)


def order_sign(a, b):
    """s(a, b) of the header: +1, -1, 0 from compares of the stored values, NaN if unordered"""
    with np.errstate(invalid="ignore"):
        return np.where(a > b, F32(1), np.where(a < b, F32(-1), np.where(a == b, F32(0), F32(np.nan)))).astype(np.float32)


def sign_sum(x):
    """k of the header for every element of x [B,12,H,W]: s(x, left) + s(x, right) + s(x, up) + s(x, down), a neighbour
    outside the patch contributes 0 -> float32, integers in -4..4 or NaN"""
    x = np.asarray(x, dtype=np.float32)
    k = np.zeros_like(x)
    k[..., :, 1:] += order_sign(x[..., :, 1:], x[..., :, :-1])       # left
    k[..., :, :-1] += order_sign(x[..., :, :-1], x[..., :, 1:])      # right
    k[..., 1:, :] += order_sign(x[..., 1:, :], x[..., :-1, :])       # up
    k[..., :-1, :] += order_sign(x[..., :-1, :], x[..., 1:, :])      # down
    return k


def prior_term(x, lam):
    """-> (c [12], k like x, t = c k: one float32 product per element)"""
    B, _, H, W = x.shape
    c = coefficients(lam, B, H, W)
    k = sign_sum(x)
    with np.errstate(invalid="ignore"):
        t = (c.reshape(1, 12, 1, 1) * k).astype(np.float32)
    return c, k, t


def smooth_gradient(g, x, lam):
    """THE TEST ORACLE: g' = g + (c k) in float32, one sum per element; a channel with lambda == 0 keeps g bit for bit"""
    c, _, t = prior_term(x, lam)
    g = np.asarray(g, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where((c != 0).reshape(1, 12, 1, 1), (g + t).astype(np.float32), g).astype(np.float32)


def expected_step(lib, c, grad, lam, t=None, bounds=None):
    """smooth_gradient, then photo_fit_checks.restatement with the library's exported scalars -> (g', x', m', v')"""
    g2 = smooth_gradient(grad, c["maps"], lam)
    return (g2,) + fc.expected_step(lib, c, g2, t=t, bounds=bounds)


# ------------------------------------------------------------------------------------------------ the GPU cases
# photo_fit_checks.CASES' tuples, all of them, and the shapes at which an index rule of the prior can fail that they lack:
# 1 x 1 (no neighbour at all), 2 x 2 (every pixel on two borders), 260 x 260 (a row spans two workgroups: up and down lie
# 260 pixels = more than a workgroup away; S = 1 keeps it quick).  With CASES' own: 7 (rows wrap inside a wave: pixels 6 and
# 7 are no neighbours), 16 (four rows per wave), 17 (a partial second workgroup; up / down across the workgroup edge),
# 64 with B = 5 (a row = a wave, 80 workgroups, the item edge: the last row of item b must not see item b + 1).
EXTRA = (
    ("b2_1_s2_w", 2, 1, (1, 1), "per-photo", True, "random", 2),
    ("b2_2_s1_shared_untied", 2, 2, (1, 0), "shared", False, "zero", 1),
    ("b1_260_s1", 1, 260, (1, 0), None, True, "random", 1000),
)
CASES = fc.CASES + EXTRA
NAMES = [c[0] for c in CASES]
ALL_K_FROM = 7       # from this size on a case's own enabled channels must show every k in -4..4


def case_inputs(native, dev, name):
    """photo_fit_checks.case_inputs for the tuples above, then the maps quantised to multiples of 1/8 on the planes
    QUANTISED (roughness on all three or none: a tied case stays tied) so that equal neighbours occur"""
    import torch
    idx = NAMES.index(name)
    if idx < len(fc.CASES):
        c = fc.case_inputs(native, dev, name)
    else:
        _, B, H, (nr, ns), layout, tied, state, t = CASES[idx]
        S = nr + ns
        sc = photo_checks.scene_table(B, 500 + idx, nr, ns)
        maps = synth.make_maps(7100 + 2 * idx, B, H, tiled_roughness=tied)
        target = synth.make_maps(7101 + 2 * idx, B, H, tiled_roughness=tied)
        photos = native.render_fwd(torch.from_numpy(target).to(dev), torch.from_numpy(sc)).clamp_(0.0, 1.0).cpu().numpy()
        weights = None
        if layout is not None and H >= 8:
            weights = wp.weight_field(7200 + idx, B, S if layout == "per-photo" else 1, H)
        elif layout is not None:        # weight_field's distribution without its masked rows: a 1 x 1 patch has a single row
            u = synth.uniform01(7200 + idx, (B, S if layout == "per-photo" else 1, H, H))
            weights = np.where(u < 0.25, F32(0), np.where(u >= 0.75, F32(1), (u - F32(0.25)) * F32(2))).astype(np.float32)
        if state == "zero":
            m, v = np.zeros(maps.shape, np.float32), np.zeros(maps.shape, np.float32)
        else:
            u = synth.uniform01(7300 + idx, (3,) + maps.shape)
            m = ((u[0] - F32(0.5)) * F32(2e-3)).astype(np.float32)
            v = (u[1] * F32(1e-5)).astype(np.float32)
            m[u[2] < 0.1] = 0.0
            v[u[2] > 0.9] = 0.0
        c = dict(name=name, B=B, H=H, S=S, t=t, maps=maps, photos=photos, scenes=sc, weights=weights, m=m, v=v)
    c = dict(c, maps=c["maps"].copy())
    for ch in QUANTISED:
        c["maps"][:, ch] = np.round(c["maps"][:, ch] * F32(8)) / F32(8)
    return c


def assert_exercises_every_k(c, lam=LAMBDA):
    """THE INPUT CONDITION: on the channels that have a lambda every k in -4..4 occurs (from ALL_K_FROM pixels a side on;
    below that, what the shape admits: 0 alone at 1 x 1, -2..2 at 2 x 2), +-3 -- the one product c k that rounds -- included.
    An input that does not exercise the rounding of 3 c is not accepted."""
    k = sign_sum(c["maps"])[:, np.asarray(lam) != 0]
    seen = set(np.unique(k).astype(int).tolist())
    H = c["H"]
    want = set(range(-4, 5)) if H >= ALL_K_FROM else ({0} if H == 1 else set(range(-2, 3)))
    assert want <= seen, (c["name"], sorted(want - seen))
    # and 3 c does round for at least one enabled channel: c k != the exact product
    cs = coefficients(lam, c["B"], H, H)
    if H >= ALL_K_FROM:
        assert any(float(F32(3) * v) != 3.0 * float(v) for v in cs[cs != 0]), cs


# ------------------------------------------------------------------------------------------------ the C ABI

def smooth_array(lam):
    arr = (ctypes.c_float * 12)(*np.asarray(lam, dtype=np.float32).tolist())
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def abi_smooth(native, dev, c, lam=LAMBDA, joint=False, t=None, bounds=None, want_grad=True, shift=0, ws=None):
    """svbrdf_photo_fit_smooth_adam_step (joint: ..._scene_grad) on the case through its own ctypes call, every buffer
    between canaries -> dict: loss [1], grad (g', or None), grad_scenes (joint), x (= maps_out), m, v after the step,
    `maps_in_intact`, `inputs_intact` (maps_in, photos, weights, table), `canaries_intact`, `launches`, `scratch_zero`"""
    import torch
    lib = native._load()
    B, S, H = c["B"], c["S"], c["H"]
    G = lambda a: fc.Guarded(a, dev, shift)
    xin, xout, m, v = G(c["maps"]), G(np.full_like(c["maps"], 3.0)), G(c["m"]), G(c["v"])
    ph, sc = G(c["photos"]), G(c["scenes"])
    w = None if c["weights"] is None else G(c["weights"])
    loss = G(np.full(1, -1.0, np.float32))
    grad = G(np.full_like(c["maps"], 7.0)) if want_grad else None
    gs = G(np.full_like(c["scenes"], 7.0)) if joint else None
    if ws is None:
        ws = jc.scratch(lib, dev, c) if joint else torch.zeros(65, dtype=torch.int64, device=dev)
    xr = native.xrow(dev, H)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    keep_b, bptr = fc.bounds_array(bounds)
    keep_s, sptr = smooth_array(lam)
    f = ctypes.c_float
    before = lib.svbrdf_debug_launch_count()
    rc = getattr(lib, JOINT_ENTRY if joint else STEP_ENTRY)(
        xin.ptr(), xout.ptr(), m.ptr(), v.ptr(), ph.ptr(), None if w is None else w.ptr(),
        0 if w is None else int(c["weights"].shape[1]), sc.ptr(), xr.data_ptr(), f(EPS), sptr, bptr, f(fc.LR), f(fc.BETA1),
        f(fc.BETA2), f(fc.ADAM_EPS), int(c["t"] if t is None else t), loss.ptr(), None if grad is None else grad.ptr(),
        *((gs.ptr(),) if joint else ()), ws.data_ptr(), ws.numel() * 8, B, S, H, H, st)
    assert rc == 0, lib.svbrdf_last_error()
    torch.cuda.synchronize(dev)
    del keep_b, keep_s
    out = dict(launches=lib.svbrdf_debug_launch_count() - before, scratch_zero=not ws.any().item())
    canaries, intact = True, True
    for key, buf in (("x", xout), ("m", m), ("v", v), ("loss", loss), ("grad", grad), ("grad_scenes", gs)):
        out[key], ok = (None, True) if buf is None else buf.get()
        canaries = canaries and ok
    for buf, src in ((xin, c["maps"]), (ph, c["photos"]), (sc, c["scenes"]), (w, c["weights"])):
        if buf is not None:
            got, ok = buf.get()
            canaries = canaries and ok
            intact = intact and fc.same_bits(got, src)
    out.update(canaries_intact=canaries, inputs_intact=intact)
    return out


# ------------------------------------------------------------------------------------------------ the hole experiment

def hole_problem(H, cell, hole, S=5, dtype=np.float32):
    """The experiment of the feature's motivation: truth = synth.make_maps(5, 1, H / cell) enlarged to constant cells of
    `cell` x `cell`, weights 0 on the block `hole` = (lo, hi) of rows and columns in ALL S photos (inside one cell) and 1
    elsewhere, start = truth + 0.3 (uniform01(77) - 0.5) on d, r, s clamped to [0.02, 0.98]
    -> (truth, start, weights [1,S,H,H], hole mask [H,H]) as numpy"""
    small = synth.make_maps(5, 1, H // cell)
    truth = np.repeat(np.repeat(small, cell, axis=2), cell, axis=3).astype(dtype)
    weights = np.ones((1, S, H, H), dtype)
    lo, hi = hole
    weights[:, :, lo:hi, lo:hi] = 0.0
    start = truth.copy()
    jitter = synth.uniform01(77, (1, 9, H, H)).astype(dtype) - dtype(0.5)
    start[:, 3:] = np.clip(start[:, 3:] + dtype(0.3) * jitter, dtype(0.02), dtype(0.98))
    mask = np.zeros((H, H), bool)
    mask[lo:hi, lo:hi] = True
    return truth, start, weights, mask


def hole_errors(x, truth, mask):
    """-> (mean |d,r,s - truth| in the hole, on the seen pixels)"""
    d = np.abs(np.asarray(x, dtype=np.float64)[:, 3:] - np.asarray(truth, dtype=np.float64)[:, 3:])
    return float(d[..., mask].mean()), float(d[..., ~mask].mean())


# ------------------------------------------------------------------------------------------------ the speed measurement

def measure_smooth_fit(dev, native, sets=6, n=40, rounds=3, lam=(0.0, 0.01, 0.01, 0.01)):
    """-> dict of medians (us per step) at the configuration-2 shape of photo_fit_checks.fit_workload (B = 8, 256 x 256,
    S = 9, per-photo weights, `sets` rotating batches), one process, the legs alternating (photo_checks.timed_legs):

        smooth_us         svbrdf_photo_fit_smooth_adam_step through the C ABI, ping-ponging two map buffers: ONE launch
        plain_us          svbrdf_photo_fit_adam_step through the C ABI on the same data: ONE launch
        photofit_us       PhotoFit(smooth=).step: the launch and the copy back into `maps`
        steps16_us        PhotoFit(smooth=).steps(16) / 16: no copy
        composed_us       PhotoLoss forward + backward, fitting.smoothness backward, torch.optim.Adam (stock), clamp_
        composed_fused_us the same with torch.optim.Adam(fused=True)
    """
    import torch
    from svbrdf_estimation_amd import fitting, losses, renderers
    lib = native._load()
    B, H, S, table, starts, photos, weights = fc.fit_workload(dev, native, sets)
    lam12 = np.repeat(np.asarray(lam, np.float32), 3)
    keep_s, sptr = smooth_array(lam12)
    keep_b, bptr = fc.bounds_array(fc.BOUNDS_FIT)
    pairs = [[a.clone(), torch.empty_like(a)] for a in starts]
    plain = [a.clone() for a in starts]
    state = [[torch.zeros_like(a) for _ in range(4)] for a in starts]       # m, v of the smooth leg; m, v of the plain one
    xr = native.xrow(dev, H)
    ws = torch.zeros(65, dtype=torch.int64, device=dev)
    loss = torch.empty(1, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    f = ctypes.c_float
    turn = [0] * sets

    def smooth(i):
        k = i % sets
        src, dst = pairs[k][turn[k] & 1], pairs[k][1 - (turn[k] & 1)]
        turn[k] += 1
        rc = getattr(lib, STEP_ENTRY)(src.data_ptr(), dst.data_ptr(), state[k][0].data_ptr(), state[k][1].data_ptr(),
                                      photos[k].data_ptr(), weights[k].data_ptr(), S, table.data_ptr(), xr.data_ptr(), f(EPS),
                                      sptr, bptr, f(fc.LR), f(fc.BETA1), f(fc.BETA2), f(fc.ADAM_EPS), turn[k], loss.data_ptr(),
                                      None, ws.data_ptr(), ws.numel() * 8, B, S, H, H, st)
        assert rc == 0, lib.svbrdf_last_error()

    steps_plain = [0] * sets

    def plain_step(i):
        k = i % sets
        steps_plain[k] += 1
        rc = getattr(lib, fc.STEP_ENTRY)(plain[k].data_ptr(), state[k][2].data_ptr(), state[k][3].data_ptr(), photos[k].data_ptr(),
                                         weights[k].data_ptr(), S, table.data_ptr(), xr.data_ptr(), f(EPS), bptr, f(fc.LR),
                                         f(fc.BETA1), f(fc.BETA2), f(fc.ADAM_EPS), steps_plain[k], loss.data_ptr(), None,
                                         ws.data_ptr(), ws.numel() * 8, B, S, H, H, st)
        assert rc == 0, lib.svbrdf_last_error()

    bounds = torch.from_numpy(fc.BOUNDS_FIT)
    fits = [fitting.PhotoFit(a.clone(), lr=fc.LR, bounds=bounds, smooth=lam) for a in starts]
    fits16 = [fitting.PhotoFit(a.clone(), lr=fc.LR, bounds=bounds, smooth=lam) for a in starts]

    def photofit(i):
        k = i % sets
        fits[k].step(photos[k], table, weights[k])

    def steps16(i):
        k = i % sets
        fits16[k].steps(16, photos[k], table, weights[k])

    def composed_leg(**adam):
        fn = losses.PhotoLoss(renderers.LocalRenderer())
        xs = [a.clone().requires_grad_(True) for a in starts]
        opts = [torch.optim.Adam([x], lr=fc.LR, **adam) for x in xs]

        def step(i):
            k = i % sets
            opts[k].zero_grad(set_to_none=True)
            (fn(xs[k], photos[k], table, weights[k]) + fitting.smoothness(xs[k], lam)).backward()
            opts[k].step()
            with torch.no_grad():
                xs[k][:, 3:].clamp_(0.0, 1.0)
        return step

    legs = (("smooth_us", smooth), ("plain_us", plain_step), ("photofit_us", photofit), ("steps16_us", steps16),
            ("composed_us", composed_leg()), ("composed_fused_us", composed_leg(fused=True)))
    out, res = photo_checks.timed_legs(legs, n, rounds, photo_checks.spinning_wave(native, dev), dev)
    del keep_s, keep_b
    out["steps16_us"] /= 16.0
    res["steps16_us"] = [v / 16.0 for v in res["steps16_us"]]
    out.update(rounds=res, device=torch.cuda.get_device_name(dev), steps_per_round=n, sets=sets,
               smooth_over_plain=out["smooth_us"] / out["plain_us"], bound=(108.0 + 48.0) / 108.0,
               smooth_over_composed=out["smooth_us"] / min(out["composed_us"], out["composed_fused_us"]))
    return out
