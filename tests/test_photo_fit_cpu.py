"""One step of a photo fit in one launch (csrc/svbrdf_photo_fit.hip: k_fit_maps*; svbrdf_photo_fit_adam_step;
fitting.PhotoFit), everything that needs no GPU:

  * the numpy float32 restatement of the update (tests/photo_fit_checks.py: the oracle of the GPU tests) stays inside the
    stated bounds of torch.optim.Adam in float64 at t = 1, 2, 1000, on inputs for which it has no subnormal intermediate;
  * svbrdf_photo_fit_adam_scalars against double arithmetic, to 1 ulp of float32;
  * the library exports the two symbols without an ABI bump, header and binding agree, and every bad argument is
    rejected before anything is launched, the buffers untouched;
  * fitting.PhotoFit on float64 CPU tensors (the composed path, a plugin renderer) is PhotoLoss +
    torch.optim.Adam(foreach=False) + clamp_ over 5 steps to 1e-12, and fitting.composed_step in float32 is the restatement
    bit for bit;
  * the two kernels, compiled with the Makefile's flags: no scratch, occupancy 4, one scene loop with transcendentals per
    loop kind, IEEE division and square root, the clamp as compares and selects.
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import photo_fit_checks as fc
import synth
import unit_build
from test_photo_loss_cpu import PHOTO_TIED_LOOP_TRANS, PHOTO_UNTIED_LOOP_TRANS, _isa_stats, needs_hipcc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from svbrdf_estimation_amd import _native
    return _native._load()


# ------------------------------------------------------------------------------------------------ the oracle itself

@pytest.mark.parametrize("t", (1, 2, 1000))
def test_restatement_is_within_the_float64_bounds_and_has_no_subnormal_intermediate(lib, t):
    """|x' - ref| <= 2^-24 |x'| + 2^-20 A, |m' - ref| <= 2^-22 (|beta1 m| + |c1 g|), |v' - ref| <= 2^-21 |v'| against
    torch.optim.Adam in float64 (photo_fit_checks.assert_within_float64_bounds has the derivation: about 10.5 roundings of
    2^-24 on the update's ingredients, cancellation in m' bounded absolutely)."""
    x, m, v, g = fc.oracle_inputs(100 + t)
    assert (g == 0).sum() > 1000 and np.abs(g[g != 0]).min() < 2e-10 and np.abs(g).max() > 5e-3 and (v >= 0).all()
    sc = fc.library_scalars(lib, fc.LR, fc.BETA1, fc.BETA2, t)
    xn, m2, v2, subnormal = fc.restatement(x, m, v, g, sc)
    assert subnormal == 0
    assert np.isfinite(xn).all() and np.isfinite(m2).all() and (v2 >= 0).all()
    worst = fc.assert_within_float64_bounds(xn, m2, v2, x, m, v, g, fc.LR, fc.BETA1, fc.BETA2, fc.ADAM_EPS, t, "t = %d" % t)
    print("[fit] restatement vs float64 Adam, t = %d: worst err/bound x' %.3f, m' %.3f, v' %.3f" % ((t,) + tuple(worst)))


def test_restatement_clamp_keeps_nan_and_infinite_bounds_do_nothing():
    x = np.zeros((1, 12, 1, 2), np.float32)
    x[0, :, 0, 0] = np.linspace(-1.0, 2.0, 12)
    x[0, 5, 0, 1] = np.nan
    z = np.zeros_like(x)
    sc = (np.float32(0.1), np.float32(0.001), np.float32(0.1), np.float32(31.6))
    free = fc.restatement(x, z, z, z, sc)[0]
    inf = fc.restatement(x, z, z, z, sc, bounds=np.array([[-np.inf, np.inf]] * 12))[0]
    assert fc.same_bits(free, inf) and fc.same_bits(free, x)          # g = m = 0: the maps do not move
    got = fc.restatement(x, z, z, z, sc, bounds=np.array([[0.0, 1.0]] * 12))[0]
    assert np.isnan(got[0, 5, 0, 1]) and got[0, 0, 0, 0] == 0.0 and got[0, 11, 0, 0] == 1.0
    assert fc.same_bits(got[0, :, 0, 0], np.clip(x[0, :, 0, 0], 0.0, 1.0))
    pin = fc.restatement(x, z, z, z, sc, bounds=np.array([[0.25, 0.25]] * 12))[0]
    assert (pin[0, :, 0, 0] == 0.25).all() and np.isnan(pin[0, 5, 0, 1])


@pytest.mark.parametrize("lr,b1,b2,t", [(1e-2, 0.9, 0.999, 1), (1e-2, 0.9, 0.999, 2), (1e-2, 0.9, 0.999, 1000),
                                        (3e-4, 0.5, 0.99, 7), (1.0, 0.0, 0.0, 3), (0.0, 0.9, 0.999, 1)])
def test_adam_scalars_against_double_arithmetic(lib, lr, b1, b2, t):
    """c1, c2, step_size, rsb2 in double from the float32 arguments, rounded once: within 1 ulp of float32 of Python's"""
    got = fc.library_scalars(lib, lr, b1, b2, t)
    lr, b1, b2 = (float(np.float32(s)) for s in (lr, b1, b2))
    want = (1.0 - b1, 1.0 - b2, lr / (1.0 - b1 ** t), 1.0 / math.sqrt(1.0 - b2 ** t))
    for g, w in zip(got, want):
        assert abs(float(g) - w) <= float(np.spacing(np.float32(abs(w)))), (got, want)
    out = (ctypes.c_float * 4)()
    fn = getattr(lib, fc.SCALARS_ENTRY)
    p = ctypes.cast(out, ctypes.c_void_p)
    f = ctypes.c_float
    assert fn(f(lr), f(b1), f(b2), 0, p) == -2 and fn(f(lr), f(1.0), f(b2), 1, p) == -2 and fn(f(lr), f(b1), f(-0.1), 1, p) == -2
    assert fn(f(-1.0), f(b1), f(b2), 1, p) == -2 and fn(f(float("nan")), f(b1), f(b2), 1, p) == -2
    assert fn(f(float("inf")), f(b1), f(b2), 1, p) == -2 and fn(f(lr), f(b1), f(b2), 1, None) == -1


# ------------------------------------------------------------------------------------------------ the C ABI

def test_library_exports_the_fit_entries_without_an_abi_bump(lib):
    from svbrdf_estimation_amd import _native
    assert lib.svbrdf_abi_version() == 8 and _native.ABI_VERSION == 8
    with open(os.path.join(ROOT, "include", "svbrdf_hip.h")) as f:
        header = f.read()
    assert "#define SVBRDF_ABI_VERSION 8" in header
    for name, count in ((fc.STEP_ENTRY, 24), (fc.SCALARS_ENTRY, 5)):
        assert hasattr(lib, name), name
        declared = header.split("SVBRDF_API int %s(" % name)[1].split(");")[0]
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == count == declared.count(",") + 1
    assert "EQUAL BIT FOR BIT" in header and "BEFORE the update" in header and "A NaN x' stays NaN" in header


def test_argument_errors_come_before_any_launch_and_touch_nothing(lib):
    """-1 null pointers (weights, bounds and grad_out may be null), -2 dims, eps, weight_planes, step < 1, lr or adam_eps
    negative or not finite, a beta outside [0, 1), a NaN bound or lo > hi, -3 misaligned, -4 workspace too small.  Host
    buffers stand in for device memory: nothing is enqueued, and not a byte of them changes."""
    fn = getattr(lib, fc.STEP_ENTRY)
    B, S, H = 1, 9, 8
    buf = (ctypes.c_float * 32768)()
    for i in range(len(buf)):
        buf[i] = float(i % 251)
    snapshot = bytes(buf)
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 63) & ~63
    need = lib.svbrdf_rendering_loss_workspace_bytes(B, S, H, H)
    good = np.array([[0.0, 1.0]] * 12, dtype=np.float32)
    nan, inf = float("nan"), float("inf")

    def call(maps=p, m=p + 4096, v=p + 8192, photos=p + 12288, weights=p + 20480, planes=S, scenes=p + 24576, xrow=p + 25600,
             eps=0.1, bounds=good, lr=1e-2, b1=0.9, b2=0.999, ae=1e-8, step=1, loss=p + 26624, grad=p + 28672, ws=p + 40960,
             ws_bytes=need, B=B, S=S, H=H, W=H):
        barr = None if bounds is None else (ctypes.c_float * 24)(*np.asarray(bounds, np.float32).reshape(-1).tolist())
        f = ctypes.c_float
        return fn(maps, m, v, photos, weights, planes, scenes, xrow, f(eps), barr, f(lr), f(b1), f(b2), f(ae), step, loss, grad,
                  ws, ws_bytes, B, S, H, W, None)

    launches = lib.svbrdf_debug_launch_count()
    for name in ("maps", "m", "v", "photos", "scenes", "xrow", "loss", "ws"):
        assert call(**{name: None}) == -1, name
        assert lib.svbrdf_last_error()
    for planes in (0, 2, S + 1, -1):
        assert call(planes=planes) == -2, planes
        assert b"weight_planes" in lib.svbrdf_last_error()
    for planes in (1, S):                                           # no weights: only 0 planes
        assert call(weights=None, planes=planes) == -2, planes
    assert call(W=H + 1) == -2 and call(B=0) == -2 and call(S=0, planes=1) == -2 and call(eps=0.0) == -2
    for bad in (dict(step=0), dict(step=-3), dict(lr=-1e-2), dict(lr=nan), dict(lr=inf), dict(ae=-1e-8), dict(ae=nan),
                dict(ae=inf), dict(b1=1.0), dict(b1=-0.1), dict(b1=nan), dict(b2=1.0), dict(b2=-0.5), dict(b2=nan)):
        assert call(**bad) == -2, bad
    for k, pair in ((0, (nan, 1.0)), (5, (0.0, nan)), (11, (1.0, 0.0)), (3, (inf, -inf))):
        b = good.copy()
        b[k] = pair
        assert call(bounds=b) == -2, (k, pair)
        assert b"bounds" in lib.svbrdf_last_error()
    assert call(maps=p + 2) == -3 and call(m=p + 4098) == -3 and call(v=p + 8194) == -3 and call(photos=p + 12290) == -3
    assert call(weights=p + 20482) == -3 and call(grad=p + 28674) == -3 and call(scenes=p + 24578) == -3 and call(ws=p + 40964) == -3
    assert call(ws_bytes=need - 8) == -4
    assert lib.svbrdf_debug_launch_count() == launches              # failed calls enqueue and count nothing
    assert bytes(buf) == snapshot


# ------------------------------------------------------------------------------------------------ the Python layer

def _toy_problem(dtype):
    from svbrdf_estimation_amd import environment
    B, S, H = 2, 3, 8
    maps = torch.from_numpy(synth.make_maps(41, B, H)).to(dtype)
    torch.manual_seed(5)
    table = torch.stack([environment.scene_table(1, S - 1) for _ in range(B)])
    photos = (torch.rand(B, S, 3, H, H) * 0.2).to(dtype)
    weights = torch.from_numpy(fc.wp.weight_field(77, B, S, H))
    return maps, photos, table, weights


@pytest.mark.parametrize("weighted", (False, True))
def test_photofit_float64_cpu_is_photoloss_adam_clamp(weighted):
    """5 steps of PhotoFit (the composed path: CPU, float64, a plugin renderer) against PhotoLoss + torch.optim.Adam(foreach=
    False) + x[:, 3:].clamp_(0, 1) from the same start: maps, exp_avg, exp_avg_sq and every loss to 1e-12"""
    from svbrdf_estimation_amd import fitting, losses
    maps, photos, table, weights = _toy_problem(torch.float64)
    w = weights if weighted else None
    lr = 0.05
    fit = fitting.PhotoFit(maps.clone(), lr=lr, bounds=fc.BOUNDS_FIT, renderer=fc.ToyRenderer())
    assert not fit.uses_fused_kernel() and fit.state["step"] == 0 and not fit.exp_avg.any() and not fit.exp_avg_sq.any()
    x = maps.clone().requires_grad_(True)
    opt = torch.optim.Adam([x], lr=lr, foreach=False)
    fn = losses.PhotoLoss(fc.ToyRenderer())
    for step in range(5):
        opt.zero_grad(set_to_none=True)
        ref = fn(x, photos, table, w)
        ref.backward()
        opt.step()
        with torch.no_grad():
            x[:, 3:].clamp_(0.0, 1.0)
        loss = fit.step(photos, table, w)
        assert loss.dim() == 0 and loss.dtype == torch.float64 and abs(loss.item() - ref.item()) <= 1e-12
        assert (fit.maps - x.detach()).abs().max().item() <= 1e-12, step
    st = opt.state[x]
    assert fit.state["step"] == 5 == int(st["step"])
    assert (fit.exp_avg - st["exp_avg"]).abs().max().item() <= 1e-12 and (fit.exp_avg_sq - st["exp_avg_sq"]).abs().max().item() <= 1e-12
    assert (x.detach() != maps).any() and x.detach()[:, 3:].min() >= 0.0
    # the state is assignable, with torch.optim.Adam's names and meaning
    fit.exp_avg, fit.exp_avg_sq = torch.zeros_like(maps), torch.zeros_like(maps)
    fit.state["step"] = 0
    again = fitting.PhotoFit(fit.maps.clone(), lr=lr, bounds=fc.BOUNDS_FIT, renderer=fc.ToyRenderer())
    assert torch.equal(fit.step(photos, table, w), again.step(photos, table, w)) and torch.equal(fit.maps, again.maps)


def test_composed_step_in_float32_is_the_restatement(lib):
    """The specification in torch ops against the test oracle in numpy: the same individually rounded float32 operations.
    exp_avg and exp_avg_sq (products and sums only) bit for bit.  The maps go through a square root, and torch's vectorised
    CPU sqrt is within 1 ulp but not correctly rounded (it differs from numpy's IEEE sqrt in under 1 % of the values): that
    moves sqrt(v') by 2^-23 relative, and each of the four roundings behind it (rsb2, + eps, the quotient, step_size) can
    then fall one ulp elsewhere, 5 * 2^-23 < 2^-20 of the update u in all; the subtraction from x adds one ulp of x'.  So
    |x' - restatement| <= 2^-20 |u| + 2^-23 |x'|, and where the update is clamped the same."""
    from svbrdf_estimation_amd import fitting, losses
    maps, photos, table, weights = _toy_problem(torch.float32)
    u = synth.uniform01(9, (2,) + tuple(maps.shape))
    m0, v0 = ((u[0] - 0.5) * 2e-3).astype(np.float32), (u[1] * 1e-5).astype(np.float32)
    for t, bounds in ((1, None), (2, fc.BOUNDS_FIT), (1000, fc.BOUNDS_FIT)):
        x = maps.clone().requires_grad_(True)
        ref = losses.PhotoLoss(fc.ToyRenderer())(x, photos, table, weights)
        ref.backward()
        want = fc.restatement(maps.numpy(), m0, v0, x.grad.numpy(), fc.library_scalars(lib, fc.LR, fc.BETA1, fc.BETA2, t),
                              bounds=bounds)
        xm, m, v = maps.clone(), torch.from_numpy(m0.copy()), torch.from_numpy(v0.copy())
        loss = fitting.composed_step(xm, m, v, t, photos, table, weights, lr=fc.LR, bounds=bounds, renderer=fc.ToyRenderer())
        assert torch.equal(loss, ref.detach())
        for got, exp, what in ((m, want[1], "exp_avg"), (v, want[2], "exp_avg_sq")):
            assert fc.same_bits(got.numpy(), exp), (t, what, fc.count_differing(got.numpy(), exp))
        free = fc.restatement(maps.numpy(), m0, v0, x.grad.numpy(), fc.library_scalars(lib, fc.LR, fc.BETA1, fc.BETA2, t))[0]
        u = np.abs(free.astype(np.float64) - maps.numpy())
        err = np.abs(xm.numpy().astype(np.float64) - want[0])
        assert (err <= 2.0 ** -20 * u + 2.0 ** -23 * np.abs(want[0])).all(), (t, err.max())

def test_photofit_rejects_bad_arguments_and_never_falls_back():
    from svbrdf_estimation_amd import _native, fitting
    maps, photos, table, _ = _toy_problem(torch.float32)
    for bad in (dict(lr=-1.0), dict(lr=float("nan")), dict(eps=-1e-8), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)),
                dict(bounds=[[0.0, 1.0]] * 11), dict(bounds=[[1.0, 0.0]] * 12), dict(bounds=[[float("nan"), 1.0]] * 12)):
        with pytest.raises(ValueError):
            fitting.PhotoFit(maps.clone(), **bad)
    with pytest.raises(ValueError):
        fitting.PhotoFit(maps[:, :9].contiguous())
    with pytest.raises(ValueError):
        fitting.PhotoFit(maps.transpose(2, 3))
    # this package's renderer computes on a ROCm device only: CPU maps are an error, never a quiet fall-back
    fit = fitting.PhotoFit(maps.clone())
    with pytest.raises(_native.NativeLibraryError):
        fit.step(photos, table)
    assert fit.state["step"] == 0


# ------------------------------------------------------------------------------------------------ the kernels

@pytest.fixture(scope="module")
def fit_asm(tmp_path_factory):
    return unit_build.compile_unit_asm(tmp_path_factory.mktemp("isa_fit"), "svbrdf_photo_fit", "SCHED_PHOTO")


@needs_hipcc
def test_fit_kernels_resources_and_scene_loops(fit_asm):
    isa_stats = _isa_stats()
    names = sorted(k for k in isa_stats.kernels(fit_asm) if "k_fit_maps" in k)
    assert len(names) == 2, names               # unweighted, weighted: forward + adjoint + update, device table
    assert not [k for k in isa_stats.kernels(fit_asm)
                if "k_photo_loss" in k or "k_head_photo" in k or "wphoto" in k or "k_exposure" in k or "k_pose" in k]
    for k in names:
        _, meta, whole, loops, ins, rng = isa_stats.analyse(fit_asm, k)
        print("%s\n   VGPRs %s, occupancy %s, %d instructions" % (k, meta["NumVgprs"], meta["Occupancy"], whole["total"]))
        assert int(meta["NumVgprs"]) <= 128 and int(meta["NumAgprs"]) == 0 and int(meta["Occupancy"]) == 4, (k, meta)
        assert int(meta["ScratchSize"]) == 0 and whole["scratch"] == 0, (k, meta)
        assert whole["v_pk"] == 0, (k, whole)
        assert not [mn for _, _, mn, _ in ins if mn and mn.startswith("flat_")], k
        # one scene loop with transcendentals per loop kind, two renders per trip, the twins' transcendental counts
        scene = sorted((c for c in loops if c["trans"]), key=lambda c: -c["valu"])
        assert len(scene) == 2, (k, [(c["valu"], c["trans"]) for c in loops])
        untied, tied = scene
        assert untied["trans"] == PHOTO_UNTIED_LOOP_TRANS and tied["trans"] == PHOTO_TIED_LOOP_TRANS, (k, scene)
        assert untied["v_div"] == 0 and tied["v_div"] == 0
        print("   tied loop %.1f VALU per pixel-render, untied %.1f" % (tied["valu"] / 2, untied["valu"] / 2))
        # the update: 12 IEEE divisions and 12 square roots behind the loops (the expansions, no bare v_rcp quotient), the
        # clamp as compares and selects
        mns = [mn for _, _, mn, _ in ins if mn]
        assert mns.count("v_div_fixup_f32") == 12 and mns.count("v_div_fmas_f32") == 12, k
        assert sum(1 for mn in mns if mn.startswith("v_sqrt_f32")) == 12, k
        # 12 gradient stores (skipped without grad_out) and the 36 of maps and state, all with the gradient stores' policy
        stores = [ops for _, _, mn, ops in ins if mn and mn.startswith("buffer_store_dword")]
        assert len(stores) == 48 and all("sc0 sc1" in s for s in stores), (k, len(stores))


@needs_hipcc
def test_makefile_builds_the_unit_into_the_library():
    unit_build.assert_makefile_builds("svbrdf_photo_fit", "SCHED_PHOTO")


def test_source_holds_no_inline_assembly_with_instructions_and_no_fma():
    # the unit and the header it owns; the photo loss's device functions come through that header
    header = unit_build.assert_includes_shared_header("svbrdf_photo_fit", "svbrdf_photo_fit_device.h")
    assert '#include "svbrdf_photo_loss_device.h"' in header
    src = unit_build.read_csrc("svbrdf_photo_fit.hip", "svbrdf_photo_fit_device.h")
    for m in re.finditer(r'asm\s+volatile\s*\(\s*"([^"]*)"', src):
        assert m.group(1) == "", "inline asm with instructions: %r" % m.group(1)
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert "fma" not in code and "rcp_" not in code and "rsq_" not in code      # the update is plain, individually rounded operations
    # the single step's epilogue stands once -- the 24 state loads between its two scheduling barriers, adam_channel, the 36
    # stores -- and fit_body calls it; fit_run_body's LDS-resident update is the only other use of adam_channel
    assert len(re.findall(r"\bvoid adam_epilogue\(", code)) == 1 and code.count("adam_epilogue(") == 2
    assert code.count("__builtin_amdgcn_sched_barrier(0)") == 2 and code.count("plane_load(mb, k)") == 2
    assert code.count("adam_channel(") == 3
    # and so do the checks of the weights and of the Adam arguments: one definition, every entry calls it
    assert "const auto bad" not in code and code.count("bounds_host[2 * k]") == 1 and code.count("adam_eps must be") == 1
    # (the weights' check is every photo entry's: svbrdf_photo_loss_device.h, tests/test_photo_loss_cpu.py)
    assert code.count("weights_check(who,") == 2 and code.count("adam_args(who,") == 2 and "int weights_check(" not in code
    assert "snprintf" not in code and "fail_as(who," in code
