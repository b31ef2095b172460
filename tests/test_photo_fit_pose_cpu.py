"""One step of a photo fit WITH the scene table's gradient in one launch (csrc/svbrdf_photo_fit_pose.hip: k_joint_fit*;
svbrdf_photo_fit_adam_step_scene_grad; fitting.PhotoFit.step with a table or an exposure that requires grad), everything
that needs no GPU:

  * the library exports the entry without an ABI bump, header and binding agree, and every bad argument is rejected
    before anything is launched, the buffers untouched;
  * the two kernels, compiled with the Makefile's flags: registers, no scratch, occupancy 4, the pose twins' scene loops,
    the fit twins' update (IEEE division and square root, 48 stores with the gradient stores' policy), their names, and
    the unit's place in the Makefile;
  * fitting.PhotoFit on float64 CPU tensors (the composed path) with a table leaf and with exposure=log_e.exp() is
    PhotoLoss + torch.optim.Adam(foreach=False) + clamp_ over 5 steps to 1e-12: maps, state, every loss, every table.grad
    and log_e.grad;
  * without anything that requires grad, and under no_grad, the loss does not require grad; the maps never get a .grad.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import photo_fit_checks as fc
import photo_fit_pose_checks as jc
import synth
import unit_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = "svbrdf_photo_fit_pose"
HEADER = "svbrdf_photo_fit_pose_device.h"     # joint_body: the unit owns it, and the smooth unit includes it too
needs_hipcc = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs /opt/rocm/bin/hipcc (cross-compiles gfx950)")
# per render (the pose loops shade one render per trip): tests/test_photo_loss_cpu.py's counts per two renders, halved
TIED_LOOP_TRANS, UNTIED_LOOP_TRANS = 10, 18
OTHER_KERNELS = ("k_photo_loss", "k_head_photo", "wphoto", "k_exposure", "k_pose", "k_fit_maps", "k_fit_run")


@pytest.fixture(scope="module")
def lib():
    from svbrdf_estimation_amd import _native
    return _native._load()


# ------------------------------------------------------------------------------------------------ the C ABI

def test_library_exports_the_entry_without_an_abi_bump(lib):
    from svbrdf_estimation_amd import _native
    assert lib.svbrdf_abi_version() == 8 and _native.ABI_VERSION == 8
    with open(os.path.join(ROOT, "include", "svbrdf_hip.h")) as f:
        header = f.read()
    assert "#define SVBRDF_ABI_VERSION 8" in header
    assert hasattr(lib, jc.JOINT_ENTRY)
    declared = header.split("SVBRDF_API int %s(" % jc.JOINT_ENTRY)[1].split(");")[0]
    assert jc.JOINT_ENTRY in _native.SIGNATURES
    assert len(_native.SIGNATURES[jc.JOINT_ENTRY][1]) == 25 == declared.count(",") + 1
    # svbrdf_photo_fit_adam_step's list with grad_scenes behind grad_out
    fit = header.split("SVBRDF_API int %s(" % fc.STEP_ENTRY)[1].split(");")[0]
    names = lambda text: [a.split()[-1].lstrip("*") for a in text.replace("\n", " ").split(",")]
    assert names(declared) == names(fit)[:17] + ["grad_scenes"] + names(fit)[17:]


def test_argument_errors_come_before_any_launch_and_touch_nothing(lib):
    """The union of the two entries' checks: -1 null pointers (grad_scenes is REQUIRED; weights, bounds and grad_out may be
    null), -2 dims, eps, weight_planes, an S beyond the LDS limit, step < 1, lr or adam_eps negative or not finite, a beta
    outside [0, 1), a NaN bound or lo > hi, -3 misaligned, -4 workspace too small.  Host buffers stand in for device memory:
    nothing is enqueued, and not a byte of them changes."""
    fn = getattr(lib, jc.JOINT_ENTRY)
    B, S, H = 1, 9, 8
    buf = (ctypes.c_float * 32768)()
    for i in range(len(buf)):
        buf[i] = float(i % 251)
    snapshot = bytes(buf)
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 63) & ~63
    need = getattr(lib, jc.WORKSPACE_BYTES)(B, S, H, H)
    assert need == (65 + 81) * 8
    good = np.array([[0.0, 1.0]] * 12, dtype=np.float32)
    nan, inf = float("nan"), float("inf")

    def call(maps=p, m=p + 4096, v=p + 8192, photos=p + 12288, weights=p + 20480, planes=S, scenes=p + 24576, xrow=p + 25600,
             eps=0.1, bounds=good, lr=1e-2, b1=0.9, b2=0.999, ae=1e-8, step=1, loss=p + 26624, grad=p + 28672, grad_s=p + 36864,
             ws=p + 40960, ws_bytes=need, B=B, S=S, H=H, W=H):
        barr = None if bounds is None else (ctypes.c_float * 24)(*np.asarray(bounds, np.float32).reshape(-1).tolist())
        f = ctypes.c_float
        return fn(maps, m, v, photos, weights, planes, scenes, xrow, f(eps), barr, f(lr), f(b1), f(b2), f(ae), step, loss, grad,
                  grad_s, ws, ws_bytes, B, S, H, W, None)

    launches = lib.svbrdf_debug_launch_count()
    for name in ("maps", "m", "v", "photos", "scenes", "xrow", "loss", "grad_s", "ws"):
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
    assert call(grad_s=p + 36866) == -3
    # the workspace is the scene-gradient entry's: one byte (and one word) short of it, and the smaller ones of the others
    assert call(ws_bytes=need - 1) == -4 and call(ws_bytes=need - 8) == -4
    assert call(ws_bytes=lib.svbrdf_rendering_loss_workspace_bytes(B, S, H, H)) == -4
    # the per-workgroup sums live in LDS: the scene-gradient entry's limit, and this entry's own (six more words per thread)
    for big in (426, 384):
        assert call(S=big, planes=big, ws_bytes=1 << 20) == -2, big
        assert b"too many scenes" in lib.svbrdf_last_error()
    assert call(grad=None, weights=None, planes=0, bounds=None, ws_bytes=need - 1) == -4      # what may be null, may
    assert lib.svbrdf_debug_launch_count() == launches              # failed calls enqueue and count nothing
    assert bytes(buf) == snapshot


# ------------------------------------------------------------------------------------------------ the Python layer

class _AsOnADevice:
    """The composed definition of PhotoLoss with this package's LocalRenderer -- composed_photo_loss, and with a table
    that requires grad renderers.render_table, stock torch ops -- runs on any device; what keeps CPU tensors away from it
    is the check in front (losses._check_fused_photo_inputs: "needs a ROCm device").  These tests stand in for a device by
    answering that check as float64 maps on a device answer it: "take the composed definition"."""

    def __init__(self, monkeypatch):
        from svbrdf_estimation_amd import losses
        monkeypatch.setattr(losses, "_check_fused_photo_inputs", lambda *a: True)


def _toy_problem(dtype):
    from svbrdf_estimation_amd import environment
    B, S, H = 2, 3, 8
    maps = torch.from_numpy(synth.make_maps(41, B, H)).to(dtype)
    torch.manual_seed(5)
    table = torch.stack([environment.scene_table(1, S - 1) for _ in range(B)])
    photos = (torch.rand(B, S, 3, H, H) * 0.2).to(dtype)
    weights = torch.from_numpy(fc.wp.weight_field(77, B, S, H))
    return maps, photos, table, weights


@pytest.mark.parametrize("with_exposure", (False, True), ids=("table", "table+exposure"))
@pytest.mark.parametrize("weighted", (False, True), ids=("unweighted", "weighted"))
def test_photofit_float64_cpu_with_a_table_leaf_is_photoloss_adam_clamp(monkeypatch, weighted, with_exposure):
    """5 steps of PhotoFit.step (the composed path: CPU, float64) with a table leaf that goes through
    renderers.render_table, plus loss.backward(), against PhotoLoss + torch.optim.Adam(foreach=False) on the maps +
    x[:, 3:].clamp_(0, 1) from the same start: maps, exp_avg, exp_avg_sq, every loss and every table.grad to 1e-12 (the
    tolerance of test_photofit_float64_cpu_is_photoloss_adam_clamp); with exposure=log_e.exp() also log_e.grad.  The
    table and log e move a little after every step, by the same rule on both sides."""
    from svbrdf_estimation_amd import fitting, losses, renderers
    _AsOnADevice(monkeypatch)
    maps, photos, table, weights = _toy_problem(torch.float64)
    w = weights if weighted else None
    lr = 0.05
    reached = []
    real = renderers.render_table
    monkeypatch.setattr(renderers, "render_table", lambda *a: (reached.append(1), real(*a))[1])

    def leaves():
        t = table.clone().requires_grad_(True)
        le = (torch.linspace(-0.3, 0.3, table.shape[0] * table.shape[1] * 3, dtype=torch.float64).reshape(2, 3, 3)
              .clone().requires_grad_(True)) if with_exposure else None
        return t, le

    def nudge(t, le):
        with torch.no_grad():
            t -= 0.01 * t.grad
            if le is not None:
                le -= 0.01 * le.grad
        t.grad = None
        if le is not None:
            le.grad = None

    fit = fitting.PhotoFit(maps.clone(), lr=lr, bounds=fc.BOUNDS_FIT)
    assert not fit.uses_fused_kernel()
    t_fit, le_fit = leaves()
    x = maps.clone().requires_grad_(True)
    t_ref, le_ref = leaves()
    opt = torch.optim.Adam([x], lr=lr, foreach=False)
    fn = losses.PhotoLoss(renderers.LocalRenderer())
    for step in range(5):
        opt.zero_grad(set_to_none=True)
        ref = fn(x, photos, t_ref, w, None if le_ref is None else le_ref.exp())
        ref.backward()
        opt.step()
        with torch.no_grad():
            x[:, 3:].clamp_(0.0, 1.0)
        n = len(reached)
        loss = fit.step(photos, t_fit, w, exposure=None if le_fit is None else le_fit.exp())
        assert len(reached) == n + 1                                # the table leaf went through render_table
        assert loss.dim() == 0 and loss.dtype == torch.float64 and loss.requires_grad
        assert abs(loss.item() - ref.item()) <= 1e-12
        assert (fit.maps - x.detach()).abs().max().item() <= 1e-12, step        # updated when step returns
        assert t_fit.grad is None
        loss.backward()
        assert t_fit.grad.dtype == t_ref.grad.dtype == torch.float32 and t_ref.grad.abs().max() > 0
        assert (t_fit.grad.double() - t_ref.grad.double()).abs().max().item() <= 1e-12, step
        if with_exposure:
            assert le_ref.grad.abs().max() > 0 and (le_fit.grad - le_ref.grad).abs().max().item() <= 1e-12, step
        with pytest.raises(RuntimeError):
            loss.backward()                                         # the graph is gone, as any loss's
        nudge(t_fit, le_fit)
        nudge(t_ref, le_ref)
    st = opt.state[x]
    assert fit.state["step"] == 5 == int(st["step"]) and fit.maps.grad is None
    assert (fit.exp_avg - st["exp_avg"]).abs().max().item() <= 1e-12 and (fit.exp_avg_sq - st["exp_avg_sq"]).abs().max().item() <= 1e-12
    assert (x.detach() != maps).any() and not torch.equal(t_fit.detach(), table)


def test_the_loss_is_once_differentiable_and_never_reaches_the_maps(monkeypatch):
    from svbrdf_estimation_amd import fitting
    _AsOnADevice(monkeypatch)
    maps, photos, table, _ = _toy_problem(torch.float64)
    leaf = maps.clone().requires_grad_(True)                        # a leaf that requires grad is updated through .data
    fit = fitting.PhotoFit(leaf, lr=0.05, bounds=fc.BOUNDS_FIT)
    t = table.clone().requires_grad_(True)
    loss = fit.step(photos, t)
    g, = torch.autograd.grad(loss, t, create_graph=True)
    assert leaf.grad is None and g.abs().max() > 0
    with pytest.raises(RuntimeError):
        g.sum().backward()                                          # once differentiable: a double backward raises
    # composed_step, the specification, the same way
    x, m, v = maps.clone(), torch.zeros_like(maps), torch.zeros_like(maps)
    loss = fitting.composed_step(x, m, v, 1, photos, t, lr=0.05, bounds=fc.BOUNDS_FIT)
    assert loss.requires_grad and not torch.equal(x, maps)
    loss.backward()
    assert t.grad is not None and x.grad is None


def test_without_a_gradient_wanted_the_loss_is_detached():
    """a plain table, a table leaf under no_grad, steps(): the returned loss does not require grad and the maps' leaf never
    receives a .grad.  (With a plugin renderer, which renders on the CPU whatever requires grad; it works with scene objects
    and has no table gradient, as in PhotoLoss -- its gains have theirs.)"""
    from svbrdf_estimation_amd import fitting
    maps, photos, table, weights = _toy_problem(torch.float64)
    leaf = maps.clone().requires_grad_(True)
    fit = fitting.PhotoFit(leaf, lr=0.05, bounds=fc.BOUNDS_FIT, renderer=fc.ToyRenderer())
    t = table.clone().requires_grad_(True)
    log_e = torch.zeros(2, 3, 3, dtype=torch.float64, requires_grad=True)
    plain = fit.step(photos, table, weights, exposure=log_e.detach().exp())
    with torch.no_grad():
        quiet = fit.step(photos, t, weights, exposure=log_e.exp())
    several = fit.steps(2, photos, t, weights, exposure=log_e.exp())
    assert not plain.requires_grad and not quiet.requires_grad and not several.requires_grad and several.shape == (2,)
    assert fit.state["step"] == 4 and leaf.grad is None and t.grad is None and log_e.grad is None
    loss = fit.step(photos, t, weights, exposure=log_e.exp())
    assert loss.requires_grad
    loss.backward()
    assert leaf.grad is None and log_e.grad is not None
    assert t.grad is None


def test_a_cpu_table_that_requires_grad_is_no_quiet_fallback():
    """this package's renderer computes on a ROCm device only (test_a_cpu_table_that_requires_grad_is_no_quiet_fallback of
    tests/test_pose_photo_loss_cpu.py): CPU float32 maps with a table leaf are an error, and nothing was updated"""
    from svbrdf_estimation_amd import _native, fitting
    x, photos = torch.rand(1, 12, 8, 8), torch.rand(1, 2, 3, 8, 8)
    table = (torch.rand(1, 2, 9) + 0.5).requires_grad_(True)
    fit = fitting.PhotoFit(x.clone())
    with pytest.raises(_native.NativeLibraryError):
        fit.step(photos, table)
    with pytest.raises(_native.NativeLibraryError):
        fit.step(photos, table.detach(), exposure=torch.ones(1, 2, 3, requires_grad=True))
    assert fit.state["step"] == 0 and torch.equal(fit.maps, x) and not fit.exp_avg.any()
    with pytest.raises(_native.NativeLibraryError):
        _native.photo_fit_adam_step(x, x.clone(), x.clone(), photos, table.detach(), 1, want_scene_grad=True)


# ------------------------------------------------------------------------------------------------ the kernels

def _isa_stats():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_stats
    return isa_stats


@pytest.fixture(scope="module")
def joint_asm(tmp_path_factory):
    return unit_build.compile_unit_asm(tmp_path_factory.mktemp("isa_joint"), UNIT, "SCHED_PHOTO")


@needs_hipcc
def test_joint_kernels_resources_scene_loops_and_update(joint_asm):
    isa_stats = _isa_stats()
    names = sorted(k for k in isa_stats.kernels(joint_asm) if "__hip_cuid" not in k)
    assert len(names) == 2 and all("k_joint_fit" in k for k in names), names    # unweighted, weighted; nothing else in the unit
    assert not [k for k in names if any(s in k for s in OTHER_KERNELS)], names
    for k in names:
        _, meta, whole, loops, ins, rng = isa_stats.analyse(joint_asm, k)
        print("%s\n   VGPRs %s, occupancy %s, LDS %s bytes + 16 (9 + 9 S), %d instructions" % (
            k, meta["NumVgprs"], meta["Occupancy"], meta["LDSByteSize"], whole["total"]))
        assert int(meta["NumVgprs"]) <= 128 and int(meta["NumAgprs"]) == 0 and int(meta["Occupancy"]) == 4, (k, meta)
        assert int(meta["ScratchSize"]) == 0 and whole["scratch"] == 0, (k, meta)
        assert whole["v_pk"] == 0, (k, whole)
        assert not [mn for _, _, mn, _ in ins if mn and mn.startswith("flat_")], k
        # the two scene loops of the pose twins, one render per trip, with their transcendental counts
        scene = sorted((c for c in loops if c["trans"] >= TIED_LOOP_TRANS // 2), key=lambda c: -c["valu"])
        assert len(scene) == 2, (k, [(c["valu"], c["trans"]) for c in loops])
        for c, tr, which in zip(scene, (UNTIED_LOOP_TRANS, TIED_LOOP_TRANS), ("untied", "tied")):
            print("   %s loop: %d VALU per pixel-render, %d transcendental" % (which, c["valu"], c["trans"]))
            assert 0 < c["trans"] <= tr and c["v_div"] == 0, (k, which, c["trans"], c["v_div"])
        # the update behind the loops: 12 IEEE divisions and 12 square roots (the expansions, no bare v_rcp quotient)
        mns = [mn for _, _, mn, _ in ins if mn]
        assert mns.count("v_div_fixup_f32") == 12 and mns.count("v_div_fmas_f32") == 12, k
        assert sum(1 for mn in mns if mn.startswith("v_sqrt_f32")) == 12, k
        # 12 gradient stores (skipped without grad_out) and the 36 of maps and state, all with the gradient stores' policy
        stores = [ops for _, _, mn, ops in ins if mn and mn.startswith("buffer_store_dword")]
        assert len(stores) == 48 and all("sc0 sc1" in s for s in stores), (k, len(stores))
        # the pose twins' hand-off: 64-bit agent-scope atomics on both sides, adds that return and exchanges
        atom = [(mn, ops) for _, _, mn, ops in ins if mn and mn.startswith("global_atomic")]
        assert any(mn == "global_atomic_add_x2" for mn, _ in atom) and any(mn == "global_atomic_swap_x2" for mn, _ in atom)
        assert all("sc0" in ops for mn, ops in atom if mn in ("global_atomic_add_x2", "global_atomic_swap_x2")), atom


@needs_hipcc
def test_makefile_builds_the_unit_into_the_library():
    unit_build.assert_makefile_builds(UNIT, "SCHED_PHOTO")
    assert "-ffp-contract=off" in unit_build.make_var("HIPFLAGS")


def test_source_reuses_the_two_units_and_restates_no_arithmetic():
    """no inline assembly with instructions, no cooperative launch; the pose loop and the update are the two units' own,
    shared through their headers, which hold no kernel and no entry point"""
    header = unit_build.assert_includes_shared_header(UNIT, HEADER)
    src = unit_build.read_csrc(HEADER, UNIT + ".hip")
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert not re.search(r"\basm\b", code) and "Cooperative" not in code and "grid_group" not in code
    assert '#include "svbrdf_photo_pose_device.h"\n#include "svbrdf_photo_fit_device.h"' in header
    for used in ("pose_scene_loop<1, WEIGHTED>", "pose_scene_loop<3, WEIGHTED>", "photo_sums_finish<true>", "adam_epilogue(",
                 "adam_args(", "plan_sums(", "fit_stash(", "expo_stash(", "wave_index(", "if (wi.live)"):
        assert used in code, used
    assert "sqrtf" not in code and "fma" not in code
    # the update and the Adam-argument check are the fit unit's, called and not restated: the epilogue inside the live
    # lanes' branch, no state load or store, no scheduling barrier and no reporter of its own here
    assert re.search(r"if \(wi\.live\) \{[^}]*\badam_epilogue\(", code)
    for own in ("plane_load(mb", "plane_store(", "adam_channel(", "adam_scalars(", "sched_barrier", "const auto bad", "a.lo["):
        assert own not in code, own
    fit_src = unit_build.read_csrc("svbrdf_photo_fit_device.h", "svbrdf_photo_fit.hip")
    fit_code = "\n".join(line.split("//")[0] for line in fit_src.splitlines())
    assert (fit_code + code).count("__builtin_amdgcn_sched_barrier(0)") == 2        # the epilogue's pair, once
    assert len(re.findall(r"\bvoid adam_epilogue\(", fit_code)) == 1 and len(re.findall(r"\bint adam_args\(", fit_code)) == 1
    assert re.findall(r"SVBRDF_JOINT_KERNEL\((k_\w+),", code) == ["k_joint_fit", "k_joint_fit_weighted"]
    for unit, shared in (("svbrdf_photo_pose", "svbrdf_photo_pose_device.h"), ("svbrdf_photo_fit", "svbrdf_photo_fit_device.h")):
        unit_build.assert_includes_shared_header(unit, shared)
