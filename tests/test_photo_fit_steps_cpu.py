"""Several steps of a photo fit in one launch (csrc/svbrdf_photo_fit.hip: k_fit_run*; svbrdf_photo_fit_adam_steps;
fitting.PhotoFit.steps), everything that needs no GPU:

  * the library exports the two symbols without an ABI bump, header and binding agree, the header carries the contract
    sentence, the workspace is n times the single step's;
  * every bad argument is rejected before anything is launched, the buffers untouched;
  * PhotoFit.steps(n) on float64 CPU tensors with a plugin renderer is n x PhotoFit.step, torch.equal, for n = 1, 3, 70; CPU
    float32 maps with this package's renderer are an error that leaves the state alone;
  * the two kernels, compiled with the Makefile's flags: no scratch, no AGPRs, at most 128 VGPRs and 40 KB of LDS, the two
    scene loops inside ONE step loop that is not unrolled, IEEE division and square root, 36 stores with the single step's
    cache policy.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import photo_fit_checks as fc
import photo_fit_steps_checks as sc
import synth
import unit_build
from test_photo_loss_cpu import PHOTO_TIED_LOOP_TRANS, PHOTO_UNTIED_LOOP_TRANS, _isa_stats, needs_hipcc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from svbrdf_estimation_amd import _native
    return _native._load()


# ------------------------------------------------------------------------------------------------ the C ABI

def test_library_exports_the_steps_entries_without_an_abi_bump(lib):
    from svbrdf_estimation_amd import _native
    assert lib.svbrdf_abi_version() == 8 and _native.ABI_VERSION == 8
    with open(os.path.join(ROOT, "include", "svbrdf_hip.h")) as f:
        header = f.read()
    assert "#define SVBRDF_ABI_VERSION 8" in header and "#define SVBRDF_PHOTO_FIT_MAX_STEPS 64" in header
    assert _native.PHOTO_FIT_MAX_STEPS == sc.MAX_STEPS == 64
    for name, ret, count in ((sc.STEPS_ENTRY, "int", 24), (sc.STEPS_BYTES, "size_t", 5)):
        assert hasattr(lib, name), name
        declared = header.split("SVBRDF_API %s %s(" % (ret, name))[1].split(");")[0]
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == count == declared.count(",") + 1
    assert _native.SIGNATURES[sc.STEPS_BYTES] == (ctypes.c_size_t, [ctypes.c_int] * 5)
    # the contract sentence, in the comment of THIS entry
    text = " ".join(header.split("SVBRDF_API size_t %s(" % sc.STEPS_BYTES)[0].split("/*")[-1].replace(" * ", " ").split())
    assert ("EQUAL BIT FOR BIT to n_steps successive calls of svbrdf_photo_fit_adam_step with step = first_step + k and the "
            "same other arguments, in one kernel launch") in text
    assert "BEFORE update k" in text and 'a NaN compares as "both NaN"' in text


@pytest.mark.parametrize("dims", ((1, 1, 7, 7), (8, 9, 256, 256), (5, 2, 64, 64)))
def test_workspace_is_n_times_the_single_steps(lib, dims):
    one = lib.svbrdf_rendering_loss_workspace_bytes(*dims)
    assert one == 65 * 8
    for n in (1, 2, 5, 16, 64):
        assert getattr(lib, sc.STEPS_BYTES)(n, *dims) == n * one


def test_argument_errors_come_before_any_launch_and_touch_nothing(lib):
    """-2 for n_steps of 0 and of 65 and for first_step of 0, -4 for a workspace sized for n - 1 steps, and each error of the
    single step once: -1 null, -2 dims, eps, weight_planes, lr, adam_eps, a beta, a bound, -3 misaligned, -4 a workspace
    below one step's.  Host buffers stand in for device memory: nothing is enqueued, and not a byte of them changes."""
    fn = getattr(lib, sc.STEPS_ENTRY)
    B, S, H, N = 1, 9, 8, 4
    buf = (ctypes.c_float * 32768)()
    for i in range(len(buf)):
        buf[i] = float(i % 251)
    snapshot = bytes(buf)
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 63) & ~63
    one = lib.svbrdf_rendering_loss_workspace_bytes(B, S, H, H)
    good = np.array([[0.0, 1.0]] * 12, dtype=np.float32)
    nan, inf = float("nan"), float("inf")

    def call(maps=p, m=p + 4096, v=p + 8192, photos=p + 12288, weights=p + 20480, planes=S, scenes=p + 24576, xrow=p + 25600,
             eps=0.1, bounds=good, lr=1e-2, b1=0.9, b2=0.999, ae=1e-8, first=1, n=N, losses=p + 26624, ws=p + 40960,
             ws_bytes=None, B=B, S=S, H=H, W=H):
        barr = None if bounds is None else (ctypes.c_float * 24)(*np.asarray(bounds, np.float32).reshape(-1).tolist())
        f = ctypes.c_float
        return fn(maps, m, v, photos, weights, planes, scenes, xrow, f(eps), barr, f(lr), f(b1), f(b2), f(ae), first, n, losses,
                  ws, max(n, 1) * one if ws_bytes is None else ws_bytes, B, S, H, W, None)

    launches = lib.svbrdf_debug_launch_count()
    # what this entry adds
    assert call(n=0) == -2 and b"n_steps" in lib.svbrdf_last_error()
    assert call(n=65, ws_bytes=65 * one) == -2 and b"n_steps" in lib.svbrdf_last_error()
    assert call(n=-1) == -2
    assert call(first=0) == -2 and b"first_step" in lib.svbrdf_last_error()
    assert call(first=-5) == -2
    assert call(ws_bytes=(N - 1) * one) == -4 and b"workspace" in lib.svbrdf_last_error()
    assert call(n=64, ws_bytes=63 * one) == -4 and call(n=1, ws_bytes=0) == -4
    # the single step's, once each
    for name in ("maps", "m", "v", "photos", "scenes", "xrow", "losses", "ws"):
        assert call(**{name: None}) == -1, name
    assert call(W=H + 1) == -2 and call(B=0) == -2 and call(eps=0.0) == -2
    assert call(planes=2) == -2 and b"weight_planes" in lib.svbrdf_last_error()
    assert call(weights=None, planes=S) == -2
    for bad in (dict(lr=-1e-2), dict(lr=nan), dict(ae=-1e-8), dict(ae=inf), dict(b1=1.0), dict(b2=-0.5)):
        assert call(**bad) == -2, bad
    for k, pair in ((0, (nan, 1.0)), (11, (1.0, 0.0))):
        b = good.copy()
        b[k] = pair
        assert call(bounds=b) == -2 and b"bounds" in lib.svbrdf_last_error(), (k, pair)
    assert call(maps=p + 2) == -3 and call(weights=p + 20482) == -3 and call(losses=p + 26626) == -3 and call(ws=p + 40964) == -3
    assert call(ws_bytes=one - 8) == -4
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


@pytest.mark.parametrize("n", (1, 3, 70))
def test_photofit_steps_on_the_composed_path_is_n_times_step(n):
    """float64 CPU maps and a plugin renderer: steps(n) equals n x PhotoFit.step on a clone -- maps, both moments, the step
    counter and all n losses, torch.equal"""
    from svbrdf_estimation_amd import fitting
    maps, photos, table, weights = _toy_problem(torch.float64)
    w = weights if n != 3 else None

    def make():
        return fitting.PhotoFit(maps.clone(), lr=0.05, bounds=fc.BOUNDS_FIT, renderer=fc.ToyRenderer())

    one, many = make(), make()
    assert not many.uses_fused_kernel()
    want = torch.stack([one.step(photos, table, w) for _ in range(n)])
    got = many.steps(n, photos, table, w)
    assert got.shape == (n,) and got.dtype == torch.float64 and torch.equal(got, want)
    assert many.state["step"] == n == one.state["step"]
    assert torch.equal(many.maps, one.maps) and (many.maps != maps).any()
    assert torch.equal(many.exp_avg, one.exp_avg) and torch.equal(many.exp_avg_sq, one.exp_avg_sq)
    # and it goes on from there as step does
    assert torch.equal(many.steps(2, photos, table, w), torch.stack([one.step(photos, table, w) for _ in range(2)]))
    assert many.state["step"] == n + 2 and torch.equal(many.maps, one.maps)
    with pytest.raises(ValueError):
        many.steps(0, photos, table, w)


def test_photofit_steps_never_falls_back():
    """this package's renderer computes on a ROCm device only: CPU float32 maps are an error, as for step, and the state is
    left alone"""
    from svbrdf_estimation_amd import _native, fitting
    maps, photos, table, _ = _toy_problem(torch.float32)
    fit = fitting.PhotoFit(maps.clone())
    with pytest.raises(_native.NativeLibraryError):
        fit.steps(3, photos, table)
    assert fit.state["step"] == 0 and torch.equal(fit.maps, maps) and not fit.exp_avg.any() and not fit.exp_avg_sq.any()


# ------------------------------------------------------------------------------------------------ the kernels

@pytest.fixture(scope="module")
def fit_asm(tmp_path_factory):
    return unit_build.compile_unit_asm(tmp_path_factory.mktemp("isa_fit_steps"), "svbrdf_photo_fit", "SCHED_PHOTO")


@needs_hipcc
def test_run_kernels_resources_loops_update_and_stores(fit_asm):
    """Kernels and resources; loops; update and stores.

    The loops: "exactly two loops with transcendentals", as the single step's test has it, counts the scene loops.
    tools/isa_stats.py reports nested ranges separately, and the step loop -- which must exist, not unrolled: 12 divisions and 12 square roots in the whole
    kernel -- necessarily holds both scene loops and the update's v_sqrt / v_rcp.  So: the INNERMOST loops with
    transcendentals are exactly the two scene loops with the twins' counts and no division, and the only other loop with
    transcendentals is one loop that encloses both."""
    isa_stats = _isa_stats()
    names = sorted(k for k in isa_stats.kernels(fit_asm) if "k_fit_run" in k)
    assert len(names) == 2, names               # unweighted, weighted
    others = [k for k in isa_stats.kernels(fit_asm) if k.startswith("_Z") and "k_fit_run" not in k]
    assert sorted(k for k in others if "k_fit_maps" in k) == sorted(others) and len(others) == 2, others
    for k in names:
        for banned in ("k_fit_maps", "k_photo_loss", "k_head_photo", "wphoto", "k_exposure", "k_pose"):
            assert banned not in k, (k, banned)
        _, meta, whole, loops, ins, rng = isa_stats.analyse(fit_asm, k)
        lds = int(meta["LDSByteSize"])
        print("%s\n   VGPRs %s, AGPRs %s, SGPRs %s, LDS %d bytes, occupancy %s, %d instructions (%d VALU, %d LDS, %d VMEM)" % (
            k, meta["NumVgprs"], meta["NumAgprs"], meta.get("TotalNumSgprs"), lds, meta["Occupancy"], whole["total"], whole["valu"],
            whole["lds"], whole["vmem"]))
        # kernels and resources
        assert int(meta["ScratchSize"]) == 0 and whole["scratch"] == 0, (k, meta)
        assert int(meta["NumAgprs"]) == 0 and int(meta["NumVgprs"]) <= 128, (k, meta)
        assert lds <= 40960 and int(meta["Occupancy"]) == 4, (k, lds, meta)
        assert not [mn for _, _, mn, _ in ins if mn and mn.startswith("flat_")], k
        assert whole["v_pk"] == 0, (k, whole)
        # loops
        with_trans = [(r, c) for r, c in zip(rng, loops) if c["trans"]]
        inner = [(r, c) for r, c in with_trans if not any(o != r and r[0] <= o[0] and o[1] <= r[1] for o, _ in with_trans)]
        assert len(inner) == 2, (k, [(r, c["trans"]) for r, c in with_trans])
        (r_untied, untied), (r_tied, tied) = sorted(inner, key=lambda rc: -rc[1]["valu"])
        assert untied["trans"] == PHOTO_UNTIED_LOOP_TRANS and tied["trans"] == PHOTO_TIED_LOOP_TRANS, (k, inner)
        assert untied["v_div"] == 0 and tied["v_div"] == 0
        outer = [(r, c) for r, c in with_trans if (r, c) not in inner]
        assert len(outer) == 1, (k, [(r, c["trans"]) for r, c in with_trans])
        (a, b), step_loop = outer[0]
        assert a <= min(r_untied[0], r_tied[0]) and max(r_untied[1], r_tied[1]) <= b, (k, outer[0][0], r_untied, r_tied)
        print("   tied loop %.1f VALU per pixel-render, untied %.1f; step loop %d instructions, %d LDS" % (
            tied["valu"] / 2, untied["valu"] / 2, step_loop["total"], step_loop["lds"]))
        # update and stores: ONE copy of the update (the step loop is not unrolled), IEEE division and square root
        mns = [mn for _, _, mn, _ in ins if mn]
        assert mns.count("v_div_fixup_f32") == 12 and mns.count("v_div_fmas_f32") == 12, k
        assert sum(1 for mn in mns if mn.startswith("v_sqrt_f32")) == 12, k
        assert step_loop["v_div"] == 48                                 # and it stands inside the step loop
        stores = [(i, ops) for i, (_, _, mn, ops) in enumerate(ins) if mn and mn.startswith("buffer_store_dword")]
        assert len(stores) == 36 and all("sc0 sc1" in ops for _, ops in stores), (k, len(stores))
        assert all(i > b for i, _ in stores), k                         # once, behind the last step
        loads = [i for i, (_, _, mn, _) in enumerate(ins) if mn and mn.startswith("buffer_load_dword")]
        assert sum(1 for i in loads if i < a) == 36, k                  # and maps and state are read once, in front of the first


@needs_hipcc
def test_makefile_builds_the_kernels_into_the_library(lib):
    unit_build.assert_makefile_builds("svbrdf_photo_fit", "SCHED_PHOTO")
    from svbrdf_estimation_amd import _codehash, _native
    for name in (("k_fit_run", "AdamArgs", "RunScalars", "9k_fit_runE"), ("k_fit_run_weighted",)):
        assert _codehash.kernel_code_sha256(_native.library_path(), name)["bytes"] > 8000, name


def test_source_holds_no_inline_assembly_with_instructions_and_no_fma():
    # the header the unit owns, then the unit: the several-steps section and its entry are the unit's own
    header = unit_build.assert_includes_shared_header("svbrdf_photo_fit", "svbrdf_photo_fit_device.h")
    assert "k_fit_run" not in header and '#include "svbrdf_photo_loss_device.h"' in header
    src = unit_build.read_csrc("svbrdf_photo_fit_device.h", "svbrdf_photo_fit.hip")
    assert "k_fit_run" in src and "svbrdf_photo_fit_adam_steps" in src
    for m in re.finditer(r'asm\s+volatile\s*\(\s*"([^"]*)"', src):
        assert m.group(1) == "", "inline asm with instructions: %r" % m.group(1)
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert "fma" not in code and "rcp_" not in code and "rsq_" not in code      # the update is plain, individually rounded operations
    # no waiting between workgroups: no grid barrier, no cooperative launch, no spinning
    assert "cooperative" not in code.lower() and "grid_group" not in code and "while (" not in code
    assert "hipLaunchCooperativeKernel" not in code
    # the steps entry checks and fills through the single step's helpers, in its own wording, and keeps what is its own: the
    # range of n_steps, the overflow guard on first_step + k, the scalars behind n_steps
    entry = code[code.index("int svbrdf_photo_fit_adam_steps("):]
    for used in ("weights_check(who,", "adam_args(who, rule,", '"first_step >= 1, a finite lr >= 0 and betas in [0, 1) are required"',
                 "first_step > 0x7fffffff - k", "n_steps < 1 || n_steps > SVBRDF_PHOTO_FIT_MAX_STEPS", "run.step_size[k] = sc[2]"):
        assert used in entry, used
    assert entry.index("weights_check(") < entry.index("n_steps < 1") < entry.index("first_step > 0x7fffffff") \
        < entry.index("adam_args(") < entry.index("svbrdf_photo_fit_steps_workspace_bytes(n_steps")
    assert "bounds_host[" not in entry and "aligned(" not in entry
