"""The photo losses with the gradient towards the scene table (csrc/svbrdf_photo_pose.hip: k_pose_*; PhotoLoss and
HeadPhotoLoss with a ``[B,S,9]`` table that requires grad), everything that needs no GPU:

  * the library exports the three entry points, added to ABI version 8 without a bump, header, binding and workspace
    function agree, and bad arguments are rejected before anything is launched;
  * the composed definition's float64 table gradient (renderers.render_table through torch autograd) is the helper's G64
    (tests/pose_photo_checks.py: forward-mode duals through oracle.eager_torch) within the bound -- backward mode against
    forward mode, the package's restatement against the oracle's;
  * G64 against central differences of the same float64 loss;
  * tests/golden/g23_photo_pose.npz -- written by the reference (tests/golden/make_golden_pose_photo.py: central differences
    of its own float64 renderings) -- is what its generator describes, and the helper's G64 and the composed float64
    gradient reproduce its table gradient within the bound;
  * the composed definition with a table that does not require grad is bit-identical to K1 / K2's, as it always was;
  * the inputs the GPU tests use satisfy the bound's conditions by the comparison values alone, and the hand-made table
    covers LN+ = 0 and VN at its clamp;
  * the four kernels, compiled with the Makefile's flags: registers, no scratch, no AGPRs, the transcendental count per
    render of their twins in svbrdf_photo_loss.hip; the VALU instructions per render against the twin are printed.
"""
import ctypes
import hashlib
import json
import os
import re

import numpy as np
import pytest
import torch

import head_checks
import photo_checks
import pose_photo_checks as pc
import synth
import tolerances
import unit_build
import weighted_photo_checks as wp
from oracle import c_oracle
from test_photo_loss_cpu import PHOTO_TIED_LOOP_TRANS, PHOTO_UNTIED_LOOP_TRANS, _isa_stats, needs_hipcc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from svbrdf_estimation_amd import _native
    return _native._load()


def test_library_exports_the_scene_grad_entries_without_an_abi_bump(lib):
    from svbrdf_estimation_amd import _native
    assert lib.svbrdf_abi_version() == 8 and _native.ABI_VERSION == 8
    with open(os.path.join(ROOT, "include", "svbrdf_hip.h")) as f:
        header = f.read()
    assert "#define SVBRDF_ABI_VERSION 8" in header
    for name in pc.ENTRIES:
        assert hasattr(lib, name), name
        assert "SVBRDF_API int %s(" % name in header
        declared = header.split("SVBRDF_API int %s(" % name)[1].split(");")[0]
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == 17 == declared.count(",") + 1
    assert hasattr(lib, pc.WORKSPACE_BYTES) and "SVBRDF_API size_t %s(" % pc.WORKSPACE_BYTES in header
    assert _native.SIGNATURES[pc.WORKSPACE_BYTES] == (ctypes.c_size_t, [ctypes.c_int] * 4)
    for B, S in ((1, 1), (2, 3), (8, 9)):
        assert getattr(lib, pc.WORKSPACE_BYTES)(B, S, 8, 8) == (65 + B * S * 9) * 8
    assert "A COLOUR MUST BE FINITE AND > 0" in header and "EQUAL BIT FOR BIT" in header


@pytest.mark.parametrize("entry", pc.ENTRIES)
def test_argument_errors_come_before_any_launch(lib, entry):
    """-1 null pointers (grad_input and grad_scenes included: forward + adjoint only; weights may be null), -2 dims, eps and a
    weight_planes that does not fit `weights`, -3 misaligned, -4 workspace too small -- the exposure entries' order and
    codes.  Host buffers stand in for device memory: nothing is enqueued."""
    fn = getattr(lib, entry)
    B, S, H = 1, 9, 8
    buf = (ctypes.c_float * 28672)()
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 63) & ~63
    need = getattr(lib, pc.WORKSPACE_BYTES)(B, S, H, H)
    assert need == (65 + 81) * 8

    def call(input=p, photos=p + 256, weights=p + 16384, planes=S, scenes=p + 512, xrow=p + 1024, eps=0.1, loss=p + 2048,
             grad=p + 4096, grad_s=p + 24000, ws=p + 8192, ws_bytes=need, B=B, S=S, H=H, W=H):
        return fn(input, photos, weights, planes, scenes, xrow, ctypes.c_float(eps), loss, grad, grad_s, ws, ws_bytes, B, S, H, W,
                  None)

    launches = lib.svbrdf_debug_launch_count()
    for name in ("input", "photos", "scenes", "xrow", "loss", "grad", "grad_s", "ws"):
        assert call(**{name: None}) == -1, name
        assert lib.svbrdf_last_error()
    for planes in (0, 2, S + 1, -1):
        assert call(planes=planes) == -2, planes
        assert b"weight_planes" in lib.svbrdf_last_error()
    for planes in (1, S, 2):                                        # no weights: only 0 planes
        assert call(weights=None, planes=planes) == -2, planes
        assert b"weight_planes" in lib.svbrdf_last_error()
    assert call(W=H + 1) == -2 and call(B=0) == -2 and call(S=0, planes=1) == -2 and call(eps=0.0) == -2
    assert call(photos=p + 258) == -3 and call(grad=p + 4098) == -3 and call(scenes=p + 514) == -3
    assert call(weights=p + 16386) == -3 and call(grad_s=p + 24002) == -3 and call(ws=p + 8196) == -3
    assert call(ws_bytes=need - 8) == -4 and call(ws_bytes=lib.svbrdf_rendering_loss_workspace_bytes(B, S, H, H)) == -4
    assert call(ws_bytes=lib.svbrdf_photo_exposure_workspace_bytes(B, S, H, H)) == -4
    assert call(S=426, planes=426, ws_bytes=1 << 20) == -2          # the per-workgroup sums live in LDS
    assert lib.svbrdf_debug_launch_count() == launches              # failed calls enqueue and count nothing


# ------------------------------------------------------------------------------------------------ the definition

CPU_CASES = (("17_s2", None, False), ("17_s2", "per-photo", True), ("33_s3", "shared", False), ("33_s3", "per-photo", False))


@pytest.mark.parametrize("name,layout,head", CPU_CASES, ids=["%s-%s-%s" % (n, l or "unweighted", "head" if h else "maps")
                                                              for n, l, h in CPU_CASES])
def test_composed_float64_scene_gradient_is_the_oracles(name, layout, head):
    """renderers.render_table + the (weighted) log-L1 mean through torch's BACKWARD autograd in float64, against the helper's
    FORWARD duals through oracle.eager_torch: two restatements, two autograd modes, the same sub-gradient conventions"""
    c, R = pc.reference(name, layout, head)
    w = None if layout is None else c["weights"][layout]
    loss, g = pc.composed_scene_grad(c["enc"] if head else c["maps"], c["photos"], c["scenes"], w, head)
    tolerances.assert_loss_close(loss, R.ref.loss64, "composed float64 loss")
    R.assert_scene_grad_close(g, "%s %s %s composed float64" % (name, layout, "head" if head else "maps"))
    wb, wa = R.worst(g)
    assert wb < 0.05, (wb, wa)      # the bound is not what holds them together: the two agree to a few 1e-6 of A


def test_oracle_scene_gradient_against_central_differences():
    """G64 (forward duals) against (L(row + h e_k) - L(row - h e_k)) / 2h of the same float64 loss: differentiation by
    autograd against differentiation by nothing at all.  A sign change or a clamp that falls inside +-h moves the quotient
    by that term's share; the bound of 1e-4 A is far above that and the h^2 truncation, and far below a wrong formula."""
    import math
    from oracle import eager_torch
    c = wp.case_inputs("17_s2")
    R = pc.PoseReference(c["maps"], c["photos"], c["scenes"], pc.EPS, False, None)
    m, ph = torch.from_numpy(c["maps"]).double(), torch.from_numpy(c["photos"]).double()
    sc = c["scenes"].astype(np.float64)
    xrow = torch.from_numpy(c_oracle.make_xrow(m.shape[-1]).astype(np.float32)).double()
    args = dict(xrow=xrow, pi=float(np.float32(math.pi)), clamp_min=float(np.float32(0.001)))
    eps, h = float(np.float32(pc.EPS)), 1e-5

    def loss_of(table):
        t = torch.from_numpy(table)
        rad = torch.stack([torch.cat([eager_torch.render_scene(m[b], t[b, s], **args) for s in range(t.shape[1])], dim=0)
                           for b in range(t.shape[0])], dim=0)
        return (torch.log(rad + eps) - torch.log(ph + eps)).abs().mean().item()

    worst = 0.0
    for b, s, k in np.ndindex(*sc.shape):
        up, dn = sc.copy(), sc.copy()
        up[b, s, k] += h
        dn[b, s, k] -= h
        err = abs((loss_of(up) - loss_of(dn)) / (2 * h) - R.G64[b, s, k])
        worst = max(worst, err / R.A[b, s, k])
        assert err <= 1e-4 * R.A[b, s, k], (b, s, k, err, R.G64[b, s, k], R.A[b, s, k])
    print("[pose] forward duals vs central differences: worst err/A %.3g" % worst)


# ------------------------------------------------------------------------------------------------ the fixture

@pytest.fixture(scope="module")
def g23(golden):
    g = golden("g23_photo_pose.npz")
    B, H = int(g["B"]), int(g["H"])
    inp = synth.make_maps(int(g["input_seed"]), B, H)
    enc = head_checks.fixture_input(int(g["enc_seed"]), B, H)
    assert synth.checksum(inp) == str(g["input_sha256"]) and synth.checksum(enc) == str(g["enc_sha256"]), \
        "synthetic inputs are not bit-reproducible here"
    return g, inp, enc


def test_fixture_is_what_its_generator_describes(g23):
    g, inp, enc = g23
    ph, w = g["photos"], g["weights"]
    assert inp.shape == (3, 12, 13, 13) and enc.shape == (3, 9, 13, 13) and g["scenes"].shape == (3, 9, 9)
    assert ph.shape == (3, 9, 3, 13, 13) and w.shape == (3, 9, 13, 13) and ph.dtype == np.float32 and w.dtype == np.float32
    assert w.min() == 0.0 and w.max() == 1.0 and not np.isnan(w).any()
    row = int(g["masked_row"])
    nan = np.isnan(ph)
    assert nan.any() and nan[:, :, :, row, :].all() and (np.broadcast_to(w[:, :, None], ph.shape)[nan] == 0.0).all()
    valid = ph[~nan]
    assert valid.min() >= 0.0 and valid.max() <= 1.0 and (valid == 0.0).any() and (valid == 1.0).any()      # the clamp, both ends
    for k in ("loss", "head_loss"):
        assert g[k].dtype == np.float32 and g[k + "_f64"].dtype == np.float64 and np.isfinite(g[k]) and np.isfinite(g[k + "_f64"])
    for k, like in (("grad_input", inp), ("grad9", enc)):
        assert g[k].dtype == np.float32 and g[k + "_f64"].dtype == np.float64 and g[k].shape == like.shape == g[k + "_f64"].shape
        assert np.isfinite(g[k]).all() and np.isfinite(g[k + "_f64"]).all() and g[k].any()
    for k in ("grad_scenes_f64", "scene_A", "scene_T", "head_grad_scenes_f64", "head_scene_A", "head_scene_T"):
        assert g[k].dtype == np.float64 and g[k].shape == (3, 9, 9) and np.isfinite(g[k]).all()
    assert g["grad_scenes_f64"].all() and (g["scene_A"] >= np.abs(g["grad_scenes_f64"])).all() and (g["scene_T"] >= 0).all()
    assert 0 < float(g["h_step"]) <= 1e-4
    gdir = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gdir, "MANIFEST_g23_photo_pose.json")) as f:
        entry = json.load(f)["fixtures"]["g23_photo_pose.npz"]
    assert entry["generator"] == "tests/golden/make_golden_pose_photo.py" and os.path.exists(os.path.join(ROOT, entry["generator"]))
    with open(os.path.join(gdir, "g23_photo_pose.npz"), "rb") as f:
        data = f.read()
    assert hashlib.sha256(data).hexdigest() == entry["sha256"] and len(data) <= 1 << 20


@pytest.mark.parametrize("head", [False, True], ids=["maps", "head"])
def test_oracle_and_composed_definition_reproduce_the_reference_fixture(g23, head):
    """the reference differentiates nothing towards its scenes: g23 holds central differences of its float64 renderings.  The
    helper's forward duals, its float32 evaluation and the package's composed float64 definition (backward autograd of
    renderers.render_table) all land inside the bound around them; A and T agree with the fixture's own"""
    g, inp, enc = g23
    R = pc.PoseReference(enc if head else inp, g["photos"], g["scenes"], float(g["eps"]), head, g["weights"])
    pre = "head_" if head else ""
    ref = R.ref
    loss, loss64 = (g["head_loss"], g["head_loss_f64"]) if head else (g["loss"], g["loss_f64"])
    grad, grad64 = (g["grad9"], g["grad9_f64"]) if head else (g["grad_input"], g["grad_input_f64"])
    gs64 = g[pre + "grad_scenes_f64"]
    print("[pose] g23 %s: fixture loss %.9g (f64 %.12g), oracle %.9g (f64 %.12g); %d tie pixels, %d tied terms, %d sign flips" % (
        "head" if head else "maps", float(loss), float(loss64), ref.loss, ref.loss64, ref.n_ties(), R.tied_terms, R.sign_flips))
    assert ref.n_ties() <= tolerances.MAX_TIE_PIXELS and R.tied_terms <= tolerances.MAX_TIE_PIXELS and R.sign_flips == 0
    tolerances.assert_loss_close(ref.loss, loss, "oracle fp32 vs reference fp32")
    tolerances.assert_loss_close(ref.loss64, loss64, "oracle fp64 vs reference fp64")
    what = "g23 %s" % ("head" if head else "maps")
    photo_checks.assert_photo_grad_close(ref.grad, grad, grad64, ref.tie, what + " oracle vs reference")
    assert np.allclose(R.A, g[pre + "scene_A"], rtol=1e-5, atol=0.0) and np.allclose(R.T, g[pre + "scene_T"], rtol=1e-3, atol=1e-12)
    R.assert_scene_grad_close(gs64, what + " reference's central differences vs the duals")
    R.assert_scene_grad_close(R.G32, what + " fp32 evaluation vs the duals")
    closs, cg = pc.composed_scene_grad(enc if head else inp, g["photos"], g["scenes"], g["weights"], head, float(g["eps"]))
    tolerances.assert_loss_close(closs, loss64, "composed float64 vs reference fp64")
    err = np.abs(cg - gs64)
    print("[pose] %s composed float64 vs the reference's central differences: worst err/bound %.3g" % (what, float((err / R.bound).max())))
    assert (err <= R.bound).all()
    R.assert_scene_grad_close(cg, what + " composed float64 vs the duals")


def test_table_without_grad_takes_k1_k2_as_before(monkeypatch):
    """composed_photo_loss with a table that does not require grad (or under no_grad) never reaches render_table: the
    renderings come from renderers._RenderFunction, whatever it returns, bit for bit"""
    from svbrdf_estimation_amd import losses, renderers
    B, S, H = 2, 3, 8
    calls = []

    class _Recorded:
        @staticmethod
        def apply(maps, scenes):
            calls.append("K1")
            return maps[:, None, 3:6] * scenes[:, :, 6:9, None, None] + 0.25

    def _never(*a):
        raise AssertionError("render_table reached without a table gradient")

    monkeypatch.setattr(renderers, "_RenderFunction", _Recorded)
    monkeypatch.setattr(renderers, "render_table", _never)
    torch.manual_seed(3)
    x, table, photos = torch.rand(B, 12, H, H, requires_grad=True), torch.rand(B, S, 9) + 0.5, torch.rand(B, S, 3, H, H)
    want = torch.nn.functional.l1_loss(torch.log(_Recorded.apply(x, table) + 0.1), torch.log(photos + 0.1))
    got = losses.composed_photo_loss(x, photos, table, 0.1)
    assert torch.equal(got, want) and calls == ["K1", "K1"]
    with torch.no_grad():
        assert torch.equal(losses.composed_photo_loss(x, photos, table.clone().requires_grad_(True), 0.1), want)
    monkeypatch.undo()
    leaf = table.clone().requires_grad_(True)
    out = losses.composed_photo_loss(x.detach().double(), photos, leaf, 0.1)          # now the torch-op render: CPU is fine
    out.backward()
    assert out.dtype == torch.float64 and leaf.grad.dtype == torch.float32 and leaf.grad.abs().min() > 0


def test_render_table_is_the_eager_oracles_render():
    """renderers.render_table against oracle.eager_torch.render_scene per scene, float64: the same ops in the same order up to
    the broadcast layout -- 1e-12 relative"""
    from oracle import eager_torch
    from svbrdf_estimation_amd import renderers
    c = wp.case_inputs("17_s2")
    maps, table = torch.from_numpy(c["maps"]).double(), torch.from_numpy(c["scenes"]).double()
    got = renderers.render_table(maps, table)
    xrow = torch.from_numpy(c_oracle.make_xrow(maps.shape[-1]).astype(np.float32)).double()
    want = torch.stack([torch.cat([eager_torch.render_scene(maps[b], table[b, s], xrow=xrow) for s in range(table.shape[1])], dim=0)
                        for b in range(maps.shape[0])], dim=0)
    assert got.shape == want.shape and got.dtype == torch.float64
    assert torch.allclose(got, want, rtol=1e-12, atol=0.0)
    with pytest.raises(ValueError):
        renderers.render_table(maps[:, :9], table)
    with pytest.raises(ValueError):
        renderers.render_table(maps, table[:1])


def test_gpu_cases_satisfy_the_bounds_conditions_by_the_comparison_values_alone():
    """tied terms within the cap and no sign flip outside them, fp32 against fp64 evaluation of the same torch ops, for every
    input tests/test_gpu_pose_photo_loss.py compares; the fp32 evaluation itself is far inside the bound"""
    cases = [(name, layout, head) for name, _, _, _, tied in wp.CASES for layout in pc.LAYOUTS
             for head in ((False, True) if tied else (False,))]
    worst = 0.0
    for name, layout, head in cases:
        c, R = pc.reference(name, layout, head)
        wb, wa = R.worst(R.G32)
        worst = max(worst, wb)
        print("[pose] %s %s %s: %d tie pixels, %d tied terms, %d sign flips; fp32 evaluation err/bound %.3g err/A %.3g; "
              "max A positions %.3g colours %.3g" % (name, layout, "head" if head else "maps", R.ref.n_ties(), R.tied_terms,
                                                      R.sign_flips, wb, wa, R.A[..., :6].max(), R.A[..., 6:].max()))
        assert R.ref.n_ties() <= tolerances.MAX_TIE_PIXELS and R.tied_terms <= tolerances.MAX_TIE_PIXELS, (name, layout, head)
        assert R.sign_flips == 0, (name, layout, head)
        R.assert_scene_grad_close(R.G32, "%s %s fp32 evaluation" % (name, layout))
    for layout, head in pc.BIG_PARAMS:
        c, R = pc.big_case(layout, head)
        assert R.ref.n_ties() <= tolerances.MAX_TIE_PIXELS and R.tied_terms <= tolerances.MAX_TIE_PIXELS and R.sign_flips == 0
        R.assert_scene_grad_close(R.G32, "%s %s %s fp32 evaluation" % (c["name"], layout, "head" if head else "maps"))
    c, loss64, wave_sum = pc.overflow_case()
    assert np.isfinite(loss64) and wave_sum > 16 * pc.WAVE_LIMIT            # finite terms, far beyond the kernels' limit
    c, R, n_dark, n_grazing = pc.edge_case()
    assert n_dark > 50 and n_grazing > 50 and R.tied_terms <= tolerances.MAX_TIE_PIXELS and R.sign_flips == 0
    R.assert_scene_grad_close(R.G32, "17_edge fp32 evaluation")
    print("[pose] worst fp32 evaluation err/bound over the cases: %.3g" % worst)


def test_a_cpu_table_that_requires_grad_is_no_quiet_fallback():
    from svbrdf_estimation_amd import _native, losses, renderers
    x, photos = torch.rand(1, 12, 8, 8), torch.rand(1, 2, 3, 8, 8)
    table = (torch.rand(1, 2, 9) + 0.5).requires_grad_(True)
    with pytest.raises(_native.NativeLibraryError):
        losses.PhotoLoss(renderers.LocalRenderer())(x, photos, table)
    with pytest.raises(ValueError):
        _native.photo_loss(x, photos, table, want_scene_grad=True, exposure=torch.ones(1, 2, 3))


# ------------------------------------------------------------------------------------------------ the kernels

@pytest.fixture(scope="module")
def pose_asm(tmp_path_factory):
    return unit_build.compile_unit_asm(tmp_path_factory.mktemp("isa_pose"), "svbrdf_photo_pose", "SCHED_PHOTO")


@needs_hipcc
def test_pose_kernels_resources_and_scene_loops(pose_asm):
    isa_stats = _isa_stats()
    names = sorted(k for k in isa_stats.kernels(pose_asm) if "k_pose" in k)
    assert len(names) == 4, names               # {maps, head} x {unweighted, weighted}: forward + adjoint, device table
    assert not [k for k in isa_stats.kernels(pose_asm)
                if "k_photo_loss" in k or "k_head_photo" in k or "wphoto" in k or "k_exposure" in k]
    for k in names:
        head = "k_pose_head" in k
        _, meta, whole, loops, ins, rng = isa_stats.analyse(pose_asm, k)
        scene = sorted((c for c in loops if c["trans"] >= PHOTO_TIED_LOOP_TRANS // 2), key=lambda c: -c["valu"])
        print("%s\n   VGPRs %s, occupancy %s, %d instructions" % (k, meta["NumVgprs"], meta["Occupancy"], whole["total"]))
        assert int(meta["NumVgprs"]) <= 128 and int(meta["NumAgprs"]) == 0 and int(meta["Occupancy"]) >= 4, (k, meta)
        assert int(meta["ScratchSize"]) == 0 and whole["scratch"] == 0, (k, meta)
        assert whole["v_div"] == 0 and whole["v_pk"] == 0, (k, whole)
        assert not [mn for _, _, mn, _ in ins if mn and mn.startswith("flat_")], k       # LDS and global, never generic
        # one render per trip here, two per trip in the twins: the transcendental count per render is the twin's -- the
        # three lengths pose_bwd needs are the rsq seeds geometry() already forms
        assert len(scene) == (1 if head else 2), (k, [(c["valu"], c["trans"]) for c in loops])
        trans = [PHOTO_TIED_LOOP_TRANS // 2] if head else [PHOTO_UNTIED_LOOP_TRANS // 2, PHOTO_TIED_LOOP_TRANS // 2]
        for c, tr, which in zip(scene, trans, ["tied"] if head else ["untied", "tied"]):
            print("   %s loop: %d VALU per render, %d transcendental" % (which, c["valu"], c["trans"]))
            assert c["trans"] <= tr, (k, which, c["trans"])
        stores = [ops for _, _, mn, ops in ins if mn and mn.startswith("buffer_store_dword")]
        assert len(stores) == (9 if head else 12) and all("sc0 sc1" in s for s in stores), (k, stores)
        # the hand-off: 64-bit agent-scope atomics on both sides, adds that return (waited for) and exchanges
        atom = [(mn, ops) for _, _, mn, ops in ins if mn and mn.startswith("global_atomic")]
        assert any(mn == "global_atomic_add_x2" for mn, _ in atom) and any(mn == "global_atomic_swap_x2" for mn, _ in atom)
        assert all("sc0" in ops for mn, ops in atom if mn in ("global_atomic_add_x2", "global_atomic_swap_x2")), atom


@needs_hipcc
def test_makefile_builds_the_unit_into_the_library():
    unit_build.assert_makefile_builds("svbrdf_photo_pose", "SCHED_PHOTO")


def test_source_holds_no_inline_assembly_with_instructions():
    for m in re.finditer(r'asm\s+volatile\s*\(\s*"([^"]*)"', unit_build.read_csrc("svbrdf_photo_pose.hip", "svbrdf_photo_pose_device.h")):
        assert m.group(1) == "", "inline asm with instructions: %r" % m.group(1)
    # its own device code in its header, the photo loss's through that header: no kernel and no entry point in either
    header = unit_build.assert_includes_shared_header("svbrdf_photo_pose", "svbrdf_photo_pose_device.h")
    assert '#include "svbrdf_photo_loss_device.h"' in header
    unit_build.assert_includes_shared_header("svbrdf_photo_loss", "svbrdf_photo_loss_device.h")
