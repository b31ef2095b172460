"""The photo losses with a per-photo exposure (csrc/svbrdf_photo_exposure.hip: k_exposure_*; PhotoLoss and HeadPhotoLoss with
`exposure`), everything that needs no GPU:

  * the library exports the three entry points, added to ABI version 8 without a bump, and rejects bad arguments before it
    launches anything;
  * tests/golden/g22_photo_exposure.npz -- written by the reference (tests/golden/make_golden_exposure_photo.py) -- is what
    its generator describes and is reproduced by the oracle's composition (tests/exposure_photo_checks.py) within the bound;
  * the oracle's float64 exposure gradient IS torch's float64 autograd of e * oracle.eager_torch renderings (1e-9);
  * the inputs the GPU tests use satisfy the bound's two conditions by the comparison values alone;
  * PhotoLoss / HeadPhotoLoss with a plugin renderer and an exposure ARE the composed definition bit for bit; argument checks;
  * the four kernels, compiled with the Makefile's flags: registers, no scratch, the transcendental counts of their twins
    in svbrdf_photo_loss.hip, the photo (+ weight) loads of a render back to back and a shading pass ahead of their wait,
    the gradient stores; the VALU instructions per render against the twin are printed (recorded, not capped);
  * svbrdf_photo_loss.hip compiled alone still lists exactly its sixteen kernels.
"""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import exposure_photo_checks as xp
import head_checks
import synth
import tolerances
import unit_build
import weighted_photo_checks as wp
from test_photo_loss_cpu import (PHOTO_TIED_LOOP_TRANS, PHOTO_UNTIED_LOOP_TRANS, PREFETCH_MIN_DISTANCE, _isa_stats, _ToyRenderer,
                                 needs_hipcc)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from svbrdf_estimation_amd import _native
    return _native._load()


def test_library_exports_the_exposure_entries_without_an_abi_bump(lib):
    from svbrdf_estimation_amd import _native
    assert lib.svbrdf_abi_version() == 8 and _native.ABI_VERSION == 8
    with open(os.path.join(ROOT, "include", "svbrdf_hip.h")) as f:
        header = f.read()
    assert "#define SVBRDF_ABI_VERSION 8" in header
    for name in xp.ENTRIES:
        assert hasattr(lib, name), name
        assert "SVBRDF_API int %s(" % name in header
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == 18
    assert hasattr(lib, xp.WORKSPACE_BYTES) and "SVBRDF_API size_t %s(" % xp.WORKSPACE_BYTES in header
    assert _native.SIGNATURES[xp.WORKSPACE_BYTES] == (ctypes.c_size_t, [ctypes.c_int] * 4)
    for B, S in ((1, 1), (2, 3), (8, 9)):
        assert lib.svbrdf_photo_exposure_workspace_bytes(B, S, 8, 8) == (65 + B * S * 3) * 8
    # the documented rules
    assert "EXPOSURE MUST BE FINITE AND > 0" in header and "BIT FOR" in header and "NO GRADIENT WITH RESPECT TO LIGHT OR CAMERA POSITIONS" in header


@pytest.mark.parametrize("entry", xp.ENTRIES)
def test_argument_errors_come_before_any_launch(lib, entry):
    """-1 null pointers (grad_input included: forward + adjoint only; grad_exposure and weights may be null), -2 dims, eps and
    a weight_planes that does not fit `weights`, -3 misaligned, -4 workspace too small.  Host buffers stand in for device
    memory: nothing is enqueued."""
    fn = getattr(lib, entry)
    B, S, H = 1, 9, 8
    buf = (ctypes.c_float * 20480)()
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 63) & ~63
    need = lib.svbrdf_photo_exposure_workspace_bytes(B, S, H, H)
    assert need == (65 + 27) * 8

    def call(input=p, photos=p + 256, weights=p + 16384, planes=S, exposure=p + 20000, scenes=p + 512, xrow=p + 1024, eps=0.1,
             loss=p + 2048, grad=p + 4096, grad_e=p + 24000, ws=p + 8192, ws_bytes=need, B=B, S=S, H=H, W=H):
        return fn(input, photos, weights, planes, exposure, scenes, xrow, ctypes.c_float(eps), loss, grad, grad_e, ws, ws_bytes,
                  B, S, H, W, None)

    launches = lib.svbrdf_debug_launch_count()
    for name in ("input", "photos", "exposure", "scenes", "xrow", "loss", "grad", "ws"):
        assert call(**{name: None}) == -1, name
        assert lib.svbrdf_last_error()
    for planes in (0, 2, S + 1, -1):
        assert call(planes=planes) == -2, planes
        assert b"weight_planes" in lib.svbrdf_last_error()
    for planes in (1, S, 2):                                        # no weights: only 0 planes
        assert call(weights=None, planes=planes) == -2, planes
        assert b"weight_planes" in lib.svbrdf_last_error()
    assert call(W=H + 1) == -2 and call(B=0) == -2 and call(S=0, planes=1) == -2 and call(eps=0.0) == -2
    assert call(photos=p + 258) == -3 and call(grad=p + 4098) == -3 and call(exposure=p + 20002) == -3
    assert call(weights=p + 16386) == -3 and call(grad_e=p + 24002) == -3 and call(ws=p + 8196) == -3
    assert call(ws_bytes=need - 8) == -4 and call(ws_bytes=lib.svbrdf_rendering_loss_workspace_bytes(B, S, H, H)) == -4
    assert call(S=1279, planes=1279, ws_bytes=1 << 20) == -2        # the per-workgroup sums live in LDS
    assert lib.svbrdf_debug_launch_count() == launches              # failed calls enqueue and count nothing


# ------------------------------------------------------------------------------------------------ the fixture

@pytest.fixture(scope="module")
def g22(golden):
    g = golden("g22_photo_exposure.npz")
    B, H = int(g["B"]), int(g["H"])
    inp = synth.make_maps(int(g["input_seed"]), B, H)
    enc = head_checks.fixture_input(int(g["enc_seed"]), B, H)
    assert synth.checksum(inp) == str(g["input_sha256"]) and synth.checksum(enc) == str(g["enc_sha256"]), \
        "synthetic inputs are not bit-reproducible here"
    return g, inp, enc


def test_fixture_is_what_its_generator_describes(g22):
    g, inp, enc = g22
    ph, w, e = g["photos"], g["weights"], g["exposure"]
    assert inp.shape == (3, 12, 13, 13) and enc.shape == (3, 9, 13, 13) and g["scenes"].shape == (3, 9, 9)
    assert ph.shape == (3, 9, 3, 13, 13) and w.shape == (3, 9, 13, 13) and e.shape == (3, 9, 3)
    assert ph.dtype == np.float32 and w.dtype == np.float32 and e.dtype == np.float32
    assert e.min() >= 0.5 and e.max() < 2.0 and e.max() > 1.5 and e.min() < 0.75
    assert w.min() == 0.0 and w.max() == 1.0 and not np.isnan(w).any()
    row = int(g["masked_row"])
    nan = np.isnan(ph)
    assert nan.any() and nan[:, :, :, row, :].all() and (np.broadcast_to(w[:, :, None], ph.shape)[nan] == 0.0).all()
    valid = ph[~nan]
    assert valid.min() >= 0.0 and valid.max() <= 1.0 and (valid == 0.0).any() and (valid == 1.0).any()      # the clamp, both ends
    for k in ("loss", "head_loss"):
        assert g[k].dtype == np.float32 and g[k + "_f64"].dtype == np.float64 and np.isfinite(g[k]) and np.isfinite(g[k + "_f64"])
    for k, like in (("grad_input", inp), ("grad9", enc), ("grad_exposure", e), ("head_grad_exposure", e)):
        assert g[k].dtype == np.float32 and g[k + "_f64"].dtype == np.float64 and g[k].shape == like.shape == g[k + "_f64"].shape
        assert np.isfinite(g[k]).all() and np.isfinite(g[k + "_f64"]).all() and g[k].any()
    gdir = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gdir, "MANIFEST_g22_photo_exposure.json")) as f:
        entry = json.load(f)["fixtures"]["g22_photo_exposure.npz"]
    assert entry["generator"] == "tests/golden/make_golden_exposure_photo.py" and os.path.exists(os.path.join(ROOT, entry["generator"]))
    with open(os.path.join(gdir, "g22_photo_exposure.npz"), "rb") as f:
        data = f.read()
    assert hashlib.sha256(data).hexdigest() == entry["sha256"] and len(data) <= 1 << 20


@pytest.mark.parametrize("head", [False, True], ids=["maps", "head"])
def test_oracle_composition_reproduces_the_reference_fixture(g22, head):
    """the reference multiplies its RENDERING by the gain, the oracle (like the kernels) the light colour in float32: the same
    loss, map gradient and exposure gradient within the project's bounds"""
    import photo_checks
    g, inp, enc = g22
    R = xp.ExposureReference(enc if head else inp, g["photos"], g["scenes"], g["exposure"], float(g["eps"]), head, g["weights"])
    ref = R.ref
    loss, loss64 = (g["head_loss"], g["head_loss_f64"]) if head else (g["loss"], g["loss_f64"])
    grad, grad64 = (g["grad9"], g["grad9_f64"]) if head else (g["grad_input"], g["grad_input_f64"])
    ge, ge64 = (g["head_grad_exposure"], g["head_grad_exposure_f64"]) if head else (g["grad_exposure"], g["grad_exposure_f64"])
    print("[exposure-photo] g22 %s: fixture loss %.9g (f64 %.12g), oracle %.9g (f64 %.12g); %d tie pixels, %d tied terms, "
          "%d sign flips" % ("head" if head else "maps", float(loss), float(loss64), ref.loss, ref.loss64, ref.n_ties(),
                             R.tied_terms, R.sign_flips))
    assert ref.n_ties() <= tolerances.MAX_TIE_PIXELS and R.tied_terms <= tolerances.MAX_TIE_PIXELS and R.sign_flips == 0
    tolerances.assert_loss_close(ref.loss, loss, "oracle fp32 vs reference fp32")
    tolerances.assert_loss_close(ref.loss64, loss64, "oracle fp64 vs reference fp64")
    what = "g22 %s oracle" % ("head" if head else "maps")
    photo_checks.assert_photo_grad_close(ref.grad, grad, grad64, ref.tie, what + " vs reference")
    for got, name in ((R.G32, "fp32"), (R.G64, "fp64"), (ge, "reference fp32"), (ge64, "reference fp64")):
        print("[exposure-photo]    %s exposure gradient: worst err/bound %.3g, err/A %.3g" % ((name,) + R.worst(got)))
    R.assert_exposure_grad_close(ge, what + " vs reference fp32 exposure gradient")
    R.assert_exposure_grad_close(ge64, what + " vs reference fp64 exposure gradient")
    R.assert_exposure_grad_close(R.G32, what + " fp32 vs fp64")
    # the masked row votes for no gain either: the same sums with that row's terms dropped
    assert not R.t64[:, :, :, int(g["masked_row"]), :].any()


def test_oracle_f64_gradient_is_torch_autograd_of_the_eager_renderings():
    """G64 against d/de of the definition by torch's float64 autograd of e * oracle.eager_torch renderings (the check
    tests/test_head_loss_cpu.py makes for the head; float32-valued inputs, pixel row, pi and clamps as there): 1e-9 relative
    to A.  The renderings take the colour fl32(colour e) / e, so that e times them is the rendering the kernels define -- the
    float32 product of the colour column -- and e stays the variable."""
    from oracle import eager_torch
    from svbrdf_estimation_amd import losses
    for name, layout in (("17_s2", "per-photo"), ("33_s3", None)):
        c, e, R = xp.reference(name, layout, False)
        maps = torch.from_numpy(c["maps"]).double()
        gain = torch.from_numpy(e).double().requires_grad_(True)
        table = torch.from_numpy(R.scaled).double()
        table[:, :, 6:9] /= gain.detach()
        xrow = torch.linspace(-1, 1, maps.shape[-1], dtype=torch.float32).to(torch.float64)
        args = dict(xrow=xrow, pi=float(np.float32(np.pi)), clamp_min=float(np.float32(0.001)))
        rendered = torch.stack([torch.cat([eager_torch.render_scene(maps[b], table[b, s], **args) for s in range(table.shape[1])], dim=0)
                                for b in range(maps.shape[0])], dim=0)
        assert rendered.dtype == torch.float64 and tuple(rendered.shape) == c["photos"].shape
        rendered = rendered * gain[..., None, None]
        eps = float(np.float32(xp.EPS))
        photos = torch.from_numpy(c["photos"]).double()
        if layout is None:
            loss = torch.nn.functional.l1_loss(torch.log(rendered + eps), torch.log(photos + eps))
        else:
            loss = losses.weighted_log_l1(rendered, photos, eps, torch.from_numpy(c["weights"][layout]))
        loss.backward()
        err = np.abs(gain.grad.numpy() - R.G64)
        print("[exposure-photo] %s %s: oracle fp64 loss %.15g vs torch %.15g, exposure gradient off by %.3g of A" % (
            name, layout, R.ref.loss64, loss.item(), float((err / R.A).max())))
        assert abs(R.ref.loss64 - loss.item()) <= 1e-12 * abs(loss.item())
        assert (err <= 1e-9 * R.A).all(), float((err / R.A).max())


def test_gpu_cases_satisfy_the_bounds_conditions_by_the_comparison_values_alone():
    """tied terms within the cap and no sign flip outside them, fp32 oracle against fp64 oracle, for every input
    tests/test_gpu_exposure_photo_loss.py compares; the fp32 oracle itself is far inside the bound"""
    cases = [(name, layout, head) for name, _, _, _, tied in wp.CASES for layout in xp.LAYOUTS
             for head in ((False, True) if tied else (False,))]
    worst = 0.0
    for name, layout, head in cases:
        c, e, R = xp.reference(name, layout, head)
        wb, wa = R.worst(R.G32)
        worst = max(worst, wb)
        print("[exposure-photo] %s %s %s: %d tie pixels, %d tied terms, %d sign flips; fp32 oracle err/bound %.3g err/A %.3g; "
              "min |G|/A %.2g" % (name, layout, "head" if head else "maps", R.ref.n_ties(), R.tied_terms, R.sign_flips, wb, wa,
                                  float((np.abs(R.G64) / np.where(R.A > 0, R.A, 1)).min())))
        assert e.min() >= 0.5 and e.max() < 2.0
        assert R.ref.n_ties() <= tolerances.MAX_TIE_PIXELS and R.tied_terms <= tolerances.MAX_TIE_PIXELS, (name, layout, head)
        assert R.sign_flips == 0, (name, layout, head)
        R.assert_exposure_grad_close(R.G32, "%s %s fp32 oracle" % (name, layout))
    c, e, R = xp.big_case()
    assert R.ref.n_ties() <= tolerances.MAX_TIE_PIXELS and R.tied_terms <= tolerances.MAX_TIE_PIXELS and R.sign_flips == 0
    assert worst < 0.01


# ------------------------------------------------------------------------------------------------ the modules

def _toy(head):
    from svbrdf_estimation_amd import environment
    B, S, H = 2, 3, 8
    x = torch.from_numpy(head_checks.full(33, B, H) if head else synth.make_maps(31, B, H))
    torch.manual_seed(5)
    table = torch.stack([environment.scene_table(1, S - 1) for _ in range(B)])
    photos = torch.rand(B, S, 3, H, H)
    w = torch.from_numpy(wp.weight_field(77, B, S, H))
    e = torch.from_numpy(xp.exposure_of(H, S, B))
    return x, photos, table, w, e


def _definition(x, photos, table, w, e, eps, head):
    """the specification, literally: the renderings times the gain, then the (weighted) log-L1 mean"""
    from svbrdf_estimation_amd import environment, losses
    R = _ToyRenderer()
    maps = losses.decode_head(x) if head else x
    rows = [torch.cat([R.render(sc, maps[b]) for sc in environment.scenes_from_table(table[b])], dim=0) for b in range(x.shape[0])]
    rendered = torch.stack(rows, dim=0) * e.to(x.dtype)[..., None, None]
    if w is None:
        return torch.nn.functional.l1_loss(torch.log(rendered + eps), torch.log(photos.to(rendered.dtype) + eps))
    return losses.weighted_log_l1(rendered, photos, eps, w)


@pytest.mark.parametrize("head", [False, True], ids=["PhotoLoss", "HeadPhotoLoss"])
def test_plugin_renderer_with_exposure_is_the_composed_definition_bitwise(head):
    from svbrdf_estimation_amd import losses
    x, photos, table, w, e = _toy(head)
    fn = (losses.HeadPhotoLoss if head else losses.PhotoLoss)(_ToyRenderer(), eps=0.05)
    assert not fn.uses_fused_kernel()
    for weights in (None, w):
        for gains in (e, e[:, :, :1], e[:, :, 0], e[:, :1, :1]):
            x0, e0 = x.clone().requires_grad_(True), gains.clone().requires_grad_(True)
            full = e0.unsqueeze(-1) if e0.dim() == 2 else e0
            ref = _definition(x0, photos, table, weights, full.expand(2, 3, 3), 0.05, head)
            ref.backward()
            x1, e1 = x.clone().requires_grad_(True), gains.clone().requires_grad_(True)
            loss = fn(x1, photos, table, weights, e1)
            assert loss.dim() == 0
            loss.backward()
            assert torch.equal(loss, ref) and torch.equal(x1.grad, x0.grad) and torch.equal(e1.grad, e0.grad)
            assert e1.grad.shape == gains.shape and e1.grad.abs().max() > 0
    # keyword and positional; None is the path without exposure; all ones changes nothing; float64 stays float64
    assert torch.equal(fn(x, photos, table, w, exposure=e), fn(x, photos, table, w, e))
    assert torch.equal(fn(x, photos, table, None, None), fn(x, photos, table))
    assert torch.equal(fn(x, photos, table, w, torch.ones_like(e)), fn(x, photos, table, w))
    assert fn(x.double(), photos.double(), table, w, e.double()).dtype == torch.float64
    assert fn(x, photos, table, w, e.double()).dtype == torch.float64


def test_exposure_is_checked():
    from svbrdf_estimation_amd import _native, losses, renderers
    for head in (False, True):
        x, photos, table, w, e = _toy(head)
        cls = losses.HeadPhotoLoss if head else losses.PhotoLoss
        for fn in (cls(_ToyRenderer()), cls(renderers.LocalRenderer())):
            for bad in (e[:, :2], e[:1], e[:, :, :2], e[0], e[:, :1], e.unsqueeze(-1), e[:, 0, 0]):     # shapes
                with pytest.raises(ValueError):
                    fn(x, photos, table, w, bad)
            for bad in (e.to(torch.int32), e > 1, e.to(torch.int64)):
                with pytest.raises(TypeError):
                    fn(x, photos, table, w, bad)
            with pytest.raises(TypeError):
                fn(x, photos, table, w, e.numpy())
            with pytest.raises(TypeError):
                fn(x, photos, table, w, e.half())
            with pytest.raises(ValueError):
                fn(x, photos, table, w, e.to("meta"))                                   # another device
        # the fused path computes on a ROCm device only: CPU tensors are an error, never a quiet fall-back
        with pytest.raises(_native.NativeLibraryError):
            cls(renderers.LocalRenderer())(x, photos, table, w, e)


# ------------------------------------------------------------------------------------------------ the kernels

@pytest.fixture(scope="module")
def exposure_asm(tmp_path_factory):
    return unit_build.compile_unit_asm(tmp_path_factory.mktemp("isa_exposure"), "svbrdf_photo_exposure", "SCHED_PHOTO")


@pytest.fixture(scope="module")
def photo_asm(tmp_path_factory):
    return unit_build.compile_unit_asm(tmp_path_factory.mktemp("isa_exposure_twin"), "svbrdf_photo_loss", "SCHED_PHOTO")


def _scene_loops(isa_stats, asm, k):
    _, meta, whole, loops, ins, rng = isa_stats.analyse(asm, k)
    scene = sorted(((r, c) for r, c in zip(rng, loops) if c["trans"] >= PHOTO_TIED_LOOP_TRANS), key=lambda rc: -rc[1]["valu"])
    return meta, whole, ins, scene


@needs_hipcc
def test_exposure_kernels_resources_and_scene_loops(exposure_asm, photo_asm):
    isa_stats = _isa_stats()
    names = sorted(k for k in isa_stats.kernels(exposure_asm) if "k_exposure" in k)
    assert len(names) == 4, names               # {maps, head} x {unweighted, weighted}: forward + adjoint, device table
    assert not [k for k in isa_stats.kernels(exposure_asm) if "k_photo_loss" in k or "k_head_photo" in k or "wphoto" in k]
    every = isa_stats.kernels(photo_asm)
    for k in names:
        head, weighted = "k_exposure_head" in k, "weighted" in k
        base = ("k_head_wphoto" if head else "8k_wphotoI") if weighted else ("k_head_photoI" if head else "k_photo_lossI")
        twin = [t for t in every if base in t and "ILb1E" in t and "_inl" not in t]
        assert len(twin) == 1, (k, twin)
        meta, whole, ins, scene = _scene_loops(isa_stats, exposure_asm, k)
        _, _, twin_ins, twin_scene = _scene_loops(isa_stats, photo_asm, twin[0])
        print("%s\n   VGPRs %s, SGPRs %s, occupancy %s, %d instructions" % (
            k, meta["NumVgprs"], meta.get("NumSgprs"), meta["Occupancy"], whole["total"]))
        assert int(meta["NumVgprs"]) <= 128 and int(meta["NumAgprs"]) == 0 and int(meta["Occupancy"]) >= 4, (k, meta)
        assert int(meta["ScratchSize"]) == 0 and whole["scratch"] == 0, (k, meta)
        assert whole["v_div"] == 0 and whole["v_pk"] == 0, (k, whole)
        assert not [mn for _, _, mn, _ in ins if mn and mn.startswith("flat_")], k       # LDS and global, never generic
        assert len(scene) == (1 if head else 2) and len(twin_scene) == len(scene), (k, len(scene))
        trans = [PHOTO_TIED_LOOP_TRANS] if head else [PHOTO_UNTIED_LOOP_TRANS, PHOTO_TIED_LOOP_TRANS]
        group = 4 if weighted else 3
        for ((a, b), c), ((ta, tb), t), tr, which in zip(scene, twin_scene, trans, ["tied"] if head else ["untied", "tied"]):
            print("   %s loop: %d VALU per trip of two renders (twin %d: %+.1f per render), %d transcendental" % (
                which, c["valu"], t["valu"], (c["valu"] - t["valu"]) / 2.0, c["trans"]))
            assert c["trans"] == t["trans"] == tr, (k, which)                           # no new transcendentals
            body = ins[a:b + 1]
            # the gains are scalar loads like the scene rows: no vector load that the twin's loop does not have, no LDS
            # read and no barrier inside the loop
            vector = [sum(bool(mn) and mn.startswith("global_load") for _, _, mn, _ in part) for part in (body, twin_ins[ta:tb + 1])]
            assert vector[0] == vector[1], (k, which, vector)
            assert not [mn for _, _, mn, _ in body if mn and mn.startswith(("s_barrier", "ds_read"))], (k, which)
            loads = [i for i, (_, _, mn, _) in enumerate(body) if mn and mn.startswith("buffer_load_dword")]
            assert len(loads) == group * 2, (k, which, len(loads))
            for g0 in range(0, len(loads), group):
                grp = loads[g0:g0 + group]
                between = [body[i][2] for i in range(grp[0], grp[-1]) if i not in grp]
                assert len(between) <= 3 and all(mn and mn.startswith(("s_mov_b32", "s_and_b32")) for mn in between), \
                    "%s %s: the %d loads are not back to back: %s" % (k, which, group, between)
                waits = [i for i, (_, _, mn, ops) in enumerate(body)
                         if i > grp[-1] and mn == "s_waitcnt" and "vmcnt(" in ops and int(ops.split("vmcnt(")[1].split(")")[0]) < group]
                assert waits, "%s: no wait behind the loads" % k
                assert waits[0] - grp[-1] >= PREFETCH_MIN_DISTANCE, "%s %s: loads waited for after %d instructions" % (
                    k, which, waits[0] - grp[-1])
        stores = [ops for _, _, mn, ops in ins if mn and mn.startswith("buffer_store_dword")]
        assert len(stores) == (9 if head else 12) and all("sc0 sc1" in s for s in stores), (k, stores)
        # the hand-off: 64-bit agent-scope atomics on both sides, adds that return (waited for) and exchanges
        atom = [(mn, ops) for _, _, mn, ops in ins if mn and mn.startswith("global_atomic")]
        assert sum(mn == "global_atomic_add_x2" for mn, _ in atom) == 3 and sum(mn == "global_atomic_swap_x2" for mn, _ in atom) == 1
        assert all("sc0" in ops for mn, ops in atom if mn in ("global_atomic_add_x2", "global_atomic_swap_x2")), atom


@needs_hipcc
def test_photo_loss_unit_alone_still_lists_its_sixteen_kernels(photo_asm):
    isa_stats = _isa_stats()
    names = [k for k in isa_stats.kernels(photo_asm) if "k_" in k]
    assert len(names) == 16 and not [k for k in names if "exposure" in k], names
    assert sum("k_photo_loss" in k for k in names) == 4 and sum("wphoto" in k for k in names) == 8
    assert sum("k_head_photo" in k for k in names) == 4


def test_sources_hold_no_inline_assembly_with_instructions():
    import re
    for name in ("svbrdf_photo_exposure.hip", "svbrdf_photo_loss.hip", "svbrdf_photo_loss_device.h"):
        for m in re.finditer(r'asm\s+volatile\s*\(\s*"([^"]*)"', unit_build.read_csrc(name)):
            assert m.group(1) == "", "inline asm with instructions in %s: %r" % (name, m.group(1))
    # the unit takes the photo loss's device functions from their header, and the build gives it the photo units' flags
    unit_build.assert_includes_shared_header("svbrdf_photo_exposure", "svbrdf_photo_loss_device.h")
    unit_build.assert_makefile_builds("svbrdf_photo_exposure", "SCHED_PHOTO")
