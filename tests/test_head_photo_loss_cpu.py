"""The head-fused photo loss (csrc/svbrdf_photo_loss.hip: k_head_photo*, losses.HeadPhotoLoss), everything that needs no GPU:

  * the library exports the two entry points, added to ABI version 8 without a bump, and rejects bad arguments before it
    launches anything;
  * tests/golden/g20_head_photo_loss.npz -- written by the reference (tests/golden/make_golden_head_photo.py) -- is what its
    generator describes and is reproduced by the oracle's composition (tests/head_photo_checks.py) within the project's bounds;
  * that composition equals an independent definition in torch float64 autograd;
  * the inputs the GPU tests use stay inside the caps by the comparison values alone;
  * HeadPhotoLoss with a plugin renderer on CPU tensors IS the composed definition, bit for bit, and rejects bad arguments;
  * the four new kernels, compiled with the Makefile's flags: 4 waves/SIMD, no scratch, ONE scene loop -- the tied one --
    within the instruction bounds of tests/test_photo_loss_cpu.py, its photo prefetch a shading pass in front of its wait.
"""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import head_checks
import head_photo_checks as hp
import photo_checks
import synth
import tolerances
import unit_build
from test_photo_loss_cpu import (PHOTO_TIED_LOOP_TRANS, PHOTO_TIED_LOOP_VALU_MAX, PREFETCH_MIN_DISTANCE, _isa_stats, _ToyRenderer,
                                 needs_hipcc)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from svbrdf_estimation_amd import _native
    return _native._load()


def test_library_exports_the_head_photo_loss_without_an_abi_bump(lib):
    from svbrdf_estimation_amd import _native
    assert lib.svbrdf_abi_version() == 8 and _native.ABI_VERSION == 8
    with open(os.path.join(ROOT, "include", "svbrdf_hip.h")) as f:
        header = f.read()
    assert "#define SVBRDF_ABI_VERSION 8" in header
    for name in hp.ENTRIES:
        assert hasattr(lib, name), name
        assert "SVBRDF_API int %s(" % name in header
    assert "WITHOUT A BUMP" in header and "symbol presence" in header


# (the argument checks of these entries: tests/test_photo_loss_cpu.py::test_argument_errors_come_before_any_launch)


# ------------------------------------------------------------------------------------------------ the fixture

@pytest.fixture(scope="module")
def g20(golden):
    g = golden("g20_head_photo_loss.npz")
    enc = head_checks.fixture_input(int(g["enc_seed"]), int(g["B"]), int(g["H"]))
    assert synth.checksum(enc) == str(g["enc_sha256"]), "synthetic inputs are not bit-reproducible here"
    return g, enc, photo_checks.Reference(enc, g["photos"], g["scenes"], float(g["eps"]), head=True)


def test_fixture_is_what_its_generator_describes(g20):
    g, enc, _ = g20
    assert enc.shape == (3, 9, 13, 13) and g["scenes"].shape == (3, 9, 9) and g["photos"].shape == (3, 9, 3, 13, 13)
    assert (13 * 13 * 4) % 16 == 4          # items 1 and 2 start four bytes off 16-byte alignment
    ph = g["photos"]
    assert ph.dtype == np.float32 and ph.min() >= 0.0 and ph.max() <= 1.0 and (ph == 0.0).any()
    assert g["grad9"].dtype == np.float32 and g["grad9_f64"].dtype == np.float64 and g["grad9"].shape == enc.shape
    assert g["loss"].dtype == np.float32 and g["loss_f64"].dtype == np.float64 and float(g["eps"]) == np.float32(0.1)
    # saturated groups: rows 0..7 hold one group at a time at -1 / +1 (head_checks.fixture_input)
    assert (enc[:, 5, 4, :] == -1.0).all() and (enc[:, 5, 5, :] == 1.0).all() and (np.abs(enc) <= 1.0).all()
    # the photos are noisy renderings of OTHER maps under the fixture's scenes
    other = synth.make_maps(int(g["photo_maps_seed"]), 3, 13)
    assert synth.checksum(other) == str(g["photo_maps_sha256"])
    assert np.abs(ph - hp.photographs(other, g["scenes"])).mean() < 0.02
    # listed in its manifest file (the "fixtures" layout of MANIFEST.json) with its generator and the file's own sha256
    gdir = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gdir, "MANIFEST_g20_head_photo_loss.json")) as f:
        entry = json.load(f)["fixtures"]["g20_head_photo_loss.npz"]
    assert entry["generator"] == "tests/golden/make_golden_head_photo.py" and os.path.exists(os.path.join(ROOT, entry["generator"]))
    with open(os.path.join(gdir, "g20_head_photo_loss.npz"), "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == entry["sha256"]


def test_oracle_composition_reproduces_the_reference_fixture(g20):
    g, enc, ref = g20
    print("[head-photo] fixture loss %.9g (f64 %.12g), oracle %.9g (f64 %.12g); %d tie pixels, %d widened" % (
        float(g["loss"]), float(g["loss_f64"]), ref.loss, ref.loss64, ref.n_ties(), ref.n_widened()))
    tolerances.assert_loss_close(ref.loss, g["loss"], "oracle fp32 vs reference fp32")
    tolerances.assert_loss_close(ref.loss64, g["loss_f64"], "oracle fp64 vs reference fp64")
    tolerances.assert_loss_close(ref.loss, g["loss_f64"], "oracle fp32 vs reference fp64")
    # (the reference's double evaluation decodes in double, the composition shades the float32 decode: the project's
    # gradient bound, not the 1e-6 of two double evaluations of the same maps)
    photo_checks.assert_photo_grad_close(ref.grad64, g["grad9_f64"], None, ref.tie, "g20 oracle fp64 vs reference fp64")
    n = photo_checks.assert_photo_grad_close(ref.grad, g["grad9"], g["grad9_f64"], ref.tie, "g20 oracle vs reference")
    assert n <= tolerances.MAX_TIE_PIXELS


@pytest.mark.parametrize("gen", sorted(head_checks.GENERATORS))
def test_oracle_composition_against_torch_float64_autograd(gen):
    """B = 2, H = 7, every input generator; the bounds of tests/test_head_loss_cpu.py's comparison of the same kind: loss
    1e-12, gradient 1e-9 of its maximum.  The composition shades the FLOAT32 decode; the torch definition is therefore
    evaluated at those map values (losses.decode_head supplies the Jacobian).  At 1e-9 two float32 roundings inside the
    composition show, and both are taken out for that comparison: the upstream gradient the oracle's adjoint receives
    (head_photo_checks.upstream_rounding_term adds the adjoint of the residue) and the float32 normal in the chain's
    Jacobian (chained at torch's own double normal instead).  The comparison values as the GPU tests use them -- with both
    roundings, each a 2^-24 relative error per term -- then stay within 1e-6 of the gradient's maximum of the same torch
    gradient: 16 times 2^-24, room for the terms of an element cancelling to a sixteenth of their absolute sum."""
    B, H = 2, 7
    enc = head_checks.GENERATORS[gen](8100, B, H)
    sc = head_checks.scene_table(81, B, 2, 3)
    photos = hp.photographs(synth.make_maps(8101, B, H, tiled_roughness=(gen != "full")), sc)
    for eps in (0.1, 0.02):
        ref = photo_checks.Reference(enc, photos, sc, eps, head=True)
        t_loss, t_grad, t_maps = hp.torch_head_photo_loss(enc, photos, sc, eps, maps_values=ref.maps)
        scale = np.abs(t_grad).max()
        exact12 = ref.grad12_64 + hp.upstream_rounding_term(ref.maps, photos, sc, eps)
        exact = photo_checks.chain9(enc, ref.maps, exact12, n=t_maps[:, 0:3])
        print("[head-photo] %s eps %.2f: loss %.15g vs torch %.15g, gradient off by %.2e of max (as compared on the GPU: %.2e)" % (
            gen, eps, ref.loss64, t_loss, np.abs(exact - t_grad).max() / scale, np.abs(ref.grad64 - t_grad).max() / scale))
        assert abs(ref.loss64 - t_loss) <= 1e-12 * abs(t_loss)
        assert np.abs(exact - t_grad).max() <= 1e-9 * scale
        assert np.abs(ref.grad64 - t_grad).max() <= 1e-6 * scale
        # the float32 decode is the double one rounded (the reference's rounding: 1 ulp of the normal at the most)
        np.testing.assert_allclose(ref.maps, t_maps, rtol=3e-7, atol=1e-7)
    if gen == "roughness-1":        # the clamp's mask: a decoded roughness of exactly 0 has no gradient
        hit = enc[:, 5] == -1.0
        assert hit.any() and not ref.grad64[:, 5][hit].any() and ref.grad64[:, 5][~hit].any()


# ------------------------------------------------------------------------------------------------ the GPU cases' caps

def _gpu_cases():
    for c in head_checks.sweep_cases():
        yield head_checks.sweep_name(c), hp.sweep_inputs(c)
    for name in ("16_host", "64_host", "64_device"):
        yield "pow2 " + name, hp.pow2_inputs(name)
    yield "pow2 %s raw" % hp.RAW_POW2, hp.pow2_inputs(hp.RAW_POW2, raw=True)
    yield "arguments", hp.argument_inputs()
    for H in (13, 17):
        yield "alignment %d" % H, hp.alignment_inputs(H)


def test_gpu_cases_stay_inside_the_caps_by_the_comparison_values_alone():
    """tie pixels and elements that need the widening, fp32 oracle against fp64 oracle, of every input
    tests/test_gpu_head_photo_loss.py compares element-wise (the 256 x 256 case is counted there, on the device's box)"""
    worst = 0
    for name, (enc, photos, sc) in _gpu_cases():
        ref = photo_checks.Reference(enc, photos, sc, head=True)
        ties, widened = ref.n_ties(), ref.n_widened()
        if ties or widened:
            print("[head-photo] %s: %d tie pixels, %d widened" % (name, ties, widened))
        assert ties <= tolerances.MAX_TIE_PIXELS and widened <= tolerances.MAX_WIDENED_GRAD, (name, ties, widened)
        worst = max(worst, ties)
    print("[head-photo] most tie pixels in one case: %d" % worst)


# ------------------------------------------------------------------------------------------------ the module

def _toy_inputs():
    from svbrdf_estimation_amd import environment
    B, S, H = 2, 3, 8
    enc = torch.from_numpy(head_checks.full(33, B, H))
    torch.manual_seed(5)
    table = torch.stack([environment.scene_table(1, S - 1) for _ in range(B)])
    photos = torch.rand(B, S, 3, H, H)
    return enc, photos, table


def test_headphotoloss_with_a_plugin_renderer_is_the_composed_definition_bitwise():
    from svbrdf_estimation_amd import environment, losses
    enc, photos, table = _toy_inputs()
    B = enc.shape[0]
    fn = losses.HeadPhotoLoss(_ToyRenderer(), eps=0.05)
    assert not fn.uses_fused_kernel() and losses.HeadPhotoLoss(_ToyRenderer()).eps == 0.1

    x0 = enc.clone().requires_grad_(True)
    ref = losses.PhotoLoss(_ToyRenderer(), 0.05)(losses.decode_head(x0), photos, table)
    ref.backward()
    # ... which is render per scene, log, L1 mean of the decoded maps
    R, maps = _ToyRenderer(), losses.decode_head(enc)
    rows = [torch.cat([R.render(sc, maps[b]) for sc in environment.scenes_from_table(table[b])], dim=0) for b in range(B)]
    assert torch.equal(ref, torch.nn.functional.l1_loss(torch.log(torch.stack(rows, dim=0) + 0.05), torch.log(photos + 0.05)))
    for scenes in (table, [environment.scenes_from_table(table[b]) for b in range(B)]):
        x = enc.clone().requires_grad_(True)
        loss = fn(x, photos, scenes)
        assert loss.dim() == 0
        loss.backward()
        assert torch.equal(loss, ref) and torch.equal(x.grad, x0.grad) and x.grad.shape == enc.shape
    # [B,3,H,W] photos mean S = 1; float64 stays float64
    assert torch.equal(fn(enc, photos[:, 0], table[:, :1]), fn(enc, photos[:, :1], table[:, :1]))
    assert fn(enc.double(), photos.double(), table).dtype == torch.float64


def test_headphotoloss_rejects_bad_arguments():
    from svbrdf_estimation_amd import _native, environment, losses, renderers
    enc, photos, table = _toy_inputs()
    maps12 = torch.from_numpy(synth.make_maps(31, 2, 8))
    for fn in (losses.HeadPhotoLoss(_ToyRenderer()), losses.HeadPhotoLoss(renderers.LocalRenderer())):
        with pytest.raises(ValueError):
            fn(maps12, photos, table)                           # [B,12,H,W]: decoded maps belong to PhotoLoss
        with pytest.raises(ValueError):
            fn(enc[0], photos[0], table[0])                     # not batched
        with pytest.raises(ValueError):
            fn(enc, photos[:1], table)                          # another B
        with pytest.raises(ValueError):
            fn(enc, photos[..., :4], table)                     # another W
        with pytest.raises(ValueError):
            fn(enc, photos, table[:, :2])                       # S of the scenes differs from S of the photos
        with pytest.raises(ValueError):
            fn(enc, photos, [environment.scenes_from_table(table[0])])
        with pytest.raises(RuntimeError):
            fn(enc, photos.clone().requires_grad_(True), table)
        with pytest.raises(ValueError):
            fn(enc, photos.to("meta"), table)                   # another device
        with pytest.raises(TypeError):
            fn(enc, (photos * 255).to(torch.uint8), table)      # not floating point
        with pytest.raises(TypeError):
            fn(enc.to(torch.int32), photos, table)
    # the fused path computes on a ROCm device only: CPU tensors are an error, never a quiet fall-back
    fused = losses.HeadPhotoLoss(renderers.LocalRenderer())
    assert fused.uses_fused_kernel()
    with pytest.raises(_native.NativeLibraryError):
        fused(enc, photos, table)
    with pytest.raises(TypeError):
        fused(enc, photos, table.double())                      # the table is float32 whatever the maps are


# ------------------------------------------------------------------------------------------------ the kernels

@pytest.fixture(scope="module")
def photo_asm(tmp_path_factory):
    return unit_build.compile_unit_asm(tmp_path_factory.mktemp("isa_head_photo"), "svbrdf_photo_loss", "SCHED_PHOTO")


@needs_hipcc
def test_head_kernels_resources_and_the_one_scene_loop(photo_asm):
    isa_stats = _isa_stats()
    every = isa_stats.kernels(photo_asm)
    assert len([k for k in every if "k_photo_loss" in k]) == 4          # the existing four, names unchanged
    names = sorted(k for k in every if "k_head_photo" in k)
    assert len(names) == 4, names        # {device table, by-value table} x {forward only, forward + adjoint}
    assert sum("ILb1E" in k for k in names) == 2 and sum("_inl" in k for k in names) == 2
    for k in names:
        _, meta, whole, loops, ins, rng = isa_stats.analyse(photo_asm, k)
        with_grad = "ILb1E" in k
        print("%s\n   VGPRs %s, SGPRs %s, occupancy %s, %d instructions (%d VALU, %d transcendental)" % (
            k, meta["NumVgprs"], meta.get("NumSgprs"), meta["Occupancy"], whole["total"], whole["valu"], whole["trans"]))
        assert int(meta["NumVgprs"]) <= 128 and int(meta["NumAgprs"]) == 0 and int(meta["Occupancy"]) >= 4, (k, meta)
        assert int(meta["ScratchSize"]) == 0 and whole["scratch"] == 0, (k, meta)
        assert whole["v_div"] == 0 and whole["v_pk"] == 0, (k, whole)
        scene = [(r, c) for r, c in zip(rng, loops) if c["trans"]]
        assert len(scene) == 1, "%s: expected the tied scene loop alone, found %d loops with transcendentals" % (k, len(scene))
        ((a, b), tied), = scene
        print("   tied %s" % tied)
        per = 2 if with_grad else 1          # renders per trip
        assert tied["trans"] == PHOTO_TIED_LOOP_TRANS // 2 * per, k        # three lobes would be 18 per render
        assert tied["valu"] <= PHOTO_TIED_LOOP_VALU_MAX // 2 * per, k
        body = ins[a:b + 1]
        loads = [i for i, (_, _, mn, _) in enumerate(body) if mn and mn.startswith("buffer_load_dword")]
        assert len(loads) == 3 * per, (k, len(loads))
        for g0 in range(0, len(loads), 3):
            grp = loads[g0:g0 + 3]
            assert grp[2] - grp[0] == 2, "%s: photo loads not back to back" % k
            waits = [i for i, (_, _, mn, ops) in enumerate(body)
                     if i > grp[2] and mn == "s_waitcnt" and "vmcnt(" in ops and int(ops.split("vmcnt(")[1].split(")")[0]) <= 2]
            assert waits, "%s: no wait behind the photo loads" % k
            assert waits[0] - grp[2] >= PREFETCH_MIN_DISTANCE, "%s: photo loads waited for after %d instructions" % (
                k, waits[0] - grp[2])
        if with_grad:       # 9 gradient planes out, write-through as the 12-channel kernels' stores
            stores = [ops for _, _, mn, ops in ins if mn and mn.startswith("buffer_store_dword")]
            assert len(stores) == 9 and all("sc0 sc1" in s for s in stores), (k, stores)
