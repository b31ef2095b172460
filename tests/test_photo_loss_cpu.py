"""The fused photo loss (csrc/svbrdf_photo_loss.hip, losses.PhotoLoss), everything that needs no GPU:

  * the library exports the two entry points of ABI version 8 and rejects bad arguments before it launches anything;
  * tests/golden/g18_photo_loss.npz -- written by the reference (tests/golden/make_golden_photo.py: its renderer, its scene
    sampler, its sensor noise, its log / L1 and autograd, in float32 and float64) -- against the oracle's composition
    (tests/photo_checks.py) within the project's bounds, tie pixels counted from the fixture's own float64 values;
  * PhotoLoss with a plugin renderer on CPU tensors IS the composed definition, bit for bit, and rejects bad arguments;
  * the translation unit compiles with the Makefile's flags: no contracted FMA on the geometry path, 4 waves/SIMD, no
    scratch, and the software prefetch of the next render's photo values sits a shading pass in front of its wait.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import photo_checks
import synth
import tolerances
import unit_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svbrdf_estimation_amd", "csrc")
ENTRIES = ("svbrdf_photo_loss_fwd_bwd", "svbrdf_photo_loss_fwd_bwd_host_scenes")


@pytest.fixture(scope="module")
def lib():
    from svbrdf_estimation_amd import _native
    return _native._load()


def test_library_exports_the_photo_loss_and_abi_8(lib):
    from svbrdf_estimation_amd import _native
    assert lib.svbrdf_abi_version() == 8 and _native.ABI_VERSION == 8
    for name in ENTRIES:
        assert hasattr(lib, name), name
    with open(os.path.join(ROOT, "include", "svbrdf_hip.h")) as f:
        header = f.read()
    assert "#define SVBRDF_ABI_VERSION 8" in header
    for name in ENTRIES:
        assert "SVBRDF_API int %s(" % name in header


# all nine fused-loss entry points share one set of argument checks (plan_loss in csrc/svbrdf_host.h); the mixed and
# head K3 entries take `l1_weight, eps_l1` after `eps`
LOSS_ENTRIES = ENTRIES + ("svbrdf_head_photo_loss_fwd_bwd", "svbrdf_head_photo_loss_fwd_bwd_host_scenes",
                          "svbrdf_rendering_loss_fwd_bwd")
LOSS_ENTRIES_L1 = ("svbrdf_mixed_loss_fwd_bwd", "svbrdf_mixed_loss_fwd_bwd_host_scenes", "svbrdf_head_loss_fwd_bwd",
                   "svbrdf_head_loss_fwd_bwd_host_scenes")


@pytest.mark.parametrize("entry", LOSS_ENTRIES + LOSS_ENTRIES_L1)
def test_argument_errors_come_before_any_launch(lib, entry):
    """error codes of every fused-loss entry point: -1 null pointer, -2 bad dims / H != W / eps out of range, -3 misaligned,
    -4 workspace too small.  Host buffers stand in for device memory: every check fails before anything is enqueued."""
    fn = getattr(lib, entry)
    B, S, H = 1, 2, 8
    buf = (ctypes.c_float * 8192)()
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 63) & ~63
    need = lib.svbrdf_rendering_loss_workspace_bytes(B, S, H, H)
    assert need == 65 * 8
    l1 = (ctypes.c_float(0.1), ctypes.c_float(0.01)) if entry in LOSS_ENTRIES_L1 else ()

    def call(input=p, other=p + 256, scenes=p + 512, xrow=p + 1024, eps=0.1, loss=p + 2048, grad=p + 4096, ws=p + 8192,
             ws_bytes=need, B=B, S=S, H=H, W=H):
        return fn(input, other, scenes, xrow, ctypes.c_float(eps), *l1, loss, grad, ws, ws_bytes, B, S, H, W, None)

    launches = lib.svbrdf_debug_launch_count()
    for name in ("input", "other", "scenes", "xrow", "loss", "ws"):
        assert call(**{name: None}) == -1, name
    assert lib.svbrdf_last_error()
    assert call(W=H + 1) == -2
    assert call(B=0) == -2 and call(S=0) == -2
    assert call(eps=0.0) == -2 and call(eps=float("nan")) == -2 and call(eps=1e10) == -2
    assert call(other=p + 2) == -3 and call(ws=p + 8196) == -3 and call(input=p + 1) == -3 and call(grad=p + 4098) == -3
    assert call(ws_bytes=need - 8) == -4
    if entry.endswith("host_scenes"):
        assert call(B=17, S=17) == -2                    # 289 rows: beyond the argument block
    assert lib.svbrdf_debug_launch_count() == launches     # failed calls enqueue and count nothing


@pytest.fixture(scope="module")
def g18(golden):
    g = golden("g18_photo_loss.npz")
    B, H = int(g["B"]), int(g["H"])
    inp = synth.make_maps(int(g["input_seed"]), B, H)
    assert synth.checksum(inp) == str(g["input_sha256"]), "synthetic inputs are not bit-reproducible here"
    return g, inp


def test_fixture_is_what_the_issue_describes(g18):
    g, inp = g18
    assert inp.shape == (2, 12, 32, 32) and g["scenes"].shape == (2, 9, 9) and g["photos"].shape == (2, 9, 3, 32, 32)
    ph = g["photos"]
    assert ph.dtype == np.float32 and ph.min() >= 0.0 and ph.max() <= 1.0 and (ph == 0.0).any() and (ph == 1.0).any()
    assert g["grad_input"].dtype == np.float32 and g["grad_input_f64"].dtype == np.float64
    gdir = os.path.join(ROOT, "tests", "golden")
    sizes = {n: os.path.getsize(os.path.join(gdir, n)) for n in os.listdir(gdir) if n.endswith(".npz")}
    assert sizes["g18_photo_loss.npz"] <= max(v for n, v in sizes.items() if n != "g18_photo_loss.npz")
    # the photos are noisy renderings of OTHER maps: close to the oracle's rendering of those, not of the input
    other = synth.make_maps(int(g["photo_maps_seed"]), 2, 32)
    assert synth.checksum(other) == str(g["photo_maps_sha256"])
    from oracle import c_oracle
    clean = np.clip(c_oracle.render_fwd(other, g["scenes"]), 0.0, 1.0)
    assert np.abs(ph - clean).mean() < 0.02 < np.abs(ph - np.clip(c_oracle.render_fwd(inp, g["scenes"]), 0.0, 1.0)).mean()


def test_oracle_composition_reproduces_the_reference_fixture(g18):
    g, inp = g18
    eps = float(g["eps"])
    loss32, grad32, _ = photo_checks.oracle_photo_loss(inp, g["photos"], g["scenes"], eps)
    loss64, grad64, delta64 = photo_checks.oracle_photo_loss(inp, g["photos"], g["scenes"], eps, f64=True)
    print("[photo-loss] fixture loss %.9g (f64 %.12g), oracle %.9g (f64 %.12g)" % (
        float(g["loss"]), float(g["loss_f64"]), loss32, loss64))
    tolerances.assert_loss_close(loss32, g["loss"], "oracle fp32 vs reference fp32")
    tolerances.assert_loss_close(loss64, g["loss_f64"], "oracle fp64 vs reference fp64")
    tolerances.assert_loss_close(loss32, g["loss_f64"], "oracle fp32 vs reference fp64")
    # ties from the fixture's OWN float64 values: the oracle's float64 deltas are the reference's (checked through the loss
    # above and the gradient below), the structural terms come from the fixture's photos and scenes
    tmap = photo_checks.tie_map(inp, g["photos"], g["scenes"], delta64)
    tolerances.assert_grad_close(grad64, g["grad_input_f64"], "oracle fp64 gradient vs reference fp64", rtol=1e-6, afrac=1e-7)
    n = photo_checks.assert_photo_grad_close(grad32, g["grad_input"], g["grad_input_f64"], tmap, "g18 oracle vs reference")
    assert n <= tolerances.MAX_TIE_PIXELS


class _ToyRenderer:
    """a plugin: any object with render(scene, svbrdf [12,H,W] or [1,12,H,W]) -> [1,3,H,W]; differentiable torch ops"""

    def render(self, scene, svbrdf):
        m = svbrdf if svbrdf.dim() == 4 else svbrdf.unsqueeze(0)
        cam = torch.as_tensor(scene.camera.pos, dtype=m.dtype).view(1, 3, 1, 1)
        col = torch.as_tensor(scene.light.color, dtype=m.dtype).view(1, 3, 1, 1)
        lz = float(torch.as_tensor(scene.light.pos)[2])
        return (m[:, 3:6] * col * 0.01 + m[:, 9:12] * torch.clamp((m[:, 0:3] * cam).sum(1, keepdim=True), min=0.0) ** 2
                + m[:, 6:9] * lz * 0.1)


def test_photoloss_with_a_plugin_renderer_is_the_composed_definition_bitwise():
    from svbrdf_estimation_amd import environment, losses
    B, S, H = 2, 3, 8
    maps = torch.from_numpy(synth.make_maps(31, B, H))
    torch.manual_seed(5)
    table = torch.stack([environment.scene_table(1, S - 1) for _ in range(B)])
    photos = torch.rand(B, S, 3, H, H)
    fn = losses.PhotoLoss(_ToyRenderer(), eps=0.05)
    assert not fn.uses_fused_kernel()

    def composed(x):
        R = _ToyRenderer()
        rows = []
        for b in range(B):
            rows.append(torch.cat([R.render(sc, x[b]) for sc in environment.scenes_from_table(table[b])], dim=0))
        return torch.nn.functional.l1_loss(torch.log(torch.stack(rows, dim=0) + 0.05), torch.log(photos + 0.05))

    x0 = maps.clone().requires_grad_(True)
    ref = composed(x0)
    ref.backward()
    for scenes in (table, [environment.scenes_from_table(table[b]) for b in range(B)]):
        x = maps.clone().requires_grad_(True)
        loss = fn(x, photos, scenes)
        assert loss.dim() == 0
        loss.backward()
        assert torch.equal(loss, ref) and torch.equal(x.grad, x0.grad)
    # [B,3,H,W] photos mean S = 1; float64 maps stay float64
    one = fn(maps, photos[:, 0], table[:, :1])
    assert torch.equal(one, fn(maps, photos[:, :1], table[:, :1]))
    assert fn(maps.double(), photos.double(), table).dtype == torch.float64


def test_photoloss_rejects_bad_arguments():
    from svbrdf_estimation_amd import _native, environment, losses, renderers
    B, S, H = 2, 3, 8
    maps = torch.from_numpy(synth.make_maps(31, B, H))
    photos = torch.rand(B, S, 3, H, H)
    torch.manual_seed(5)
    table = torch.stack([environment.scene_table(1, S - 1) for _ in range(B)])
    for fn in (losses.PhotoLoss(_ToyRenderer()), losses.PhotoLoss(renderers.LocalRenderer())):
        assert fn.eps == 0.1
        with pytest.raises(ValueError):
            fn(maps[:, :9], photos, table)                      # not 12 channels
        with pytest.raises(ValueError):
            fn(maps[0], photos[0], table[0])                    # not batched
        with pytest.raises(ValueError):
            fn(maps, photos[:1], table)                         # another B
        with pytest.raises(ValueError):
            fn(maps, photos[:, :, :2], table)                   # not RGB
        with pytest.raises(ValueError):
            fn(maps, photos[..., :4], table)                    # another W
        with pytest.raises(ValueError):
            fn(maps, photos, table[:, :2])                      # S of the scenes differs from S of the photos
        with pytest.raises(ValueError):
            fn(maps, photos, [environment.scenes_from_table(table[0])])      # one item's scenes for two items
        with pytest.raises(RuntimeError):
            fn(maps, photos.clone().requires_grad_(True), table)
    # the fused path computes on a ROCm device only: CPU tensors are an error, never a quiet fall-back
    fused = losses.PhotoLoss(renderers.LocalRenderer())
    assert fused.uses_fused_kernel()
    with pytest.raises(_native.NativeLibraryError):
        fused(maps, photos, table)


# ---------------------------------------------------------------------------------------------------------------------
# the translation unit, compiled with the Makefile's own flags (as tests/test_isa_guard.py does for K3)
# ---------------------------------------------------------------------------------------------------------------------
needs_hipcc = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs /opt/rocm/bin/hipcc (cross-compiles gfx950)")
PHOTO_TIED_LOOP_VALU_MAX = 496       # per two renders (geometry ping-pong): measured 477-479 = 239 per render (K3: 301)
PHOTO_TIED_LOOP_TRANS = 20           # 10 per render: 3 rsq (geometry), 2 rsq + 1 rcp (lobe), 1 rcp + 3 log (loss)
PHOTO_UNTIED_LOOP_VALU_MAX = 672     # three lobes: measured 647
PHOTO_UNTIED_LOOP_TRANS = 36
PREFETCH_MIN_DISTANCE = 100          # instructions between the issue of a render's photo loads and the wait that needs them


@pytest.fixture(scope="module")
def photo_asm(tmp_path_factory):
    return unit_build.compile_unit_asm(tmp_path_factory.mktemp("isa_photo"), "svbrdf_photo_loss", "SCHED_PHOTO")


def _isa_stats():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_stats
    return isa_stats


@needs_hipcc
def test_makefile_builds_the_unit_into_the_library():
    unit_build.assert_makefile_builds("svbrdf_photo_loss", "SCHED_PHOTO")
    assert "-ffp-contract=off" in unit_build.make_var("HIPFLAGS")
    # K3's source is not touched by the feature's translation unit: its header only includes K3's device code and the host checks
    unit_build.assert_includes_shared_header("svbrdf_photo_loss", "svbrdf_photo_loss_device.h")
    assert "rendering_loss_body" in unit_build.assert_includes_shared_header("svbrdf_photo_loss_device.h", "svbrdf_device.h")
    assert "plan_loss" in unit_build.assert_includes_shared_header("svbrdf_photo_loss_device.h", "svbrdf_host.h")
    import re
    for m in re.finditer(r'asm\s+volatile\s*\(\s*"([^"]*)"', unit_build.read_csrc("svbrdf_photo_loss.hip", "svbrdf_photo_loss_device.h")):
        assert m.group(1) == "", "inline asm with instructions: %r" % m.group(1)


def test_units_share_code_through_headers_only():
    """the layout of csrc/, stated once: no .hip file includes another .hip file (shared code lives in headers; no file is
    compiled "minus its kernels"), no guard macro of that kind is left anywhere, and a header holds no entry point and --
    but for the K3 kernel templates, which three units instantiate -- no kernel"""
    import re
    names = sorted(os.listdir(CSRC))
    units = [n for n in names if n.endswith(".hip")]
    assert len(units) >= 12, units
    for name in units:
        included = re.findall(r'^\s*#\s*include\s*"([^"]+\.hip)"', unit_build.read_csrc(name), flags=re.M)
        assert not included, (name, included)
    for name in names:
        if os.path.isfile(os.path.join(CSRC, name)):
            text = unit_build.read_csrc(name)
            assert "SHARED_ONLY" not in text and "SVBRDF_TU" not in text, name
            if name.endswith(".h"):
                assert 'extern "C" {' not in text, name
                assert "__global__" not in text or name == "svbrdf_k3_kernels.h", name


def test_photo_units_hold_each_shared_piece_once():
    """the small pieces every photo body is made of -- the guards against non-finite maps (the numerics contract), the
    pixel's coordinates, the positivity check, the weights' rule and the "<who>: <what>" reporter -- stand
    once across the seven photo units, their headers and svbrdf_host.h"""
    import re
    files = sorted(n for n in os.listdir(CSRC) if n.startswith("svbrdf_photo_")) + ["svbrdf_host.h"]
    assert len(files) == 7 + 4 + 1, files
    code = "\n".join(line.split("//")[0] for line in unit_build.read_csrc(*files).splitlines())
    shared = "\n".join(line.split("//")[0] for line in unit_build.read_csrc("svbrdf_photo_loss_device.h").splitlines())

    def body(signature):        # the text of the one function whose definition starts with `signature`
        assert code.count(signature) == 1 and signature in shared, signature
        return code[code.index(signature):code.index("\n}\n", code.index(signature))]

    # 1. the guards: `chk - chk` and `ds - ds` in maps_guard alone, the encoded planes' e[k] - e[k] in head_guard alone
    assert code.count("chk - chk") == body("void maps_guard(const Maps &in,").count("chk - chk") == 2
    assert code.count("ds - ds") == body("void maps_guard(const Maps &in,").count("ds - ds") == 1
    assert len(re.findall(r"e\[(\d)\] - e\[\1\]", code)) == len(re.findall(r"e\[(\d)\] - e\[\1\]", body("float head_guard("))) == 9
    assert code.count("poison += head_chk") == 1 and "poison += head_chk" in body("void head_guard_apply(")
    # 2. the coordinates: the shift and mask in pixel_xy and in photo_loss_body's early branch, pixel_coords in pixel_xy alone
    assert code.count("__builtin_ctz(") == 2 and "__builtin_ctz(" in body("void pixel_xy(") and code.count("pixel_coords<1>(") == 1
    # 3. the loss tail: RELAXED, no once-only check.  photo_loss_body, photo_grad_body and fit_body write their twelve lines out
    # (with fit_run_body's two-set tail and photo_sums_finish: five callers of loss_arrive).  As one function the tail moved
    # two instruction lines in each of the 28 kernels, and on an MI355X, against the parent's library in the same call, two
    # launch kinds then missed "median <= parent's median + parent's spread": the photo-gradient launch with both gradients,
    # 51.02 us against 50.68 + 0.06, and PhotoFit(smooth=).step, 84.52 us against 82.06 + 0.66
    # (profiles/r29_photo_shared_pieces.txt)
    assert code.count("loss_arrive(t,") == 5 and code.count("float wave_part[") == 5 and "workgroup_loss_arrive" not in code
    # 4. the item's base pointers: RELAXED, no once-only check.  The seven bodies write their four lines out: as one function
    # the same expressions made the compiler schedule the scalar address arithmetic otherwise, loops with transcendentals of
    # seven kernels carried other registers and the joint kernels gained an instruction (profiles/r29_photo_shared_pieces.txt)
    assert code.count("weight_planes == 1 ? 0 : plane") == 7 and "item_ptrs" not in code
    # 5. the positivity check of the light colours and of the gains
    assert code.count("< __builtin_inff())") == 1 and code.count("positive_check(") == 1 + 3
    # 6., 7. the host side: one reporter, one rule of the weights (its sentence, and the older entries' shorter one)
    # (the second "%s: %s" is plan_loss's own reporter in svbrdf_host.h: K3's too, and not this layer's)
    assert code.count('"%s: %s"') == 2 and code.count("int fail_as(") == 1
    assert code.count("weight_planes != 1 && weight_planes != S") == 1 and code.count("int weights_check(") == 1
    assert code.count("with weights, 0 without") == 1 and code.count('"pointers must be 4-byte aligned"') == 1
    assert code.count("weight_planes must be 1 (one plane per item) or S (one per photo)") == 2


@needs_hipcc
def test_kernel_resources_and_scene_loops(photo_asm):
    isa_stats = _isa_stats()
    assert '.amdgcn_target "amdgcn-amd-amdhsa--gfx950"' in photo_asm
    names = sorted(k for k in isa_stats.kernels(photo_asm) if "k_photo_loss" in k)
    assert len(names) == 4, names        # {device table, by-value table} x {forward only, forward + adjoint}
    for k in names:
        _, meta, whole, loops, ins, rng = isa_stats.analyse(photo_asm, k)
        with_grad = "ILb1E" in k
        assert int(meta["NumVgprs"]) <= 128 and int(meta["NumAgprs"]) == 0 and int(meta["Occupancy"]) >= 4, (k, meta)
        assert int(meta["ScratchSize"]) == 0 and whole["scratch"] == 0, (k, meta)
        assert whole["v_div"] == 0 and whole["v_pk"] == 0, (k, whole)
        scene = [(r, c) for r, c in zip(rng, loops) if c["trans"]]
        assert len(scene) == 2, "%s: expected the three-lobe and the tied scene loop, found %d" % (k, len(scene))
        (_, untied), (_, tied) = sorted(scene, key=lambda rc: -rc[1]["valu"])
        print("%s\n   tied %s\n   untied %s" % (k, tied, untied))
        per = 2 if with_grad else 1          # renders per trip
        assert tied["trans"] == PHOTO_TIED_LOOP_TRANS // 2 * per and untied["trans"] == PHOTO_UNTIED_LOOP_TRANS // 2 * per, k
        assert tied["valu"] <= PHOTO_TIED_LOOP_VALU_MAX // 2 * per and untied["valu"] <= PHOTO_UNTIED_LOOP_VALU_MAX // 2 * per, k
        # Software prefetch: the three photo values of the next render are the only buffer loads in a scene loop, issued
        # back to back, and no wait that they could satisfy (vmcnt(n), n <= 2, with nothing younger in flight) follows
        # within PREFETCH_MIN_DISTANCE instructions: they have a shading pass to arrive.
        for (a, b), c in scene:
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


@needs_hipcc
def test_geometry_path_holds_no_contracted_fma(tmp_path):
    """numerics contract: dot3 -- the coords -> NH path -- is three separately rounded products summed (p0+p1)+p2 in THIS
    unit's build too (its own flag set): the probe kernel must compile to 3 v_mul + 2 v_add and no FMA."""
    mns, fma = unit_build.dot3_probe_instructions(tmp_path, "svbrdf_photo_loss", "SCHED_PHOTO")
    muls = [m for m in mns if m.startswith("v_mul_f32")]
    adds = [m for m in mns if m.startswith("v_add_f32")]
    assert len(muls) == 3 and len(adds) == 2 and fma == 0, mns
