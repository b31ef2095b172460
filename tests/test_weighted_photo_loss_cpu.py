"""The photo losses with per-pixel confidence weights (csrc/svbrdf_photo_loss.hip: k_wphoto*, k_head_wphoto*; PhotoLoss and
HeadPhotoLoss with `weights`), everything that needs no GPU:

  * the library exports the four weighted entry points, added to ABI version 8 without a bump, and rejects bad weight
    arguments before it launches anything;
  * tests/golden/g21_weighted_photo_loss.npz -- written by the reference (tests/golden/make_golden_weighted_photo.py), NaN
    in the photos under zero weights -- is what its generator describes and is reproduced by the oracle's composition
    (tests/photo_checks.py with `weights`) within the project's bounds, maps and head;
  * the inputs the GPU tests use stay inside the caps by the comparison values alone;
  * PhotoLoss / HeadPhotoLoss with a plugin renderer and weights ARE the composed definition bit for bit; NaN photos under
    zero weights give a finite loss and a finite gradient through autograd; normalize="weights"; argument checks;
  * the eight new kernels, compiled with the Makefile's flags: registers, no scratch, the transcendental counts of the
    unweighted loops, four back-to-back loads per render a shading pass in front of their wait, and at most
    WEIGHT_VALU_MARGIN more VALU instructions per render than the unweighted kernel's loops of the same compile.
"""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import head_checks
import photo_checks
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


def test_library_exports_the_weighted_entries_without_an_abi_bump(lib):
    from svbrdf_estimation_amd import _native
    assert lib.svbrdf_abi_version() == 8 and _native.ABI_VERSION == 8
    with open(os.path.join(ROOT, "include", "svbrdf_hip.h")) as f:
        header = f.read()
    assert "#define SVBRDF_ABI_VERSION 8" in header
    for name in wp.ENTRIES:
        assert hasattr(lib, name), name
        assert "SVBRDF_API int %s(" % name in header
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == 16
    assert "WEIGHTS MUST LIE IN [0, 1]" in header and "(12 + 3 S + P + 12) * 4" in header and "(9 + 3 S + P + 9) * 4" in header


@pytest.mark.parametrize("entry", wp.ENTRIES)
def test_weight_argument_errors_come_before_any_launch(lib, entry):
    """-1 null weights, -3 misaligned weights, -2 weight_planes that is neither 1 nor S; and the unweighted siblings' checks
    still hold with the two arguments in place.  Host buffers stand in for device memory: nothing is enqueued."""
    fn = getattr(lib, entry)
    B, S, H = 1, 9, 8
    buf = (ctypes.c_float * 16384)()
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 63) & ~63
    need = lib.svbrdf_rendering_loss_workspace_bytes(B, S, H, H)

    def call(input=p, photos=p + 256, weights=p + 16384, planes=S, scenes=p + 512, xrow=p + 1024, eps=0.1, loss=p + 2048,
             grad=p + 4096, ws=p + 8192, ws_bytes=need, B=B, S=S, H=H, W=H):
        return fn(input, photos, weights, planes, scenes, xrow, ctypes.c_float(eps), loss, grad, ws, ws_bytes, B, S, H, W, None)

    launches = lib.svbrdf_debug_launch_count()
    assert call(weights=None) == -1
    assert lib.svbrdf_last_error()
    assert call(weights=p + 16386) == -3 and call(weights=p + 16385) == -3
    for planes in (0, 2, S + 1, -1):
        assert call(planes=planes) == -2, planes
        assert b"weight_planes" in lib.svbrdf_last_error()
    for name in ("input", "photos", "scenes", "xrow", "loss", "ws"):
        assert call(**{name: None}) == -1, name
    assert call(W=H + 1) == -2 and call(B=0) == -2 and call(S=0, planes=1) == -2 and call(eps=0.0) == -2
    assert call(photos=p + 258) == -3 and call(grad=p + 4098) == -3
    assert call(ws_bytes=need - 8) == -4
    if entry.endswith("host_scenes"):
        assert call(B=17, S=17, planes=17) == -2
    assert lib.svbrdf_debug_launch_count() == launches     # failed calls enqueue and count nothing


# ------------------------------------------------------------------------------------------------ the fixture

@pytest.fixture(scope="module")
def g21(golden):
    g = golden("g21_weighted_photo_loss.npz")
    B, H = int(g["B"]), int(g["H"])
    inp = synth.make_maps(int(g["input_seed"]), B, H)
    enc = head_checks.fixture_input(int(g["enc_seed"]), B, H)
    assert synth.checksum(inp) == str(g["input_sha256"]) and synth.checksum(enc) == str(g["enc_sha256"]), \
        "synthetic inputs are not bit-reproducible here"
    return g, inp, enc


def test_fixture_is_what_its_generator_describes(g21):
    g, inp, enc = g21
    ph, w = g["photos"], g["weights"]
    assert inp.shape == (3, 12, 13, 13) and enc.shape == (3, 9, 13, 13) and g["scenes"].shape == (3, 9, 9)
    assert ph.shape == (3, 9, 3, 13, 13) and w.shape == (3, 9, 13, 13) and ph.dtype == np.float32 and w.dtype == np.float32
    assert w.min() == 0.0 and w.max() == 1.0 and not np.isnan(w).any()
    n0, n1, mid = int((w == 0).sum()), int((w == 1).sum()), int(((w > 0) & (w < 1)).sum())
    assert n0 > w.size // 5 and n1 > w.size // 5 and mid > w.size // 3, (n0, n1, mid)
    row = int(g["masked_row"])
    assert not w[:, :, row, :].any() and w[:, :, row + 1, :].any()                  # a fully masked row
    nan = np.isnan(ph)
    assert nan.any() and nan[:, :, :, row, :].all()
    assert (np.broadcast_to(w[:, :, None], ph.shape)[nan] == 0.0).all()             # NaN only under zero weights
    assert ((w == 0.0) & ~nan[:, :, 0]).any()                                       # ... and not under all of them
    valid = ph[~nan]
    assert valid.min() >= 0.0 and valid.max() <= 1.0
    for k in ("loss", "head_loss"):
        assert g[k].dtype == np.float32 and g[k + "_f64"].dtype == np.float64 and np.isfinite(g[k]) and np.isfinite(g[k + "_f64"])
    assert g["grad_input"].dtype == np.float32 and g["grad_input_f64"].dtype == np.float64 and g["grad_input"].shape == inp.shape
    assert g["grad9"].dtype == np.float32 and g["grad9_f64"].dtype == np.float64 and g["grad9"].shape == enc.shape
    for k in ("grad_input", "grad_input_f64", "grad9", "grad9_f64"):
        assert np.isfinite(g[k]).all() and not g[k][:, :, row, :].any(), k          # the masked row: all-zero gradient
    gdir = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gdir, "MANIFEST_g21_weighted_photo_loss.json")) as f:
        entry = json.load(f)["fixtures"]["g21_weighted_photo_loss.npz"]
    assert entry["generator"] == "tests/golden/make_golden_weighted_photo.py" and os.path.exists(os.path.join(ROOT, entry["generator"]))
    with open(os.path.join(gdir, "g21_weighted_photo_loss.npz"), "rb") as f:
        data = f.read()
    assert hashlib.sha256(data).hexdigest() == entry["sha256"] and len(data) <= 1 << 20


@pytest.mark.parametrize("head", [False, True], ids=["maps", "head"])
def test_oracle_composition_reproduces_the_reference_fixture(g21, head):
    g, inp, enc = g21
    ref = photo_checks.Reference(enc if head else inp, g["photos"], g["scenes"], float(g["eps"]), head=head, weights=g["weights"])
    loss, loss64 = (g["head_loss"], g["head_loss_f64"]) if head else (g["loss"], g["loss_f64"])
    grad, grad64 = (g["grad9"], g["grad9_f64"]) if head else (g["grad_input"], g["grad_input_f64"])
    print("[weighted-photo] g21 %s: fixture loss %.9g (f64 %.12g), oracle %.9g (f64 %.12g); %d tie pixels, %d widened" % (
        "head" if head else "maps", float(loss), float(loss64), ref.loss, ref.loss64, ref.n_ties(), ref.n_widened()))
    tolerances.assert_loss_close(ref.loss, loss, "oracle fp32 vs reference fp32")
    tolerances.assert_loss_close(ref.loss64, loss64, "oracle fp64 vs reference fp64")
    tolerances.assert_loss_close(ref.loss, loss64, "oracle fp32 vs reference fp64")
    what = "g21 %s oracle" % ("head" if head else "maps")
    if head:    # (the reference's double evaluation decodes in double, the composition shades the float32 decode)
        photo_checks.assert_photo_grad_close(ref.grad64, grad64, None, ref.tie, what + " fp64 vs reference fp64")
    else:
        tolerances.assert_grad_close(ref.grad64, grad64, what + " fp64 vs reference fp64", rtol=1e-6, afrac=1e-7)
    n = photo_checks.assert_photo_grad_close(ref.grad, grad, grad64, ref.tie, what + " vs reference")
    assert n <= tolerances.MAX_TIE_PIXELS
    assert not ref.grad[:, :, int(g["masked_row"]), :].any()


def test_gpu_cases_stay_inside_the_caps_by_the_comparison_values_alone():
    """tie pixels and elements that need the widening, fp32 oracle against fp64 oracle, of every input
    tests/test_gpu_weighted_photo_loss.py compares element-wise"""
    for name, H, _, _, tied in wp.CASES:
        for layout in wp.LAYOUTS:
            for head in (False, True) if tied else (False,):
                c, ref = wp.reference(name, layout, head)
                ties, widened = ref.n_ties(), ref.n_widened()
                w = c["weights"][layout]
                print("[weighted-photo] %s %s %s: loss %.9g, %d tie pixels, %d widened; weights %.2f zero, %.2f one" % (
                    name, layout, "head" if head else "maps", ref.loss, ties, widened, (w == 0).mean(), (w == 1).mean()))
                assert ties <= tolerances.MAX_TIE_PIXELS and widened <= tolerances.MAX_WIDENED_GRAD, (name, layout, head)
                assert not ref.grad[:, :, :max(H // 4, 1), :].any() and ref.grad[:, :, H // 4 + 1:, :].any()


# ------------------------------------------------------------------------------------------------ the modules

def _toy(head):
    from svbrdf_estimation_amd import environment
    B, S, H = 2, 3, 8
    x = torch.from_numpy(head_checks.full(33, B, H) if head else synth.make_maps(31, B, H))
    torch.manual_seed(5)
    table = torch.stack([environment.scene_table(1, S - 1) for _ in range(B)])
    photos = torch.rand(B, S, 3, H, H)
    w = torch.from_numpy(wp.weight_field(77, B, S, H))
    return x, photos, table, w


def _definition(x, photos, table, w, eps, head):
    """the specification, literally: (1/N) sum w |log(render + eps) - log(where(w > 0, photo, 0) + eps)|"""
    from svbrdf_estimation_amd import environment, losses
    R = _ToyRenderer()
    maps = losses.decode_head(x) if head else x
    rows = [torch.cat([R.render(sc, maps[b]) for sc in environment.scenes_from_table(table[b])], dim=0) for b in range(x.shape[0])]
    rendered = torch.stack(rows, dim=0)
    wb = w.to(rendered.dtype).unsqueeze(2)
    p = torch.where((wb > 0).expand_as(photos), photos.to(rendered.dtype), torch.zeros((), dtype=rendered.dtype))
    return (wb * (torch.log(rendered + eps) - torch.log(p + eps)).abs()).sum() / rendered.numel()


@pytest.mark.parametrize("head", [False, True], ids=["PhotoLoss", "HeadPhotoLoss"])
def test_plugin_renderer_with_weights_is_the_composed_definition_bitwise(head):
    from svbrdf_estimation_amd import losses
    x, photos, table, w = _toy(head)
    fn = (losses.HeadPhotoLoss if head else losses.PhotoLoss)(_ToyRenderer(), eps=0.05)
    assert not fn.uses_fused_kernel() and fn.normalize == "count"
    spoiled = photos.clone()
    spoiled[(w == 0).unsqueeze(2).expand_as(photos)] = float("nan")        # a zero weight excuses whatever is under it
    for weights in (w, w[:, :1]):
        x0 = x.clone().requires_grad_(True)
        ref = _definition(x0, photos, table, weights, 0.05, head)
        ref.backward()
        assert torch.isfinite(ref) and x0.grad.abs().max() > 0
        for ph in (photos, spoiled if weights is w else photos):
            x1 = x.clone().requires_grad_(True)
            loss = fn(x1, ph, table, weights)
            assert loss.dim() == 0
            loss.backward()
            assert torch.equal(loss, ref) and torch.equal(x1.grad, x0.grad)
            assert torch.isfinite(x1.grad).all() and not x1.grad[:, :, :2, :].any()     # rows masked in every plane
    # [B,H,W] means one shared plane; bool and uint8 masks are converted; positional None is the unweighted path
    assert torch.equal(fn(x, photos, table, w[:, 0]), fn(x, photos, table, w[:, :1]))
    mask = w > 0.5
    assert torch.equal(fn(x, photos, table, mask), fn(x, photos, table, mask.float()))
    assert torch.equal(fn(x, photos, table, mask.to(torch.uint8)), fn(x, photos, table, mask.float()))
    assert torch.equal(fn(x, photos, table, None), fn(x, photos, table))
    assert torch.equal(fn(x, photos, table, torch.ones_like(w)), (_definition(x, photos, table, torch.ones_like(w), 0.05, head)))
    # float64 stays float64
    assert fn(x.double(), photos.double(), table, w).dtype == torch.float64


@pytest.mark.parametrize("head", [False, True], ids=["PhotoLoss", "HeadPhotoLoss"])
def test_normalize_weights_is_the_weighted_mean(head):
    from svbrdf_estimation_amd import losses
    x, photos, table, w = _toy(head)
    cls = losses.HeadPhotoLoss if head else losses.PhotoLoss
    with pytest.raises(ValueError):
        cls(_ToyRenderer(), normalize="mean")
    fn = cls(_ToyRenderer(), eps=0.05, normalize="weights")
    x64, ph64 = x.double(), photos.double()
    for weights in (w, w[:, :1], w[:, 0]):
        w4 = weights if weights.dim() == 4 else weights.unsqueeze(1)
        full = w4.double().expand(w.shape)
        want = _definition(x64, ph64, table, w4, 0.05, head) * (x.shape[0] * 3 * 3 * 64) / (3.0 * full.sum())
        got = fn(x64, ph64, table, weights)
        assert got.dtype == torch.float64 and abs(got.item() - want.item()) <= 1e-12 * abs(want.item()), (got.item(), want.item())
    zero = fn(x64, ph64, table, torch.zeros_like(w))
    assert zero.item() == 0.0
    x1 = x64.clone().requires_grad_(True)
    fn(x1, ph64, table, torch.zeros_like(w)).backward()
    assert not x1.grad.any()
    assert torch.equal(fn(x64, ph64, table), cls(_ToyRenderer(), eps=0.05)(x64, ph64, table))       # no weights: nothing to normalise


def test_weights_are_checked():
    from svbrdf_estimation_amd import _native, losses, renderers
    for head in (False, True):
        x, photos, table, w = _toy(head)
        cls = losses.HeadPhotoLoss if head else losses.PhotoLoss
        for fn in (cls(_ToyRenderer()), cls(renderers.LocalRenderer())):
            with pytest.raises(ValueError, match="minimum over the channels"):
                fn(x, photos, table, w.unsqueeze(2).expand(-1, -1, 3, -1, -1))      # per-channel weights
            with pytest.raises(ValueError):
                fn(x, photos, table, w[:, :2])                                      # neither S nor 1 planes
            with pytest.raises(ValueError):
                fn(x, photos, table, w[:1])                                         # another B
            with pytest.raises(ValueError):
                fn(x, photos, table, w[..., :4])                                    # another W
            with pytest.raises(ValueError):
                fn(x, photos, table, w[0, 0])                                       # [H,W]
            with pytest.raises(TypeError):
                fn(x, photos, table, w.double())
            with pytest.raises(TypeError):
                fn(x, photos, table, w.to(torch.int32))
            with pytest.raises(TypeError):
                fn(x, photos, table, w.numpy())
            with pytest.raises(RuntimeError):
                fn(x, photos, table, w.clone().requires_grad_(True))
            with pytest.raises(ValueError):
                fn(x, photos, table, w.to("meta"))                                  # another device
        # the fused path computes on a ROCm device only: CPU tensors are an error, never a quiet fall-back
        with pytest.raises(_native.NativeLibraryError):
            cls(renderers.LocalRenderer())(x, photos, table, w)


# ------------------------------------------------------------------------------------------------ the kernels
WEIGHT_VALU_MARGIN = 12     # per render over the unweighted loop of the same compile: range check <= 3, one multiply into
                            # 1/N, <= 3 for w |lg|, <= 3 selects, a little for scheduling (measured: 5)


@pytest.fixture(scope="module")
def photo_asm(tmp_path_factory):
    return unit_build.compile_unit_asm(tmp_path_factory.mktemp("isa_wphoto"), "svbrdf_photo_loss", "SCHED_PHOTO")


def _scene_loops(isa_stats, asm, k):
    _, meta, whole, loops, ins, rng = isa_stats.analyse(asm, k)
    scene = sorted(((r, c) for r, c in zip(rng, loops) if c["trans"]), key=lambda rc: -rc[1]["valu"])
    return meta, whole, ins, scene


@needs_hipcc
def test_weighted_kernels_resources_and_scene_loops(photo_asm):
    isa_stats = _isa_stats()
    every = isa_stats.kernels(photo_asm)
    names = sorted(k for k in every if "wphoto" in k)
    assert len(names) == 8, names       # {maps, head} x {device table, by-value table} x {forward only, forward + adjoint}
    assert not [k for k in names if "k_photo_loss" in k or "k_head_photo" in k]
    assert sum("ILb1E" in k for k in names) == 4 and sum("_inl" in k for k in names) == 4 and sum("k_head_w" in k for k in names) == 4
    for k in names:
        meta, whole, ins, scene = _scene_loops(isa_stats, photo_asm, k)
        with_grad, head = "ILb1E" in k, "k_head_w" in k
        # the unweighted kernel of the same shape, same compile
        base = "k_head_photo" if head else "k_photo_loss"
        twin = [t for t in every if base in t and ("_inl" in t) == ("_inl" in k) and ("ILb1E" in t) == with_grad]
        assert len(twin) == 1, (k, twin)
        _, _, _, twin_scene = _scene_loops(isa_stats, photo_asm, twin[0])
        print("%s\n   VGPRs %s, SGPRs %s, occupancy %s, %d instructions" % (
            k, meta["NumVgprs"], meta.get("NumSgprs"), meta["Occupancy"], whole["total"]))
        assert int(meta["NumVgprs"]) <= 128 and int(meta["NumAgprs"]) == 0 and int(meta["Occupancy"]) >= 4, (k, meta)
        assert int(meta["ScratchSize"]) == 0 and whole["scratch"] == 0, (k, meta)
        assert whole["v_div"] == 0 and whole["v_pk"] == 0, (k, whole)
        assert len(scene) == (1 if head else 2) and len(twin_scene) == len(scene), (k, len(scene))
        per = 2 if with_grad else 1          # renders per trip
        trans = [PHOTO_TIED_LOOP_TRANS] if head else [PHOTO_UNTIED_LOOP_TRANS, PHOTO_TIED_LOOP_TRANS]
        for ((a, b), c), (_, t), tr, which in zip(scene, twin_scene, trans, ["tied"] if head else ["untied", "tied"]):
            print("   %s loop: %d VALU per trip (unweighted %d: %+.1f per render), %d transcendental" % (
                which, c["valu"], t["valu"], (c["valu"] - t["valu"]) / per, c["trans"]))
            assert c["trans"] == t["trans"] == tr // 2 * per, (k, which)        # no new transcendentals
            assert c["valu"] <= t["valu"] + WEIGHT_VALU_MARGIN * per, (k, which, c["valu"], t["valu"])
            # the weight is the fourth load of each render's group: nothing but scalar moves of the second resource between
            # them, and no wait the group could satisfy (vmcnt(n), n <= 3) within PREFETCH_MIN_DISTANCE instructions
            body = ins[a:b + 1]
            loads = [i for i, (_, _, mn, _) in enumerate(body) if mn and mn.startswith("buffer_load_dword")]
            assert len(loads) == 4 * per, (k, which, len(loads))
            for g0 in range(0, len(loads), 4):
                grp = loads[g0:g0 + 4]
                between = [body[i][2] for i in range(grp[0], grp[3]) if i not in grp]
                assert len(between) <= 3 and all(mn and mn.startswith(("s_mov_b32", "s_and_b32")) for mn in between), \
                    "%s %s: the four loads are not back to back: %s" % (k, which, between)
                waits = [i for i, (_, _, mn, ops) in enumerate(body)
                         if i > grp[3] and mn == "s_waitcnt" and "vmcnt(" in ops and int(ops.split("vmcnt(")[1].split(")")[0]) <= 3]
                assert waits, "%s: no wait behind the loads" % k
                assert waits[0] - grp[3] >= PREFETCH_MIN_DISTANCE, "%s %s: loads waited for after %d instructions" % (
                    k, which, waits[0] - grp[3])
        if with_grad:
            stores = [ops for _, _, mn, ops in ins if mn and mn.startswith("buffer_store_dword")]
            assert len(stores) == (9 if head else 12) and all("sc0 sc1" in s for s in stores), (k, stores)


def test_source_holds_no_inline_assembly_with_instructions():
    import re
    src = unit_build.read_csrc("svbrdf_photo_loss.hip", "svbrdf_photo_loss_device.h")
    for m in re.finditer(r'asm\s+volatile\s*\(\s*"([^"]*)"', src):
        assert m.group(1) == "", "inline asm with instructions: %r" % m.group(1)
    assert "template <bool WITH_GRAD, bool EARLY_COORDS, bool HEAD = false, bool WEIGHTED = false>" in src
