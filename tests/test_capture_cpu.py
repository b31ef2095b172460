"""Captured photographs onto the patch grid (svbrdf_estimation_amd/capture.py; csrc/svbrdf_capture.hip: k_rectify;
svbrdf_rectify_photos), everything that needs no GPU:

  * the float64 restatement of the definition (tests/capture_checks.py) against torch's float64 grid_sample, to 1e-10;
  * the float32 restatement -- the oracle of the GPU tests -- against the float64 one, inside a bound that scales with the
    source size and the local spread of the taps, at pixels where validity and tap indices agree (at most 1e-3 of them
    may disagree);
  * the homography helpers: patch_homography lands on the corners, camera_from_corners inverts camera_corners,
    to_perspective's matrix at t = 0 is the identity, and camera_corners equals the reference's own target_points
    (tests/golden/g24_capture_corners.npz) to 1e-12;
  * the library exports the entry without an ABI bump, header and binding agree, every bad argument is rejected before
    anything is launched;
  * the lookup tables;
  * the six kernels, compiled with the Makefile's flags: IEEE division, no fused multiply-add outside it, no scratch.
"""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import capture_checks as cc
import unit_build
from svbrdf_estimation_amd import capture
from test_photo_loss_cpu import _isa_stats, needs_hipcc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = (((97, 131), (32, 32)), ((480, 640), (64, 64)), ((1200, 1600), (256, 256)))


@pytest.fixture(scope="module")
def lib():
    from svbrdf_estimation_amd import _native
    return _native._load()


@pytest.fixture(scope="module")
def restated():
    """the three shapes of the issue, uniform-random float sources through the `mild` and `outside` matrices, restated once
    in float32 and once in float64 (shared by the tests below, never modified)"""
    out = {}
    for n, (src_size, dst_size) in enumerate(SHAPES):
        src = cc.float_source(300 + n, 2, *src_size)
        M = np.stack((cc.matrix("mild", src_size, dst_size, 0), cc.matrix("outside", src_size, dst_size, 1)))
        out[src_size] = (src, M, dst_size, cc.restatement(src, M, dst_size, detail=True),
                         cc.restatement(src, M, dst_size, dtype=np.float64, detail=True))
    return out


# ------------------------------------------------------------------------------------------------ the oracle itself

@pytest.mark.parametrize("src_size", [s for s, _ in SHAPES])
def test_float64_restatement_is_torch_grid_sample(restated, src_size):
    src, M, dst_size, _, (v64, w64, _) = restated[src_size]
    ref, wref = cc.torch_composition(torch.from_numpy(src).double(), torch.from_numpy(M), dst_size, dtype=torch.float64)
    valid = w64 > 0
    assert np.array_equal(valid, wref.numpy() > 0) and valid[0].all() and 0 < valid[1].mean() < 1
    err = np.abs(v64 - ref.numpy())[np.broadcast_to(valid[:, None], v64.shape)].max()
    print("[capture] float64 restatement vs torch float64 grid_sample, %dx%d -> %dx%d: max err %.3g" % (src_size + dst_size + (err,)))
    assert err <= 1e-10
    assert not v64[~np.broadcast_to(valid[:, None], v64.shape)].any()


@pytest.mark.parametrize("src_size", [s for s, _ in SHAPES])
def test_float32_restatement_against_float64(restated, src_size):
    """err <= F32_ERROR_FACTOR (2^-23 max(Hs, Ws) spread + 2^-22 |value|) where validity and every tap index agree; the
    share of pixels where they do not is printed and capped at 1e-3"""
    src, M, dst_size, (v32, w32, i32), (v64, w64, i64) = restated[src_size]
    assert v32.dtype == np.float32 and v64.dtype == np.float64
    agree = ((i32["valid"] == i64["valid"]) & (i32["x0"] == i64["x0"]) & (i32["y0"] == i64["y0"])).all(axis=1) & (w32 == w64)
    excluded = 1.0 - agree.mean()
    bound = 2.0 ** -23 * max(src_size) * i64["spread"][:, None] + 2.0 ** -22 * np.abs(v64)
    sel = np.broadcast_to((agree & (w64 > 0))[:, None], v64.shape)
    ratio = (np.abs(v32.astype(np.float64) - v64)[sel] / bound[sel]).max()
    print("[capture] float32 vs float64 restatement, %dx%d -> %dx%d: %d of %d pixels excluded (share %.2e), max err %.3g, "
          "err/bound-unit %.3f (asserted <= %.3f)" % (src_size + dst_size + (int((~agree).sum()), agree.size, excluded,
          np.abs(v32 - v64)[sel].max(), ratio, cc.F32_ERROR_FACTOR)))
    assert excluded <= cc.MAX_EXCLUDED_SHARE
    assert ratio <= cc.F32_ERROR_FACTOR
    assert cc.F32_ERROR_FACTOR == 2.0 * cc.F32_ERROR_MEASURED


def test_restatement_rules_on_a_hand_made_case():
    """identity on a 4x5 source: the output is the source; a NaN texel zeroes itself only (x1, y1 clamp at the far edges
    apart: the texel left of and above it too, whose taps b, c, d touch it); k = 2 touches the neighbours on every side,
    and refuses the border pixels, whose outer sub-samples lie a quarter pixel outside the source"""
    src = cc.float_source(1, 1, 4, 5)
    M = np.eye(3, dtype=np.float32).reshape(1, 9)
    v, w = cc.restatement(src, M, (4, 5))
    assert cc.same_bits(v, src) and (w == 1).all()
    src[0, 1, 2, 3] = np.nan
    v, w = cc.restatement(src, M, (4, 5))
    dead = np.zeros((4, 5), bool)
    dead[1:3, 2:4] = True
    assert np.array_equal(w[0] == 0, dead) and not v[0][:, dead].any() and cc.same_bits(v[0][:, ~dead], src[0][:, ~dead])
    v2, w2 = cc.restatement(src, M, (4, 5), k=2)
    dead2 = np.zeros((4, 5), bool)
    dead2[1:4, 2:5] = True                                  # sub-samples a quarter pixel off touch the texels on every side
    dead2[0], dead2[-1], dead2[:, 0], dead2[:, -1] = True, True, True, True     # and the outermost ones leave the source
    assert np.array_equal(w2[0] == 0, dead2) and (~dead2).sum() == 2
    # thresholds: <= lo and >= hi refuse, the values between pass; pixel 2's tap b is texel 3, refused with fx = 0 too
    src = np.full((1, 3, 1, 4), 0.5, np.float32)
    src[0, 0, 0, 0], src[0, 2, 0, 3] = 0.25, 0.75
    eye = np.eye(3, dtype=np.float32).reshape(1, 9)
    assert cc.restatement(src, eye, (1, 4), clip=(0.25, 0.75))[1].tolist() == [[[0.0, 1.0, 0.0, 0.0]]]
    assert cc.restatement(src, eye, (1, 4), clip=(0.2, 0.8))[1].tolist() == [[[1.0, 1.0, 1.0, 1.0]]]


# ------------------------------------------------------------------------------------------------ homography helpers

CAMERAS = ((0.0, 0.0, 2.0), (0.3, -0.4, 1.5), (-1.2, 0.8, 2.5), (1.0, 1.0, 1.0), (0.0, -1.5, 0.9), (-0.2, 0.1, 3.0))


def test_patch_homography_lands_on_the_corners():
    corners = np.array([[101.25, 57.5], [80.0, 420.75], [590.5, 455.0], [560.0, 40.125]])
    for size in ((256, 256), (33, 31), 64):
        H, W = (size, size) if isinstance(size, int) else size
        M = capture.patch_homography(corners, size, dtype=np.float64)
        grid = np.array([[0, 0, 1], [0, H - 1, 1], [W - 1, H - 1, 1], [W - 1, 0, 1]], np.float64)
        img = (M @ grid.T).T
        got = img[:, :2] / img[:, 2:3]
        assert np.abs(got - corners).max() <= 1e-9 * np.abs(corners).max()
        M32 = capture.patch_homography(corners, size)
        assert M32.dtype == np.float32 and np.array_equal(M32, M.astype(np.float32))       # rounded once, at the end
    with pytest.raises(ValueError):
        capture.patch_homography(corners, (1, 8))


@pytest.mark.parametrize("sensor", ((640, 480), (512, 512)))
def test_camera_from_corners_inverts_camera_corners(sensor):
    assert len(CAMERAS) == 6 and CAMERAS[0][:2] == (0.0, 0.0)          # one straight overhead
    for C in CAMERAS:
        back = capture.camera_from_corners(capture.camera_corners(C, sensor), sensor)
        assert np.abs(back - np.asarray(C)).max() <= 1e-6, (C, back)


def test_overhead_camera_sees_the_patch_fill_the_sensor():
    """from one unit above, focal length = half the width: the 2x2 patch spans the sensor's width, its centre the centre"""
    c = capture.camera_corners((0.0, 0.0, 1.0), (200, 200))
    assert np.allclose(c, [[0, 0], [0, 200], [200, 200], [200, 0]], atol=1e-12)


def test_to_perspective_matrix_is_the_identity_at_t_zero_and_the_inverse_at_one():
    for C in CAMERAS[:3]:
        assert np.array_equal(capture.perspective_matrix(C, (640, 480), (32, 32), t=0.0), np.eye(3, dtype=np.float32))
        G = capture.patch_homography(capture.camera_corners(C, (640, 480)), (32, 32), dtype=np.float64)
        Minv = capture.perspective_matrix(C, (640, 480), (32, 32), t=1.0, dtype=np.float64)
        assert np.abs(Minv @ G - np.eye(3)).max() <= 1e-9


def test_camera_corners_equal_the_reference_fixture(golden):
    """tests/golden/g24_capture_corners.npz: OrthoToPerspectiveMapping(camera, sensor_size).target_points of the reference
    itself, eight cameras x three sensor sizes, the overhead case among them"""
    g = golden("g24_capture_corners.npz")
    cams, sensors, want = g["cameras"], g["sensor_sizes"], g["target_points"]
    assert cams.shape == (8, 3) and sensors.shape == (3, 2) and want.shape == (8, 3, 4, 3)
    assert any(c[0] == 0.0 and c[1] == 0.0 for c in cams)
    for a, C in enumerate(cams):
        for b, sensor in enumerate(sensors):
            got = capture.camera_corners(C, tuple(int(s) for s in sensor))
            assert np.abs(got - want[a, b][:, :2]).max() <= 1e-12 * np.abs(want[a, b]).max(), (C, sensor)
            assert np.array_equal(want[a, b][:, 2], np.ones(4))
    with open(os.path.join(ROOT, "tests", "golden", "MANIFEST_g24_capture.json")) as f:
        entry = json.load(f)["fixtures"]["g24_capture_corners.npz"]
    assert "cv2" in entry["not_covered"]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g24_capture_corners.npz")) < 10 * 1024


# ------------------------------------------------------------------------------------------------ lookup tables

def test_lookup_tables():
    for lut in (capture.gamma_lut(), capture.gamma_lut(1.0), capture.srgb_lut()):
        t = lut.numpy()
        assert t.dtype == np.float32 and t.shape == (256,) and t[0] == 0.0 and t[255] == 1.0 and (np.diff(t) > 0).all()
    g = capture.gamma_lut().numpy()
    assert np.array_equal(g, ((np.arange(256) / 255.0) ** 2.2).astype(np.float32))
    assert np.array_equal(capture.gamma_lut(1.0).numpy(), (np.arange(256) / 255.0).astype(np.float32))
    s = capture.srgb_lut().numpy()
    assert abs(float(s[10]) - 10 / 255.0 / 12.92) < 1e-9 and abs(float(s[128]) - 0.2158605) < 1e-6


# ------------------------------------------------------------------------------------------------ the C ABI and the binding

ENTRY = "svbrdf_rectify_photos"


def test_library_exports_the_entry_without_an_abi_bump(lib):
    from svbrdf_estimation_amd import _native
    assert lib.svbrdf_abi_version() == 8 and _native.ABI_VERSION == 8
    with open(os.path.join(ROOT, "include", "svbrdf_hip.h")) as f:
        header = f.read()
    assert "#define SVBRDF_ABI_VERSION 8" in header
    assert hasattr(lib, ENTRY)
    declared = header.split("SVBRDF_API int %s(" % ENTRY)[1].split(");")[0]
    assert ENTRY in _native.SIGNATURES and len(_native.SIGNATURES[ENTRY][1]) == 15 == declared.count(",") + 1
    assert "#define SVBRDF_RECTIFY_F32_PLANAR 0" in header and "#define SVBRDF_RECTIFY_U8_INTERLEAVED 1" in header
    assert (capture.F32_PLANAR, capture.U8_INTERLEAVED) == (0, 1) == (cc.F32_PLANAR, cc.U8_INTERLEAVED)


def test_argument_errors_come_before_any_launch_and_touch_nothing(lib):
    """-2 for a bad format, k outside {1, 2, 4}, a size < 1 or beyond the limits, a NaN threshold; -1 for a null src,
    matrices, out, or lut with uint8 sources (weights_out and a float source's lut may be null); -3 for a misaligned float
    pointer.  Host buffers stand in for device memory and the stream is null: nothing is enqueued, no byte changes."""
    fn = getattr(lib, ENTRY)
    buf = (ctypes.c_float * 8192)()
    for i in range(len(buf)):
        buf[i] = float(i % 251)
    snapshot = bytes(buf)
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 63) & ~63
    nan = float("nan")

    def call(src=p, fmt=1, P=2, Hs=4, Ws=5, mats=p + 4096, Hd=3, Wd=3, k=1, lut=p + 8192, lo=-1.0, hi=256.0, out=p + 12288,
             w=p + 16384):
        f = ctypes.c_float
        return fn(src, fmt, P, Hs, Ws, mats, Hd, Wd, k, lut, f(lo), f(hi), out, w, None)

    launches = lib.svbrdf_debug_launch_count()
    for fmt in (-1, 2, 7):
        assert call(fmt=fmt) == -2, fmt
        assert b"src_format" in lib.svbrdf_last_error()
    for k in (0, 3, 5, 8, -1):
        assert call(k=k) == -2, k
        assert b"k must be" in lib.svbrdf_last_error()
    for bad in (dict(P=0), dict(Hs=0), dict(Ws=0), dict(Hd=0), dict(Wd=0), dict(P=-1), dict(Hs=-4), dict(P=65536), dict(Ws=32769),
                dict(Hd=32769), dict(lo=nan), dict(hi=nan)):
        assert call(**bad) == -2, bad
    for name in ("src", "mats", "out", "lut"):
        assert call(**{name: None}) == -1, name
        assert lib.svbrdf_last_error()
    assert call(fmt=0, lut=None, src=None) == -1
    assert call(mats=p + 4098) == -3 and call(out=p + 12290) == -3 and call(w=p + 16385) == -3 and call(lut=p + 8194) == -3
    assert call(fmt=0, src=p + 2) == -3
    assert lib.svbrdf_debug_launch_count() == launches
    assert bytes(buf) == snapshot


def test_python_layer_rejects_bad_arguments_and_never_falls_back():
    from svbrdf_estimation_amd import _native
    img = torch.zeros(2, 8, 9, 3, dtype=torch.uint8)
    with pytest.raises(_native.NativeLibraryError):         # a host tensor: no CPU path
        capture.rectify(img, np.eye(3), 4, lut=capture.gamma_lut())
    with pytest.raises(TypeError):
        capture.rectify(img.numpy(), np.eye(3), 4)
    with pytest.raises(TypeError):
        capture.to_perspective(torch.zeros(3, 8, 8, dtype=torch.float64), (0, 0, 2), (64, 48))
    with pytest.raises(ValueError):
        capture.camera_corners((0.0, 0.0, 0.0), (64, 48))
    with pytest.raises(ValueError):
        capture._device_matrices(np.zeros((3, 3, 3)), (2,), torch.device("cpu"))
    m = capture._device_matrices(np.eye(3), (2, 3), torch.device("cpu"))
    assert tuple(m.shape) == (6, 9) and m.dtype == torch.float32 and torch.equal(m[4], torch.eye(3).reshape(9))


# ------------------------------------------------------------------------------------------------ the kernels

def test_makefile_builds_the_unit_into_the_library_and_earlier_kernels_kept_their_code():
    unit_build.assert_makefile_builds("svbrdf_capture")        # HIPFLAGS and no scheduler option set
    # profiles/r21_capture_codehash.txt: the diff against the parent's listing holds added lines only, the six k_rectify
    with open(os.path.join(ROOT, "profiles", "r21_capture_codehash.txt")) as f:
        text = f.read()
    diff = text.split("## diff parent new")[1].split("## new")[0]
    changed = [ln for ln in diff.splitlines() if ln[:1] in ("<", ">")]
    assert len(changed) == 6 and all(ln.startswith("> ") and "k_rectify" in ln for ln in changed), changed
    # and the library as built here holds the six kernels
    from svbrdf_estimation_amd import _codehash, _native
    for u8 in "01":
        for k in "124":
            assert _codehash.kernel_code_sha256(_native.library_path(), ("k_rectify", "ILb%sELi%sE" % (u8, k)))["bytes"] > 1000


def test_source_holds_no_inline_assembly_and_no_fma():
    src = unit_build.read_csrc("svbrdf_capture.hip", "svbrdf_capture_device.h")     # the unit and the capture header it includes
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert not re.search(r"\basm\b|\b(__builtin_)?fmaf?\(|\bfma_\(|\brcp_\(|\bdiv_rn\(|atomic", code)
    assert code.count("fminf(fmaxf(") == 1 and code.index("fminf(fmaxf(") < code.index("(int)x0f")     # one clamp, for u and v
    assert "int fail(" in unit_build.assert_includes_shared_header("svbrdf_capture", "svbrdf_host.h")
    text = unit_build.assert_includes_shared_header("svbrdf_capture", "svbrdf_capture_device.h")
    assert "rectify_cell" in text and "rectify_accumulate" in text and "rectify_store" in text and "rectify_dispatch" in text
    assert re.findall(r'#include "(svbrdf_capture\w*\.h)"', unit_build.read_csrc("svbrdf_capture.hip")) == ["svbrdf_capture_device.h"]


@needs_hipcc
def test_compiled_kernels_divide_in_ieee_and_use_no_scratch(tmp_path):
    """the unit compiled exactly as the Makefile compiles it: HIPFLAGS and no scheduler option set"""
    flags = unit_build.make_var("HIPFLAGS")
    assert "-ffp-contract=off" in flags and "-fno-fast-math" in flags
    asm = unit_build.compile_unit_asm(tmp_path, "svbrdf_capture")
    isa_stats = _isa_stats()
    names = sorted(k for k in isa_stats.kernels(asm) if "k_rectify" in k)
    assert len(names) == 6, names
    for k in names:
        _, meta, whole, loops, ins, rng = isa_stats.analyse(asm, k)
        K = int(re.search(r"ILb[01]ELi(\d)E", k).group(1))
        u8 = "ILb1E" in k
        mns = [mn for _, _, mn, _ in ins if mn]
        print("%s\n   VGPRs %s, SGPRs %s, occupancy %s, LDS %s, %d instructions" % (
            k, meta["NumVgprs"], meta.get("NumSgprs"), meta["Occupancy"], meta.get("LDSByteSize"), whole["total"]))
        assert int(meta["ScratchSize"]) == 0 and whole["scratch"] == 0 and int(meta["NumAgprs"]) == 0, (k, meta)
        assert int(meta["Occupancy"]) == 8 and int(meta["NumVgprs"]) <= 64, (k, meta)
        # two IEEE quotients per sub-sample, and every fused multiply-add belongs to their expansion (5 each)
        assert mns.count("v_div_fixup_f32") == 2 * K * K == mns.count("v_div_fmas_f32"), k
        fmas = sum(1 for mn in mns if mn.startswith(("v_fma_f32", "v_fmac_f32", "v_mad_f32", "v_mac_f32", "v_pk_fma_f32", "v_fma_mix")))
        assert fmas == 5 * 2 * K * K, (k, fmas)
        assert not [mn for mn in mns if mn.startswith("flat_") or "atomic" in mn], k
        stores = [mn for mn in mns if mn.startswith(("global_store", "buffer_store"))]
        assert len(stores) == 4 and all(mn.endswith("dword") for mn in stores), (k, stores)
        loads = [mn for mn in mns if mn.startswith(("global_load", "buffer_load"))]
        if u8:      # the table's load, then a tap's three bytes in three byte loads or (the compiler's merge) a short and a byte
            assert loads[0] == "global_load_dword" and 8 * K * K <= len(loads) - 1 <= 12 * K * K, (k, len(loads))
            assert all(mn.endswith(("ubyte", "ushort")) for mn in loads[1:]), (k, set(loads))
        else:
            assert len(loads) == 12 * K * K and all(mn.endswith("dword") for mn in loads), (k, len(loads), set(loads))
