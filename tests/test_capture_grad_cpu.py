"""The gradient of capture.rectify towards its matrices (svbrdf_estimation_amd/capture.py; csrc/svbrdf_capture_grad.hip:
k_homography_grad; svbrdf_rectify_photos_grad_matrices), everything that needs no GPU:

  * the numpy restatement of the nine terms (tests/capture_grad_checks.py): its pixels' `ok` is the forward restatement's
    weight; in float64, on the float32 run's cells, its sums equal torch's float64 autograd of the composed forward with
    the cell held constant to 1e-10 relative, for k = 1, 2, 4 and both formats, and obey the gauge identity
    sum_i m_i grad_i = 0 (scaling a matrix changes nothing);
  * capture.corner_matrices: patch_homography in float64 to 1e-12, and torch.autograd.gradcheck;
  * the autograd wrapper's argument handling: no CPU path, and matrices without grad take the old path;
  * header, binding and library agree on the two new entries and on D; bad arguments are refused before any launch;
  * the six kernels, compiled with the Makefile's flags: no scratch, IEEE division, an integer atomic only; every earlier
    kernel's machine code was the parent commit's when they came (profiles/r23_capture_grad_codehash.txt), and the library
    holds the code recorded in profiles/r27_capture_refactor_codehash.txt.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import capture_checks as cc
import capture_grad_checks as gc
import synth
import unit_build
from svbrdf_estimation_amd import capture
from test_photo_loss_cpu import _isa_stats, needs_hipcc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC_SIZE, DST_SIZE = (37, 53), (9, 30)


@pytest.fixture(scope="module")
def lib():
    from svbrdf_estimation_amd import _native
    return _native._load()


def _case(u8, k):
    P = 3
    src = cc.u8_source(40 + k, P, *SRC_SIZE, blobs=True) if u8 else cc.float_source(50 + k, P, *SRC_SIZE)
    M = np.stack([cc.matrix(kind, SRC_SIZE, DST_SIZE, p) for p, kind in enumerate(("mild", "outside", "horizon"))])
    G = synth.uniform01(60 + k, (P, 3) + DST_SIZE).astype(np.float32) * 2.0 - 1.0
    lut = capture.gamma_lut().numpy() if u8 else None
    clip = (5, 250) if u8 else (0.02, 0.98)
    return src, M, G, lut, clip


# ------------------------------------------------------------------------------------------------ the oracle itself

@pytest.mark.parametrize("u8", (False, True), ids=("float", "uint8"))
@pytest.mark.parametrize("k", (1, 2, 4))
def test_float64_restatement_is_torch_autograd_and_obeys_the_gauge(u8, k):
    src, M, G, lut, clip = _case(u8, k)
    t32, ok32, cells = gc.grad_terms(src, M, DST_SIZE, G, k, lut, clip)
    assert t32.dtype == np.float32
    # the pixels that contribute are the forward's weight-1 pixels, and the case has refused ones of every kind
    _, w = cc.restatement(src, M, DST_SIZE, k, lut, clip)
    assert np.array_equal(ok32, w > 0) and 0 < ok32[1].mean() < 1 and 0 < ok32[2].mean() < 1 and ok32.any(axis=(1, 2)).all()
    assert not t32[np.broadcast_to(~ok32[:, None, None], t32.shape)].any()
    t64, ok64, _ = gc.grad_terms(src, M, DST_SIZE, G, k, lut, clip, dtype=np.float64, cells=cells)
    assert t64.dtype == np.float64 and np.array_equal(ok64, ok32)
    ref, A = gc.sums(t64)
    auto = gc.autograd_grad(src, M, DST_SIZE, G, k, lut, cells)
    rel = np.abs(ref - auto).max() / np.abs(auto).max()
    gauge = np.abs((M.astype(np.float64) * ref).sum(axis=1))
    scale = np.abs(M.astype(np.float64) * ref).sum(axis=1)
    r32, A32 = gc.sums(t32)
    print("[capture grad] %s k=%d: float64 restatement vs autograd %.3g relative; gauge |sum m g| / sum |m g| %.3g; "
          "float32 terms vs float64 terms, |sum32 - sum64| / A: %.3g" % ("uint8" if u8 else "float", k, rel, (gauge / scale).max(),
                                                                        (np.abs(r32 - ref) / A).max()))
    assert rel <= 1e-10
    assert (gauge <= 1e-10 * scale).all() and (scale > 0).all()


def test_restatement_rules_on_a_hand_made_case():
    """identity on a 4x5 source: fx = fy = 0 everywhere, du = b - a with the right-hand neighbour, and 0 in the last column,
    where the clamped x1 = x0; a pixel whose tap is refused contributes nothing, whatever grad_values holds under it"""
    src = cc.float_source(1, 1, 4, 5)
    M = np.eye(3, dtype=np.float32).reshape(1, 9)
    G = np.ones((1, 3, 4, 5), np.float32)
    t, ok, _ = gc.grad_terms(src, M, (4, 5), G)
    assert ok.all()
    du = np.zeros((3, 4, 5), np.float32)
    du[:, :, :-1] = src[0][:, :, 1:] - src[0][:, :, :-1]
    want = (du[0] + du[1]) + du[2]
    assert cc.same_bits(t[0, 0, 2], want) and not t[0, 0, 2][:, -1].any()           # term 2 = pu = gu / Z = gu
    assert not t[0, 0, 5][-1].any()                                                  # pv: the last row's y1 = y0
    src[0, 1, 2, 3] = np.nan
    G[0, :, 1:3, 2:4] = np.nan
    t2, ok2, _ = gc.grad_terms(src, M, (4, 5), G)
    dead = np.zeros((4, 5), bool)
    dead[1:3, 2:4] = True
    assert np.array_equal(~ok2[0], dead) and np.isfinite(t2).all() and not t2[0, 0][:, dead].any()
    assert cc.same_bits(t2[0, 0][:, ~dead], t[0, 0][:, ~dead])


# ------------------------------------------------------------------------------------------------ corner_matrices

def test_corner_matrices_equal_patch_homography(golden):
    g = golden("g24_capture_corners.npz")
    pts = g["target_points"][..., :2]                       # [8,3,4,2]: eight cameras x three sensors
    for size in ((256, 256), (33, 31)):
        got = capture.corner_matrices(torch.from_numpy(pts), size)
        assert got.dtype == torch.float64 and tuple(got.shape) == (8, 3, 3, 3)
        for a in range(8):
            for b in range(3):
                want = capture.patch_homography(pts[a, b], size, dtype=np.float64)
                assert np.abs(got[a, b].numpy() - want).max() <= 1e-12 * np.abs(want).max(), (a, b)
    one = capture.corner_matrices(torch.from_numpy(pts[0, 0]).float(), 64)          # no leading dimension, float32 in
    assert tuple(one.shape) == (3, 3) and one.dtype == torch.float64 and float(one[2, 2]) == 1.0
    with pytest.raises(ValueError):
        capture.corner_matrices(torch.zeros(4, 3), 64)
    with pytest.raises(ValueError):
        capture.corner_matrices(torch.zeros(4, 2), (1, 8))


def test_corner_matrices_pass_gradcheck():
    c = np.array([[101.25, 57.5], [80.0, 420.75], [590.5, 455.0], [560.0, 40.125]])
    x = torch.tensor(np.stack((c, c + 1.5, c * 0.5)), dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: capture.corner_matrices(t, (33, 31)), (x,))


def test_the_registration_seed_converges_in_float64_on_the_cpu():
    """the GPU suite's registration case, as the issue asks before its seed is fixed: the same loop through the float64
    composition on the CPU ends below half its start error (it ends near 0.0007 px from 3.0)"""
    s = torch.from_numpy(gc.band_limited_source(7, *gc.REG_SRC)).double()

    def rectify(M):
        return cc.torch_composition(s, M.reshape(1, 9), gc.REG_GRID, dtype=torch.float64)

    with torch.no_grad():
        target, tw = rectify(capture.corner_matrices(torch.tensor(gc.REG_CORNERS[None]), gc.REG_GRID))
    assert bool((tw == 1).all())
    c0 = gc.start_corners(gc.REG_SEED)
    end = gc.corner_error(gc.registration_loop(rectify, target, tw, c0, "cpu"))
    print("[capture grad] registration in float64 on the CPU: %.3f -> %.5f px" % (gc.corner_error(c0), end))
    assert abs(gc.corner_error(c0) - gc.REG_OFF) < 1e-9 and end < 0.5 * gc.REG_OFF


# ------------------------------------------------------------------------------------------------ the wrapper's arguments

def test_wrapper_has_no_cpu_path_and_leaves_the_old_path_alone(monkeypatch):
    from svbrdf_estimation_amd import _native
    img = torch.zeros(2, 3, 8, 9)
    M = torch.eye(3, dtype=torch.float64).repeat(2, 1, 1).requires_grad_(True)
    with pytest.raises(_native.NativeLibraryError, match="no CPU fallback"):
        capture.rectify(img, M, 4)
    # matrices without grad (and any matrices under no_grad) take the launch that existed before: no autograd node
    seen = []

    def launch(src, mats, lut, args, lead, want_weights, lens=None):
        assert lens is None
        seen.append((tuple(mats.shape), mats.dtype, args))
        return torch.zeros(lead + (3, 4, 4)), torch.zeros(lead + (4, 4))

    monkeypatch.setattr(capture, "_launch_rectify", launch)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    out, w = capture.rectify(img, M.detach(), 4)
    assert out.grad_fn is None and w.grad_fn is None
    with torch.no_grad():
        out, _ = capture.rectify(img, M, 4)
    assert out.grad_fn is None
    out, w = capture.rectify(img, M, 4, samples=2)
    assert out.grad_fn is not None and out.requires_grad and not w.requires_grad
    assert seen[-1] == ((2, 9), torch.float32, (cc.F32_PLANAR, 2, 8, 9, 4, 4, 2, -np.inf, np.inf)) and len(seen) == 3


# ------------------------------------------------------------------------------------------------ the C ABI and the binding

ENTRY, QUERY = "svbrdf_rectify_photos_grad_matrices", "svbrdf_rectify_grad_workspace_bytes"


def test_library_exports_the_entries_without_an_abi_bump(lib):
    from svbrdf_estimation_amd import _native
    assert lib.svbrdf_abi_version() == 8 and _native.ABI_VERSION == 8
    with open(os.path.join(ROOT, "include", "svbrdf_hip.h")) as f:
        header = f.read()
    assert "#define SVBRDF_ABI_VERSION 8" in header
    assert hasattr(lib, ENTRY) and hasattr(lib, QUERY)
    declared = header.split("SVBRDF_API int %s(" % ENTRY)[1].split(");")[0]
    assert len(_native.SIGNATURES[ENTRY][1]) == 17 == declared.count(",") + 1
    declared = header.split("SVBRDF_API size_t %s(" % QUERY)[1].split(");")[0]
    assert len(_native.SIGNATURES[QUERY][1]) == 3 == declared.count(",") + 1 and _native.SIGNATURES[QUERY][0] is ctypes.c_size_t
    # D: header, binding and the condition of the design
    D = int(re.search(r"#define SVBRDF_RECTIFY_GRAD_DEPTH (\d+)", header).group(1))
    assert D == _native.RECTIFY_GRAD_DEPTH == gc.depth() and 4 * 4 - 1 + 6 + 2 <= D <= 24
    # tickets (4 bytes a photo, padded) and nine words per 64 x 4 tile; 0 outside the limits
    for P, Hd, Wd in ((1, 1, 1), (5, 5, 65), (72, 256, 256), (65535, 4, 64)):
        tiles = ((Wd + 63) // 64) * ((Hd + 3) // 4)
        n = lib.svbrdf_rectify_grad_workspace_bytes(P, Hd, Wd)
        assert 4 * P + 36 * P * tiles <= n <= 4 * P + 36 * P * tiles + 256 and n % 4 == 0, (P, Hd, Wd, n)
    for bad in ((0, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 4, 32769)):
        assert lib.svbrdf_rectify_grad_workspace_bytes(*bad) == 0, bad


def test_argument_errors_come_before_any_launch_and_touch_nothing(lib):
    """the forward's checks with grad_matrices in the place of out, and: -1 for a null grad_values or workspace, -3 for
    grad_values off 4 bytes or a workspace off 8, -4 for a workspace that is too small.  Host buffers stand in for device
    memory and the stream is null: nothing is enqueued, no byte changes."""
    fn = getattr(lib, ENTRY)
    buf = (ctypes.c_float * 16384)()
    for i in range(len(buf)):
        buf[i] = float(i % 251)
    snapshot = bytes(buf)
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 63) & ~63
    nan = float("nan")
    need = lib.svbrdf_rectify_grad_workspace_bytes(2, 3, 3)

    def call(src=p, fmt=1, P=2, Hs=4, Ws=5, mats=p + 4096, Hd=3, Wd=3, k=1, lut=p + 8192, lo=-1.0, hi=256.0, gv=p + 12288,
             gm=p + 16384, ws=p + 20480, nbytes=need):
        f = ctypes.c_float
        return fn(src, fmt, P, Hs, Ws, mats, Hd, Wd, k, lut, f(lo), f(hi), gv, gm, ws, nbytes, None)

    launches = lib.svbrdf_debug_launch_count()
    for fmt in (-1, 2, 7):
        assert call(fmt=fmt) == -2, fmt
        assert b"src_format" in lib.svbrdf_last_error() and ENTRY.encode() in lib.svbrdf_last_error()
    for k in (0, 3, 5, 8, -1):
        assert call(k=k) == -2, k
    for bad in (dict(P=0), dict(Hs=0), dict(Ws=0), dict(Hd=0), dict(Wd=0), dict(P=-1), dict(P=65536), dict(Ws=32769),
                dict(Hd=32769), dict(lo=nan), dict(hi=nan)):
        assert call(**bad) == -2, bad
    for name in ("src", "mats", "gm", "lut", "gv", "ws"):
        assert call(**{name: None}) == -1, name
        assert lib.svbrdf_last_error()
    assert call(fmt=0, lut=None, src=None) == -1
    assert call(mats=p + 4098) == -3 and call(gm=p + 16386) == -3 and call(gv=p + 12289) == -3 and call(lut=p + 8194) == -3
    assert call(fmt=0, src=p + 2) == -3 and call(ws=p + 20484) == -3
    assert call(nbytes=need - 1) == -4 and call(nbytes=0) == -4
    assert b"workspace" in lib.svbrdf_last_error()
    assert lib.svbrdf_debug_launch_count() == launches
    assert bytes(buf) == snapshot


# ------------------------------------------------------------------------------------------------ the kernels

def test_makefile_builds_the_unit_and_earlier_kernels_kept_their_code():
    unit_build.assert_makefile_builds("svbrdf_capture_grad")        # HIPFLAGS and no scheduler option set
    for unit in ("svbrdf_capture", "svbrdf_capture_grad"):
        text = unit_build.assert_includes_shared_header(unit, "svbrdf_capture_device.h")
        assert "int fail(" in unit_build.assert_includes_shared_header(unit, "svbrdf_host.h")
    assert "rectify_cell" in text and "fminf(fmaxf(" in text and "rectify_tap" in text
    text = unit_build.assert_includes_shared_header("svbrdf_capture_grad", "svbrdf_capture_grad_device.h")
    assert "rectify_grad_reduce" in text and "rectify_grad_taps" in text and "shfl_xor_f64" in text and "static_assert" in text
    # profiles/r23_capture_grad_codehash.txt: the diff against the parent's listing holds added lines only, the six kernels
    with open(os.path.join(ROOT, "profiles", "r23_capture_grad_codehash.txt")) as f:
        listing = f.read()
    diff = listing.split("## diff parent new")[1].split("## nm")[0]
    changed = [ln for ln in diff.splitlines() if ln[:1] in ("<", ">")]
    assert len(changed) == 6 and all(ln.startswith("> ") and "k_homography_grad" in ln for ln in changed), changed
    # and the library as built here holds the six kernels and the forward's six with the code recorded when the capture units
    # were put on shared device functions (profiles/r27_capture_refactor_codehash.txt)
    from svbrdf_estimation_amd import _codehash, _native
    with open(os.path.join(ROOT, "profiles", "r27_capture_refactor_codehash.txt")) as f:
        new = f.read().split("## new")[1]
    for u8 in "01":
        for k in "124":
            for name in ("17k_homography_gradILb%sELi%sE" % (u8, k), "9k_rectifyILb%sELi%sE" % (u8, k)):
                got = _codehash.kernel_code_sha256(_native.library_path(), (name,))
                assert got["bytes"] > 1000 and re.search(r"%s\S*\s+%d\s+%s" % (name, got["bytes"], got["sha256"]), new), (name, got)


def test_source_holds_no_float_atomic_no_fma_and_the_clamp_before_the_conversion():
    src = unit_build.read_csrc("svbrdf_capture_grad.hip", "svbrdf_capture_device.h", "svbrdf_capture_grad_device.h")
    assert re.findall(r'#include "(svbrdf_capture\w*\.h)"', src) == ["svbrdf_capture_device.h", "svbrdf_capture_grad_device.h"]
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert not re.search(r"\b(__builtin_)?fmaf?\(|\bfma_\(|\brcp_\(|\bdiv_rn\(|atomicAdd|unsafeAtomic", code)
    # one integer atomic, the ticket; the two atomic stores are plain write-through stores (the partial's words, the reset)
    # (twice: k_homography_grad keeps its own reduction, profiles/r27_capture_refactor.txt, beside the shared one of the header)
    assert re.findall(r"__hip_atomic_\w+", code) == ["__hip_atomic_store", "__hip_atomic_fetch_add", "__hip_atomic_store"] * 2
    assert [m for m in re.findall(r'asm\s+volatile\s*\(\s*"([^"]*)"', code) if m != "s_waitcnt vmcnt(0)"] == []
    # the header's one clamp, and u's and v's of the cell k_homography_grad keeps
    assert code.count("fminf(fmaxf(") == 3 and code.index("fminf(fmaxf(") < code.index("(int)x0f")
    shared = "\n".join(line.split("//")[0] for line in unit_build.read_csrc("svbrdf_capture_device.h", "svbrdf_capture_grad_device.h").splitlines())
    assert shared.count("fminf(fmaxf(") == 1 and shared.index("fminf(fmaxf(") < shared.index("(int)x0f")
    assert re.findall(r"__hip_atomic_\w+", shared) == ["__hip_atomic_store", "__hip_atomic_fetch_add", "__hip_atomic_store"]
    order = [shared.index(w) for w in ("__hip_atomic_store(reinterpret_cast<unsigned *>(mine)", 'asm volatile("s_waitcnt vmcnt(0)"',
                                       "__hip_atomic_fetch_add", "__ATOMIC_ACQUIRE", "(double)all[")]
    assert order == sorted(order) and "__ATOMIC_RELEASE" not in shared
    # the partial goes out write-through and is drained before the ticket; the acquire stands between the ticket and the
    # partials' loads
    order = [code.index(w) for w in ("__hip_atomic_store(reinterpret_cast<unsigned *>(mine)", 'asm volatile("s_waitcnt vmcnt(0)"',
                                     "__hip_atomic_fetch_add", "__ATOMIC_ACQUIRE", "(double)all[")]
    assert order == sorted(order) and "__ATOMIC_RELEASE" not in code


@needs_hipcc
def test_compiled_kernels_use_no_scratch_divide_in_ieee_and_add_no_float_atomically(tmp_path):
    """the unit compiled exactly as the Makefile compiles it: HIPFLAGS and no scheduler option set"""
    asm = unit_build.compile_unit_asm(tmp_path, "svbrdf_capture_grad")
    isa_stats = _isa_stats()
    names = sorted(k for k in isa_stats.kernels(asm) if "k_homography_grad" in k)
    assert len(names) == 6, names
    for k in names:
        _, meta, whole, loops, ins, rng = isa_stats.analyse(asm, k)
        K = int(re.search(r"ILb[01]ELi(\d)E", k).group(1))
        mns = [mn for _, _, mn, _ in ins if mn]
        print("%s\n   VGPRs %s, SGPRs %s, occupancy %s, LDS %s, scratch %s, %d instructions" % (
            k, meta["NumVgprs"], meta.get("NumSgprs"), meta["Occupancy"], meta.get("LDSByteSize"), meta["ScratchSize"], whole["total"]))
        assert int(meta["ScratchSize"]) == 0 and whole["scratch"] == 0 and int(meta["NumAgprs"]) == 0, (k, meta)
        assert int(meta["Occupancy"]) >= 7 and int(meta["NumVgprs"]) <= 72, (k, meta)
        # three IEEE quotients per sub-sample (u, v, 1/Z), and every fused multiply-add belongs to their expansion (5 each)
        assert mns.count("v_div_fixup_f32") == 3 * K * K == mns.count("v_div_fmas_f32"), k
        fmas = sum(1 for mn in mns if mn.startswith(("v_fma_f32", "v_fmac_f32", "v_mad_f32", "v_mac_f32", "v_pk_fma_f32", "v_fma_mix")))
        assert fmas == 5 * 3 * K * K, (k, fmas)
        assert not [mn for mn in mns if mn.startswith("flat_")], k
        atomics = [mn for mn in mns if "atomic" in mn]
        assert atomics == ["global_atomic_add"], (k, atomics)                    # the ticket: an integer, returned
        assert "buffer_inv" in mns and "buffer_wbl2" not in mns, k      # one agent-scope acquire, no L2 write-back
    # per kernel: the partial's write-through store and the ticket's reset, and the acquire
    assert asm.count("buffer_inv sc1") == 6 and len(re.findall(r"global_store_dword v\d+, v\d+, s\[\d+:\d+\] sc1", asm)) == 12


def test_the_recorded_bits_are_the_file_the_manifest_lists(golden):
    """tests/golden/g24_capture_bits.npz (the GPU suite's bit pin of the four entries): 36 float32 arrays of record_bits' shapes,
    the manifest's checksum, and small"""
    import hashlib
    import json
    path = os.path.join(ROOT, "tests", "golden", "g24_capture_bits.npz")
    with open(os.path.join(ROOT, "tests", "golden", "MANIFEST_g24_capture.json")) as f:
        entry = json.load(f)["fixtures"]["g24_capture_bits.npz"]
    with open(path, "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == entry["sha256"]
    assert os.path.getsize(path) < 256 * 1024 and "record_bits" in entry["generator"]
    g = golden("g24_capture_bits.npz")
    P, (Hd, Wd) = gc.BITS_P, gc.BITS_DST
    shapes = {"values": (P, 3, Hd, Wd), "weights": (P, Hd, Wd), "grad_matrices": (P, 9), "lens_values": (P, 3, Hd, Wd),
              "lens_weights": (P, Hd, Wd), "lens_grad": (P, 18)}
    assert sorted(g.files) == sorted("%s_k%d_%s" % (fmt, k, what) for fmt, k in gc.BITS_CASES for what in shapes)
    for name in g.files:
        assert g[name].dtype == np.float32 and g[name].shape == shapes[name.split("_", 2)[2]], name
