"""capture.rectify(..., lens=) (svbrdf_estimation_amd/capture.py; csrc/svbrdf_capture_lens.hip, svbrdf_capture_lens_grad.hip;
svbrdf_rectify_photos_lens, svbrdf_rectify_photos_lens_grad), everything that needs no GPU:

  * the numpy restatement (tests/capture_lens_checks.py): with the null lens it is capture_checks.restatement bit for bit;
    in float64 it is torch's grid_sample on distorted coordinates; float32 against float64 within a measured factor;
  * a hand-made case: distort_points against OpenCV's documented formula worked out by hand, and a sub-sample with mono <= 0;
  * undistort_points inverts distort_points, and raises beyond the fold;
  * the eighteen gradient terms in float64 on the float32 cells against torch's float64 autograd, and gradcheck;
  * the refinement dry run: k1 alone, then k1 with the corners, in float64 on the CPU;
  * the wrapper's argument handling, the C ABI's checks, the Makefile, the source text and the compiled kernels.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import capture_checks as cc
import capture_grad_checks as gc
import capture_lens_checks as lc
import synth
import unit_build
from svbrdf_estimation_amd import capture
from test_gpu_capture import HOSTILE
from test_photo_loss_cpu import _isa_stats, needs_hipcc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = (((97, 131), (32, 32)), ((480, 640), (64, 64)), ((1200, 1600), (256, 256)))
SRC_SIZE, DST_SIZE = (37, 53), (9, 30)
FORWARD, GRAD, QUERY = "svbrdf_rectify_photos_lens", "svbrdf_rectify_photos_lens_grad", "svbrdf_rectify_lens_grad_workspace_bytes"


@pytest.fixture(scope="module")
def lib():
    from svbrdf_estimation_amd import _native
    return _native._load()


@pytest.fixture(scope="module")
def restated():
    """the three shapes, uniform-random float sources; photo 0: `mild` under `barrel`, photo 1: `outside` under `pincushion`,
    photo 2: `mild` under `pincushion`, photo 3: `outside` under `barrel`; restated once in float32 and once in float64
    (shared by the tests below, never modified)"""
    out = {}
    for n, (src_size, dst_size) in enumerate(SHAPES):
        src = cc.float_source(500 + n, 4, *src_size)
        M = np.stack([cc.matrix(kind, src_size, dst_size, p) for p, kind in enumerate(("mild", "outside", "mild", "outside"))])
        L = np.stack([lc.lens(kind, src_size, p) for p, kind in enumerate(("barrel", "pincushion", "pincushion", "barrel"))])
        out[src_size] = (src, M, L, dst_size, lc.restatement(src, M, L, dst_size, detail=True),
                         lc.restatement(src, M, L, dst_size, dtype=np.float64, detail=True))
    return out


# ------------------------------------------------------------------------------------------------ the oracle itself

@pytest.mark.parametrize("k", (1, 2))
@pytest.mark.parametrize("shape", (((5, 7), (3, 70)), ((37, 53), (9, 30)), ((97, 131), (32, 32))), ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
def test_null_lens_is_the_pinhole_restatement_bit_for_bit(shape, k):
    """all five matrix kinds and the hostile matrices, both formats: every added statement is exact under (1,1,0,...,0)"""
    src_size, dst_size = shape
    for fmt in ("float32", "uint8"):
        rows = [cc.matrix(kind, src_size, dst_size, p) for p, kind in enumerate(cc.KINDS)] + list(HOSTILE.values())
        M = np.stack(rows)
        P = len(rows)
        src = cc.u8_source(7, P, *src_size, blobs=True) if fmt == "uint8" else cc.float_source(8, P, *src_size)
        lut = capture.gamma_lut().numpy() if fmt == "uint8" else None
        clip = (5, 250) if fmt == "uint8" else (0.02, 0.98)
        want = cc.restatement(src, M, dst_size, k, lut, clip)
        got = lc.restatement(src, M, lc.lenses("null", src_size, P), dst_size, k, lut, clip)
        assert cc.same_bits(got[0], want[0]) and cc.same_bits(got[1], want[1]), (fmt, cc.count_differing(got[0], want[0]))
        assert want[1][:3].any() and not want[1][5:].any()
        # and the nine matrix terms of the gradient are the pinhole gradient's (up to the sign of a zero)
        G = synth.uniform01(9, (P, 3) + dst_size).astype(np.float32) * 2.0 - 1.0
        t_lens, ok_lens, _ = lc.grad_terms(src, M, lc.lenses("null", src_size, P), dst_size, G, k, lut, clip)
        t_pin, ok_pin, _ = gc.grad_terms(src, M, dst_size, G, k, lut, clip)
        assert np.array_equal(ok_lens, ok_pin) and np.array_equal(t_lens[:, :, :9], t_pin)


@pytest.mark.parametrize("src_size", [s for s, _ in SHAPES])
def test_float64_restatement_is_torch_grid_sample_on_distorted_coordinates(restated, src_size):
    src, M, L, dst_size, _, (v64, w64, _) = restated[src_size]
    ref, wref = lc.torch_composition(torch.from_numpy(src).double(), torch.from_numpy(M), torch.from_numpy(L), dst_size,
                                     dtype=torch.float64)
    valid = w64 > 0
    assert np.array_equal(valid, wref.numpy() > 0) and valid[0].all() and 0 < valid[1].mean() < 1
    err = np.abs(v64 - ref.numpy())[np.broadcast_to(valid[:, None], v64.shape)].max()
    print("[capture lens] float64 restatement vs torch float64 grid_sample, %dx%d -> %dx%d: max err %.3g" % (src_size + dst_size + (err,)))
    assert err <= 1e-10
    assert not v64[~np.broadcast_to(valid[:, None], v64.shape)].any()
    # the lens moves the taps: not the pinhole result
    pin, _ = cc.restatement(src, M, dst_size, dtype=np.float64)
    assert np.abs(pin - v64)[np.broadcast_to(valid[:, None], v64.shape)].max() > 1e-3


@pytest.mark.parametrize("src_size", [s for s, _ in SHAPES])
def test_float32_restatement_against_float64(restated, src_size):
    """err <= F32_LENS_ERROR_FACTOR (2^-23 max(Hs, Ws) spread + 2^-22 |value|) where validity and every tap cell agree; the
    share of pixels where they do not is printed and capped at capture_checks.MAX_EXCLUDED_SHARE"""
    src, M, L, dst_size, (v32, w32, i32), (v64, w64, i64) = restated[src_size]
    assert v32.dtype == np.float32 and v64.dtype == np.float64
    agree = ((i32["valid"] == i64["valid"]) & (i32["x0"] == i64["x0"]) & (i32["y0"] == i64["y0"])).all(axis=1) & (w32 == w64)
    excluded = 1.0 - agree.mean()
    bound = 2.0 ** -23 * max(src_size) * i64["spread"][:, None] + 2.0 ** -22 * np.abs(v64)
    sel = np.broadcast_to((agree & (w64 > 0))[:, None], v64.shape)
    ratio = (np.abs(v32.astype(np.float64) - v64)[sel] / bound[sel]).max()
    print("[capture lens] float32 vs float64 restatement, %dx%d -> %dx%d: %d of %d pixels excluded (share %.2e), max err %.3g, "
          "err/bound-unit %.3f (asserted <= %.3f)" % (src_size + dst_size + (int((~agree).sum()), agree.size, excluded,
          np.abs(v32 - v64)[sel].max(), ratio, lc.F32_LENS_ERROR_FACTOR)))
    assert excluded <= cc.MAX_EXCLUDED_SHARE == 1e-3
    assert ratio <= lc.F32_LENS_ERROR_FACTOR
    assert lc.F32_LENS_ERROR_FACTOR == 2.0 * lc.F32_LENS_ERROR_MEASURED


def test_hand_made_case():
    """OpenCV's documented model, worked out by hand.  Lens fx = 100, fy = 50, cx = 10, cy = 20, k1 = -0.5, k2 = 0.25, p1 =
    0.01, p2 = -0.02, k3 = 0.125.
      (10, 20): xn = yn = 0 -> the principal point stays.
      (110, 20): xn = 1, yn = 0, r2 = 1: rad = 1 - 0.5 + 0.25 + 0.125 = 0.875; xd = 0.875 + 2 p1 0 + p2 (1 + 2) = 0.815;
                 yd = 0 + p1 (1 + 0) + 0 = 0.01 -> (91.5, 20.5).
      (60, 70): xn = 0.5, yn = 1, r2 = 1.25: rad = 1 - 0.625 + 0.390625 + 0.244140625 = 1.009765625;
                 xd = 0.5048828125 + 2 (0.01) 0.5 + (-0.02)(1.25 + 0.5) = 0.4798828125;
                 yd = 1.009765625 + 0.01 (1.25 + 2) + 2 (-0.02) 0.5 = 1.022265625 -> (57.98828125, 71.11328125)."""
    L = capture.lens_table(100, 50, 10, 20, -0.5, 0.25, 0.01, -0.02, 0.125)
    assert L.dtype == torch.float32 and tuple(L.shape) == (9,)
    pts = np.array([[10.0, 20.0], [110.0, 20.0], [60.0, 70.0]])
    want = np.array([[10.0, 20.0], [91.5, 20.5], [57.98828125, 71.11328125]])
    got = capture.distort_points(pts, np.array([100, 50, 10, 20, -0.5, 0.25, 0.01, -0.02, 0.125]))
    assert np.abs(got - want).max() <= 1e-12, got
    # (the float32 table holds roundings of 0.01 and -0.02: 2^-24 relative, times fx)
    assert np.abs(capture.distort_points(pts, L) - want).max() <= 1e-6
    # pinhole_lens: this module's camera
    assert capture.pinhole_lens((640, 480)).tolist() == [320.0, 320.0, 320.0, 240.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    # a 2 x 2 source under k1 = -1, fx = fy = 1, centre (0, 0), k = 2 on a 1 x 1 grid whose sub-samples sit at (+-0.25, +-0.25)
    # after a translation by (0.5, 0.5) -> ideal points (0.25, 0.25), (0.75, 0.25), (0.25, 0.75), (0.75, 0.75):
    # r2 = 0.125, 0.625, 0.625, 1.125 -> mono = 1 - 3 r2 = 0.625, -0.875, -0.875, -2.375: three of four refused by mono
    # alone although rad = 1 - r2 keeps (ud, vd) inside the 2 x 2 source for the first three
    src = np.full((1, 3, 2, 2), 0.5, np.float32)
    M = np.array([[1, 0, 0.5, 0, 1, 0.5, 0, 0, 1]], np.float32)
    fold = np.array([[1, 1, 0, 0, -1, 0, 0, 0, 0]], np.float32)
    v, w, info = lc.restatement(src, M, fold, (1, 1), k=2, detail=True)
    assert info["valid"][0, :, 0, 0].tolist() == [True, False, False, False]
    assert info["mono_refused"][0, :, 0, 0].tolist() == [False, True, True, False]      # the fourth also leaves: rad < 0
    assert not v.any() and not w.any()
    v1, w1 = lc.restatement(src, np.array([[1, 0, 0.25, 0, 1, 0.25, 0, 0, 1]], np.float32), fold, (1, 1), k=1)
    assert w1.all() and (v1 == 0.5).all()


def test_the_restatements_polynomial_is_distort_points():
    """capture.distort_points is the one statement of the polynomial that is held against values worked out by hand (above);
    the numpy restatement's (ud, vd) and torch_lens_map -- which the kernel's oracle and the composed check are written from
    -- must be it: with the identity matrix u = x, v = y, so the map of a grid of points is the lens alone.  A lens with all
    nine entries distinct and p1 != p2, so that a transposition of the two shows."""
    L = np.array([100, 50, 10, 20, -0.5, 0.25, 0.01, -0.02, 0.125])
    xs, ys = np.meshgrid(np.linspace(-40.0, 90.0, 14), np.linspace(-15.0, 60.0, 11))
    want = capture.distort_points(np.stack((xs, ys), axis=-1), L)
    g = lc._lens_map(np.eye(3).reshape(9), L, xs, ys, np.float64)
    assert np.abs(g["ud"] - want[..., 0]).max() <= 1e-11 and np.abs(g["vd"] - want[..., 1]).max() <= 1e-11
    ud, vd, mono = lc.torch_lens_map(torch.from_numpy(xs), torch.from_numpy(ys), [float(v) for v in L])
    assert np.abs(ud.numpy() - want[..., 0]).max() <= 1e-11 and np.abs(vd.numpy() - want[..., 1]).max() <= 1e-11
    assert np.abs(mono.numpy() - g["mono"]).max() <= 1e-12
    swapped = L.copy()
    swapped[6], swapped[7] = L[7], L[6]
    assert np.abs(capture.distort_points(np.stack((xs, ys), axis=-1), swapped) - want).max() > 1e-2     # the check can see it
    # and in float32, through the whole restatement: the cell of every valid sub-sample is floor(distort_points)
    src = cc.float_source(2, 1, 80, 120)
    row = np.array([[100, 50, 60, 40, -0.5, 0.25, 0.01, -0.02, 0.125]], np.float32)
    _, w, info = lc.restatement(src, np.eye(3, dtype=np.float32).reshape(1, 9), row, (80, 120), detail=True)
    yy, xx = np.mgrid[0:80, 0:120].astype(np.float64)
    there = capture.distort_points(np.stack((xx, yy), axis=-1), row[0].astype(np.float64))
    clear = info["valid"][0, 0] & (np.abs(there - np.round(there)).min(axis=-1) > 1e-3)      # (not within a rounding of a cell's edge)
    assert clear.mean() > 0.5
    assert np.array_equal(info["x0"][0, 0][clear], np.floor(there[..., 0]).astype(np.int64)[clear])
    assert np.array_equal(info["y0"][0, 0][clear], np.floor(there[..., 1]).astype(np.int64)[clear])


def test_undistort_points_inverts_distort_points_and_raises_beyond_the_fold():
    Hs, Ws = 480, 640
    yy, xx = np.mgrid[0:Hs:16, 0:Ws:16].astype(np.float64)
    pts = np.stack((xx, yy), axis=-1)
    for kind in ("barrel", "pincushion"):
        L = lc.lens(kind, (Hs, Ws)).astype(np.float64)
        there = capture.distort_points(pts, L)
        assert np.abs(there - pts).max() > 2.0              # the lens bends by pixels
        back = capture.undistort_points(there, L)
        err = np.abs(back - pts).max()
        print("[capture lens] undistort(distort(x)) - x over the frame, %s: %.3g px" % (kind, err))
        assert err <= 1e-9 and back.shape == pts.shape
    assert np.array_equal(capture.undistort_points(pts, lc.NULL), pts)
    fold = lc.lens("folding", (Hs, Ws)).astype(np.float64)
    near = np.array([[fold[2] + 10.0, fold[3] + 5.0]])
    assert np.abs(capture.undistort_points(capture.distort_points(near, fold), fold) - near).max() <= 1e-9
    # the radial map tops out at r rad(r) = 0.406 (r = 0.609): no ideal point lands at a normalised radius of 0.6
    with pytest.raises(ValueError):
        capture.undistort_points(np.array([[fold[2] + 0.6 * fold[0], fold[3]]]), fold)
    with pytest.raises(ValueError):
        capture.undistort_points(np.zeros((3,)), fold)
    with pytest.raises(ValueError):
        capture.distort_points(np.zeros((4, 2)), np.zeros(8))


def test_the_tools_ideal_corners_carry_the_implicit_inverses_gradients():
    """tools/fit_photos.py --fit-lens: Registration.ideal_of takes the clicked (distorted) corners and the current lens to
    the ideal corners -- the host's undistort_points for the value, one Newton step in torch ops for the gradients.  Value =
    undistort_points; d / d k1 and d / d clicked = central differences of undistort_points (step 1e-5: its own error
    1e-10 relative, the solve's 1e-12 px / 1e-5) to 1e-6 relative; a corner beyond Newton's reach keeps the known ideal
    position, moved by what its parameter moved."""
    import importlib.util
    import types
    spec = importlib.util.spec_from_file_location("fit_photos_tool", os.path.join(ROOT, "tools", "fit_photos.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    lens = capture.pinhole_lens((640, 480)).double().numpy()
    lens[4], lens[5] = -0.18, 0.04
    ideal = np.array([[[[100.0, 80.0], [90.0, 400.0], [560.0, 420.0], [19678.0, 4063.0]]]])
    clicked = capture.distort_points(ideal, lens)
    back, beyond = tool.ideal_corners(clicked, lens, ideal)
    assert beyond.tolist() == [[[False, False, False, True]]] and np.abs(back - ideal).max() <= 1e-9
    args = types.SimpleNamespace(registration_lr=0.1, lens_lr=0.01)
    reg = tool.Registration(args, None, clicked, clicked + 1.0, 64, lens, (ideal, beyond))
    assert reg.k1.item() == 0.0 and reg.lens[4].item() == 0.0 and len(reg.opt.param_groups) == 2
    assert reg.opt.param_groups[1]["lr"] == 0.01 and reg.opt.param_groups[1]["params"][0] is reg.k1
    L = reg.lens.clone()
    L[4] = -0.1
    L.requires_grad_(True)
    out = reg.ideal_of(L)
    c0, l0 = reg.corners.detach().numpy(), L.detach().numpy()
    assert np.abs(out.detach().numpy()[0, 0, :3] - capture.undistort_points(c0[0, 0, :3], l0)).max() <= 1e-9
    assert np.abs(out.detach().numpy()[0, 0, 3] - (ideal[0, 0, 3] + 1.0)).max() <= 1e-9
    w = torch.from_numpy(synth.uniform01(3, out.shape)) + 0.5
    (out * w).sum().backward()

    def f(c, l):
        return float((capture.undistort_points(c[0, 0, :3], l) * w.numpy()[0, 0, :3]).sum())

    e = 1e-5
    up, down = l0.copy(), l0.copy()
    up[4] += e
    down[4] -= e
    want = (f(c0, up) - f(c0, down)) / (2 * e)
    assert abs(L.grad[4].item() - want) <= 1e-6 * abs(want) and abs(want) > 1.0
    for idx in ((0, 0, 0, 0), (0, 0, 1, 1), (0, 0, 2, 0)):
        up, down = c0.copy(), c0.copy()
        up[idx] += e
        down[idx] -= e
        want = (f(up, l0) - f(down, l0)) / (2 * e)
        assert abs(reg.corners.grad[idx].item() - want) <= 1e-6 * abs(want), idx
    assert torch.equal(reg.corners.grad[0, 0, 3], w[0, 0, 3])       # beyond reach: the identity


# ------------------------------------------------------------------------------------------------ the gradient's restatement

def _case(u8, k):
    P = 4
    src = cc.u8_source(40 + k, P, *SRC_SIZE, blobs=True) if u8 else cc.float_source(50 + k, P, *SRC_SIZE)
    M = np.stack([cc.matrix(kind, SRC_SIZE, DST_SIZE, p) for p, kind in enumerate(("mild", "outside", "horizon", "outside"))])
    L = np.stack([lc.lens(kind, SRC_SIZE, p) for p, kind in enumerate(("barrel", "pincushion", "barrel", "folding"))])
    G = synth.uniform01(60 + k, (P, 3) + DST_SIZE).astype(np.float32) * 2.0 - 1.0
    lut = capture.gamma_lut().numpy() if u8 else None
    clip = (5, 250) if u8 else (0.02, 0.98)
    return src, M, L, G, lut, clip


@pytest.mark.parametrize("u8", (False, True), ids=("float", "uint8"))
@pytest.mark.parametrize("k", (1, 2, 4))
def test_float64_terms_are_torch_autograd_towards_all_eighteen_inputs(u8, k):
    src, M, L, G, lut, clip = _case(u8, k)
    t32, ok32, cells = lc.grad_terms(src, M, L, DST_SIZE, G, k, lut, clip)
    assert t32.dtype == np.float32 and tuple(t32.shape) == (4, k * k, 18) + DST_SIZE
    _, w, info = lc.restatement(src, M, L, DST_SIZE, k, lut, clip, detail=True)
    assert np.array_equal(ok32, w > 0) and ok32.any(axis=(1, 2)).all() and not ok32.all(axis=(1, 2)).any()
    assert info["mono_refused"][3].any()                            # the folding lens refuses inside the footprint
    assert not t32[np.broadcast_to(~ok32[:, None, None], t32.shape)].any()
    t64, ok64, _ = lc.grad_terms(src, M, L, DST_SIZE, G, k, lut, clip, dtype=np.float64, cells=cells)
    assert t64.dtype == np.float64 and np.array_equal(ok64, ok32)
    ref, A = lc.sums(t64)
    auto = lc.autograd_grad(src, M, L, DST_SIZE, G, k, lut, cells)
    rel = (np.abs(ref - auto).max(axis=0) / np.abs(auto).max(axis=0)).max()     # per input, over the photos
    r32, _ = lc.sums(t32)
    print("[capture lens grad] %s k=%d: float64 restatement vs autograd %.3g relative (worst of the 18 inputs); float32 terms "
          "vs float64 terms, |sum32 - sum64| / A: %.3g" % ("uint8" if u8 else "float", k, rel, (np.abs(r32 - ref) / A).max()))
    assert (np.abs(auto).max(axis=0) > 0).all()
    assert rel <= 1e-12


def test_torch_forward_passes_gradcheck():
    src_size, dst_size, P = (5, 7), (3, 4), 2
    src = cc.float_source(3, P, *src_size)
    M = np.stack((cc.matrix("mild", src_size, dst_size, 0), cc.matrix("mild", src_size, dst_size, 1)))
    L = np.stack((lc.lens("barrel", src_size, 0), lc.lens("pincushion", src_size, 1)))
    _, ok, cells = lc.grad_terms(src, M, L, dst_size, np.zeros((P, 3) + dst_size, np.float32), 2)
    assert ok[0].sum() >= 6 and ok[1].sum() >= 3       # (the refused pixels' values are the constant 0)
    img = torch.from_numpy(src).double()
    m = torch.from_numpy(M.astype(np.float64)).requires_grad_(True)
    rows = torch.from_numpy(L.astype(np.float64)).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: lc.torch_forward(img, a, b, dst_size, 2, cells), (m, rows))


def test_the_refinement_dry_run_in_float64_on_the_cpu():
    """96 x 128 band-limited source, 32 x 32 grid, REG_CORNERS; the lens k1 = -0.18, k2 = 0.04, focal length 0.8 Ws (k2 known).
    Adam on k1 alone from 0 (lr 0.01, squared log difference, 150 steps), then k1 together with the corners from
    start_corners(REG_SEED), 3 px off.  Asserted: |k1 - truth| <= 1e-3 and corner error <= 0.01 px."""
    src = gc.band_limited_source(7, *gc.REG_SRC)
    rectify = lc.cpu_float64_rectify(src)
    true_lens = torch.from_numpy(lc.reference_lens())
    Mtrue = capture.corner_matrices(torch.tensor(gc.REG_CORNERS[None]), gc.REG_GRID)
    with torch.no_grad():
        target, tw = rectify(Mtrue, true_lens)
        blind, bw = rectify(Mtrue, torch.from_numpy(lc.reference_lens(0.0, 0.0)))
    assert bool((tw == 1).all()) and bool((bw == 1).all())
    print("[capture lens] rectifying without the lens: mean |value error| %.4f" % float((blind - target).abs().mean()))
    assert float((blind - target).abs().mean()) > 0.005
    k1, _ = lc.refinement_loop(rectify, target, tw)
    print("[capture lens] k1 alone: %.5f (truth %.2f)" % (k1, lc.REF_K1))
    assert abs(k1 - lc.REF_K1) <= 1e-3
    k1, corners = lc.refinement_loop(rectify, target, tw, gc.start_corners(gc.REG_SEED))
    print("[capture lens] k1 with the corners from 3 px off: k1 %.5f, corner error %.5f px" % (k1, gc.corner_error(corners)))
    assert abs(k1 - lc.REF_K1) <= 1e-3 and gc.corner_error(corners) <= 0.01


# ------------------------------------------------------------------------------------------------ the wrapper's arguments

def test_wrapper_has_no_cpu_path_and_lens_none_is_the_old_launch(monkeypatch):
    from svbrdf_estimation_amd import _native
    img = torch.zeros(2, 3, 8, 9)
    M = torch.eye(3, dtype=torch.float64).repeat(2, 1, 1)
    with pytest.raises(_native.NativeLibraryError, match="no CPU fallback"):
        capture.rectify(img, M, 4, lens=lc.NULL)
    with pytest.raises(_native.NativeLibraryError, match="no CPU fallback"):
        capture.rectify(img, M, 4, lens=torch.from_numpy(lc.NULL).requires_grad_(True))
    old, new = [], []

    def launch(src, mats, lut, args, lead, want_weights, lens=None):
        """the one launcher: without lens rows it calls svbrdf_rectify_photos (`old`), with them svbrdf_rectify_photos_lens"""
        if lens is None:
            old.append((tuple(mats.shape), mats.dtype, args))
        else:
            new.append((tuple(mats.shape), tuple(lens.shape), lens.dtype, args))
        return torch.zeros(lead + (3, 4, 4)), torch.zeros(lead + (4, 4))

    monkeypatch.setattr(capture, "_launch_rectify", launch)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    args = (cc.F32_PLANAR, 2, 8, 9, 4, 4, 2, -np.inf, np.inf)
    out, w = capture.rectify(img, M, 4, samples=2, lens=None)
    assert old == [((2, 9), torch.float32, args)] and not new and out.grad_fn is None
    out, w = capture.rectify(img, M, 4, samples=2, lens=np.asarray(lc.NULL, np.float64))       # one [9] for all, an array
    assert new == [((2, 9), (2, 9), torch.float32, args)] and len(old) == 1 and out.grad_fn is None
    # either input asking makes a node; the weights never require grad
    Lr = torch.stack((torch.from_numpy(lc.NULL),) * 2).double().requires_grad_(True)
    out, w = capture.rectify(img, M, 4, samples=2, lens=Lr)
    assert out.grad_fn is not None and not w.requires_grad and len(new) == 2
    out, w = capture.rectify(img, M.clone().requires_grad_(True), 4, samples=2, lens=lc.NULL)
    assert out.grad_fn is not None and len(new) == 3 and len(old) == 1
    with torch.no_grad():
        assert capture.rectify(img, M, 4, lens=Lr)[0].grad_fn is None
    with pytest.raises(ValueError):
        capture.rectify(img, M, 4, lens=np.zeros(8))
    with pytest.raises(ValueError):
        capture.rectify(img, M, 4, lens=np.zeros((3, 9)))
    # and the launcher itself: the entry it names, and the lens pointer only behind the lens entry
    monkeypatch.undo()
    calls = []
    monkeypatch.setattr(_native, "_call", lambda name, device, *a: calls.append((name, len(a))))
    rows = torch.zeros(2, 9)
    capture._launch_rectify(img, rows, None, args, (2,), True)
    capture._launch_rectify(img, rows, None, args, (2,), True, rows)
    assert calls == [("svbrdf_rectify_photos", 14), ("svbrdf_rectify_photos_lens", 15)]


def test_backward_returns_each_gradient_in_its_inputs_shape_dtype_and_device(monkeypatch):
    """the one launch of the backward replaced by rows of known numbers: per-photo inputs get their rows, a shared matrix
    or a shared lens the float64 sum over the photos, an input that did not ask gets none"""
    from svbrdf_estimation_amd import _native
    img = torch.zeros(2, 3, 8, 9)
    rows = (torch.arange(18, dtype=torch.float32).reshape(2, 9) + 0.5, -torch.arange(18, dtype=torch.float32).reshape(2, 9))
    calls = []

    def grad(src, fmt, P, Hs, Ws, mats, lens, Hd, Wd, k, lut, lo, hi, g):
        calls.append((tuple(mats.shape), tuple(lens.shape), tuple(g.shape), g.dtype, g.is_contiguous()))
        return rows

    monkeypatch.setattr(capture, "_launch_rectify", lambda src, mats, lut, args, lead, ww, lens=None: (
        torch.zeros(lead + (3, 4, 4)), torch.zeros(lead + (4, 4))))
    monkeypatch.setattr(_native, "rectify_lens_grad", grad)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    M = torch.eye(3, dtype=torch.float64).repeat(2, 1, 1).requires_grad_(True)
    L = torch.stack((torch.from_numpy(lc.NULL),) * 2).requires_grad_(True)
    capture.rectify(img, M, 4, lens=L)[0].sum().backward()
    assert calls == [((2, 9), (2, 9), (2, 3, 4, 4), torch.float32, True)]
    assert M.grad.dtype == torch.float64 and tuple(M.grad.shape) == (2, 3, 3) and torch.equal(M.grad.reshape(2, 9), rows[0].double())
    assert L.grad.dtype == torch.float32 and tuple(L.grad.shape) == (2, 9) and torch.equal(L.grad, rows[1])
    Ms = torch.eye(3).requires_grad_(True)
    Ls = torch.from_numpy(lc.NULL).double().requires_grad_(True)
    capture.rectify(img, Ms, 4, lens=Ls)[0].sum().backward()
    assert tuple(Ms.grad.shape) == (3, 3) and torch.equal(Ms.grad.reshape(9), rows[0].sum(dim=0))
    assert tuple(Ls.grad.shape) == (9,) and Ls.grad.dtype == torch.float64 and torch.equal(Ls.grad, rows[1].double().sum(dim=0))
    M2 = torch.eye(3, dtype=torch.float64).repeat(2, 1, 1).requires_grad_(True)
    L2 = torch.from_numpy(lc.NULL)
    capture.rectify(img, M2, 4, lens=L2)[0].sum().backward()
    assert M2.grad is not None and L2.grad is None
    L3 = torch.from_numpy(lc.NULL).requires_grad_(True)
    M3 = torch.eye(3)
    capture.rectify(img, M3, 4, lens=L3)[0].sum().backward()
    assert M3.grad is None and torch.equal(L3.grad, rows[1].double().sum(dim=0).float())


# ------------------------------------------------------------------------------------------------ the C ABI and the binding

def test_library_exports_the_entries_without_an_abi_bump(lib):
    from svbrdf_estimation_amd import _native
    assert lib.svbrdf_abi_version() == 8 and _native.ABI_VERSION == 8
    with open(os.path.join(ROOT, "include", "svbrdf_hip.h")) as f:
        header = f.read()
    assert "#define SVBRDF_ABI_VERSION 8" in header
    for name, count in ((FORWARD, 16), (GRAD, 19)):
        assert hasattr(lib, name)
        declared = header.split("SVBRDF_API int %s(" % name)[1].split(");")[0]
        assert len(_native.SIGNATURES[name][1]) == count == declared.count(",") + 1, name
    assert hasattr(lib, QUERY)
    declared = header.split("SVBRDF_API size_t %s(" % QUERY)[1].split(");")[0]
    assert len(_native.SIGNATURES[QUERY][1]) == 3 == declared.count(",") + 1 and _native.SIGNATURES[QUERY][0] is ctypes.c_size_t
    assert int(re.search(r"#define SVBRDF_RECTIFY_GRAD_DEPTH (\d+)", header).group(1)) == 24 == _native.RECTIFY_GRAD_DEPTH
    # tickets (4 bytes a photo, padded) and eighteen words per 64 x 4 tile; 0 outside the limits
    for P, Hd, Wd in ((1, 1, 1), (5, 5, 65), (72, 256, 256), (65535, 4, 64)):
        tiles = ((Wd + 63) // 64) * ((Hd + 3) // 4)
        n = getattr(lib, QUERY)(P, Hd, Wd)
        assert 4 * P + 72 * P * tiles <= n <= 4 * P + 72 * P * tiles + 256 and n % 4 == 0, (P, Hd, Wd, n)
    for bad in ((0, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 4, 32769)):
        assert getattr(lib, QUERY)(*bad) == 0, bad


def _host_block():
    buf = (ctypes.c_float * 16384)()
    for i in range(len(buf)):
        buf[i] = float(i % 251)
    return buf, bytes(buf), (ctypes.cast(buf, ctypes.c_void_p).value + 63) & ~63


def test_forward_argument_errors_come_before_any_launch_and_touch_nothing(lib):
    """svbrdf_rectify_photos' checks, then -1 for a null lens and -3 for one off 4 bytes.  Host buffers stand in for device
    memory and the stream is null: nothing is enqueued, no byte changes."""
    fn = getattr(lib, FORWARD)
    buf, snapshot, p = _host_block()
    nan = float("nan")

    def call(src=p, fmt=1, P=2, Hs=4, Ws=5, mats=p + 4096, lens=p + 6144, Hd=3, Wd=3, k=1, lut=p + 8192, lo=-1.0, hi=256.0,
             out=p + 12288, w=p + 16384):
        f = ctypes.c_float
        return fn(src, fmt, P, Hs, Ws, mats, lens, Hd, Wd, k, lut, f(lo), f(hi), out, w, None)

    launches = lib.svbrdf_debug_launch_count()
    for fmt in (-1, 2, 7):
        assert call(fmt=fmt) == -2, fmt
        assert b"src_format" in lib.svbrdf_last_error() and FORWARD.encode() in lib.svbrdf_last_error()
    for k in (0, 3, 5, 8, -1):
        assert call(k=k) == -2, k
    for bad in (dict(P=0), dict(Hs=0), dict(Ws=0), dict(Hd=0), dict(Wd=0), dict(P=-1), dict(Hs=-4), dict(P=65536), dict(Ws=32769),
                dict(Hd=32769), dict(lo=nan), dict(hi=nan)):
        assert call(**bad) == -2, bad
    for name in ("src", "mats", "out", "lut", "lens"):
        assert call(**{name: None}) == -1, name
        assert lib.svbrdf_last_error()
    assert b"lens" in lib.svbrdf_last_error()
    assert call(fmt=0, lut=None, src=None) == -1
    assert call(mats=p + 4098) == -3 and call(out=p + 12290) == -3 and call(w=p + 16385) == -3 and call(lut=p + 8194) == -3
    assert call(fmt=0, src=p + 2) == -3 and call(lens=p + 6146) == -3 and call(lens=p + 6145) == -3
    assert lib.svbrdf_debug_launch_count() == launches
    assert bytes(buf) == snapshot


def test_gradient_argument_errors_come_before_any_launch_and_touch_nothing(lib):
    """svbrdf_rectify_photos_grad_matrices' checks with the lens's: -1 for a null lens, grad_lens, grad_values or workspace, -3
    for one of them off its alignment, -4 for a workspace that is too small"""
    fn = getattr(lib, GRAD)
    buf, snapshot, p = _host_block()
    nan = float("nan")
    need = getattr(lib, QUERY)(2, 3, 3)

    def call(src=p, fmt=1, P=2, Hs=4, Ws=5, mats=p + 4096, lens=p + 6144, Hd=3, Wd=3, k=1, lut=p + 8192, lo=-1.0, hi=256.0,
             gv=p + 12288, gm=p + 16384, gl=p + 18432, ws=p + 20480, nbytes=need):
        f = ctypes.c_float
        return fn(src, fmt, P, Hs, Ws, mats, lens, Hd, Wd, k, lut, f(lo), f(hi), gv, gm, gl, ws, nbytes, None)

    launches = lib.svbrdf_debug_launch_count()
    for fmt in (-1, 2, 7):
        assert call(fmt=fmt) == -2, fmt
        assert b"src_format" in lib.svbrdf_last_error() and GRAD.encode() in lib.svbrdf_last_error()
    for k in (0, 3, 5, 8, -1):
        assert call(k=k) == -2, k
    for bad in (dict(P=0), dict(Hs=0), dict(Ws=0), dict(Hd=0), dict(Wd=0), dict(P=-1), dict(P=65536), dict(Ws=32769),
                dict(Hd=32769), dict(lo=nan), dict(hi=nan)):
        assert call(**bad) == -2, bad
    for name in ("src", "mats", "lens", "gm", "gl", "lut", "gv", "ws"):
        assert call(**{name: None}) == -1, name
        assert lib.svbrdf_last_error()
    assert call(fmt=0, lut=None, src=None) == -1
    assert call(mats=p + 4098) == -3 and call(gm=p + 16386) == -3 and call(gv=p + 12289) == -3 and call(lut=p + 8194) == -3
    assert call(fmt=0, src=p + 2) == -3 and call(ws=p + 20484) == -3 and call(lens=p + 6146) == -3 and call(gl=p + 18434) == -3
    assert call(nbytes=need - 1) == -4 and call(nbytes=0) == -4
    assert b"workspace" in lib.svbrdf_last_error()
    assert lib.svbrdf_debug_launch_count() == launches
    assert bytes(buf) == snapshot


# ------------------------------------------------------------------------------------------------ the kernels

UNITS = ("svbrdf_capture_lens", "svbrdf_capture_lens_grad")


def test_makefile_builds_the_units_and_earlier_kernels_kept_their_code():
    for unit in UNITS:
        unit_build.assert_makefile_builds(unit)             # HIPFLAGS and no scheduler option set
        text = unit_build.assert_includes_shared_header(unit, "svbrdf_capture_lens_device.h")
        shared = unit_build.assert_includes_shared_header(unit, "svbrdf_capture_device.h")
        assert "int fail(" in unit_build.assert_includes_shared_header(unit, "svbrdf_host.h")
    assert "rectify_lens_map" in text and "mono" in text and "rectify_cell" in shared and "fminf(fmaxf(" in shared
    assert "rectify_grad_reduce" in unit_build.assert_includes_shared_header(UNITS[1], "svbrdf_capture_grad_device.h")
    # profiles/r25_capture_lens_codehash.txt: the diff against the parent's listing holds added lines only, the twelve kernels
    with open(os.path.join(ROOT, "profiles", "r25_capture_lens_codehash.txt")) as f:
        listing = f.read()
    diff = listing.split("## diff parent new")[1].split("## nm")[0]
    changed = [ln for ln in diff.splitlines() if ln[:1] in ("<", ">")]
    assert len(changed) == 12 and all(ln.startswith("> ") for ln in changed), changed
    assert sum("k_lens_rectify" in ln for ln in changed) == 6 == sum("k_lens_grad" in ln for ln in changed)
    # profiles/r27_capture_refactor_codehash.txt, the capture units on shared device functions: the diff against the parent's
    # listing touches only lines that name the four kernel templates -- the six k_rectify and the six k_lens_grad on both
    # sides; k_homography_grad and k_lens_rectify got their old bodies back and keep the parent's code -- every other
    # function of the library keeps symbol, size and sha256, and the exported symbols are the parent's
    with open(os.path.join(ROOT, "profiles", "r27_capture_refactor_codehash.txt")) as f:
        listing = f.read()
    diff = listing.split("## diff parent new")[1].split("## nm")[0]
    changed = [ln for ln in diff.splitlines() if ln[:1] in ("<", ">")]
    templates = ("9k_rectifyIL", "17k_homography_gradIL", "14k_lens_rectifyIL", "11k_lens_gradIL")
    assert len(changed) == 24 and all(sum(t in ln for t in templates) == 1 for ln in changed), changed
    assert sum("9k_rectifyIL" in ln for ln in changed) == 12 == sum("11k_lens_gradIL" in ln for ln in changed)
    assert sorted(ln.split()[1] for ln in changed if ln[0] == "<") == sorted(ln.split()[1] for ln in changed if ln[0] == ">")
    assert [ln for ln in listing.split("## nm")[1].split("## new")[0].splitlines()[1:] if ln.strip()] == []
    # and the library as built here holds the 24 capture kernels with the code recorded there
    from svbrdf_estimation_amd import _codehash, _native
    new = listing.split("## new")[1]
    for u8 in "01":
        for k in "124":
            for name in ("14k_lens_rectifyILb%sELi%sE", "11k_lens_gradILb%sELi%sE", "9k_rectifyILb%sELi%sE", "17k_homography_gradILb%sELi%sE"):
                name = name % (u8, k)
                got = _codehash.kernel_code_sha256(_native.library_path(), (name,))
                assert got["bytes"] > 1000 and re.search(r"%s\S*\s+%d\s+%s" % (name, got["bytes"], got["sha256"]), new), (name, got)


def test_source_holds_no_float_atomic_no_fma_and_the_clamp_before_the_conversion():
    header = unit_build.read_csrc("svbrdf_capture_lens_device.h")
    for unit in UNITS:
        headers = re.findall(r'#include "(svbrdf_capture\w*\.h)"', unit_build.read_csrc(unit + ".hip"))
        assert headers == ["svbrdf_capture_device.h"] + ["svbrdf_capture_grad_device.h"] * unit.endswith("_grad") + ["svbrdf_capture_lens_device.h"]
        src = unit_build.read_csrc(unit + ".hip", *headers)     # the unit and every capture header it includes
        code = "\n".join(line.split("//")[0] for line in src.splitlines())
        assert not re.search(r"\b(__builtin_)?fmaf?\(|\bfma_\(|\brcp_\(|\bdiv_rn\(|atomicAdd|unsafeAtomic", code), unit
        assert [m for m in re.findall(r'asm\s+volatile\s*\(\s*"([^"]*)"', code) if m != "s_waitcnt vmcnt(0)"] == [], unit
        assert len(re.findall(r"\basm\b", code)) == (2 if unit.endswith("_grad") else 0), unit
        # one clamp in the shared header; k_lens_rectify keeps its own cell with u's and v's (profiles/r27_capture_refactor.txt)
        assert code.count("fminf(fmaxf(") == (1 if unit.endswith("_grad") else 3) and code.index("fminf(fmaxf(") < code.index("(int)x0f"), unit
        assert "__ATOMIC_RELEASE" not in code
        atomics = re.findall(r"__hip_atomic_\w+", code)
        assert atomics == (["__hip_atomic_store", "__hip_atomic_fetch_add", "__hip_atomic_store"] if unit.endswith("_grad") else []), unit
    code = "\n".join(line.split("//")[0] for line in header.splitlines())
    assert "atomic" not in code and "asm" not in code
    grad = unit_build.read_csrc("svbrdf_capture_lens_grad.hip", "svbrdf_capture_grad_device.h")
    order = [grad.index(w) for w in ("__hip_atomic_store(reinterpret_cast<unsigned *>(mine)", 'asm volatile("s_waitcnt vmcnt(0)"',
                                     "__hip_atomic_fetch_add", "__ATOMIC_ACQUIRE", "(double)all[")]
    assert order == sorted(order)


QUOTIENTS = {"svbrdf_capture_lens": 4, "svbrdf_capture_lens_grad": 7}      # u, v, xn, yn;  and gu, gv, 1 / Z


@needs_hipcc
@pytest.mark.parametrize("unit", UNITS)
def test_compiled_kernels_use_no_scratch_and_divide_in_ieee(tmp_path, unit):
    """the unit compiled exactly as the Makefile compiles it: HIPFLAGS and no scheduler option set.  VGPRs and occupancy are
    printed (README), not asserted."""
    asm = unit_build.compile_unit_asm(tmp_path, unit)
    isa_stats = _isa_stats()
    names = sorted(k for k in isa_stats.kernels(asm) if "k_lens_rectify" in k or "k_lens_grad" in k)
    assert len(names) == 6, names
    q = QUOTIENTS[unit]
    for k in names:
        _, meta, whole, loops, ins, rng = isa_stats.analyse(asm, k)
        K = int(re.search(r"ILb[01]ELi(\d)E", k).group(1))
        mns = [mn for _, _, mn, _ in ins if mn]
        print("%s\n   VGPRs %s, SGPRs %s, occupancy %s, LDS %s, scratch %s, %d instructions" % (
            k, meta["NumVgprs"], meta.get("NumSgprs"), meta["Occupancy"], meta.get("LDSByteSize"), meta["ScratchSize"], whole["total"]))
        assert int(meta["ScratchSize"]) == 0 and whole["scratch"] == 0 and int(meta["NumAgprs"]) == 0, (k, meta)
        assert mns.count("v_div_fixup_f32") == q * K * K == mns.count("v_div_fmas_f32"), (k, mns.count("v_div_fixup_f32"))
        fmas = sum(1 for mn in mns if mn.startswith(("v_fma_f32", "v_fmac_f32", "v_mad_f32", "v_mac_f32", "v_pk_fma_f32", "v_fma_mix")))
        assert fmas == 5 * q * K * K, (k, fmas)
        assert not [mn for mn in mns if mn.startswith("flat_")], k
        atomics = [mn for mn in mns if "atomic" in mn]
        assert atomics == (["global_atomic_add"] if unit.endswith("_grad") else []), (k, atomics)    # the ticket: an integer
        if unit.endswith("_grad"):
            assert "buffer_inv" in mns and "buffer_wbl2" not in mns, k      # one agent-scope acquire, no L2 write-back
        else:
            stores = [mn for mn in mns if mn.startswith(("global_store", "buffer_store"))]
            assert len(stores) == 4 and all(mn.endswith("dword") for mn in stores), (k, stores)
