"""svbrdf_rectify_photos_lens_grad (csrc/svbrdf_capture_lens_grad.hip: k_lens_grad) and the autograd path of
capture.rectify(..., lens=) on the MI355X, against the numpy float32 restatement of tests/capture_lens_checks.py.

The bound is test_gpu_capture_grad.py's with the same D.  ref_n is the float64 sum of the restatement's float32 term planes
and A_n that of their absolute values; the kernel's terms are those planes, so what separates got_n from ref_n is D float32
additions, the term's own last rounding and the final rounding:  |got_n - ref_n| <= (D + 2) 2^-24 A_n,  for all eighteen
entries of every photo, no element excluded.  Every case prints its largest err / A in units of 2^-24.
"""
import numpy as np
import pytest
import torch

import capture_checks as cc
import capture_grad_checks as gc
import capture_lens_checks as lc
from test_gpu_capture import HOSTILE
from test_gpu_capture_lens import CASES, MATRIX_KINDS

pytestmark = pytest.mark.gpu
CLIPS = {"uint8": (5, 250), "float32": (0.02, 0.98)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def native():
    from svbrdf_estimation_amd import _native
    return _native


@pytest.fixture(scope="module")
def capture():
    from svbrdf_estimation_amd import capture
    return capture


@pytest.fixture(scope="module")
def lut(capture):
    return capture.gamma_lut().numpy()


def source(fmt, seed, P, size):
    return cc.u8_source(seed, P, *size) if fmt == "uint8" else cc.float_source(seed, P, *size)


def normal(seed, shape):
    return np.random.RandomState(seed).standard_normal(shape).astype(np.float32)


def assert_within(got, terms, what):
    """-> the largest |got - ref| / A in units of 2^-24 (0 where A = 0, where got must be 0 as well)"""
    ref, A = lc.sums(terms)
    err = np.abs(got.astype(np.float64) - ref)
    assert np.isfinite(got).all(), what
    assert (err <= gc.bound(A)).all(), (what, (err / np.maximum(gc.bound(A), 1e-300)).max(), got, ref)
    return float((err[A > 0] / (2.0 ** -24 * A[A > 0])).max()) if (A > 0).any() else 0.0


# ------------------------------------------------------------------------------------------------ parity

@pytest.mark.parametrize("fmt", ("uint8", "float32"))
@pytest.mark.parametrize("dst_size", list(CASES), ids=lambda s: "dst%dx%d" % s)
def test_sums_against_the_restatement(native, dev, lut, dst_size, fmt):
    """the forward test's shape list; P = 5 with a matrix and a lens row each and P = 1 (photo 0 of the five on its own): one
    restatement serves both launches.  Measured on the MI355X: at most 2.40 x 2^-24 A over all cases (bound 26)."""
    sources, pairs, ks = CASES[dst_size]
    P = 5
    table = lut if fmt == "uint8" else None
    worst = 0.0
    for src_size in sources:
        src = source(fmt, 100 + P, P, src_size)
        for mkind, lkind in [pair[:2] for pair in pairs or [(m, l) for m in MATRIX_KINDS for l in lc.LENS_KINDS]]:
            M, L = cc.matrices(mkind, src_size, dst_size, P), lc.lenses(lkind, src_size, P)
            for k in ks:
                G = normal(7 * k + len(mkind), (P, 3) + dst_size)
                terms, ok, _ = lc.grad_terms(src, M, L, dst_size, G, k, table)
                out5 = lc.abi_lens_grad(native, dev, src, M, L, dst_size, G, k, table)
                out1 = lc.abi_lens_grad(native, dev, src[:1], M[:1], L[:1], dst_size, G[:1], k, table)
                what = "%s %s %s k=%d" % (src_size, mkind, lkind, k)
                for out in (out5, out1):
                    assert out["canaries_intact"] and out["launches"] == 1 and out["workspace_zero"], what
                worst = max(worst, assert_within(out5["grad"], terms, what), assert_within(out1["grad"], terms[:1], what + " P=1"))
                assert cc.same_bits(out1["grad"][0], out5["grad"][0]), what      # a photo's rows do not depend on the others
                if lkind == "null":     # the nine matrix sums are the pinhole entry's bit for bit
                    pin = gc.abi_grad(native, dev, src, M, dst_size, G, k, table)["grad"]
                    assert cc.same_bits(out5["grad"][:, :9], pin), what
    print("[capture lens grad] %s -> %dx%d: max err/A %.2f x 2^-24 (bound %d)" % (fmt, dst_size[0], dst_size[1], worst, gc.depth() + 2))


# ------------------------------------------------------------------------------------------------ edge cases

@pytest.mark.parametrize("fmt", ("uint8", "float32"))
def test_nan_under_zero_weight_pixels_changes_no_bit(native, dev, lut, fmt):
    src_size, dst_size, P, k = (97, 131), (9, 130), 3, 2
    src = cc.u8_source(5, P, *src_size, blobs=True) if fmt == "uint8" else cc.float_source(5, P, *src_size)
    M = np.stack([cc.matrix(kind, src_size, dst_size, p) for p, kind in enumerate(("outside", "horizon", "outside"))])
    L = np.stack([lc.lens(kind, src_size, p) for p, kind in enumerate(("barrel", "pincushion", "folding"))])
    table = lut if fmt == "uint8" else None
    G = normal(3, (P, 3) + dst_size)
    terms, ok, _ = lc.grad_terms(src, M, L, dst_size, G, k, table, CLIPS[fmt])
    assert all(0 < ok[p].mean() < 1 for p in range(P))
    base = lc.abi_lens_grad(native, dev, src, M, L, dst_size, G, k, table, CLIPS[fmt])["grad"]
    assert_within(base, terms, "base")
    dead = np.broadcast_to(~ok[:, None], G.shape)
    zeros, nans = np.where(dead, np.float32(0.0), G), np.where(dead, np.float32(np.nan), G)
    got_z = lc.abi_lens_grad(native, dev, src, M, L, dst_size, zeros, k, table, CLIPS[fmt])["grad"]
    got_n = lc.abi_lens_grad(native, dev, src, M, L, dst_size, nans, k, table, CLIPS[fmt])["grad"]
    assert cc.same_bits(got_n, got_z) and cc.same_bits(got_n, base) and np.isfinite(got_n).all()
    y, x = np.argwhere(ok[1])[0]
    G2 = G.copy()
    G2[1, 0, y, x] = np.nan
    out = lc.abi_lens_grad(native, dev, src, M, L, dst_size, G2, k, table, CLIPS[fmt])
    assert np.isnan(out["grad"][1]).any() and cc.same_bits(out["grad"][[0, 2]], base[[0, 2]]) and out["workspace_zero"]
    again = lc.abi_lens_grad(native, dev, src, M, L, dst_size, G, k, table, CLIPS[fmt], workspace=out["workspace"])["grad"]
    assert cc.same_bits(again, base)        # the scratch that saw a NaN serves the next call


@pytest.mark.parametrize("fmt", ("uint8", "float32"))
def test_hostile_lens_or_matrix_rows_give_zero_rows(native, dev, lut, fmt):
    src_size, dst_size = (97, 131), (9, 130)
    rows = lc.hostile_lenses(src_size)
    table = lut if fmt == "uint8" else None
    for M, L in ((cc.matrices("mild", src_size, dst_size, len(rows)), np.stack(list(rows.values()))),
                 (np.stack(list(HOSTILE.values())), lc.lenses("barrel", src_size, len(HOSTILE)))):
        P = len(M)
        src = source(fmt, 21, P, src_size)
        for k in (1, 2, 4):
            G = normal(k, (P, 3) + dst_size)
            terms, ok, _ = lc.grad_terms(src, M, L, dst_size, G, k, table)
            assert not ok.any() and not terms.any()
            out = lc.abi_lens_grad(native, dev, src, M, L, dst_size, G, k, table)
            assert not out["grad"].any() and out["canaries_intact"] and out["workspace_zero"], (k, out["grad"])
    M2, L2 = cc.matrices("mild", src_size, dst_size, P), lc.lenses("barrel", src_size, P)   # and the next ordinary call is right
    t2, _, _ = lc.grad_terms(src, M2, L2, dst_size, G, 4, table)
    assert_within(lc.abi_lens_grad(native, dev, src, M2, L2, dst_size, G, 4, table)["grad"], t2, "after hostile")


@pytest.mark.parametrize("fmt", ("uint8", "float32"))
def test_bitwise_reproducible_on_fresh_and_reused_scratch_and_off_alignment(native, capture, dev, lut, fmt):
    src_size, dst_size, P, k = (97, 131), (260, 260), 4, 2
    src = source(fmt, 31, P, src_size)
    M, L = cc.matrices("outside", src_size, dst_size, P), lc.lenses("barrel", src_size, P)
    G = normal(8, (P, 3) + dst_size)
    table = lut if fmt == "uint8" else None
    first = lc.abi_lens_grad(native, dev, src, M, L, dst_size, G, k, table)
    second = lc.abi_lens_grad(native, dev, src, M, L, dst_size, G, k, table)
    reused = lc.abi_lens_grad(native, dev, src, M, L, dst_size, G, k, table, workspace=first["workspace"])
    third = lc.abi_lens_grad(native, dev, src, M, L, dst_size, G, k, table, workspace=first["workspace"])
    assert first["grad"][:, :9].any() and first["grad"][:, 9:].any()
    for other in (second, reused, third):
        assert cc.same_bits(other["grad"], first["grad"]) and other["workspace_zero"] and other["canaries_intact"]
    off = lc.abi_lens_grad(native, dev, src, M, L, dst_size, G, k, table, src_offset=1, ptr_offset=1)
    assert cc.same_bits(off["grad"], first["grad"]) and off["canaries_intact"]
    # leading dimensions [B,S] through the Python layer give the rows of [P]
    s = torch.from_numpy(src).to(dev)
    t = None if table is None else torch.from_numpy(table)
    Gd = torch.from_numpy(G).to(dev)
    Mb = torch.from_numpy(M).reshape(2, 2, 3, 3).to(dev).requires_grad_(True)
    Lb = torch.from_numpy(L).reshape(2, 2, 9).to(dev).requires_grad_(True)
    capture.rectify(s.reshape((2, 2) + s.shape[1:]), Mb, dst_size, lut=t, samples=k, lens=Lb)[0].backward(Gd.reshape((2, 2) + Gd.shape[1:]))
    assert tuple(Mb.grad.shape) == (2, 2, 3, 3) and tuple(Lb.grad.shape) == (2, 2, 9)
    assert cc.same_bits(Mb.grad.cpu().numpy().reshape(P, 9), first["grad"][:, :9])
    assert cc.same_bits(Lb.grad.cpu().numpy().reshape(P, 9), first["grad"][:, 9:])


# ------------------------------------------------------------------------------------------------ autograd

def test_autograd_is_the_entry_bit_for_bit(native, capture, dev, lut):
    src_size, dst_size, P, k = (97, 131), (9, 130), 5, 2
    src = cc.u8_source(41, P, *src_size)
    M, L = cc.matrices("outside", src_size, dst_size, P), lc.lenses("barrel", src_size, P)
    G = normal(9, (P, 3) + dst_size)
    want = lc.abi_lens_grad(native, dev, src, M, L, dst_size, G, k, lut, (5, 250))["grad"]
    s, t, Gd = torch.from_numpy(src).to(dev), torch.from_numpy(lut), torch.from_numpy(G).to(dev)
    # float32 on the device, both inputs
    Md, Ld = torch.from_numpy(M).to(dev).requires_grad_(True), torch.from_numpy(L).to(dev).requires_grad_(True)
    before = native.launch_count()
    vals, w = capture.rectify(s, Md, dst_size, lut=t, clip=(5, 250), samples=k, lens=Ld)
    assert vals.grad_fn is not None and not w.requires_grad and native.launch_count() - before == 1
    plain = capture.rectify(s, Md.detach(), dst_size, lut=t, clip=(5, 250), samples=k, lens=Ld.detach())
    assert plain[0].grad_fn is None and torch.equal(plain[0], vals.detach()) and torch.equal(plain[1], w)
    before = native.launch_count()
    vals.backward(Gd)
    assert native.launch_count() - before == 1
    for t_, cols in ((Md, slice(0, 9)), (Ld, slice(9, 18))):
        assert t_.grad.dtype == torch.float32 and t_.grad.device == t_.device and tuple(t_.grad.shape) == (P, 9)
        assert cc.same_bits(t_.grad.cpu().numpy(), want[:, cols])
    # float64 on the host, [P,3,3] and [P,9], through a non-contiguous grad_output
    Mh = torch.from_numpy(M.astype(np.float64)).reshape(P, 3, 3).requires_grad_(True)
    Lh = torch.from_numpy(L.astype(np.float64)).requires_grad_(True)
    vals, _ = capture.rectify(s, Mh, dst_size, lut=t, clip=(5, 250), samples=k, lens=Lh)
    (vals.transpose(-1, -2) * Gd.transpose(-1, -2)).sum().backward()
    assert Mh.grad.dtype == torch.float64 and Mh.grad.device.type == "cpu" and tuple(Mh.grad.shape) == (P, 3, 3)
    assert np.array_equal(Mh.grad.numpy().reshape(P, 9), want[:, :9].astype(np.float64))
    assert Lh.grad.dtype == torch.float64 and np.array_equal(Lh.grad.numpy(), want[:, 9:].astype(np.float64))
    # only one of the two asks
    Mo = torch.from_numpy(M).to(dev).requires_grad_(True)
    capture.rectify(s, Mo, dst_size, lut=t, clip=(5, 250), samples=k, lens=L)[0].backward(Gd)
    assert cc.same_bits(Mo.grad.cpu().numpy(), want[:, :9])
    Lo = torch.from_numpy(L).to(dev).requires_grad_(True)
    capture.rectify(s, M, dst_size, lut=t, clip=(5, 250), samples=k, lens=Lo)[0].backward(Gd)
    assert cc.same_bits(Lo.grad.cpu().numpy(), want[:, 9:])
    # no double backward
    Md2 = torch.from_numpy(M).to(dev).requires_grad_(True)
    g, = torch.autograd.grad(capture.rectify(s, Md2, dst_size, lut=t, samples=k, lens=L)[0], Md2, Gd, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


def test_one_shared_lens_gets_the_sum_of_the_rows(native, capture, dev):
    src_size, dst_size, P, k = (97, 131), (9, 130), 5, 1
    src = cc.float_source(43, P, *src_size)
    M = cc.matrices("mild", src_size, dst_size, P)
    row = lc.lens("pincushion", src_size)
    L = np.broadcast_to(row, (P, 9)).copy()
    G = normal(10, (P, 3) + dst_size)
    shared = torch.from_numpy(row).to(dev).requires_grad_(True)
    vals, _ = capture.rectify(torch.from_numpy(src).to(dev), M, dst_size, samples=k, lens=shared)
    vals.backward(torch.from_numpy(G).to(dev))
    assert tuple(shared.grad.shape) == (9,)
    rows = lc.abi_lens_grad(native, dev, src, M, L, dst_size, G, k)["grad"][:, 9:]
    assert np.array_equal(shared.grad.cpu().numpy(), rows.astype(np.float64).sum(axis=0).astype(np.float32))


def test_torch_composition_backward_agrees(native, dev):
    """k = 1, float source, `mild` matrices under `barrel`: grid_sample's backward and the chain through the polynomial to M
    and the lens in float32 on the device, against the one launch.  As test_gpu_capture_grad.py states it: the composed
    form's own float32 error is MEASURED here, on the CPU, against the same composition in float64 -- the largest
    |float32 - float64| / A over the entries -- and added to the bound."""
    src_size, dst_size, P = (97, 131), (9, 130), 5
    src = cc.float_source(11, P, *src_size)
    M, L = cc.matrices("mild", src_size, dst_size, P), lc.lenses("barrel", src_size, P)
    G = normal(5, (P, 3) + dst_size)
    terms, ok, _ = lc.grad_terms(src, M, L, dst_size, G)
    assert ok.all()
    _, A = lc.sums(terms)

    def composed(device, dtype):
        m = torch.from_numpy(M).to(device=device, dtype=dtype).requires_grad_(True)
        rows = torch.from_numpy(L).to(device=device, dtype=dtype).requires_grad_(True)
        v, _ = lc.torch_composition(torch.from_numpy(src).to(device=device, dtype=dtype), m, rows, dst_size, dtype=dtype)
        v.backward(torch.from_numpy(G).to(device=device, dtype=dtype))
        return torch.cat((m.grad, rows.grad), dim=1).double().cpu().numpy()

    own = float((np.abs(composed("cpu", torch.float32) - composed("cpu", torch.float64)) / (2.0 ** -24 * A)).max())
    got = lc.abi_lens_grad(native, dev, src, M, L, dst_size, G)["grad"]
    diff = np.abs(got.astype(np.float64) - composed(dev, torch.float32))
    print("[capture lens grad] composed backward: own float32 error %.2f x 2^-24 A (measured on the CPU against float64), "
          "one launch against it %.2f x 2^-24 A" % (own, (diff / (2.0 ** -24 * A)).max()))
    assert (diff <= gc.bound(A) + own * 2.0 ** -24 * A).all()


# ------------------------------------------------------------------------------------------------ refinement

def test_refinement_ends_where_the_composed_loop_ends(capture, dev):
    """the dry run's two loops (tests/test_capture_lens_cpu.py) through capture.rectify(..., lens=) on the device, against the
    same loops through torch_composition and autograd on the same device: k1 alone from 0, then k1 with the corners from
    start_corners(REG_SEED).  Asserted: |k1 - truth| and the corner error at most 1.01 x the composed loop's + 1e-3 -- the
    squared log difference has a vanishing gradient at the optimum, so the end of the loop is a place and not a jitter
    (test_gpu_capture_grad.py's margin and reasoning)."""
    src = gc.band_limited_source(7, *gc.REG_SRC)
    s = torch.from_numpy(src).to(dev)
    true_lens = torch.from_numpy(lc.reference_lens())
    Mtrue = capture.corner_matrices(torch.tensor(gc.REG_CORNERS[None]), gc.REG_GRID)
    with torch.no_grad():
        target, tw = capture.rectify(s, Mtrue, gc.REG_GRID, lens=true_lens)
    assert bool((tw == 1).all())

    def fused(M, L):
        return capture.rectify(s, M, gc.REG_GRID, lens=L)

    def comp(M, L):
        return lc.torch_composition(s, M.reshape(1, 9), L.reshape(1, 9), gc.REG_GRID)

    c0 = gc.start_corners(gc.REG_SEED)
    for corners0 in (None, c0):
        k_f, c_f = lc.refinement_loop(fused, target, tw, corners0)
        k_c, c_c = lc.refinement_loop(comp, target, tw, corners0)
        e_f, e_c = gc.corner_error(c_f), gc.corner_error(c_c)
        print("[capture lens] refinement %s: k1 fused %.5f, composed %.5f (truth %.2f); corner error fused %.5f, composed %.5f px"
              % ("k1 alone" if corners0 is None else "k1 with the corners", k_f, k_c, lc.REF_K1, e_f, e_c))
        assert abs(k_f - lc.REF_K1) <= 1.01 * abs(k_c - lc.REF_K1) + 1e-3
        assert e_f <= 1.01 * e_c + 1e-3


# ------------------------------------------------------------------------------------------------ speed

def test_the_lens_launches_are_no_slower_than_the_composition(native, dev):
    """P = 8, uint8, 480 x 640 -> 256 x 256, k = 1; alternating legs in one process (capture_lens_checks.measure_lens).
    Asserted: the lens forward <= torch_composition, the lens gradient <= the composition's backward.  The ratios to the
    pinhole launches are printed, not asserted: the bytes are equal and the extra work is ALU, no bound is derivable."""
    r = lc.measure_lens(dev, native)
    print("[capture lens] P=8 uint8 480x640 -> 256x256 k=1: forward lens %.1f us, pinhole %.1f us (ratio %.2f), composed %.1f us; "
          "gradient lens %.1f us, pinhole %.1f us (ratio %.2f), composed backward %.1f us; rounds %s" % (
              r["lens_us"], r["pinhole_us"], r["lens_us"] / r["pinhole_us"], r["composed_us"], r["lens_grad_us"],
              r["pinhole_grad_us"], r["lens_grad_us"] / r["pinhole_grad_us"], r["composed_grad_us"], r["rounds"]))
    assert r["lens_us"] <= r["composed_us"]
    assert r["lens_grad_us"] <= r["composed_grad_us"]
