"""capture.rectify(..., lens=) on the device (csrc/svbrdf_capture_lens.hip: k_lens_rectify; svbrdf_rectify_photos_lens).  The
oracle is the numpy float32 restatement of tests/capture_lens_checks.py (held against float64 and torch's grid_sample in
tests/test_capture_lens_cpu.py): every comparison of values and weights here is BIT FOR BIT, no tolerance, no exclusions.
"""
import numpy as np
import pytest
import torch

import capture_checks as cc
import capture_lens_checks as lc
from test_gpu_capture import HOSTILE

pytestmark = pytest.mark.gpu

MATRIX_KINDS = ("mild", "outside", "horizon")
# destination -> (sources, (matrix kind, lens kind[, k of the forward]) pairs or None for the whole product, the k of the case)
SMALL, MIDDLE, LARGE = ((5, 7), (97, 131)), ((97, 131), (480, 640)), ((480, 640),)
LARGE_PAIRS = (("outside", "barrel", (1, 2, 4)), ("mild", "pincushion"), ("horizon", "folding"), ("outside", "null"))
CASES = {
    (1, 1): (SMALL, None, (1, 2, 4)),
    (3, 70): (SMALL, None, (1, 2, 4)),          # partial tiles in x
    (5, 65): (SMALL, None, (1, 2, 4)),          # partial tiles both ways
    (32, 32): (SMALL, None, (1, 2, 4)),
    (64, 64): (MIDDLE, None, (1, 2, 4)),
    # 5 x 65 tiles per photo; the numpy restatement sets the price of this one: k = 4 for one pair in the forward (the
    # gradient test keeps to k = 1, 2 here)
    (260, 260): (LARGE, LARGE_PAIRS, (1, 2)),
}


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
    return capture.gamma_lut()


def source(fmt, seed, P, size, blobs=False):
    return cc.u8_source(seed, P, *size, blobs=blobs) if fmt == "uint8" else cc.float_source(seed, P, *size)


def rectify(capture, dev, src, M, L, size, k=1, lut=None, clip=None, want_weights=True):
    """capture.rectify on numpy inputs -> numpy (values, weights)"""
    u8 = src.dtype == np.uint8
    v, w = capture.rectify(torch.from_numpy(src).to(dev), M, size, lut=lut if u8 else None, clip=clip, samples=k, lens=L,
                           want_weights=want_weights)
    assert v.dtype == torch.float32 and v.device == dev
    return v.cpu().numpy(), None if w is None else w.cpu().numpy()


def assert_same(got, want, what):
    for name, g, e in zip(("values", "weights"), got, want):
        assert cc.same_bits(g, e), "%s: %s differ from the restatement in %d of %d" % (what, name, cc.count_differing(g, e), e.size)


@pytest.mark.parametrize("fmt", ("uint8", "float32"))
@pytest.mark.parametrize("dst_size", list(CASES), ids=lambda s: "dst%dx%d" % s)
def test_rectify_lens_is_the_restatement_bit_for_bit(capture, dev, lut, dst_size, fmt):
    """P = 5 with a matrix and a lens row each, and P = 1 (photo 0 of the five on its own: one restatement serves both)"""
    sources, pairs, ks = CASES[dst_size]
    P = 5
    seen_fold = False
    for src_size in sources:
        src = source(fmt, 140 + P, P, src_size)
        for pair in pairs or [(m, l) for m in MATRIX_KINDS for l in lc.LENS_KINDS]:
            mkind, lkind = pair[:2]
            M, L = cc.matrices(mkind, src_size, dst_size, P), lc.lenses(lkind, src_size, P)
            for k in pair[2] if len(pair) > 2 else ks:
                want = lc.restatement(src, M, L, dst_size, k=k, lut=lut.numpy(), detail=True)
                got = rectify(capture, dev, src, M, L, dst_size, k=k, lut=lut)
                what = "%s %s %s k=%d" % (src_size, mkind, lkind, k)
                assert_same(got, want[:2], what)
                assert set(np.unique(got[1])) <= {0.0, 1.0} and not got[0][np.broadcast_to(got[1][:, None] == 0, got[0].shape)].any()
                one = rectify(capture, dev, src[:1], M[:1], L[:1], dst_size, k=k, lut=lut)
                assert_same(one, (want[0][:1], want[1][:1]), what + " P=1")
                seen_fold = seen_fold or (lkind == "folding" and bool(want[2]["mono_refused"].any()))
                if lkind in ("barrel", "pincushion") and mkind == "mild" and min(dst_size) >= 32 and min(src_size) >= 97:
                    pin = cc.restatement(src, M, dst_size, k=k, lut=lut.numpy())
                    assert want[1].mean() > 0.5 and not cc.same_bits(pin[0], want[0])      # the lens moves the taps
    if min(dst_size) >= 32:
        assert seen_fold        # mono <= 0 refuses sub-samples that are inside the frame otherwise


@pytest.mark.parametrize("fmt", ("uint8", "float32"))
def test_null_lens_is_the_pinhole_launch_bit_for_bit(capture, dev, lut, fmt):
    for src_size, dst_size in (((5, 7), (3, 70)), ((97, 131), (32, 32)), ((480, 640), (64, 64))):
        P = len(cc.KINDS) + len(HOSTILE)
        M = np.stack([cc.matrix(kind, src_size, dst_size, p) for p, kind in enumerate(cc.KINDS)] + list(HOSTILE.values()))
        src = source(fmt, 7, P, src_size, blobs=True)
        s = torch.from_numpy(src).to(dev)
        t = lut if fmt == "uint8" else None
        clip = (5, 250) if fmt == "uint8" else (0.02, 0.98)
        for k in (1, 2, 4):
            pin = capture.rectify(s, M, dst_size, lut=t, clip=clip, samples=k)
            got = capture.rectify(s, M, dst_size, lut=t, clip=clip, samples=k, lens=lc.NULL)      # one [9] for all
            assert torch.equal(pin[0].view(torch.int32), got[0].view(torch.int32)) and torch.equal(pin[1], got[1]), (src_size, k)
            assert bool(pin[1][:3].any())


@pytest.mark.parametrize("fmt", ("uint8", "float32"))
def test_hostile_lens_rows_and_matrices_give_zeros_and_a_clean_return(native, capture, dev, lut, fmt):
    """NaN, +-inf, fx = 0, fx < 0, 1e30 in the lens; NaN, +-inf, 1e30, m8 = 0 in the matrices: all-zero values and weights,
    nothing written outside the outputs, and the next ordinary call is right"""
    src_size, dst_size = (97, 131), (33, 70)
    rows = lc.hostile_lenses(src_size)
    for M, L in ((cc.matrices("mild", src_size, dst_size, len(rows)), np.stack(list(rows.values()))),
                 (np.stack(list(HOSTILE.values())), lc.lenses("barrel", src_size, len(HOSTILE))),
                 (np.stack(list(HOSTILE.values())), np.stack(list(rows.values()))[:len(HOSTILE)])):
        P = len(M)
        src = source(fmt, 70, P, src_size)
        for k in (1, 2, 4):
            want = lc.restatement(src, M, L, dst_size, k=k, lut=lut.numpy())
            dirty = [name for name, w in zip(rows, want[1]) if w.any()]
            assert not want[0].any() and not want[1].any(), dirty
            out = lc.abi_rectify_lens(native, dev, src, M, L, dst_size, k=k, lut=lut if fmt == "uint8" else None)
            assert out["canaries_intact"] and out["launches"] == 1 and not out["values"].any() and not out["weights"].any(), k
    M, L = cc.matrices("mild", src_size, dst_size, P), lc.lenses("barrel", src_size, P)
    assert_same(rectify(capture, dev, src, M, L, dst_size, lut=lut), lc.restatement(src, M, L, dst_size, lut=lut.numpy()), "after")


@pytest.mark.parametrize("fmt", ("uint8", "float32"))
def test_pointers_off_alignment_leading_dimensions_shared_lens_and_no_weights(native, capture, dev, lut, fmt):
    src_size, dst_size, P, k = (97, 131), (5, 65), 6, 2
    src = source(fmt, 31, P, src_size)
    M, L = cc.matrices("outside", src_size, dst_size, P), lc.lenses("barrel", src_size, P)
    table = lut if fmt == "uint8" else None
    want = lc.restatement(src, M, L, dst_size, k=k, lut=lut.numpy())
    for so, po in ((0, 0), (1, 0), (0, 1), (3, 1)):     # a code is one byte, a float four
        out = lc.abi_rectify_lens(native, dev, src, M, L, dst_size, k=k, lut=table, src_offset=so, ptr_offset=po)
        assert out["canaries_intact"] and out["launches"] == 1
        assert_same((out["values"], out["weights"]), want, "offsets %d %d" % (so, po))
    out = lc.abi_rectify_lens(native, dev, src, M, L, dst_size, k=k, lut=table, want_weights=False)
    assert out["canaries_intact"] and cc.same_bits(out["values"], want[0])
    v, w = rectify(capture, dev, src, M, L, dst_size, k=k, lut=lut, want_weights=False)
    assert w is None and cc.same_bits(v, want[0])
    # [B,S] leading dimensions: matrices [2,3,3,3], lens [2,3,9]
    s = torch.from_numpy(src).to(dev)
    v, w = capture.rectify(s.reshape((2, 3) + s.shape[1:]), M.reshape(2, 3, 3, 3), dst_size, lut=table, samples=k,
                           lens=torch.from_numpy(L).reshape(2, 3, 9))
    assert tuple(v.shape) == (2, 3, 3) + dst_size and tuple(w.shape) == (2, 3) + dst_size
    assert_same((v.cpu().numpy().reshape(want[0].shape), w.cpu().numpy().reshape(want[1].shape)), want, "[B,S]")
    # one lens for all photos, as float64 on the host
    shared = lc.restatement(src, M, np.broadcast_to(L[0], (P, 9)), dst_size, k=k, lut=lut.numpy())
    assert_same(rectify(capture, dev, src, M, L[0].astype(np.float64), dst_size, k=k, lut=lut), shared, "shared lens")


def test_clip_and_lut_with_the_blobs_source(capture, dev):
    """saturated and black discs under a lens: the clip thresholds refuse their taps, and another table gives other values"""
    src_size, dst_size, P = (97, 131), (32, 32), 3
    src = cc.u8_source(5, P, *src_size, blobs=True)
    M, L = cc.matrices("mild", src_size, dst_size, P), lc.lenses("barrel", src_size, P)
    shares = []
    for table in (capture.gamma_lut(), capture.srgb_lut()):
        for clip in (None, (5, 250), (-1, 256), (19.5, 235.5)):
            for k in (1, 2):
                want = lc.restatement(src, M, L, dst_size, k=k, lut=table.numpy(), clip=clip)
                assert_same(rectify(capture, dev, src, M, L, dst_size, k=k, lut=table, clip=clip), want, "clip %s k=%d" % (clip, k))
                shares.append(float((want[1] == 0).mean()))
    assert shares[0] == 0.0 and 0.0 < shares[2] < 0.5 and shares[4] == 0.0 and shares[6] >= shares[2]
