"""svbrdf_rectify_photos_grad_matrices (csrc/svbrdf_capture_grad.hip: k_homography_grad) and the autograd path of
capture.rectify on the MI355X, against the numpy float32 restatement of tests/capture_grad_checks.py.

The bound.  ref_n is the float64 sum of the restatement's float32 term planes and A_n that of their absolute values; the
kernel's terms are those planes, so what separates got_n from ref_n is D float32 additions, the term's own last rounding and
the final rounding:  |got_n - ref_n| <= (D + 2) 2^-24 A_n,  for all nine entries of every photo, no element excluded.  D is
the binding's RECTIFY_GRAD_DEPTH.  Every case prints its largest err / A in units of 2^-24.
"""
import numpy as np
import pytest
import torch

import capture_checks as cc
import capture_grad_checks as gc
from test_gpu_capture import HOSTILE

pytestmark = pytest.mark.gpu

DESTINATIONS = ((1, 1), (3, 5), (4, 64), (5, 65), (9, 130), (260, 260))    # one pixel .. 325 partials for the finisher
SOURCES = ((7, 9), (37, 53))
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


def assert_within(got, terms, what, extra=0.0):
    """-> the largest |got - ref| / A in units of 2^-24 (0 where A = 0, where got must be 0 as well)"""
    ref, A = gc.sums(terms)
    err = np.abs(got.astype(np.float64) - ref)
    assert np.isfinite(got).all(), what
    assert (err <= gc.bound(A) + extra).all(), (what, (err / np.maximum(gc.bound(A) + extra, 1e-300)).max(), got, ref)
    units = float((err[A > 0] / (2.0 ** -24 * A[A > 0])).max()) if (A > 0).any() else 0.0
    return units


# ------------------------------------------------------------------------------------------------ parity

@pytest.mark.parametrize("kind", cc.KINDS)
@pytest.mark.parametrize("k", (1, 2, 4))
@pytest.mark.parametrize("fmt", ("uint8", "float32"))
@pytest.mark.parametrize("src_size", SOURCES, ids=lambda s: "src%dx%d" % s)
@pytest.mark.parametrize("dst_size", DESTINATIONS, ids=lambda s: "dst%dx%d" % s)
def test_parity_with_the_restatement(native, dev, lut, dst_size, src_size, fmt, k, kind):
    """P = 5 with a matrix each and P = 1 (photo 0 of the five on its own): one restatement serves both launches"""
    P = 5
    src = source(fmt, 100 + k, P, src_size)
    M = cc.matrices(kind, src_size, dst_size, P)
    G = normal(7 * k + len(kind), (P, 3) + dst_size)
    table = lut if fmt == "uint8" else None
    terms, ok, _ = gc.grad_terms(src, M, dst_size, G, k, table)
    out5 = gc.abi_grad(native, dev, src, M, dst_size, G, k, table)
    out1 = gc.abi_grad(native, dev, src[:1], M[:1], dst_size, G[:1], k, table)
    for out in (out5, out1):
        assert out["canaries_intact"] and out["launches"] == 1 and out["workspace_zero"]
    units = max(assert_within(out5["grad"], terms, "P=5"), assert_within(out1["grad"], terms[:1], "P=1"))
    assert cc.same_bits(out1["grad"][0], out5["grad"][0])           # a photo's row does not depend on the others
    print("[capture grad] %s %dx%d -> %dx%d k=%d %s: ok share %.3f, max err/A %.2f x 2^-24 (bound %d)" % (
        fmt, src_size[0], src_size[1], dst_size[0], dst_size[1], k, kind, ok.mean(), units, gc.depth() + 2))
    if kind == "identity" and k == 1 and src_size[1] >= dst_size[1] and src_size[0] >= dst_size[0]:
        assert ok.all()         # fx = 0 everywhere and the x1 clamp where the destination reaches the last column
    if kind == "horizon" and dst_size[1] >= 5:
        assert not ok.all()


# ------------------------------------------------------------------------------------------------ edge cases

@pytest.mark.parametrize("fmt", ("uint8", "float32"))
def test_nan_under_zero_weight_pixels_changes_no_bit_and_under_an_ok_pixel_its_photos_row(native, dev, lut, fmt):
    src_size, dst_size, P, k = (37, 53), (9, 130), 3, 2
    src = cc.u8_source(5, P, *src_size, blobs=True) if fmt == "uint8" else cc.float_source(5, P, *src_size)
    M = np.stack([cc.matrix(kind, src_size, dst_size, p) for p, kind in enumerate(("outside", "horizon", "mild"))])
    table = lut if fmt == "uint8" else None
    G = normal(3, (P, 3) + dst_size)
    terms, ok, _ = gc.grad_terms(src, M, dst_size, G, k, table, CLIPS[fmt])
    assert 0 < ok[0].mean() < 1 and 0 < ok[1].mean() < 1 and ok[2].any()
    base = gc.abi_grad(native, dev, src, M, dst_size, G, k, table, CLIPS[fmt])["grad"]
    assert_within(base, terms, "base")
    dead = np.broadcast_to(~ok[:, None], G.shape)
    zeros, nans = np.where(dead, np.float32(0.0), G), np.where(dead, np.float32(np.nan), G)
    got_z = gc.abi_grad(native, dev, src, M, dst_size, zeros, k, table, CLIPS[fmt])["grad"]
    got_n = gc.abi_grad(native, dev, src, M, dst_size, nans, k, table, CLIPS[fmt])["grad"]
    assert cc.same_bits(got_n, got_z) and cc.same_bits(got_n, base) and np.isfinite(got_n).all()
    y, x = np.argwhere(ok[1])[0]
    G2 = G.copy()
    G2[1, 0, y, x] = np.nan
    out = gc.abi_grad(native, dev, src, M, dst_size, G2, k, table, CLIPS[fmt])
    assert np.isnan(out["grad"][1]).any() and cc.same_bits(out["grad"][[0, 2]], base[[0, 2]]) and out["workspace_zero"]
    # and the scratch that saw a NaN serves the next call
    again = gc.abi_grad(native, dev, src, M, dst_size, G, k, table, CLIPS[fmt], workspace=out["workspace"])["grad"]
    assert cc.same_bits(again, base)


def test_a_clipped_tap_drops_its_pixel(native, dev):
    src_size, dst_size, k = (37, 53), (9, 30), 1
    src = 0.1 + 0.8 * cc.float_source(9, 1, *src_size)
    M = cc.matrices("mild", src_size, dst_size, 1)
    G = normal(4, (1, 3) + dst_size)
    clip = (0.05, 0.95)
    t0, ok0, cells = gc.grad_terms(src, M, dst_size, G, k, None, clip)
    assert ok0.all()
    y, x = 4, 17
    src[0, 1, int(cells["y0f"][0, 0, y, x]) + 1, int(cells["x0f"][0, 0, y, x])] = 0.97       # tap c of one channel
    t1, ok1, _ = gc.grad_terms(src, M, dst_size, G, k, None, clip)
    assert not ok1[0, y, x] and ok1.any() and not t1[0, :, :, y, x].any() and t0[0, :, :, y, x].any()
    got = gc.abi_grad(native, dev, src, M, dst_size, G, k, None, clip)["grad"]
    assert_within(got, t1, "clipped")
    unclipped = gc.abi_grad(native, dev, src, M, dst_size, G, k, None, None)["grad"]
    assert not cc.same_bits(got, unclipped)


@pytest.mark.parametrize("fmt", ("uint8", "float32"))
def test_hostile_matrices_give_zero_rows_and_a_clean_return(native, dev, lut, fmt):
    src_size, dst_size = (37, 53), (9, 130)
    P = len(HOSTILE)
    src = source(fmt, 21, P, src_size)
    M = np.stack(list(HOSTILE.values()))
    table = lut if fmt == "uint8" else None
    for k in (1, 2, 4):
        G = normal(k, (P, 3) + dst_size)
        terms, ok, _ = gc.grad_terms(src, M, dst_size, G, k, table)
        assert not ok.any() and not terms.any()
        out = gc.abi_grad(native, dev, src, M, dst_size, G, k, table)
        assert not out["grad"].any() and out["canaries_intact"] and out["workspace_zero"], (k, out["grad"])
    M2 = cc.matrices("mild", src_size, dst_size, P)                 # and the next ordinary call is right
    t2, _, _ = gc.grad_terms(src, M2, dst_size, G, 4, table)
    assert_within(gc.abi_grad(native, dev, src, M2, dst_size, G, 4, table)["grad"], t2, "after hostile")


# ------------------------------------------------------------------------------------------------ reproducibility

@pytest.mark.parametrize("fmt", ("uint8", "float32"))
def test_bitwise_reproducible_on_fresh_and_reused_scratch_and_off_alignment(native, capture, dev, lut, fmt):
    src_size, dst_size, P, k = (37, 53), (260, 260), 4, 2
    src = source(fmt, 31, P, src_size)
    M = cc.matrices("outside", src_size, dst_size, P)
    G = normal(8, (P, 3) + dst_size)
    table = lut if fmt == "uint8" else None
    first = gc.abi_grad(native, dev, src, M, dst_size, G, k, table)
    second = gc.abi_grad(native, dev, src, M, dst_size, G, k, table)
    reused = gc.abi_grad(native, dev, src, M, dst_size, G, k, table, workspace=first["workspace"])
    third = gc.abi_grad(native, dev, src, M, dst_size, G, k, table, workspace=first["workspace"])
    assert first["grad"].any()
    for other in (second, reused, third):
        assert cc.same_bits(other["grad"], first["grad"]) and other["workspace_zero"] and other["canaries_intact"]
    # pointers 4 bytes (a code: 1 byte) off their allocation's alignment
    off = gc.abi_grad(native, dev, src, M, dst_size, G, k, table, src_offset=1, ptr_offset=1)
    assert cc.same_bits(off["grad"], first["grad"]) and off["canaries_intact"]
    # leading dimensions [B,S] through the Python layer give the rows of [P]
    s = torch.from_numpy(src).to(dev)
    t = None if table is None else torch.from_numpy(table)
    Gd = torch.from_numpy(G).to(dev)
    Mp = torch.from_numpy(M).to(dev).requires_grad_(True)
    capture.rectify(s, Mp, dst_size, lut=t, samples=k)[0].backward(Gd)
    Mb = torch.from_numpy(M).reshape(2, 2, 3, 3).to(dev).requires_grad_(True)
    capture.rectify(s.reshape((2, 2) + s.shape[1:]), Mb, dst_size, lut=t, samples=k)[0].backward(Gd.reshape((2, 2) + Gd.shape[1:]))
    assert tuple(Mb.grad.shape) == (2, 2, 3, 3) and cc.same_bits(Mb.grad.cpu().numpy().reshape(P, 9), first["grad"])
    assert cc.same_bits(Mp.grad.cpu().numpy(), first["grad"])


# ------------------------------------------------------------------------------------------------ autograd

def test_autograd_is_the_entry_bit_for_bit(native, capture, dev, lut):
    src_size, dst_size, P, k = (37, 53), (9, 130), 5, 2
    src = cc.u8_source(41, P, *src_size)
    M = cc.matrices("outside", src_size, dst_size, P)
    G = normal(9, (P, 3) + dst_size)
    want = gc.abi_grad(native, dev, src, M, dst_size, G, k, lut, (5, 250))["grad"]
    s, t, Gd = torch.from_numpy(src).to(dev), torch.from_numpy(lut), torch.from_numpy(G).to(dev)
    # float32 on the device
    Md = torch.from_numpy(M).to(dev).requires_grad_(True)
    before = native.launch_count()
    vals, w = capture.rectify(s, Md, dst_size, lut=t, clip=(5, 250), samples=k)
    assert vals.grad_fn is not None and not w.requires_grad and native.launch_count() - before == 1
    plain = capture.rectify(s, Md.detach(), dst_size, lut=t, clip=(5, 250), samples=k)
    assert plain[0].grad_fn is None and torch.equal(plain[0], vals.detach()) and torch.equal(plain[1], w)
    before = native.launch_count()
    vals.backward(Gd)
    assert native.launch_count() - before == 1
    assert Md.grad.dtype == torch.float32 and Md.grad.device == Md.device and tuple(Md.grad.shape) == (P, 9)
    assert cc.same_bits(Md.grad.cpu().numpy(), want)
    # float64 on the host, [P,3,3], through a non-contiguous grad_output
    Mh = torch.from_numpy(M.astype(np.float64)).reshape(P, 3, 3).requires_grad_(True)
    vals, _ = capture.rectify(s, Mh, dst_size, lut=t, clip=(5, 250), samples=k)
    (vals.transpose(-1, -2) * Gd.transpose(-1, -2)).sum().backward()
    assert Mh.grad.dtype == torch.float64 and Mh.grad.device.type == "cpu" and tuple(Mh.grad.shape) == (P, 3, 3)
    assert np.array_equal(Mh.grad.numpy().reshape(P, 9), want.astype(np.float64))
    # no double backward
    Md2 = torch.from_numpy(M).to(dev).requires_grad_(True)
    g, = torch.autograd.grad(capture.rectify(s, Md2, dst_size, lut=t, samples=k)[0], Md2, Gd, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


def test_one_shared_matrix_gets_the_sum_of_the_rows(native, capture, dev):
    src_size, dst_size, P, k = (37, 53), (9, 130), 5, 1
    src = cc.float_source(43, P, *src_size)
    m = cc.matrix("mild", src_size, dst_size, 0)
    M = np.broadcast_to(m, (P, 9)).copy()
    G = normal(10, (P, 3) + dst_size)
    terms, _, _ = gc.grad_terms(src, M, dst_size, G, k)
    shared = torch.from_numpy(m).reshape(3, 3).to(dev).requires_grad_(True)
    vals, _ = capture.rectify(torch.from_numpy(src).to(dev), shared, dst_size, samples=k)
    vals.backward(torch.from_numpy(G).to(dev))
    assert tuple(shared.grad.shape) == (3, 3)
    ref, A = gc.sums(terms)
    # each row within its bound, their float64 sum rounded once more
    err = np.abs(shared.grad.cpu().numpy().reshape(9).astype(np.float64) - ref.sum(axis=0))
    assert (err <= gc.bound(A).sum(axis=0) + 2.0 ** -24 * np.abs(ref.sum(axis=0))).all(), err
    rows = gc.abi_grad(native, dev, src, M, dst_size, G, k)["grad"]
    assert np.array_equal(shared.grad.cpu().numpy().reshape(9), rows.astype(np.float64).sum(axis=0).astype(np.float32))


def test_torch_composition_backward_agrees(native, capture, dev):
    """k = 1, float source, `mild` matrices: grid_sample's backward and the chain to M in float32 on the device, against
    the one launch.  The composed form's own float32 error is MEASURED here, on the CPU, against the same composition in
    float64 -- the largest |float32 - float64| / A over the entries, 3.74 x 2^-24 at this shape (and 9.7 at 96x128 -> 32x32,
    207 at 37x53 -> 260x260: it grows with the number of pixels, whose coordinate roundings it sums) -- and added to the
    bound."""
    src_size, dst_size, P = (37, 53), (9, 130), 5
    src = cc.float_source(11, P, *src_size)
    M = cc.matrices("mild", src_size, dst_size, P)
    G = normal(5, (P, 3) + dst_size)
    terms, ok, _ = gc.grad_terms(src, M, dst_size, G)
    assert ok.all()
    _, A = gc.sums(terms)

    def composed(device, dtype):
        m = torch.from_numpy(M).to(device=device, dtype=dtype).requires_grad_(True)
        v, _ = cc.torch_composition(torch.from_numpy(src).to(device=device, dtype=dtype), m, dst_size, dtype=dtype)
        v.backward(torch.from_numpy(G).to(device=device, dtype=dtype))
        return m.grad.double().cpu().numpy()

    own = float((np.abs(composed("cpu", torch.float32) - composed("cpu", torch.float64)) / (2.0 ** -24 * A)).max())
    got = gc.abi_grad(native, dev, src, M, dst_size, G)["grad"]
    diff = np.abs(got.astype(np.float64) - composed(dev, torch.float32))
    print("[capture grad] composed backward: own float32 error %.2f x 2^-24 A (measured on the CPU against float64), "
          "one launch against it %.2f x 2^-24 A" % (own, (diff / (2.0 ** -24 * A)).max()))
    assert (diff <= gc.bound(A) + own * 2.0 ** -24 * A).all()


# ------------------------------------------------------------------------------------------------ registration

def test_registration_converges_as_the_composed_loop_does(capture, dev):
    """32 x 32 grid, k = 1, a 96 x 128 band-limited float source, every corner 3 source pixels off (seed REG_SEED), 150 Adam
    steps at lr 0.2 on the corners against the rectification under the true corners.  Asserted: the fused loop ends below
    its start, and at most 1.01 x the composed loop's end + 1e-3 px.
    The loss is mean w (log(rect + eps) - log(target + eps))^2.  The float64 loop on the CPU (torch_composition in float64)
    ends at 0.0007 px from 3.0 for this seed (seeds 0..3: 0.00095, 0.00100, 0.00069, 0.00099), and the same loop in float32
    ends at the same five digits: the end is a property of the loop, not of its roundings.
    With the ABSOLUTE log difference instead (the tool's loss) the ratio of two end errors is no statement about either
    loop: the gradient does not vanish at the optimum, Adam at lr 0.2 jitters between 0.007 and 0.07 px over the last 30
    steps, and step 150 falls somewhere in it.  torch_composition on the CPU alone, float64 against float32, seeds 0..3:
    0.0167 / 0.0194, 0.0167 / 0.0327, 0.0132 / 0.0093, 0.0292 / 0.0272.  Measured on the MI355X with that loss, fused /
    composed, seeds 0..7: 0.033 / 0.016, 0.043 / 0.024, 0.046 / 0.026, 0.016 / 0.046, 0.023 / 0.027, 0.030 / 0.062,
    0.018 / 0.023, 0.045 / 0.037 -- four of eight either way, the two trajectories equal to four digits down to 0.05 px
    (step 60).  The absolute-difference loop is printed, not asserted."""
    src = gc.band_limited_source(7, *gc.REG_SRC)
    s = torch.from_numpy(src).to(dev)
    with torch.no_grad():
        target, tw = capture.rectify(s, capture.corner_matrices(torch.tensor(gc.REG_CORNERS[None]), gc.REG_GRID), gc.REG_GRID)
    assert bool((tw == 1).all())
    c0 = gc.start_corners(gc.REG_SEED)
    start = gc.corner_error(c0)
    fused = gc.registration_loop(lambda M: capture.rectify(s, M, gc.REG_GRID), target, tw, c0, dev)
    comp = gc.registration_loop(lambda M: cc.torch_composition(s, M.reshape(1, 9), gc.REG_GRID), target, tw, c0, dev)
    e_fused, e_comp = gc.corner_error(fused), gc.corner_error(comp)
    print("[capture grad] registration: mean corner error %.3f px -> fused %.5f, composed %.5f" % (start, e_fused, e_comp))
    l1 = gc.registration_loop(lambda M: capture.rectify(s, M, gc.REG_GRID), target, tw, c0, dev, power=1)
    print("[capture grad] registration with the absolute difference, fused: %.5f px (not asserted)" % gc.corner_error(l1))
    assert abs(start - gc.REG_OFF) < 1e-9
    assert e_fused < start
    assert e_fused <= 1.01 * e_comp + 1e-3


# ------------------------------------------------------------------------------------------------ speed

def test_one_launch_is_no_slower_than_the_composed_backward(native, dev):
    """P = 8, uint8, 480 x 640 -> 256 x 256, k = 1; alternating legs in one process (capture_grad_checks.measure_grad).  No
    absolute time is asserted."""
    r = gc.measure_grad(dev, native)
    print("[capture grad] P=8 uint8 480x640 -> 256x256 k=1: one launch %.1f us, composed backward %.1f us (ratio %.3f), forward "
          "launch %.1f us (backward / forward %.2f); rounds %s" % (r["fused_us"], r["composed_us"], r["fused_us"] / r["composed_us"],
                                                                  r["forward_us"], r["fused_us"] / r["forward_us"], r["rounds"]))
    assert r["fused_us"] <= r["composed_us"]


# ------------------------------------------------------------------------------------------------ the bits

def test_the_four_entries_return_the_recorded_bits(native, dev, golden):
    """tests/golden/g24_capture_bits.npz holds what the four rectify entries returned on the MI355X at the commit before the
    capture units were put on shared device functions (capture_grad_checks.record_bits: P = 3, 37 x 53 -> 9 x 70, both
    formats, k = 1, 2, 4, a hostile lens row).  The library under test returns exactly those bits for values, weights,
    grad_matrices and grad_lens, leaves each workspace all zero, and a second call on the same workspace returns the same
    bits.  The bits are stable because the source fixes every rounding and the whole order of the reduction -- a thread's
    sub-samples in (j, i) order, the 64-lane butterfly, (w0 + w1) + (w2 + w3), the lane-strided float64 sum in index order,
    one rounding to float32 -- and no operation may be fused or reassociated (-ffp-contract=off, IEEE division): they are a
    property of the definition, not of the compiler's register allocation or schedule."""
    want = golden("g24_capture_bits.npz")
    bits, facts = gc.record_bits(native, dev)
    assert sorted(bits) == sorted(want.files) and len(bits) == 6 * len(gc.BITS_CASES) == 36
    for name, (intact, one_launch, zeroed, repeats) in facts.items():
        assert intact and one_launch and zeroed and repeats, (name, intact, one_launch, zeroed, repeats)
    for name in sorted(bits):
        assert bits[name].dtype == np.float32 == want[name].dtype and bits[name].shape == want[name].shape, name
        assert cc.same_bits(bits[name], want[name]), (name, cc.count_differing(bits[name], want[name]))
    # the case is not empty: pixels of both kinds, non-zero gradients for the first two photos, zeros under the hostile lens
    for fmt, k in gc.BITS_CASES:
        name = "%s_k%d_" % (fmt, k)
        assert 0 < want[name + "weights"].mean() < 1 and want[name + "lens_weights"][:2].any(), name
        assert want[name + "grad_matrices"].all(axis=1).any() and want[name + "lens_grad"][:2].any(axis=1).all(), name
        assert not want[name + "lens_weights"][2].any() and not want[name + "lens_grad"][2].any(), name
