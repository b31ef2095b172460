"""The photo losses with per-pixel confidence weights on the device (csrc/svbrdf_photo_loss.hip: k_wphoto*, k_head_wphoto*;
losses.PhotoLoss / HeadPhotoLoss with `weights`):

    L = (1/N) sum w | log(render(scene[b,s], input[b]) + eps) - log(where(w > 0, photo[b,s], 0) + eps) |

against the reference (tests/golden/g21_weighted_photo_loss.npz) and the C oracle's composition
(tests/photo_checks.py with `weights`), through the C ABI -- scene table in device memory and by value -- and through the
modules, with one weight plane per photo and one per item.  Bounds: tests/tolerances.py unchanged -- loss 1e-6 relative;
gradient 1e-4 |b| + 1e-5 max|b|, widened by 2 |b - f64| for at most MAX_WIDENED_GRAD elements; at most MAX_TIE_PIXELS tie
pixels.  By the oracle alone the cases have 0 tie pixels and at most 2 widened elements
(tests/test_weighted_photo_loss_cpu.py::test_gpu_cases_stay_inside_the_caps_by_the_comparison_values_alone).

Speed at the configuration-2 shape (B = 8, 256 x 256, S = 9, per-photo weights, maps from HBM), medians of event-timed
launches, legs alternating in one process:  fused weighted <= the unfused weighted composition, and weighted <= 60/51 x the
unweighted kernel -- 60/51 = (12 + 27 + 9 + 12) / (12 + 27 + 12) is the byte ratio, the most a purely HBM-bound kernel could
lose; this kernel is VALU-bound and its loop grows by 5 of about 239 instructions per render.  Measured on an MI355X
(profiles/r13_weighted_photo_loss.txt): weighted 38.06 us, unweighted 35.58 us (ratio 1.070 against the bound of 1.176),
the unfused composition 340.84 us (9.0x).
"""
import os

import numpy as np
import pytest
import torch

import head_checks
import photo_checks
import synth
import tolerances
import weighted_photo_checks as wp
from photo_checks import assert_scratch_is_zero as _scratch_is_zero, to_device as _t, to_numpy as _np

pytestmark = pytest.mark.gpu
EPS = wp.EPS


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X (select CPU tests with -m 'not gpu')"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def native():
    from svbrdf_estimation_amd import _native
    _native._load()
    return _native


def _module(head, normalize="count"):
    from svbrdf_estimation_amd import losses, renderers
    fn = (losses.HeadPhotoLoss if head else losses.PhotoLoss)(renderers.LocalRenderer(), normalize=normalize)
    assert fn.uses_fused_kernel() and fn.eps == EPS
    return fn


def _run_all_ways(native, dev, what, x, ph, w, sc, head, ref=None, cap=tolerances.MAX_TIE_PIXELS):
    """C ABI with the device table and with the by-value table, the module through backward(): each within the bounds of
    `ref` (a photo_checks.Reference, or None), the same bits as each other, forward-only the same loss bitwise, scratch zeroed
    -> (loss, gradient) of the device-table C ABI call"""
    d_x, d_ph, d_w, d_sc, h_sc = _t(x, dev), _t(ph, dev), _t(w, dev), _t(sc, dev), torch.from_numpy(np.ascontiguousarray(sc))
    results = {}
    for form, table in (("device table", d_sc), ("by-value table", h_sc)):
        loss, grad = native.photo_loss(d_x, d_ph, table, EPS, head=head, weights=d_w)
        results["C ABI, " + form] = (loss.item(), _np(grad))
        leaf = d_x.clone().requires_grad_(True)
        l = _module(head)(leaf, d_ph, table, d_w)
        assert l.dim() == 0
        l.backward()
        results["module, " + form] = (l.item(), _np(leaf.grad))
        l, g = native.photo_loss(d_x, d_ph, table, EPS, want_grad=False, head=head, weights=d_w)
        assert g is None
        results["forward only, " + form] = (l.item(), None)
    first = results["C ABI, device table"]
    for how, (loss, grad) in results.items():
        print("[weighted-photo] %s, %s: loss %.9g%s" % (what, how, loss, "" if ref is None else " (oracle %.9g)" % ref.loss))
        if ref is not None and grad is not None:
            ref.assert_close(loss, grad, "%s %s" % (what, how), max_ties=cap)
        assert loss == first[0] or (np.isnan(loss) and np.isnan(first[0])), "%s: %s: another loss than the device-table call" % (what, how)
        assert grad is None or np.array_equal(grad, first[1], equal_nan=True), "%s: %s: other gradient bits" % (what, how)
    _scratch_is_zero(native)
    return first


CASE_PARAMS = [(name, layout, head) for name, _, _, _, tied in wp.CASES for layout in wp.LAYOUTS
               for head in ((False, True) if tied else (False,))]


@pytest.mark.parametrize("name,layout,head", CASE_PARAMS,
                         ids=["%s-%s-%s" % (n, l, "head" if h else "maps") for n, l, h in CASE_PARAMS])
def test_against_the_oracle(dev, native, name, layout, head):
    c, ref = wp.reference(name, layout, head)
    x, w, H = (c["enc"] if head else c["maps"]), c["weights"][layout], c["H"]
    loss, grad = _run_all_ways(native, dev, "%s %s %s" % (name, layout, "head" if head else "maps"), x, c["photos"], w,
                               c["scenes"], head, ref)
    # the top quarter of the rows carries weight 0 for every photo: an all-zero gradient there, and a live one below
    assert np.isfinite(grad).all() and not grad[:, :, :max(H // 4, 1), :].any() and grad[:, :, H // 4 + 1:, :].any()


@pytest.mark.parametrize("head", [False, True], ids=["maps", "head"])
def test_reference_fixture(dev, native, golden, head):
    """NaN in the photos under zero weights, a fully masked row, H = 13 (items 1 and 2 start 4 bytes off 16-byte alignment):
    against the values the reference's renderer and torch autograd wrote"""
    g = golden("g21_weighted_photo_loss.npz")
    B, H = int(g["B"]), int(g["H"])
    x = head_checks.fixture_input(int(g["enc_seed"]), B, H) if head else synth.make_maps(int(g["input_seed"]), B, H)
    assert synth.checksum(x) == str(g["enc_sha256" if head else "input_sha256"])
    ref = photo_checks.Reference(x, g["photos"], g["scenes"], EPS, head=head, weights=g["weights"])
    loss, grad = _run_all_ways(native, dev, "g21 %s vs the oracle" % ("head" if head else "maps"), x, g["photos"], g["weights"],
                               g["scenes"], head, ref)
    ref_loss, ref_grad, ref_grad64 = (g["head_loss"], g["grad9"], g["grad9_f64"]) if head else \
        (g["loss"], g["grad_input"], g["grad_input_f64"])
    tolerances.assert_loss_close(loss, ref_loss, "g21 vs the reference loss")
    photo_checks.assert_photo_grad_close(grad, ref_grad, ref_grad64, ref.tie, "g21 %s vs the reference" % ("head" if head else "maps"))
    assert not grad[:, :, int(g["masked_row"]), :].any()


@pytest.mark.parametrize("name", ["17_s2", "64_s9"])
@pytest.mark.parametrize("head", [False, True], ids=["maps", "head"])
def test_all_ones_weights_are_the_unweighted_loss_bit_for_bit(dev, native, name, head):
    c = wp.case_inputs(name)
    d_x, d_ph = _t(c["enc"] if head else c["maps"], dev), _t(c["photos"], dev)
    for table in (_t(c["scenes"], dev), torch.from_numpy(c["scenes"])):
        plain_loss, plain_grad = native.photo_loss(d_x, d_ph, table, EPS, head=head)
        plain_fwd, _ = native.photo_loss(d_x, d_ph, table, EPS, head=head, want_grad=False)
        for P in (c["S"], 1):
            ones = torch.ones((wp.B_CASES, P, c["H"], c["H"]), device=dev)
            loss, grad = native.photo_loss(d_x, d_ph, table, EPS, head=head, weights=ones)
            assert loss.item() == plain_loss.item() and torch.equal(grad, plain_grad), (name, head, P)
            fwd, _ = native.photo_loss(d_x, d_ph, table, EPS, head=head, want_grad=False, weights=ones)
            assert fwd.item() == plain_fwd.item() == plain_loss.item()
    _scratch_is_zero(native)


@pytest.mark.parametrize("head", [False, True], ids=["maps", "head"])
def test_a_zero_weight_excuses_whatever_the_photo_holds(dev, native, head):
    """a {0, 1} mask with NaN, +inf and -1 written into the photos under the zeros: the loss of the oracle with those terms
    dropped, exactly zero gradient at every fully masked pixel; one NaN under a weight of 1e-3 is not excused"""
    c = wp.case_inputs("45_s9")
    x, sc, H = (c["enc"] if head else c["maps"]), c["scenes"], c["H"]
    mask = (c["weights"]["per-photo"] >= 0.5).astype(np.float32)
    assert (mask == 0).any() and (mask == 1).any() and not mask[:, :, :H // 4].any()
    junk = np.array([np.nan, np.inf, -1.0], np.float32)[(synth.uniform01(991, mask.shape) * 3).astype(np.int64)]
    spoiled = np.where((mask == 0)[:, :, None], junk[:, :, None], c["photos"]).astype(np.float32)
    assert np.isnan(spoiled).any() and np.isposinf(spoiled).any() and (spoiled == -1.0).any()
    ref = photo_checks.Reference(x, c["photos"], sc, EPS, head=head, weights=mask)     # the clean photos: the spoiled terms dropped
    loss, grad = _run_all_ways(native, dev, "mask over spoiled photos", x, spoiled, mask, sc, head, ref)
    assert np.isfinite(loss) and np.isfinite(grad).all()
    dead = np.broadcast_to((mask.max(axis=1) == 0)[:, None], grad.shape)
    assert dead.any() and not grad[dead].any() and grad[~dead].any()
    # the same bits as with the clean photos: nothing of the excused values gets anywhere
    clean_loss, clean_grad = native.photo_loss(_t(x, dev), _t(c["photos"], dev), _t(sc, dev), EPS, head=head, weights=_t(mask, dev))
    assert clean_loss.item() == loss and np.array_equal(_np(clean_grad), grad)
    # a weight of 1e-3 is not 0: a NaN under it is the caller's error
    b, s, i, j = [int(v[0]) for v in np.nonzero(mask)]
    almost = mask.copy()
    almost[b, s, i, j] = 1e-3
    bad = c["photos"].copy()
    bad[b, s, 1, i, j] = np.nan
    for want_grad in (True, False):
        l, _ = native.photo_loss(_t(x, dev), _t(bad, dev), _t(sc, dev), EPS, want_grad=want_grad, head=head, weights=_t(almost, dev))
        assert np.isnan(l.item())
        _scratch_is_zero(native)


@pytest.mark.parametrize("head", [False, True], ids=["maps", "head"])
def test_bad_weights_and_bad_maps_give_nan_and_leave_the_scratch_zeroed(dev, native, head):
    c = wp.case_inputs("33_s3")
    x, ph, sc, H = (c["enc"] if head else c["maps"]), c["photos"], c["scenes"], c["H"]
    d_x, d_ph, d_sc = _t(x, dev), _t(ph, dev), _t(sc, dev)
    for layout in wp.LAYOUTS:
        w = c["weights"][layout]
        good, _ = native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=_t(w, dev))
        assert np.isfinite(good.item())
        for value in (-0.5, 1.5, np.nan, np.inf, -np.inf):
            for where in ((1, -1, H - 1, H - 1), (0, 0, 0, 0)):     # a live pixel of the last workgroup; a masked one
                bad = w.copy()
                bad[where] = value
                for want_grad in (True, False):
                    l, _ = native.photo_loss(d_x, d_ph, torch.from_numpy(sc) if want_grad else d_sc, EPS, want_grad=want_grad,
                                             head=head, weights=_t(bad, dev))
                    assert np.isnan(l.item()), (layout, value, where, want_grad)
                    _scratch_is_zero(native)
        # a weight does not excuse the maps: NaN / inf at a pixel whose weights are 0 for every photo
        assert not w[:, :, 0, :].any()
        for channel in range(x.shape[1]):
            for value in (np.nan, np.inf):
                bad = x.copy()
                bad[1, channel, 0, 3] = value
                l, _ = native.photo_loss(_t(bad, dev), d_ph, d_sc, EPS, head=head, weights=_t(w, dev), want_grad=(channel % 2 == 0))
                assert np.isnan(l.item()), (layout, channel, value)
        _scratch_is_zero(native)
        again, _ = native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=_t(w, dev))
        assert again.item() == good.item()                      # nothing sticks


@pytest.mark.parametrize("head", [False, True], ids=["maps", "head"])
def test_misaligned_pointers_give_the_same_bits(dev, native, head):
    c = wp.case_inputs("17_s2")
    d_x, d_ph, d_sc = _t(c["enc"] if head else c["maps"], dev), _t(c["photos"], dev), _t(c["scenes"], dev)

    def off(t):
        flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
        view = flat[1:].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == 4
        return view

    for layout in wp.LAYOUTS:
        d_w = _t(c["weights"][layout], dev)
        loss, grad = native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w)
        for args in ((d_x, d_ph, d_sc, off(d_w)), (off(d_x), off(d_ph), off(d_sc), off(d_w))):
            l, g = native.photo_loss(args[0], args[1], args[2], EPS, head=head, weights=args[3])
            assert l.item() == loss.item() and torch.equal(g, grad)
    _scratch_is_zero(native)


@pytest.mark.parametrize("head", [False, True], ids=["maps", "head"])
def test_edge_forms_of_the_module(dev, native, head):
    c = wp.case_inputs("17_s1")                     # S = 1: [B,3,H,W] photos with [B,H,W] weights
    x, ph, sc, w = (c["enc"] if head else c["maps"]), c["photos"], c["scenes"], c["weights"]["shared"]
    d_x, d_ph, d_sc, d_w = _t(x, dev), _t(ph, dev), _t(sc, dev), _t(w, dev)
    fn = _module(head)
    ref_loss, ref_grad = native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w)
    leaf = d_x.clone().requires_grad_(True)
    n0 = native.launch_count()
    l = fn(leaf, d_ph[:, 0], d_sc, d_w[:, 0])
    l.backward()
    torch.cuda.synchronize()
    assert native.launch_count() - n0 == 1                                  # still ONE launch per step
    assert l.item() == ref_loss.item() and torch.equal(leaf.grad, ref_grad)
    # bool and uint8 masks
    mask = d_w > 0.5
    want, _ = native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=mask.float())
    with torch.no_grad():
        assert fn(d_x, d_ph, d_sc, mask).item() == want.item() == fn(d_x, d_ph, d_sc, mask.to(torch.uint8)).item()
    # normalize="weights" against float64: sum w|d| / (3 sum w)
    c9 = wp.case_inputs("45_s9")
    x9 = c9["enc"] if head else c9["maps"]
    for layout in wp.LAYOUTS:
        w9 = c9["weights"][layout]
        _, ref = wp.reference("45_s9", layout, head)
        full = photo_checks.broadcast_weights(w9, c9["S"]).astype(np.float64)
        want = ref.loss64 * full.size * 3 / (3.0 * full.sum())
        leaf = _t(x9, dev).requires_grad_(True)
        got = _module(head, "weights")(leaf, _t(c9["photos"], dev), _t(c9["scenes"], dev), _t(w9, dev))
        got.backward()
        tolerances.assert_loss_close(got.item(), want, "normalize=weights %s" % layout)
        scale = full.size / full.sum()
        photo_checks.assert_photo_grad_close(_np(leaf.grad), ref.grad * scale, ref.grad64 * scale, ref.tie,
                                             "normalize=weights %s grad" % layout)
        with torch.no_grad():
            zero = _module(head, "weights")(_t(x9, dev), _t(c9["photos"], dev), _t(c9["scenes"], dev), torch.zeros_like(_t(w9, dev)))
        assert zero.item() == 0.0
    _scratch_is_zero(native)


@pytest.mark.parametrize("head", [False, True], ids=["maps", "head"])
def test_float64_and_second_order_take_the_composed_definition(dev, native, head):
    c, ref = wp.reference("33_s3", "per-photo", head)
    x, w = (c["enc"] if head else c["maps"]), c["weights"]["per-photo"]
    spoiled = c["photos"].copy()
    spoiled[np.broadcast_to((w == 0)[:, :, None], spoiled.shape)] = np.nan          # excused in the composed paths too
    d_ph, d_sc, d_w = _t(spoiled, dev), _t(c["scenes"], dev), _t(w, dev)
    fn = _module(head)
    leaf = _t(x, dev).requires_grad_(True)
    fused = fn(leaf, d_ph, d_sc, d_w)
    fused.backward()
    x64 = _t(x, dev).double().requires_grad_(True)
    composed = fn(x64, d_ph, d_sc, d_w)
    assert composed.dtype == torch.float64
    composed.backward()
    assert torch.isfinite(x64.grad).all()
    tolerances.assert_loss_close(fused.item(), composed.item(), "fused vs float64 composed")
    photo_checks.assert_photo_grad_close(_np(leaf.grad), _np(x64.grad), ref.grad64, ref.tie, "weighted fused vs float64 composed")
    x2 = _t(x, dev).requires_grad_(True)
    g, = torch.autograd.grad(fn(x2, d_ph, d_sc, d_w), x2, create_graph=True)
    assert g.requires_grad and g.dtype == torch.float32 and torch.isfinite(g).all()
    photo_checks.assert_photo_grad_close(_np(g), _np(x64.grad), ref.grad64, ref.tie, "weighted create_graph vs float64 composed")
    g.square().sum().backward()
    assert x2.grad is not None and torch.isfinite(x2.grad).all() and x2.grad.abs().max() > 0


def test_weighted_is_faster_than_its_composition_and_within_the_byte_ratio_of_the_unweighted(dev, native):
    res = wp.measure_weighted_photo_loss(dev, native, "per-photo")
    bound = 60.0 / 51.0
    text = ("weighted photo loss %.2f us per launch, unweighted %.2f (ratio %.3f, bound %.3f), unfused weighted composition "
            "%.2f us per step (%.1fx); %.3f of 8 TB/s at the algorithmic bytes; per round %s" % (
                res["weighted_us"], res["unweighted_us"], res["weighted_us"] / res["unweighted_us"], bound,
                res["composition_us"], res["composition_us"] / res["weighted_us"], res["weighted_frac_of_8TBps"], res["rounds"]))
    print("[weighted-photo] config-2 shape, per-photo weights: " + text)
    out = os.environ.get("SVBRDF_RESULTS_DIR")
    with open(os.path.join(out, "weighted_photo_loss_speed.txt") if out else os.devnull, "w") as f:
        f.write("# tests/test_gpu_weighted_photo_loss.py speed test on %s\n%s\n" % (res["device"], text))
    assert res["weighted_us"] <= res["composition_us"], res
    assert res["weighted_us"] <= bound * res["unweighted_us"], res
