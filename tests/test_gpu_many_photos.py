"""The photo-loss family on the device at MANY photos per item, up to the limits the header documents: every entry of
csrc/svbrdf_photo_{loss,exposure,pose,fit,fit_pose,fit_smooth}.hip at the S where its code takes another path than at the
S <= 9 of the other photo tests (tests/many_photos_checks.py lists them) and at its largest S -- where the launch needs up
to 128 bytes less than 64 KiB of LDS and plan_loss's fixed-point scale is 2^23, 2^22 or 2^21 instead of 2^24.

Every case is 17 x 17 (two workgroups; the second holds one partial wave and three waves without pixels), so a test is a
handful of launches on 578 pixels or fewer.  The tolerances are the project's own, through the helpers that keep the
ledger: photo_checks.Reference.assert_close (loss 1e-6 relative, tests/tolerances.py's gradient rule),
PoseReference.assert_scene_grad_close, ExposureReference.assert_exposure_grad_close.  ONE FINDING: in five head cases at S >=
425 the loss is 1.0e-6 to 2.0e-6 off, beyond 1e-6 -- a thread's sequential float32 sum of 3 S terms; those five, and no
other, are held to (3 S + 16) 2^-24 sum |term| / N instead (_assert_close below; many_photos_checks.LOSS_BEYOND_RTOL).  The conditions on the inputs are
asserted by the oracle alone at the top of every comparison (and in tests/test_many_photos_cpu.py).  Every call is made twice
on a scratch that nobody clears in between and must give the same bits; the whole scratch, accumulator words included,
must be zero afterwards; the per-scene gradients stand between guard words.

Measured on an MI355X: profiles/r24_many_photos.txt.
"""
import ctypes

import numpy as np
import pytest
import torch

import many_photos_checks as mp
import photo_checks
import photo_fit_checks as fc
import photo_fit_pose_checks as jc
import photo_fit_smooth_checks as sm
import photo_fit_steps_checks as st
import pose_photo_checks as pc
import tolerances
from photo_checks import assert_scratch_is_zero as _scratch_is_zero, to_device as _t, to_numpy as _np

pytestmark = pytest.mark.gpu
EPS = mp.EPS
H = mp.H
BAD_VALUES = (0.0, -1.0, np.nan, np.inf)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X (select CPU tests with -m 'not gpu')"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def native():
    from svbrdf_estimation_amd import _native
    _native._load()
    return _native


def _module(head):
    from svbrdf_estimation_amd import losses, renderers
    fn = (losses.HeadPhotoLoss if head else losses.PhotoLoss)(renderers.LocalRenderer())
    assert fn.uses_fused_kernel() and fn.eps == EPS
    return fn


def _ids(uses):
    return [mp.what(*u).replace(" ", "-") for u in uses]


def _same(a, b):
    return all((x is None and y is None) or fc.same_bits(x, y) for x, y in zip(a, b))


def _host(result):
    """a binding call's tensors -> numpy (the loss as a [1] array), None kept"""
    return tuple(None if t is None else _np(t).reshape(-1) if t.dim() <= 1 else _np(t) for t in result)


def _twice(native, call, label):
    """`call()` twice on the binding's scratch, which nobody clears in between: the same bits, and the whole scratch zero
    after each -> the first result as numpy"""
    first = _host(call())
    _scratch_is_zero(native)
    second = _host(call())
    _scratch_is_zero(native)
    assert _same(first, second), "%s: a second call on the same scratch gives other bits" % label
    return first


def _assert_close(ref, loss, grad, label, key, S, weights):
    """the loss and the map gradient against a photo_checks.Reference `ref`, by Reference.assert_close: the loss within
    LOSS_RTOL = 1e-6 of the fp32 oracle's, the gradient by tests/tolerances.py's rule.  The cases `key` = (case, layout, head)
    of many_photos_checks.LOSS_BEYOND_RTOL are the exception, and a finding: there the kernels' loss was measured beyond
    1e-6 (1.0e-6 to 2.0e-6; five head cases at S >= 425) because a thread adds its 3 S terms one after the other in float32
    -- the same sum of the ORACLE's terms on the CPU is off by as much (tests/test_many_photos_cpu.py).  Their loss is held to
    what such a sum can be off by, (3 S + 16) 2^-24 sum |term| / N against the float64 oracle, each use recorded in the
    ledger; their gradient by the same rule as ever.  include/svbrdf_hip.h says so beside the limits of S."""
    if key not in mp.LOSS_BEYOND_RTOL:
        return ref.assert_close(loss, grad, label)
    bound = mp.sequential_sum_bound(ref.delta64, weights, S)
    err = abs(float(loss) - ref.loss64)
    print("[many-photos] %-40s loss beyond 1e-6 (recorded %.2e): rel. error vs the fp32 oracle %.3e; error %.3e against the "
          "sequential-sum bound %.3e (ratio %.4f)" % (label, mp.LOSS_BEYOND_RTOL[key], abs(float(loss) - ref.loss) / abs(ref.loss),
                                                     err, bound, err / bound))
    tolerances._record(label + " loss", "beyond 1e-6: sum bound", 1, 1, 1)
    assert err <= bound, "%s loss: %r vs %r, error %.3e beyond (3 S + 16) 2^-24 sum|term| / N = %.3e" % (
        label, float(loss), ref.loss64, err, bound)
    return photo_checks.assert_photo_grad_close(grad, ref.grad, ref.grad64, ref.tie, label + (" grad9" if ref.head else " grad"))


def _loss_line(label, S, loss, ref, k):
    """the loss against the fp64 oracle, beside the fp32 oracle's own error and the sequential-sum bound"""
    rel = abs(float(loss) - ref.loss64) / abs(ref.loss64)
    own = abs(ref.loss - ref.loss64) / abs(ref.loss64)
    print("[many-photos] %-40s k = %d, loss %.9g, rel. error vs fp64 %.3e (fp32 oracle's own %.3e), tie pixels %d, widened %d" % (
        label, k, float(loss), rel, own, ref.n_ties(), ref.n_widened()))
    return rel


def test_device_reports_the_lds_the_limits_need(dev):
    """the launches below ask for nearly all of the 64 KiB of LDS per workgroup that tests/test_many_photos_cpu.py holds
    static + dynamic to (its table has the sums); what the device reports is recorded beside that budget"""
    per_block = torch.cuda.get_device_properties(dev).shared_memory_per_block
    print("[many-photos] %s: sharedMemPerBlock %d bytes; the budget static + dynamic LDS of every launch is held to: %d" % (
        torch.cuda.get_device_name(dev), per_block, mp.LDS_BUDGET))
    assert per_block >= mp.LDS_BUDGET


# ------------------------------------------------------------------------------------------------ a. the photo loss

PHOTO_USES = [u[1:] for u in mp.USES if u[0] == "photo" and u[1] not in ("s144", "s1707_b1")]


@pytest.mark.parametrize("name,layout,head", PHOTO_USES, ids=_ids(PHOTO_USES))
def test_photo_loss_against_the_oracle(dev, native, name, layout, head):
    """with the gradient: photo_checks.Reference's bounds; forward only (the table staged in LDS: a second trip of the
    staging loop from S = 29 on, 61,416 of its 61,440 bytes at S = 1706): the same loss bit for bit"""
    c, R = mp.reference("photo", name, layout, head)
    label = mp.what(name, layout, head)
    mp.assert_conditions("photo", R, label)
    d_x, d_ph, d_sc = _t(c["enc"] if head else c["maps"], dev), _t(c["photos"], dev), _t(c["scenes"], dev)
    d_w = None if layout is None else _t(c["weights"][layout], dev)
    loss, grad = _twice(native, lambda: native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w), label)
    _loss_line(label, c["S"], loss[0], R, mp.EXPONENTS[name])
    _assert_close(R, loss[0], grad, label, (name, layout, head), c["S"], None if layout is None else c["weights"][layout])
    fwd, none = _twice(native, lambda: native.photo_loss(d_x, d_ph, d_sc, EPS, want_grad=False, head=head, weights=d_w),
                       label + " forward only")
    assert none is None and fc.same_bits(fwd, loss), (label, fwd, loss)


@pytest.mark.parametrize("head", [False, True], ids=["maps", "head"])
def test_one_scene_beyond_the_forward_only_stage(dev, native, head):
    """S = 1707, B = 1: refused forward only ("too many scenes": the stage holds 1706 rows), accepted with the gradient,
    whose kernels read the table from memory -- as K3 (test_extreme_shapes_at_the_limits_of_the_abi)"""
    for layout in (None, "per-photo"):
        c, R = mp.reference("photo", "s1707_b1", layout, head)
        label = mp.what("s1707_b1", layout, head)
        mp.assert_conditions("photo", R, label)
        assert c["scenes"].shape == (1, 1707, 9)
        weights = None if layout is None else c["weights"][layout]
        d_x, d_ph, d_sc = _t(c["enc"] if head else c["maps"], dev), _t(c["photos"], dev), _t(c["scenes"], dev)
        d_w = None if weights is None else _t(weights, dev)
        loss, grad = _twice(native, lambda: native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w), label)
        _loss_line(label, 1707, loss[0], R, mp.EXPONENTS["s1707_b1"])
        _assert_close(R, loss[0], grad, label, ("s1707_b1", layout, head), 1707, weights)
        n0 = native.launch_count()
        with pytest.raises(native.NativeLibraryError, match="too many scenes"):
            native.photo_loss(d_x, d_ph, d_sc, EPS, want_grad=False, head=head, weights=d_w)
        assert native.launch_count() == n0
        _scratch_is_zero(native)


# ------------------------------------------------------------------------------------------------ b. the by-value table

@pytest.mark.parametrize("layout", [None, "per-photo"], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("head", [False, True], ids=["maps", "head"])
def test_by_value_table_at_its_capacity(dev, native, monkeypatch, head, layout):
    """B S = 288 rows ride in the launch's argument block (svbrdf_[head_]photo_loss[_weighted]_fwd_bwd_host_scenes): the
    device-table entry's loss and gradient bit for bit, inside the oracle's bounds"""
    c, R = mp.reference("photo", "s144", layout, head)
    label = mp.what("s144", layout, head)
    mp.assert_conditions("photo", R, label)
    assert c["B"] * c["S"] == native.host_scenes_max_rows() == 288
    d_x, d_ph, d_sc = _t(c["enc"] if head else c["maps"], dev), _t(c["photos"], dev), _t(c["scenes"], dev)
    d_w = None if layout is None else _t(c["weights"][layout], dev)
    table = torch.from_numpy(np.ascontiguousarray(c["scenes"]))
    device = _twice(native, lambda: native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w), label)

    def no_upload(*a, **k):
        raise AssertionError("288 rows travel by value")
    monkeypatch.setattr(native, "upload_scene_table", no_upload)
    entries = []
    real = native._call
    monkeypatch.setattr(native, "_call", lambda entry, *a, **k: (entries.append(entry), real(entry, *a, **k))[1])
    by_value = _twice(native, lambda: native.photo_loss(d_x, d_ph, table, EPS, head=head, weights=d_w), label + " by value")
    want = "svbrdf_%sphoto_loss%s_fwd_bwd_host_scenes" % ("head_" if head else "", "" if layout is None else "_weighted")
    assert entries == [want, want], entries
    assert _same(by_value, device), label
    _loss_line(label, 144, by_value[0][0], R, 24)
    R.assert_close(by_value[0][0], by_value[1], label + " by value")
    fwd = _twice(native, lambda: native.photo_loss(d_x, d_ph, table, EPS, want_grad=False, head=head, weights=d_w),
                 label + " by value, forward only")
    assert fc.same_bits(fwd[0], device[0])


# ------------------------------------------------------------------------------------------------ c. the exposure entries

EXPOSURE_USES = [u[1:] for u in mp.USES if u[0] == "exposure"]


@pytest.mark.parametrize("name,layout,head", EXPOSURE_USES, ids=_ids(EXPOSURE_USES))
def test_exposure_entries_against_the_oracle(dev, native, name, layout, head):
    """the pattern of test_gpu_exposure_photo_loss._run_all_ways: the C ABI with grad_exposure and without, a host table
    (uploaded), the module through backward(), and the direct call between guard words on a scratch of its own -- each
    inside the bounds, all the same bits.  3 S = 258 sums at S = 86: the scenes from 64 on are added in the second trip of
    the workgroup-sum loop.  61,408 bytes of dynamic LDS at S = 1278."""
    c, R = mp.reference("exposure", name, layout, head)
    label = mp.what(name, layout, head)
    mp.assert_conditions("exposure", R, label)
    x, w, e = (c["enc"] if head else c["maps"]), (None if layout is None else c["weights"][layout]), c["e"]
    d_x, d_ph, d_sc, d_e = _t(x, dev), _t(c["photos"], dev), _t(c["scenes"], dev), _t(e, dev)
    d_w = None if w is None else _t(w, dev)
    call = lambda **k: native.photo_loss(d_x, d_ph, k.pop("table", d_sc), EPS, head=head, weights=d_w, exposure=d_e, **k)
    results = {"C ABI": _twice(native, lambda: call(want_exposure_grad=True), label)}
    results["C ABI, grad_exposure = NULL"] = _twice(native, call, label + " without grad_exposure")
    results["C ABI, host table"] = _twice(native, lambda: call(table=torch.from_numpy(np.ascontiguousarray(c["scenes"])),
                                                                 want_exposure_grad=True), label + " host table")
    leaf, e_leaf = d_x.clone().requires_grad_(True), d_e.clone().requires_grad_(True)
    l = _module(head)(leaf, d_ph, d_sc, d_w, e_leaf)
    l.backward()
    results["module"] = (_np(l.detach()).reshape(1), _np(leaf.grad), _np(e_leaf.grad))
    _scratch_is_zero(native)
    direct = mp.abi_sums(native, dev, "exposure", c, layout, head)
    again = mp.abi_sums(native, dev, "exposure", c, layout, head, ws=direct["ws"])
    for out in (direct, again):
        assert out["guards_intact"] and out["scratch_zero"], (label, out["guards_intact"], out["scratch_zero"])
    results["direct call"] = (direct["loss"], direct["grad"], direct["sums"])
    results["direct call, second on its scratch"] = (again["loss"], again["grad"], again["sums"])
    first = results["C ABI"]
    _loss_line(label, c["S"], first[0][0], R.ref, mp.EXPONENTS[name])
    for how, (loss, grad, ge) in results.items():
        assert fc.same_bits(loss, first[0]) and fc.same_bits(grad, first[1]), "%s: %s: other bits than the first call" % (label, how)
        if ge is not None:
            assert fc.same_bits(ge, first[2]), "%s: %s: other exposure gradient bits" % (label, how)
    ge = first[2]
    print("[many-photos] %-40s grad_exposure worst err/bound %.3e, err/A %.3e; tied terms %d" % ((label,) + R.worst(ge) + (R.tied_terms,)))
    R.assert_exposure_grad_close(ge, label)
    if c["S"] > 64:
        err = np.abs(ge.astype(np.float64) - R.G64)[:, 64:]
        assert (err <= R.bound[:, 64:]).all() and ge[:, 64:].all(), label            # the second trip's scenes, by themselves
    _assert_close(R.ref, first[0][0], first[1], label, (name, layout, head), c["S"], w)
    assert np.isfinite(first[1]).all() and np.isfinite(ge).all() and ge.all()


@pytest.mark.parametrize("head", [False, True], ids=["maps", "head"])
def test_exposure_entry_is_the_weighted_entry_on_the_scaled_table(dev, native, head):
    """S = 86: loss and map gradient are bit for bit those of the (weighted) photo entry on the table whose colour columns
    were multiplied by the gains in float32"""
    c = mp.case_inputs("s86")
    d_x, d_ph, d_sc, d_e = _t(c["enc"] if head else c["maps"], dev), _t(c["photos"], dev), _t(c["scenes"], dev), _t(c["e"], dev)
    d_scaled = torch.cat((d_sc[..., :6], d_sc[..., 6:] * d_e), dim=-1).contiguous()
    assert np.array_equal(_np(d_scaled), mp.xp.scaled_table(c["scenes"], c["e"]))
    for layout in mp.LAYOUTS:
        d_w = None if layout is None else _t(c["weights"][layout], dev)
        label = mp.what("s86", layout, head)
        scaled = _twice(native, lambda: native.photo_loss(d_x, d_ph, d_scaled, EPS, head=head, weights=d_w), label + " scaled table")
        got = _twice(native, lambda: native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w, exposure=d_e,
                                                       want_exposure_grad=True), label)
        assert _same(got[:2], scaled), label
        ones = _twice(native, lambda: native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w, exposure=torch.ones_like(d_e),
                                                        want_exposure_grad=True), label + " unit gains")
        plain = _twice(native, lambda: native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w), label + " plain")
        assert _same(ones[:2], plain) and np.isfinite(ones[2]).all(), label


@pytest.mark.parametrize("head", [False, True], ids=["maps", "head"])
def test_bad_gain_in_a_late_scene(dev, native, head):
    """S = 22: e[0, 21, 1] is word 64 of the item's gains, the first of the check loop's second trip.  0, -1, NaN and +inf
    there, or in e[1, 21, 2], give a NaN loss and an all-NaN grad_exposure -- with weights, without, and with all-zero
    weights: a weight does not excuse a gain --, the scratch is zero after each and the next good call gives the earlier
    bits"""
    c, R = mp.reference("exposure", "s22", "per-photo", head)
    mp.assert_conditions("exposure", R, mp.what("s22", "per-photo", head))
    d_x, d_ph, d_sc, d_e = _t(c["enc"] if head else c["maps"], dev), _t(c["photos"], dev), _t(c["scenes"], dev), _t(c["e"], dev)
    d_w = _t(c["weights"]["per-photo"], dev)
    good = _twice(native, lambda: native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w, exposure=d_e,
                                                    want_exposure_grad=True), "s22 good")
    assert np.ravel_multi_index((21, 1), (22, 3)) == 64
    for value in BAD_VALUES:
        for where in ((0, 21, 1), (1, 21, 2)):
            for weights in (d_w, None, torch.zeros_like(d_w)):
                bad = c["e"].copy()
                bad[where] = value
                loss, grad, ge = native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=weights, exposure=_t(bad, dev),
                                                   want_exposure_grad=True)
                assert np.isnan(loss.item()) and torch.isnan(ge).all() and ge.shape == (2, 22, 3), (value, where)
                _scratch_is_zero(native)
    again = _host(native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w, exposure=d_e, want_exposure_grad=True))
    assert _same(again, good)
    R.assert_exposure_grad_close(again[2], "s22 after the bad gains")


# ------------------------------------------------------------------------------------------------ d. the scene gradient

POSE_USES = [u[1:] for u in mp.USES if u[0] == "pose" and u[1] != "s383"]


def _pose_all_ways(native, dev, name, layout, head):
    """the C ABI twice, the module, the direct call between guard words on a scratch of its own, twice: loss and map
    gradient the plain entry's bits, grad_scenes inside PoseReference's bound and the same bits every way"""
    c, R = mp.reference("pose", name, layout, head)
    label = mp.what(name, layout, head)
    mp.assert_conditions("pose", R, label)
    x, w = (c["enc"] if head else c["maps"]), (None if layout is None else c["weights"][layout])
    d_x, d_ph, d_sc = _t(x, dev), _t(c["photos"], dev), _t(c["scenes"], dev)
    d_w = None if w is None else _t(w, dev)
    plain = _twice(native, lambda: native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w), label + " plain")
    results = {"C ABI": _twice(native, lambda: native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w, want_scene_grad=True), label)}
    leaf, t_leaf = d_x.clone().requires_grad_(True), d_sc.clone().requires_grad_(True)
    l = _module(head)(leaf, d_ph, t_leaf, d_w)
    l.backward()
    results["module"] = (_np(l.detach()).reshape(1), _np(leaf.grad), _np(t_leaf.grad))
    _scratch_is_zero(native)
    direct = mp.abi_sums(native, dev, "pose", c, layout, head)
    again = mp.abi_sums(native, dev, "pose", c, layout, head, ws=direct["ws"])
    for out in (direct, again):
        assert out["guards_intact"] and out["scratch_zero"], (label, out["guards_intact"], out["scratch_zero"])
    results["direct call"] = (direct["loss"], direct["grad"], direct["sums"])
    results["direct call, second on its scratch"] = (again["loss"], again["grad"], again["sums"])
    first = results["C ABI"]
    assert _same(first[:2], plain), "%s: loss or map gradient differ from the entry without the scene gradient" % label
    for how, res in results.items():
        assert _same(res, first), "%s: %s: other bits than the first call" % (label, how)
    _loss_line(label, c["S"], first[0][0], R.ref, mp.EXPONENTS[name])
    print("[many-photos] %-40s grad_scenes worst err/bound %.3e, err/A %.3e; tied terms %d" % ((label,) + R.worst(first[2]) + (R.tied_terms,)))
    R.assert_scene_grad_close(first[2], label)
    _assert_close(R.ref, first[0][0], first[1], label, (name, layout, head), c["S"], w)
    assert np.isfinite(first[1]).all() and first[2].all()
    return c, R, first


@pytest.mark.parametrize("name,layout,head", POSE_USES, ids=_ids(POSE_USES))
def test_scene_gradient_entries_against_the_oracle(dev, native, name, layout, head):
    """9 S = 261 sums at S = 29: the second trip of the workgroup-sum loop; the three-lobe loop at the untied S = 29; 61,344
    bytes of dynamic LDS at S = 425"""
    _pose_all_ways(native, dev, name, layout, head)


@pytest.mark.parametrize("head", [False, True], ids=["maps", "head"])
def test_bad_colour_in_a_late_scene(dev, native, head):
    """S = 22: the colours of scene 21 are words 63..65 of the item's 3 S, the last of the check loop's first trip and the
    first two of its second.  0, -1, NaN and +inf in scenes[0, 21, 7] or scenes[1, 21, 8] give a NaN loss and an all-NaN
    grad_scenes of all B S 9 entries, whatever the weights; nothing sticks"""
    c, R = mp.reference("pose", "s22", "per-photo", head)
    mp.assert_conditions("pose", R, mp.what("s22", "per-photo", head))
    d_x, d_ph, d_sc = _t(c["enc"] if head else c["maps"], dev), _t(c["photos"], dev), _t(c["scenes"], dev)
    d_w = _t(c["weights"]["per-photo"], dev)
    good = _twice(native, lambda: native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w, want_scene_grad=True), "s22 good")
    for value in BAD_VALUES:
        for where in ((0, 21, 7), (1, 21, 8)):
            for weights in (d_w, None, torch.zeros_like(d_w)):
                bad = c["scenes"].copy()
                bad[where] = value
                loss, grad, gs = native.photo_loss(d_x, d_ph, _t(bad, dev), EPS, head=head, weights=weights, want_scene_grad=True)
                assert np.isnan(loss.item()) and torch.isnan(gs).all() and gs.shape == (2, 22, 9), (value, where)
                _scratch_is_zero(native)
    again = _host(native.photo_loss(d_x, d_ph, d_sc, EPS, head=head, weights=d_w, want_scene_grad=True))
    assert _same(again, good)
    R.assert_scene_grad_close(again[2], "s22 after the bad colours")


@pytest.mark.parametrize("head", [False, True], ids=["maps", "head"])
def test_nan_in_the_maps_at_the_scene_gradient_limit(dev, native, head):
    """S = 425: one NaN map value gives a NaN loss and all 2 * 425 * 9 entries of grad_scenes NaN; the scratch -- 7,650
    accumulator words behind the 65 -- is zero afterwards and the next call is right"""
    c, R = mp.reference("pose", "s425", "shared", head)
    mp.assert_conditions("pose", R, mp.what("s425", "shared", head))
    x = c["enc"] if head else c["maps"]
    d_ph, d_sc, d_w = _t(c["photos"], dev), _t(c["scenes"], dev), _t(c["weights"]["shared"], dev)
    bad = x.copy()
    bad[1, 1, 11, 7] = np.nan
    assert c["weights"]["shared"][1, 0, 11, 7] >= 0.0               # (a weight does not excuse the maps: zero or not)
    for weights in (d_w, None):
        loss, grad, gs = native.photo_loss(_t(bad, dev), d_ph, d_sc, EPS, head=head, weights=weights, want_scene_grad=True)
        assert np.isnan(loss.item()) and torch.isnan(gs).all() and gs.shape == (2, 425, 9)
        _scratch_is_zero(native)
    loss, grad, gs = _host(native.photo_loss(_t(x, dev), d_ph, d_sc, EPS, head=head, weights=d_w, want_scene_grad=True))
    R.assert_scene_grad_close(gs, "s425 behind a NaN call")
    R.ref.assert_close(loss[0], grad, "s425 behind a NaN call")
    _scratch_is_zero(native)


def test_wave_sum_limit_in_a_late_scene(dev, native):
    """pose_photo_checks.overflow_case's construction in scene 28 of the S = 29 case: the camera of item 0 stands 1e-9 above
    pixel (3, 5), whose finite camera terms carry its wave's sum of N |term| some 700 times beyond 2^19 while every other
    (item, scene) stays 800 times below it (by the oracle's float64 values).  The workgroup-sum loop's first trip ends in
    the middle of this scene's nine sums (252..260 of item 0).  Reported as NaN, the map gradient's bits stay what they
    are, the scratch is zero and the next call is clean."""
    c, R = mp.reference("pose", "s29", None, False)
    mp.assert_conditions("pose", R, mp.what("s29", None, False))
    xrow = mp.c_oracle.make_xrow(H).astype(np.float32)
    sc = c["scenes"].copy()
    sc[0, 28, 0:3] = (xrow[5], -xrow[3], np.float32(1e-9))
    t64, delta = pc.pose_terms(c["maps"], c["photos"], sc, None, True, batched=True)
    loss64 = photo_checks.oracle_photo_loss(c["maps"], c["photos"], sc, EPS, f64=True, want_grad=False)[0]
    per_pixel = float(delta.size) * t64.sum(axis=3).reshape(2, 29, 9, H * H)                      # N t, channels summed
    waves = np.pad(per_pixel, ((0, 0), (0, 0), (0, 0), (0, (-H * H) % 64))).reshape(2, 29, 9, -1, 64).sum(axis=-1)
    worst = np.abs(waves[:, :, 0:3]).max(axis=(2, 3))
    assert np.isfinite(loss64) and worst[0, 28] > 16 * pc.WAVE_LIMIT and np.delete(worst.reshape(-1), 28).max() < pc.WAVE_LIMIT / 16
    d_x, d_ph, d_sc = _t(c["maps"], dev), _t(c["photos"], dev), _t(sc, dev)
    plain_loss, plain_grad = native.photo_loss(d_x, d_ph, d_sc, EPS)
    tolerances.assert_loss_close(plain_loss.item(), loss64, "the loss itself is finite", rtol=1e-4)
    for weights in (None, torch.ones((2, 1, H, H), device=dev)):
        loss, grad, gs = native.photo_loss(d_x, d_ph, d_sc, EPS, weights=weights, want_scene_grad=True)
        assert np.isnan(loss.item()) and torch.isnan(gs).all(), (loss.item(), gs)
        assert torch.equal(grad.view(torch.int32), plain_grad.view(torch.int32))
        _scratch_is_zero(native)
    loss, grad, gs = _host(native.photo_loss(d_x, d_ph, _t(c["scenes"], dev), EPS, want_scene_grad=True))
    R.assert_scene_grad_close(gs, "s29 after the overflow report")
    _scratch_is_zero(native)


# ------------------------------------------------------------------------------------------------ e. the joint fit steps

def _assert_clean(out, label):
    assert out["launches"] == 1 and out["scratch_zero"] and out["canaries_intact"] and out["inputs_intact"], (
        label, {k: out[k] for k in ("launches", "scratch_zero", "canaries_intact", "inputs_intact")})


def _assert_keys_same(a, b, keys, label):
    for key in keys:
        assert fc.same_bits(a[key], b[key]), "%s: %s differs in %d values" % (label, key, fc.count_differing(a[key], b[key]))


@pytest.mark.parametrize("layout", [None, "per-photo"], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("name", ["s29", "s383"])
def test_joint_fit_steps_at_many_photos(dev, native, name, layout):
    """svbrdf_photo_fit_adam_step_scene_grad and svbrdf_photo_fit_smooth_adam_step_scene_grad (some lambda > 0, and all
    zero): loss_out, grad_out and grad_scenes are the scene-gradient entry's bits -- which at S = 383 is held to
    PoseReference here --, maps', m', v' the plain fit step's (with lambda: the smooth restatement's).  55,296 bytes of
    dynamic LDS at S = 383, on top of 9,248 / 10,112 static.  Each call twice on its scratch."""
    lib = native._load()
    label = mp.what(name, layout, False)
    c = mp.fit_case(name, layout, 7400 + mp.CASES[name][0])
    ref_loss, ref_grad, ref_gs = jc.abi_scene_grad(native, dev, c)
    assert np.isfinite(ref_loss).all() and np.isfinite(ref_gs).all() and ref_gs.all()
    if name == "s383":
        _, R = mp.reference("pose", name, layout, False)
        mp.assert_conditions("pose", R, label)
        _loss_line(label, 383, ref_loss[0], R.ref, mp.EXPONENTS[name])
        print("[many-photos] %-40s grad_scenes worst err/bound %.3e, err/A %.3e; tied terms %d" % ((label,) + R.worst(ref_gs) + (R.tied_terms,)))
        R.assert_scene_grad_close(ref_gs, label)
        R.ref.assert_close(ref_loss[0], ref_grad, label)
    plain = fc.abi_fit(native, dev, c, bounds=fc.BOUNDS_FIT)
    _assert_clean(plain, label + " plain step")
    assert fc.same_bits(plain["loss"], ref_loss) and fc.same_bits(plain["grad"], ref_grad)
    want = fc.expected_step(lib, c, ref_grad, bounds=fc.BOUNDS_FIT)
    ws = jc.scratch(lib, dev, c)
    joint = jc.abi_joint(native, dev, c, bounds=fc.BOUNDS_FIT, ws=ws)
    again = jc.abi_joint(native, dev, c, bounds=fc.BOUNDS_FIT, ws=ws)
    for out in (joint, again):
        _assert_clean(out, label + " joint")
        assert fc.same_bits(out["loss"], ref_loss) and fc.same_bits(out["grad"], ref_grad) and fc.same_bits(out["grad_scenes"], ref_gs), label
        _assert_keys_same(out, plain, ("x", "m", "v"), label + " joint vs the plain step")
        for key, exp in zip(("x", "m", "v"), want):
            assert fc.same_bits(out[key], exp), (label, key)
    assert not fc.same_bits(joint["x"], c["maps"])
    zero = sm.abi_smooth(native, dev, c, np.zeros(12, np.float32), joint=True, bounds=fc.BOUNDS_FIT, ws=ws)
    _assert_clean(zero, label + " smooth joint, all-zero lambda")
    _assert_keys_same(zero, joint, ("x", "m", "v", "loss", "grad", "grad_scenes"), label + " all-zero lambda")
    g2, *smooth_want = sm.expected_step(lib, c, ref_grad, sm.LAMBDA, bounds=fc.BOUNDS_FIT)
    assert not fc.same_bits(g2, ref_grad)
    for _ in range(2):
        out = sm.abi_smooth(native, dev, c, sm.LAMBDA, joint=True, bounds=fc.BOUNDS_FIT, ws=ws)
        _assert_clean(out, label + " smooth joint")
        assert fc.same_bits(out["loss"], ref_loss) and fc.same_bits(out["grad_scenes"], ref_gs), label
        assert fc.same_bits(out["grad"], g2), fc.count_differing(out["grad"], g2)
        for key, exp in zip(("x", "m", "v"), smooth_want):
            assert fc.same_bits(out[key], exp), (label, key)


def test_joint_fit_steps_refuse_one_scene_more(dev, native):
    """S = 384: both joint steps are refused before any launch (SVBRDF_ERR_DIMS, "max 383") and no buffer is touched"""
    lib = native._load()
    B, S = 2, 384
    c = mp.case_inputs("s383")
    G = lambda a: fc.Guarded(a, dev)
    x, xo, m, v = G(c["maps"]), G(np.full_like(c["maps"], 3.0)), G(np.full_like(c["maps"], 0.25)), G(np.full_like(c["maps"], 0.5))
    ph, sc = G(np.zeros((B, S, 3, H, H), np.float32)), G(np.ones((B, S, 9), np.float32))
    loss, grad, gs = G(np.full(1, -1.0, np.float32)), G(np.full_like(c["maps"], 7.0)), G(np.full((B, S, 9), 7.0, np.float32))
    ws = torch.zeros(getattr(lib, jc.WORKSPACE_BYTES)(B, S, H, H) // 8, dtype=torch.int64, device=dev)
    keep, sptr = sm.smooth_array(sm.LAMBDA)
    f, stream = ctypes.c_float, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    adam = (None, f(fc.LR), f(fc.BETA1), f(fc.BETA2), f(fc.ADAM_EPS), 2)
    tail = (loss.ptr(), grad.ptr(), gs.ptr(), ws.data_ptr(), ws.numel() * 8, B, S, H, H, stream)
    before = lib.svbrdf_debug_launch_count()
    rc = getattr(lib, jc.JOINT_ENTRY)(x.ptr(), m.ptr(), v.ptr(), ph.ptr(), None, 0, sc.ptr(), native.xrow(dev, H).data_ptr(),
                                      f(EPS), *adam, *tail)
    assert rc == -2 and b"max 383" in lib.svbrdf_last_error(), (rc, lib.svbrdf_last_error())
    rc = getattr(lib, sm.JOINT_ENTRY)(x.ptr(), xo.ptr(), m.ptr(), v.ptr(), ph.ptr(), None, 0, sc.ptr(),
                                      native.xrow(dev, H).data_ptr(), f(EPS), sptr, *adam, *tail)
    assert rc == -2 and b"max 383" in lib.svbrdf_last_error(), (rc, lib.svbrdf_last_error())
    torch.cuda.synchronize(dev)
    del keep
    assert lib.svbrdf_debug_launch_count() == before and not ws.any().item()
    for buf, value in ((x, c["maps"]), (xo, 3.0), (m, 0.25), (v, 0.5), (loss, -1.0), (grad, 7.0), (gs, 7.0), (ph, 0.0), (sc, 1.0)):
        got, intact = buf.get()
        assert intact and np.array_equal(got, np.broadcast_to(np.asarray(value, np.float32), got.shape))


# ------------------------------------------------------------------------------------------------ f. the steps without the scene gradient

@pytest.mark.parametrize("layout", [None, "shared"], ids=["unweighted", "shared"])
def test_fit_steps_without_the_scene_gradient(dev, native, layout):
    """S = 29 through the existing helpers (S changes no path there): the single step against photo_fit_checks'
    restatement, n_steps = 3 against the sequential run, the smooth step against its restatement on the twin's gradient"""
    lib = native._load()
    label = mp.what("s29", layout, False)
    c = mp.fit_case("s29", layout, 7429)
    ref_loss, ref_grad = fc.abi_loss(native, dev, c)
    ws = torch.zeros(65, dtype=torch.int64, device=dev)
    for _ in range(2):
        out = fc.abi_fit(native, dev, c, bounds=fc.BOUNDS_FIT, ws=ws)
        _assert_clean(out, label)
        assert fc.same_bits(out["loss"], ref_loss) and fc.same_bits(out["grad"], ref_grad), label
        for key, exp in zip(("x", "m", "v"), fc.expected_step(lib, c, ref_grad, bounds=fc.BOUNDS_FIT)):
            assert fc.same_bits(out[key], exp), (label, key)
    states = st.sequential(native, dev, c, 3, bounds=fc.BOUNDS_FIT)
    run = st.abi_steps(native, dev, c, 3, bounds=fc.BOUNDS_FIT)
    st.assert_clean(run, label + " three steps")
    st.assert_same_run(run, states, 3, label + " three steps")
    g2, *want = sm.expected_step(lib, c, ref_grad, sm.LAMBDA, bounds=fc.BOUNDS_FIT)
    for _ in range(2):
        out = sm.abi_smooth(native, dev, c, sm.LAMBDA, bounds=fc.BOUNDS_FIT, ws=ws)
        _assert_clean(out, label + " smooth step")
        assert fc.same_bits(out["loss"], ref_loss) and fc.same_bits(out["grad"], g2), label
        for key, exp in zip(("x", "m", "v"), want):
            assert fc.same_bits(out[key], exp), (label, key)
