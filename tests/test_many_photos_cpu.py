"""The photo-loss family at many photos per item, without a GPU (tests/many_photos_checks.py has the cases and says which S
takes which path): the batched dual-number oracle against the loop it replaces, the conditions on the inputs of every
comparison tests/test_gpu_many_photos.py makes, the fixed-point exponent each case is chosen for, and the LDS budget of the
kernels that take dynamic LDS at the header's limits of S.
"""
import os

import numpy as np
import pytest

import many_photos_checks as mp
import pose_photo_checks as pc
import unit_build


@pytest.mark.parametrize("f64", (False, True), ids=("fp32", "fp64"))
def test_batched_dual_renderings_are_the_loop_bit_for_bit(f64):
    """torch.vmap over the rows and the nine unit tangents of torch.func.jvp against one eager dual-number render per (b, s,
    k), at S = 29, B = 2: the same bits of the renderings and of every derivative, so PoseReference may take either"""
    c = mp.case_inputs("s29")
    loop = pc.dual_renderings(c["maps"], c["scenes"], f64)
    batched = pc.dual_renderings(c["maps"], c["scenes"], f64, batched=True)
    assert loop[0] is not batched[0]                                  # two evaluations, not one cached
    for name, a, b in zip(("rad", "drad"), loop, batched):
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert np.array_equal(a.view(np.uint64 if a.dtype == np.float64 else np.uint32),
                              b.view(np.uint64 if b.dtype == np.float64 else np.uint32)), name
    assert np.isfinite(batched[1]).all() and batched[1].any(axis=(3, 4, 5)).all()


def test_pose_reference_of_an_existing_case_does_not_change_with_the_batched_form():
    import weighted_photo_checks as wp
    c = wp.case_inputs("17_s2")
    w = c["weights"]["per-photo"]
    a = pc.PoseReference(c["maps"], c["photos"], c["scenes"], pc.EPS, False, w)
    b = pc.PoseReference(c["maps"], c["photos"], c["scenes"], pc.EPS, False, w, batched=True)
    for key in ("G32", "G64", "A", "T", "bound"):
        assert np.array_equal(getattr(a, key), getattr(b, key)), key


@pytest.mark.parametrize("kind,name,layout,head", mp.USES, ids=["%s-%s" % (u[0], mp.what(*u[1:]).replace(" ", "-")) for u in mp.USES])
def test_inputs_meet_the_conditions(kind, name, layout, head):
    """by the oracle alone: at most MAX_TIE_PIXELS tie pixels, MAX_WIDENED_GRAD elements that need the 2|ref - f64| widening,
    8 tied terms, no sign flip -- caps, not measurements; and the fp32 oracle's own per-scene gradient is inside the bound
    the kernels are held to"""
    c, R = mp.reference(kind, name, layout, head)
    assert c["maps"].shape == (c["B"], 12, 17, 17) and c["photos"].shape == (c["B"], c["S"], 3, 17, 17)
    own = mp.assert_conditions(kind, R, mp.what(name, layout, head))[4]
    assert own is None or own < 1.0, own
    if kind == "exposure":
        assert R.G64.all() and (R.A > 0).all()                       # every scene has a gradient to get wrong
    if kind == "pose":
        assert R.G64.any(axis=2).all() and (R.A > 0).all()


def test_fixed_point_exponent_of_every_case():
    """plan_loss's rule, restated: k = 24 below S = 330 at 17 x 17 with B = 2, and 23 / 23 / 22 / 21 at S = 383 / 425 / 1278 /
    1706 (B = 1) -- and the source still states the rule that is restated here"""
    assert mp.rule_in_source(unit_build.read_csrc("svbrdf_host.h")) == mp.RULE
    text = unit_build.read_csrc("svbrdf_device.h")
    assert "constexpr int kLossSlots = %d;" % mp.LOSS_SLOTS in text and "constexpr int kLossThreads = %d;" % mp.LOSS_THREADS in text
    assert "constexpr int kLossCountShift = %d;" % mp.COUNT_SHIFT in text
    k = lambda B, S: mp.fixed_point_exponent(B, S, 17, 17)
    assert all(k(2, S) == 24 for S in range(1, 330)) and k(2, 330) == 23
    assert (k(2, 383), k(2, 425), k(2, 1278), k(1, 1706)) == (23, 23, 22, 21)
    for name, (S, B, _, _, _) in mp.CASES.items():
        assert k(B, S) == mp.EXPONENTS[name], name
    assert k(1, 1707) == mp.EXPONENTS["s1707_b1"] == 21
    # the speed shape of every photo test stays at 2^-24: none of them reaches the coarser scales
    assert mp.fixed_point_exponent(8, 9, 256, 256) == 24


BEYOND = sorted(mp.LOSS_BEYOND_RTOL, key=str)


@pytest.mark.parametrize("name,layout,head", BEYOND, ids=[mp.what(*k).replace(" ", "-") for k in BEYOND])
def test_sequential_float32_sum_of_the_oracles_terms_explains_the_loss_beyond_1e_6(name, layout, head):
    """The finding of tests/test_gpu_many_photos.py, from the oracle alone: the fp32 oracle's OWN terms, added as a thread of
    the kernels adds them (3 S float32 adds one after the other per pixel), give a loss as far from the exact sum of the same
    terms as the kernels' loss was measured from the oracle's -- within a quarter of the recorded figure -- while the terms
    themselves are good to 2e-8.  The error is inside the bound the GPU test holds these cases to, (3 S + 16) 2^-24 sum
    |term| / N, and that bound stays below 1e-3 of the loss."""
    import photo_checks
    c, R = mp.reference("exposure" if name == "s1278" else "photo", name, layout, head)
    ref = R.ref if name == "s1278" else R
    table = R.scaled if name == "s1278" else c["scenes"]
    w = None if layout is None else c["weights"][layout]
    loss32, _, d32 = photo_checks.oracle_photo_loss(ref.maps, c["photos"], table, mp.EPS, want_grad=False, weights=w)
    assert loss32 == ref.loss
    if w is not None:       # the kernels' weighted sum: w |term|, the same sequential adds
        d32 = d32 * photo_checks.broadcast_weights(w, c["S"])[:, :, None]
    got = mp.sequential_sum_loss(d32)
    err, recorded = abs(got - loss32) / loss32, mp.LOSS_BEYOND_RTOL[(name, layout, head)]
    bound = mp.sequential_sum_bound(ref.delta64, w, c["S"])
    print("[many-photos] %-32s sequential float32 sum of the oracle's terms: rel. error %.3e (kernels, recorded: %.2e); fp32 "
          "oracle vs fp64 %.3e; bound / loss %.3e" % (mp.what(name, layout, head), err, recorded,
                                                      abs(ref.loss - ref.loss64) / ref.loss64, bound / ref.loss64))
    assert abs(err - recorded) <= 0.25 * recorded, (err, recorded)
    assert abs(ref.loss - ref.loss64) <= 2e-8 * ref.loss64
    assert abs(got - ref.loss64) <= bound < 1e-3 * ref.loss64


def test_lds_budget_at_the_documented_limits(tmp_path):
    """static LDS of every kernel that is launched with dynamic LDS -- from the unit's device assembly, compiled with the
    Makefile's own flags -- plus the largest dynamic size its launcher accepts, 16 (spill + per_scene S_max) bytes at the
    header's limit of S, is at most 64 KiB: the budget the launchers' 60 * 1024 was chosen against.  (What the device itself
    allows is settled by the launches of tests/test_gpu_many_photos.py.)"""
    header = open(os.path.join(unit_build.ROOT, "include", "svbrdf_hip.h")).read()
    shared = unit_build.read_csrc("svbrdf_photo_loss_device.h", "svbrdf_photo_pose_device.h")
    assert "constexpr int kExpoSpill = 4;" in shared and "constexpr int kPoseSpill = 9;" in shared
    assert "kLdsMax = 60 * 1024" in shared
    rows = []
    for unit, (prefix, spill, per_scene, s_max) in mp.LDS_UNITS.items():
        assert "S <= %d" % s_max in header, (unit, s_max)
        dynamic = mp.largest_dynamic_lds(unit)
        extra = 6 * mp.LOSS_THREADS * 4 if s_max == 383 else 0         # the joint steps' launchers count their six stashed words
        assert dynamic + extra <= 60 * 1024 < mp.ROW_BYTES * (spill + per_scene * (s_max + 1)) + extra, unit
        kernels = {k: v for k, v in mp.static_lds(unit_build.compile_unit_asm(tmp_path, unit, "SCHED_PHOTO")).items()
                   if prefix in k}
        assert len(kernels) >= 2, (unit, kernels)
        for kernel, static in sorted(kernels.items()):
            rows.append((kernel, static, dynamic, static + dynamic))
    print("[many-photos] LDS at the header's limits of S: kernel, static, largest dynamic, sum (budget %d)" % mp.LDS_BUDGET)
    for row in rows:
        print("[many-photos]   %-64s %6d %6d %6d" % row)
    assert all(total <= mp.LDS_BUDGET for _, _, _, total in rows), [r for r in rows if r[3] > mp.LDS_BUDGET]
