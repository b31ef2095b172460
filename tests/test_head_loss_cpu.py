"""The head-fused loss (svbrdf_head_loss_fwd_bwd*, losses.FusedHeadLoss), everything that needs no GPU -- what the
comparison values of tests/test_gpu_head_loss.py rest on:

  * tests/golden/g19_head_loss_edges.npz -- written by the reference (tests/golden/make_golden_head.py: its head decode, its
    MixedLoss / RenderingLoss, its autograd) at B = 3, H = 13 with tanh-distributed and saturated encoded values -- against
    the oracle's head_decode and head_loss, with the bounds tests/test_oracle_golden.py uses for g11;
  * the oracle's float64 head_loss against an independent definition, torch float64 autograd of losses.decode_head and
    oracle/eager_torch.py, for every input generator of tests/head_checks.py: to 1e-9 of max|gradient|, the sub-gradients at
    sign(0) and at the clamps included;
  * the inputs of every GPU case stay inside the caps BY THE ORACLE ALONE: at most 48 tie pixels, at most MAX_WIDENED_GRAD
    elements (tie pixels excluded) where the fp32 oracle itself is outside the strict bound against the fp64 oracle.  This is
    what licenses those caps on the GPU; a case that breaks one here gets other inputs, never a larger cap;
  * the 9-channel tie allowance of tests/head_checks.py is a bound: nudging a tie pixel's diffuse value by one float32 step,
    so that a tied term takes a sign, moves no gradient element by more than the allowance plus the strict bound.
"""
import json
import os

import numpy as np
import pytest

import head_checks as hc
import synth
import tolerances
from tolerances import assert_grad_close, assert_loss_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = "g19_head_loss_edges.npz"


@pytest.fixture(scope="module")
def g19(golden):
    return golden(FIXTURE)


def test_fixture_is_what_the_issue_describes(g19):
    g = g19
    B, H = int(g["B"]), int(g["H"])
    assert (B, H) == (3, 13) and (H * H) % 4 == 1            # items 1 and 2 start 4 and 8 bytes off 16-byte alignment
    enc = g["enc9"]
    assert enc.dtype == np.float32 and enc.shape == (B, 9, H, H) and g["target"].shape == (B, 12, H, H)
    assert g["scenes"].shape == (B, 9, 9) and g["mixed_grad9"].shape == enc.shape and g["render_grad9"].shape == enc.shape
    # regenerated from tests/synth.py here (one float64 tanh on top of it: checked, not assumed)
    assert np.array_equal(hc.fixture_input(int(g["enc_seed"]), B, H), enc) and synth.checksum(enc) == str(g["enc_sha256"])
    tgt = synth.make_maps(int(g["target_seed"]), B, H)
    assert np.array_equal(tgt, g["target"]) and synth.checksum(tgt) == str(g["target_sha256"])
    assert np.abs(enc).max() == 1.0
    for k, name in enumerate(("normal", "diffuse", "roughness", "specular")):     # one group at a time, a whole image row
        assert (enc[:, hc.GROUPS[name], 2 * k] == -1.0).all() and (enc[:, hc.GROUPS[name], 2 * k + 1] == 1.0).all()
        others = np.delete(enc[:, :, 2 * k:2 * k + 2], np.r_[hc.GROUPS[name]], axis=1)
        assert (np.abs(others) < 1.0).any()
    free = enc[:, :, 8:]
    assert ((free == 1.0) | (free == -1.0)).any(), "tanh(4 z) reaches exactly +-1 in float32 at this size"
    dec = g["decoded12"]
    assert (dec[:, 3:6, 2] == 0.0).all() and (dec[:, 3:6, 3] == 1.0).all() and (dec[:, 6:9, 4] == 0.0).all()
    assert np.allclose(np.abs(dec[:, 0:2, 0:2]), 3.0 / np.sqrt(19.0), rtol=1e-6)
    gdir = os.path.join(ROOT, "tests", "golden")
    assert os.path.getsize(os.path.join(gdir, FIXTURE)) <= os.path.getsize(os.path.join(gdir, "g11_head_loss.npz"))
    with open(os.path.join(gdir, "MANIFEST.json")) as f:
        entry = json.load(f)["fixtures"][FIXTURE]
    assert entry["generator"] == "tests/golden/make_golden_head.py"
    assert entry["sha256"] == synth.checksum(np.fromfile(os.path.join(gdir, FIXTURE), np.uint8))


def test_oracle_against_the_reference_fixture(oracle, g19):
    """head_decode, and head_loss in fp32 and fp64 at l1_weight 0.1 and 0: the bounds of
    tests/test_oracle_golden.py::test_head_decode_and_head_loss.  The fixture has tie pixels (a saturated input renders
    exactly as dark as the target where the light is behind both): counted, capped and bounded by the 9-channel allowance."""
    g = g19
    np.testing.assert_allclose(oracle.head_decode(g["enc9"]), g["decoded12"], rtol=3e-7, atol=1e-7)
    tie, allow = hc.allowance9(g["enc9"], g["target"], g["scenes"])
    for tag, w in (("mixed", 0.1), ("render", 0.0)):
        loss, grad = oracle.head_loss(g["enc9"], g["target"], g["scenes"], w)
        loss64, g64 = oracle.head_loss(g["enc9"], g["target"], g["scenes"], w, f64=True)
        print("[head-loss] g19 %s: reference %.9g, oracle fp32 %.9g, fp64 %.12g" % (tag, float(g[tag + "_loss"]), loss, loss64))
        assert_loss_close(loss, g[tag + "_loss"], tag)
        assert_loss_close(loss64, g[tag + "_loss"], tag + " fp64")
        assert_grad_close(grad, g[tag + "_grad9"], "g19 %s grad9 oracle vs reference" % tag, f64=g64, tie_map=tie,
                          tie_allowance=allow, max_ties=hc.MAX_TIES)
        # the double evaluation against the reference's float32 gradient: no widening by the reference's own error to lean on
        assert_grad_close(g64, g[tag + "_grad9"], "g19 %s grad9 oracle fp64 vs reference" % tag, tie_map=tie,
                          tie_allowance=allow, max_ties=hc.MAX_TIES)


@pytest.mark.parametrize("l1_weight", [0.1, 0.0])
@pytest.mark.parametrize("gen", sorted(hc.GENERATORS))
def test_oracle_fp64_against_torch_float64_autograd(oracle, gen, l1_weight):
    """B = 2, H = 7.  Saturated channels put sign(0) (a diffuse value of exactly 0 on both sides is not needed: the light
    behind the surface is enough) and the roughness clamp's mask into the gradient; both sides take PyTorch's
    sub-gradients there (sign(0) = 0; the clamp passes the gradient at the bound and above), so they agree everywhere."""
    B, H = 2, 7
    enc = hc.GENERATORS[gen](8100, B, H)
    tgt = synth.make_maps(8101, B, H, tiled_roughness=(gen != "full"))
    sc = hc.scene_table(81, B, 2, 3)
    for kw in (dict(l1_weight=l1_weight), dict(l1_weight=l1_weight and 0.35, eps=0.02, eps_l1=0.05)):
        loss, grad = oracle.head_loss(enc, tgt, sc, f64=True, **kw)
        t_loss, t_grad = hc.torch_head_loss(enc, tgt, sc, **kw)
        scale = np.abs(t_grad).max()
        print("[head-loss] %s %s: loss %.15g vs torch %.15g, gradient off by %.2e of max" % (
            gen, kw, loss, t_loss, np.abs(grad - t_grad).max() / scale))
        assert abs(loss - t_loss) <= 1e-12 * abs(t_loss)
        assert np.abs(grad - t_grad).max() <= 1e-9 * scale
    if gen == "roughness-1":        # the clamp's mask: a roughness of exactly 0 has no gradient, in the rendering loss and in all
        hit = enc[:, 5] == -1.0
        _, g0 = oracle.head_loss(enc, tgt, sc, 0.0, f64=True)
        assert hit.any() and not g0[:, 5][hit].any() and g0[:, 5][~hit].any()


# ---------------------------------------------------------------------------------------------- the GPU cases' caps

def _gpu_cases():
    for c in hc.sweep_cases():
        yield hc.sweep_name(c), (lambda c=c: hc.sweep_inputs(c)), dict(l1_weight=c["l1_weight"]), None
    for name, B, H, *_ in hc.POW2_CASES:
        # the tie cap scales as tolerances.assert_loss_at_size does; the widening cap does not
        yield "pow2 " + name, (lambda n=name: hc.pow2_inputs(n)), {}, max(hc.MAX_TIES, int(2e-6 * B * 9 * 3 * H * H))
    for H in (16, 13):
        yield "alignment H=%d" % H, (lambda H=H: hc.alignment_inputs(H)), {}, None
    for e, w, e1 in hc.ARGUMENT_TRIPLES:
        yield "arguments (%g, %g, %g)" % (e, w, e1), hc.argument_inputs, dict(eps=e, l1_weight=w, eps_l1=e1), None
        yield ("arguments (%g, %g, %g) module table" % (e, w, e1),
               lambda: hc.argument_inputs()[:2] + (hc.module_scene_table(2).numpy(),), dict(eps=e, l1_weight=w, eps_l1=e1), None)


_CASES = list(_gpu_cases())


def test_the_sweep_is_what_the_issue_describes():
    cases = hc.sweep_cases()
    assert len(cases) == 24 and {c["gen"] for c in cases} == set(hc.GENERATORS)
    assert all(1 <= c["B"] <= 5 and c["H"] in hc.SWEEP_SIZES and c["n_random"] + c["n_specular"] >= 1 for c in cases)
    assert hc.SWEEP_SIZES == (1, 2, 3, 5, 7, 8, 13, 16, 17, 31, 32, 33, 45)
    assert {c["H"] for c in cases} == set(hc.SWEEP_SIZES), "every size the issue names runs"
    assert {1, 2, 5} <= {c["B"] for c in cases}
    assert all(c["H"] <= 16 and c["B"] <= 2 for c in cases if c["gen"] in hc.SMALL_ONLY)
    # the generators with many exact ties run at the largest planes they may, each at both, and once with an item off alignment
    for gen in hc.SMALL_ONLY:
        assert {c["H"] for c in cases if c["gen"] == gen} == {13, 16}, gen
        assert any(c["B"] == 2 and c["H"] == 13 for c in cases if c["gen"] == gen), gen
    for key, n in (("tied", 2), ("host_table", 2), ("l1_weight", 2)):
        assert len({c[key] for c in cases}) == n, key
    assert [c["host_table"] for c in cases] == [bool(t % 2) for t in range(24)]
    # the sizes at the ends, and a power-of-two and an odd plane of more than one workgroup, run with both table forms
    for H in (1, 45, 33, 32, 17):
        assert {c["host_table"] for c in cases if c["H"] == H} == {False, True}, H
    # an odd plane with B > 1 (items off 16-byte alignment) at the largest sizes, and the one-pixel plane with B > 1
    for H in (1, 33, 45):
        assert any(c["B"] > 1 for c in cases if c["H"] == H), H


@pytest.mark.parametrize("case", _CASES, ids=[c[0].split(" (")[0].replace(" ", "_") for c in _CASES])
def test_gpu_case_inputs_stay_inside_the_caps(oracle, case):
    what, inputs, kw, tie_cap = case
    oracle.set_threads(min(16, oracle.max_threads()))
    ref = hc.Reference(*inputs(), **kw)
    n_ties, n_widened = ref.n_ties(), ref.n_widened()
    tolerances._record(what + " [oracle]", "tie pixels", n_ties, ref.tie.size, tie_cap or hc.MAX_TIES)
    tolerances._record(what + " [oracle]", "widened by 2|ref-f64|", n_widened, ref.grad.size, tolerances.MAX_WIDENED_GRAD)
    assert n_ties <= (tie_cap or hc.MAX_TIES) and n_widened <= tolerances.MAX_WIDENED_GRAD


@pytest.mark.parametrize("channel", range(9))
def test_isolation_cases_have_exact_zeros_and_no_near_ties(oracle, channel):
    """tests/test_gpu_head_loss.py::test_each_encoded_channel_in_isolation compares without a tie map: every term of these
    cases is either exactly tied (both sides computed from the same bits: sign(0) = 0 in every implementation) or clearly
    not.  The planes `isolation_exact_planes` names are exactly zero in the fp32 oracle."""
    enc, tgt, sc = hc.isolation_inputs(channel)
    maps = oracle.head_decode(enc)
    assert np.array_equal(np.delete(maps, hc.decoded_planes(channel), axis=1), np.delete(tgt, hc.decoded_planes(channel), axis=1))
    delta = np.log(oracle.render_fwd(maps, sc, f64=True) + 0.1) - np.log(oracle.render_fwd(tgt, sc, f64=True) + 0.1)
    assert not ((np.abs(delta) < tolerances.TIE_LEVEL) & (delta != 0.0)).any()
    loss, grad = oracle.head_loss(enc, tgt, sc, 0.1)
    _, g64 = hc.head_loss_f64_on_f32_decode(enc, tgt, sc, 0.1)
    assert loss > 0.0 and grad[:, channel].any()
    # on the changed channel's own plane this is the oracle's own double evaluation, to the rounding of the decode
    _, g64_full = oracle.head_loss(enc, tgt, sc, 0.1, f64=True)
    assert np.abs(g64[:, channel] - g64_full[:, channel]).max() <= 2e-5 * np.abs(g64_full[:, channel]).max()
    for plane in hc.isolation_exact_planes(channel):
        assert not grad[:, plane].any(), plane
    assert (channel in (0, 1, 5)) == (not hc.isolation_exact_planes(channel))
    # every plane that is not exact, each at the bound of its own largest element: the fp32 oracle inside the strict bound
    # against the fp64 oracle, but for a few
    for plane in sorted(set(range(9)) - set(hc.isolation_exact_planes(channel))):
        assert grad[:, plane].any(), plane
        strict = tolerances.GRAD_RTOL * np.abs(g64[:, plane]) + tolerances.GRAD_ATOL_FRAC * np.abs(g64[:, plane]).max()
        n_widened = int((np.abs(grad[:, plane] - g64[:, plane]) > strict).sum())
        tolerances._record("head isolation %d plane %d [oracle]" % (channel, plane), "widened by 2|ref-f64|", n_widened,
                           strict.size, tolerances.MAX_WIDENED_GRAD)
        assert n_widened <= tolerances.MAX_WIDENED_GRAD
    # nothing changed at all: loss and gradient exactly zero
    enc0, tgt0, _ = hc.isolation_inputs(None)
    l0, g0 = oracle.head_loss(enc0, tgt0, sc, 0.1)
    assert l0 == 0.0 and not g0.any()


# ---------------------------------------------------------------------------------------------- the allowance is a bound

def test_the_9_channel_allowance_bounds_what_a_tied_sign_can_move(oracle):
    """`all_saturated` at B = 2, H = 16 has tie pixels of one kind: the target renders exactly 0 under some light (behind its
    surface) and the input, with a saturated roughness or diffuse value, renders 0 or next to nothing (1e-16 ... 1e-8 of eps)
    -- |log difference| far below what fp32 resolves, so an fp32 evaluation gives the term sign 0 and the double
    evaluation +1.  One float32 step on a diffuse value of such a pixel moves a term between those two, or leaves it: the
    fp64 gradient may then change by no more than the allowance (what ALL the pixel's tied terms can move) plus the
    strict bound, at every element, and does not change at all at other pixels."""
    B, H = 2, 16
    enc, tgt, sc = hc.all_saturated(7800, B, H), synth.make_maps(7850, B, H), hc.scene_table(690, B, 3, 4)
    ref = hc.Reference(enc, tgt, sc, 0.0)
    ties = np.argwhere(ref.tie < tolerances.TIE_LEVEL)
    assert 4 <= len(ties) <= hc.MAX_TIES
    assert not ref.allow[np.broadcast_to((ref.tie >= tolerances.TIE_LEVEL)[:, None], ref.allow.shape)].any()
    scale = np.abs(ref.grad64).max()
    strict = tolerances.GRAD_RTOL * np.abs(ref.grad64) + tolerances.GRAD_ATOL_FRAC * scale
    moved, used, worst = 0, 0, 0.0
    for b, i, j in ties:
        for k in (2, 3, 4):
            for towards in (-2.0, 2.0):
                if enc[b, k, i, j] == np.sign(towards):
                    continue
                nudged = enc.copy()
                nudged[b, k, i, j] = np.nextafter(enc[b, k, i, j], np.float32(towards))
                _, g = oracle.head_loss(nudged, tgt, sc, 0.0, f64=True)
                change = np.abs(g - ref.grad64)
                others = np.ones(change.shape, bool)
                others[b, :, i, j] = False
                assert not change[others].any()
                assert (change <= ref.allow + strict).all(), (b, i, j, k, float((change - ref.allow - strict).max() / scale))
                moved += bool((change > 1e-9 * scale).any())
                used += bool((change > strict).any())
                with np.errstate(divide="ignore", invalid="ignore"):
                    worst = max(worst, float(np.nanmax(np.where(ref.allow > 0, change / ref.allow, 0.0))))
    print("[head-loss] allowance: %d tie pixels, %d nudges moved the fp64 gradient, %d beyond the strict bound, largest "
          "change / allowance %.3e" % (len(ties), moved, used, worst))
    assert moved > 0, "no nudge changed anything: the test does not reach the tied terms"


def test_the_allowance_bounds_a_gradient_that_is_all_tied_terms(oracle):
    """The tied terms of `all_saturated` carry next to nothing (the test above never needs the allowance beyond the strict
    bound), so the bound is also checked where it carries everything: with the target equal to the float32-decoded input,
    every term of a lit pixel is tied -- exactly in float32 (sign 0), to ~1e-8 with whatever sign in the double evaluation,
    whose decode does not round e + 1.  One float32 step up or down on the three diffuse planes decides all those signs
    one way or the other.  The fp64 gradient then changes by sign flips of tied terms and nothing else -- in the normal planes
    through the decode's Jacobian, in the roughness plane through the sum of three, in diffuse and specular through the
    factor 1/2 -- so every element must stay within the allowance of the unnudged input plus the strict bound, and
    somewhere the change must come to more than half of the allowance (a flip from -1 to +1), or the factor 2 in it
    would never have been exercised."""
    enc, tgt, sc = hc.isolation_inputs(None)
    tie, allow = hc.allowance9(enc, tgt, sc)
    lit = tie == 0.0                        # the other pixels have every light behind the surface: no term, no allowance
    assert lit.sum() > 48 and (tie[~lit] > 1.0).all() and allow[:, [2, 3, 4, 6, 7, 8]][:, :, lit[0]].all()
    _, g32 = oracle.head_loss(enc, tgt, sc, 0.0)
    assert not g32.any()
    _, g0 = oracle.head_loss(enc, tgt, sc, 0.0, f64=True)
    scale = np.abs(allow).max()
    strict = tolerances.GRAD_RTOL * np.abs(g0) + tolerances.GRAD_ATOL_FRAC * np.abs(g0).max()
    largest = 0.0
    for towards in (-2.0, 2.0):
        nudged = enc.copy()
        nudged[:, 2:5] = np.nextafter(enc[:, 2:5], np.float32(towards))
        _, g = oracle.head_loss(nudged, tgt, sc, 0.0, f64=True)
        change = np.abs(g - g0)
        assert change[:, [0, 1, 5]].any(axis=(0, 2, 3)).all() and not change[:, :, ~lit[0]].any()
        assert (change <= allow + strict).all(), float((change - allow - strict).max() / scale)
        big = allow > 1e-3 * scale
        largest = max(largest, float((change[big] / allow[big]).max()))
    print("[head-loss] allowance with every term tied: largest change / allowance %.3f" % largest)
    assert 0.5 < largest <= 1.0 + 1e-3
