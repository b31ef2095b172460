"""CPU: the exact tie allowance of the rendering-loss gradient (oracle.loss_tie_allowance, tests/tolerances.py).

At a tie pixel some term |log(r_in + 0.1) - log(r_tg + 0.1)| is below TIE_LEVEL and its sign() is rounding noise, so an
fp32 gradient may carry either sign for it.  The allowance of an element is 2 * the sum over the pixel's tied terms of
the term's absolute sign-free contribution (1 / (r_in + eps)) * d r_in / d map / count.  These tests pin the C export
against an independent numpy construction from render_fwd / render_bwd, show that the oracle's own fp32 gradient meets
the bound against its fp64 gradient, and show that the bound catches an error the old blanket TIE_SLACK rule let pass."""
import numpy as np
import pytest
import torch

import synth
import tolerances
from tolerances import TIE_LEVEL, TIE_SLACK, assert_grad_close

# sweep-style cases with ties (tests/test_gpu_parity.py seeded sweep, trials 0, 5, 10, 25):
# (trial, B, H, n_random, n_specular, roughness range, tied roughness, tilt, target's roughness tied)
CASES = [
    (0, 2, 5, 3, 3, (0.0, 0.01), True, 0.3, False),
    (5, 5, 8, 3, 3, (0.95, 1.0), True, 0.9, True),
    (10, 4, 8, 1, 3, (0.0, 0.01), False, 2.0, True),
    (25, 4, 13, 0, 3, (0.2, 0.9), False, 0.3, False),
]


def _case(trial, B, H, n_random, n_specular, r_range, tied, tilt, tgt_tied):
    from svbrdf_estimation_amd import environment
    inp = synth.make_maps(9000 + trial, B, H, tilt=tilt, r_lo=r_range[0], r_hi=r_range[1], tiled_roughness=tied)
    tgt = synth.make_maps(9500 + trial, B, H, tilt=0.3, tiled_roughness=tgt_tied)
    if trial % 5 == 0:      # specular at 1 and 0, diffuse at 0: the ends of the ranges, exactly
        inp[:, 9:12, : (H + 1) // 2] = np.float32(1.0)
        inp[:, 9:12, (H + 1) // 2:] = np.float32(0.0)
        inp[:, 3:6, :, : (H + 1) // 2] = np.float32(0.0)
    torch.manual_seed(400 + trial)
    table = torch.stack([environment.scene_table(n_random, n_specular) for _ in range(B)]).numpy()
    return inp, tgt, table


def _numpy_allowance(oracle, inp, tgt, table, eps=0.1):
    """the same quantity built from the fp64 renderings and one fp64 render_bwd per (scene, channel): a unit cotangent
    at the tied pixels of that plane, scaled afterwards by 1 / (count * (r_in + eps)) -- the backward is linear in it"""
    B, _, H, W = inp.shape
    S = table.shape[1]
    r_in, r_tg = oracle.render_fwd(inp, table, f64=True), oracle.render_fwd(tgt, table, f64=True)
    a_in = r_in + float(np.float32(eps))
    tied = np.abs(np.log(a_in) - np.log(r_tg + float(np.float32(eps)))) < TIE_LEVEL
    allow = np.zeros(inp.shape)
    for s in range(S):
        for k in range(3):
            if not tied[:, s, k].any():
                continue
            cot = np.zeros((B, S, 3, H, W), np.float32)
            cot[:, s, k] = tied[:, s, k]
            g = oracle.render_bwd(inp, table, cot, f64=True)
            allow += np.abs(g / ((B * S * 3 * H * W) * a_in[:, s, k])[:, None])
    return 2.0 * allow, tied.any(axis=(1, 2))


@pytest.mark.parametrize("case", CASES, ids=["trial%d" % c[0] for c in CASES])
def test_c_allowance_equals_the_numpy_construction(oracle, case):
    inp, tgt, table = _case(*case)
    allow = oracle.loss_tie_allowance(inp, tgt, table)
    ref, tied_pix = _numpy_allowance(oracle, inp, tgt, table)
    tie_pix = oracle.loss_tie_map(inp, tgt, table) < TIE_LEVEL
    assert tie_pix.any() and allow.any(), "the case was chosen for its ties"
    # a structural zero (light below both horizons) renders both exactly 0 and contributes exactly 0 to the gradient:
    # the numpy side may count it as tied, the C side does not, and the allowance is the same
    assert (allow.max(axis=1) > 0).sum() > 0 and not (allow.max(axis=1) > 0)[~tie_pix].any()
    assert not tie_pix[~tied_pix].any()
    np.testing.assert_allclose(allow, ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())
    # the MixedLoss's L1 part has no such ties: the same allowance
    assert np.array_equal(oracle.loss_tie_allowance(inp, tgt, table, l1_weight=0.1), allow)
    # and it is the only widening: the level 0 leaves nothing tied
    assert not oracle.loss_tie_allowance(inp, tgt, table, tie_level=0.0).any()


@pytest.mark.parametrize("case", CASES, ids=["trial%d" % c[0] for c in CASES])
def test_oracle_fp32_gradient_meets_the_exact_bound_against_fp64(oracle, case):
    inp, tgt, table = _case(*case)
    tie, allow = oracle.loss_tie_map(inp, tgt, table), oracle.loss_tie_allowance(inp, tgt, table)
    for l1w in (0.0, 0.1):
        _, g32 = oracle.mixed_loss(inp, tgt, table, l1w)
        _, g64 = oracle.mixed_loss(inp, tgt, table, l1w, f64=True)
        assert_grad_close(g32, g64, "oracle32 vs oracle64 trial %d l1=%.1f" % (case[0], l1w), tie_map=tie,
                          tie_allowance=allow, max_ties=48)


def _passes_the_old_rule(a, b, tie_map):
    """the rule before the exact allowance: tie pixels excluded, only held to TIE_SLACK * max|b|"""
    err = np.abs(np.asarray(a, np.float64) - b)
    scale = np.abs(b).max()
    ties = np.broadcast_to((tie_map < TIE_LEVEL)[:, None], err.shape)
    tol = tolerances.GRAD_RTOL * np.abs(b) + tolerances.GRAD_ATOL_FRAC * scale
    return bool(np.where(ties, err, 0).max() <= TIE_SLACK * scale and (ties | (err <= tol)).all())


def test_a_wrong_tie_element_is_caught_that_the_old_rule_let_pass(oracle):
    inp, tgt, table = _case(*CASES[2])
    tie, allow = oracle.loss_tie_map(inp, tgt, table), oracle.loss_tie_allowance(inp, tgt, table)
    _, g32 = oracle.rendering_loss(inp, tgt, table)
    _, g64 = oracle.rendering_loss(inp, tgt, table, f64=True)
    scale = np.abs(g64).max()
    ties = np.broadcast_to((tie < TIE_LEVEL)[:, None], allow.shape)
    cand = np.argwhere(ties & (allow < 1e-3 * scale))
    assert len(cand), "trial 10 has tie elements with a small allowance (measured: dozens with exactly 0)"
    idx = tuple(cand[len(cand) // 2])
    bad = g32.copy()
    bad[idx] += np.float32(1e-2 * scale)
    assert_grad_close(g32, g64, "unperturbed", tie_map=tie, tie_allowance=allow, max_ties=48)
    assert _passes_the_old_rule(bad, g64, tie), "the old TIE_SLACK rule (0.5 of max at tie pixels) lets this pass"
    with pytest.raises(AssertionError, match="tie elements beyond the bound"):
        assert_grad_close(bad, g64, "perturbed tie element", tie_map=tie, tie_allowance=allow, max_ties=48)


def test_allowance_is_required_with_a_tie_map_and_must_sit_at_tie_pixels(oracle):
    inp, tgt, table = _case(*CASES[0])
    tie, allow = oracle.loss_tie_map(inp, tgt, table), oracle.loss_tie_allowance(inp, tgt, table)
    _, g = oracle.rendering_loss(inp, tgt, table, f64=True)
    with pytest.raises(AssertionError, match="go together"):
        assert_grad_close(g, g, "tie map alone", tie_map=tie, max_ties=48)
    moved = np.zeros_like(allow)
    moved[0, 0, 0, 0] = 1.0
    assert tie[0, 0, 0] >= TIE_LEVEL, "the case's pixel (0, 0) was expected untied"
    with pytest.raises(AssertionError, match="outside the tie pixels"):
        assert_grad_close(g, g, "allowance off the ties", tie_map=tie, tie_allowance=moved, max_ties=48)
