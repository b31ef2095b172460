"""Shared by tests/test_photo_loss_cpu.py and tests/test_gpu_photo_loss.py: the ORACLE's photo loss and the tie rule.

The C oracle needs no photo loss of its own -- it is the composition

    rad  = c_oracle.render_fwd(input, scenes)
    loss = mean | log(rad + eps) - log(photo + eps) |
    g    = sign(delta) / (N (rad + eps))
    grad = c_oracle.render_bwd(input, scenes, g)

(with photo = render_fwd(target) it reproduces c_oracle.rendering_loss: loss to 7 digits, gradient to 1.1e-7 of its
maximum).  f64=True evaluates everything in double on the same float32 inputs: the comparison value's own error.

Ties.  A term (b, s, c, i, j) whose |delta| in float64 is below tolerances.TIE_LEVEL has an undetermined sign in any fp32
evaluation, the reference's included -- unless it is STRUCTURAL: the photo value is exactly 0 and the light is behind the
surface (unclamped n.wi < -1e-6, computed here in float64 from the scene row and the pixel grid), where both sides are
exactly eps in every evaluation and the term is exactly 0 with gradient 0.  A tie pixel has a non-structural tied term.  Tie
pixels are left out of the element-wise comparison, must stay within TIE_SLACK * max|g| and are counted against a cap.
"""
import numpy as np

import tolerances
from oracle import c_oracle


def oracle_photo_loss(inp, photos, scenes, eps=0.1, f64=False, want_grad=True):
    """-> (loss: float, grad [B,12,H,W] float32 / float64 or None, delta [B,S,3,H,W])"""
    inp = np.ascontiguousarray(inp, np.float32)
    scenes = np.ascontiguousarray(scenes, np.float32)
    photos = np.asarray(photos, np.float32)
    rad = c_oracle.render_fwd(inp, scenes, f64=f64)
    assert rad.shape == photos.shape, (rad.shape, photos.shape)
    if f64:
        a = rad + np.float64(np.float32(eps))
        b = photos.astype(np.float64) + np.float64(np.float32(eps))
    else:
        a = rad + np.float32(eps)
        b = photos + np.float32(eps)
    with np.errstate(invalid="ignore", divide="ignore"):
        delta = np.log(a) - np.log(b)
    loss = float(np.abs(delta.astype(np.float64)).mean())
    if not want_grad:
        return loss, None, delta
    g = (np.sign(delta).astype(np.float64) / (float(delta.size) * a.astype(np.float64))).astype(np.float32)
    return loss, c_oracle.render_bwd(inp, scenes, g, f64=f64), delta


def unclamped_n_dot_wi(inp, scenes):
    """[B,S,H,W] float64: n . normalize(light - pixel) with the pixel grid of renderers.py:73-76"""
    inp = np.asarray(inp, np.float64)
    scenes = np.asarray(scenes, np.float64)
    B, _, H, W = inp.shape
    xrow = c_oracle.make_xrow(W).astype(np.float64)
    x = xrow[None, None, None, :]                       # pixel (i, j) sits at (xrow[j], -xrow[i], 0)
    y = -xrow[None, None, :, None]
    lx = scenes[:, :, 3, None, None] - x
    ly = scenes[:, :, 4, None, None] - y
    lz = scenes[:, :, 5, None, None] + 0.0 * x
    inv = 1.0 / np.sqrt(lx * lx + ly * ly + lz * lz)
    n = inp[:, None, 0:3]                               # [B,1,3,H,W]
    return (n[:, :, 0] * lx + n[:, :, 1] * ly + n[:, :, 2] * lz) * inv


def tie_map(inp, photos, scenes, delta_f64):
    """[B,H,W] float64: smallest |delta_f64| over the pixel's NON-structural terms (inf where all are structural)"""
    structural = (np.asarray(photos)[:, :, :, :, :] == 0.0) & (unclamped_n_dot_wi(inp, scenes) < -1e-6)[:, :, None]
    d = np.where(structural, np.inf, np.abs(np.asarray(delta_f64, np.float64)))
    return d.min(axis=(1, 2))


def assert_photo_grad_close(got, ref, f64, tmap, what, max_ties=tolerances.MAX_TIE_PIXELS):
    """tests/tolerances.py's gradient bound (1e-4 |b| + 1e-5 max|b|, widened by 2|b - f64| for at most MAX_WIDENED_GRAD
    elements) with the tie rule above.  Goes through tolerances.assert_grad_close, so every use lands in the session
    ledger: the allowance of a tie pixel's elements is the outer bound TIE_SLACK * max|b| itself."""
    ref = np.asarray(ref)
    scale = float(np.abs(ref).max())
    ties = np.asarray(tmap) < tolerances.TIE_LEVEL
    allow = np.where(np.broadcast_to(ties[:, None], ref.shape), tolerances.TIE_SLACK * scale, 0.0)
    tolerances.assert_grad_close(got, ref, what, f64=f64, tie_map=tmap, tie_allowance=allow, max_ties=max_ties,
                                 scale=scale)
    return int(ties.sum())
