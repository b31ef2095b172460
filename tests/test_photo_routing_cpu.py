"""Which mode of the binding PhotoLoss and HeadPhotoLoss ask for under every combination of things that require grad, with
no GPU and no library: the module-level routing (losses._PhotoLossModule._forward, losses._FusedPhotoLoss) as rules.

The device is stood in for as tests/test_photo_fit_pose_cpu.py does it: ``losses._check_fused_photo_inputs`` answers "float32,
fused", ``_native.photo_loss`` is a recorder that returns tensors of the documented shapes filled with one recognisable
constant per slot (a constant loss: no composed arithmetic is needed), ``_native.scale_inplace_`` is ``g.mul_(scale)``, and
``losses.composed_photo_loss`` only notes that it was taken.  B = 1, S = 2, 2 x 2 pixels: the routing does not depend on
size, and this is the smallest shape that tells [B,S,..] from [B,1,..].  On the CPU a "host" and a "device" table are the
same kind of tensor; both are driven, so that the product is the one the modules see on a device.

The expected answers are written out below as rules, independent of the code under test:

  * photos that require grad (``differentiable_photos=True``) under grad mode together with a table or an exposure that
    requires grad: the composed definition, the binding is not called;
  * else an exposure is folded into the table's colour columns in float32 in front of the call when, under grad mode, the
    photos or the table want a gradient, or when neither the input nor the exposure requires grad under grad mode (so
    always under ``no_grad``) -- detached unless it is the table's gradient that is wanted, where autograd chains the
    colour gradient back to the gains; any other exposure is handed to the binding;
  * the binding's mode is picked from what REQUIRES grad among the tensors handed over -- autograd's ``needs_input_grad``,
    which does not look at grad mode: the photo-gradient entries for photos that require grad, else the scene-gradient
    entries for a table that does (a folded one only where its gradient was wanted), else the exposure entries where an
    exposure was handed over, else the plain entries; ``want_grad`` is "the input requires grad", ``want_exposure_grad``
    "the exposure handed over requires grad";
  * the loss requires grad under grad mode when any of these does, and is then a ``_PhotoLossTensor`` unless
    ``normalize="weights"`` rescales it; ``backward()`` hands every leaf the recorder's buffer of its slot times the
    upstream scale.
"""
import itertools

import pytest
import torch

B, S, H = 1, 2, 2
LOSS, G_INPUT, G_EXPOSURE, G_SCENES, G_PHOTOS = 3.0, 2.0, 5.0, 7.0, 11.0        # one recognisable constant per slot
WEIGHT = 0.5        # every weight: normalize="weights" then scales the loss by N / (3 sum w) = 2 exactly


class _Recorder:
    """stands in for _native.photo_loss: its modes, its return shapes, nothing computed"""

    def __init__(self):
        self.calls = []

    def __call__(self, input, photos, scenes, eps=0.1, want_grad=True, head=False, weights=None, exposure=None,
                 want_exposure_grad=False, want_scene_grad=False, want_photo_grad=False):
        assert not (want_scene_grad and exposure is not None)                   # the binding's two ValueErrors
        assert not (want_photo_grad and (exposure is not None or want_scene_grad))
        self.calls.append(dict(head=bool(head), weights=weights is not None, exposure=exposure is not None,
                               want_grad=bool(want_grad), want_exposure_grad=bool(want_exposure_grad),
                               want_scene_grad=bool(want_scene_grad), want_photo_grad=bool(want_photo_grad),
                               table=scenes.detach().clone(), eps=eps))
        loss = torch.full((1,), LOSS)
        grad = torch.full(input.shape, G_INPUT) if want_grad else None
        if exposure is not None:
            return loss, grad, (torch.full((B, S, 3), G_EXPOSURE) if want_exposure_grad else None)
        if want_scene_grad:
            return loss, grad, torch.full((B, S, 9), G_SCENES)
        if want_photo_grad:
            return loss, grad, torch.full(photos.shape, G_PHOTOS)
        return loss, grad


@pytest.fixture
def stand_ins(monkeypatch):
    from svbrdf_estimation_amd import _native, losses
    rec, composed = _Recorder(), []
    monkeypatch.setattr(losses, "_check_fused_photo_inputs", lambda *a: False)
    monkeypatch.setattr(_native, "photo_loss", rec)
    monkeypatch.setattr(_native, "scale_inplace_", lambda g, scale: g.mul_(scale))

    def composed_photo_loss(input, photos, scenes, eps, weights=None, exposure=None):
        composed.append(1)
        return torch.full((), LOSS)
    monkeypatch.setattr(losses, "composed_photo_loss", composed_photo_loss)
    return rec, composed


def _operands(head, weighted, expo, table, photos_rg, x_rg):
    """fresh leaves for one combination (values fixed: the fold is compared by value)"""
    x = (torch.arange(B * (9 if head else 12) * H * H, dtype=torch.float32).reshape(B, -1, H, H) / 64.0).requires_grad_(x_rg)
    photos = (0.25 + torch.arange(B * S * 3 * H * H, dtype=torch.float32).reshape(B, S, 3, H, H) / 128.0).requires_grad_(photos_rg)
    scenes = (1.0 + torch.arange(B * S * 9, dtype=torch.float32).reshape(B, S, 9) / 8.0).requires_grad_(table == "grad")
    weights = torch.full((B, S, H, H), WEIGHT) if weighted else None
    gains = None if expo == "none" else (0.5 + torch.arange(B * S * 3, dtype=torch.float32).reshape(B, S, 3) / 4.0
                                         ).requires_grad_(expo == "grad")
    return x, photos, scenes, weights, gains


def _expected(weighted, normalize, expo, table, photos_rg, x_rg, grad_on):
    """the rules of the module docstring for one combination"""
    e_rg, t_rg = expo == "grad", table == "grad"
    if photos_rg and grad_on and (t_rg or e_rg):
        return dict(composed=True)
    want_t = t_rg and grad_on
    folded = expo != "none" and ((photos_rg and grad_on) or want_t or not (grad_on and (x_rg or e_rg)))
    given = expo != "none" and not folded
    table_rg = want_t if folded else t_rg               # of the table handed over
    mode = "photos" if photos_rg else "scenes" if table_rg else "exposure" if given else None
    want_e = given and e_rg
    requires_grad = grad_on and (x_rg or photos_rg or table_rg or want_e)
    return dict(composed=False, folded=folded, chained=folded and want_t and e_rg, requires_grad=requires_grad,
                subclass=requires_grad and (not weighted or normalize == "count"),
                keywords=dict(weights=weighted, exposure=given, want_grad=x_rg, want_exposure_grad=want_e,
                              want_scene_grad=mode == "scenes", want_photo_grad=mode == "photos"),
                leaves=dict(x=x_rg, photos=photos_rg, scenes=t_rg, gains=want_e or (folded and want_t and e_rg)))


CASES = [(head, weighted, normalize) for head in (False, True) for weighted, normalize in
         ((False, "count"), (True, "count"), (True, "weights"))]


@pytest.mark.parametrize("head,weighted,normalize", CASES,
                         ids=["%s-%s" % ("head" if h else "maps", "weights_by_" + n if w else "unweighted") for h, w, n in CASES])
def test_module_routing_over_everything_that_can_require_grad(stand_ins, head, weighted, normalize):
    from svbrdf_estimation_amd import losses, renderers
    rec, composed = stand_ins
    seen = set()
    for expo, table, photos_rg, x_rg, grad_on in itertools.product(("none", "constant", "grad"), ("host", "constant", "grad"),
                                                                   (False, True), (False, True), (True, False)):
        what = (head, weighted, normalize, expo, table, photos_rg, x_rg, grad_on)
        x, photos, scenes, weights, gains = _operands(head, weighted, expo, table, photos_rg, x_rg)
        fn = (losses.HeadPhotoLoss if head else losses.PhotoLoss)(renderers.LocalRenderer(), normalize=normalize,
                                                                  differentiable_photos=photos_rg)
        assert fn.uses_fused_kernel()
        del rec.calls[:], composed[:]
        with torch.set_grad_enabled(grad_on):
            out = fn(x, photos, scenes, weights, gains)
        want = _expected(weighted, normalize, expo, table, photos_rg, x_rg, grad_on)
        assert out.dim() == 0, what
        if want["composed"]:
            assert composed == [1] and not rec.calls, what
            seen.add("composed")
            continue
        assert not composed and len(rec.calls) == 1, what
        call = rec.calls[0]
        assert call.pop("head") is head and call.pop("eps") == 0.1, what
        handed = call.pop("table")
        assert call == want["keywords"], (what, call)
        # the table handed over: the given one, or the one with the gains folded into its colour columns, by value
        given = scenes.detach()
        folded = torch.cat((given[..., :6], given[..., 6:] * (1.0 if gains is None else gains.detach())), dim=-1)
        assert torch.equal(handed, folded if want["folded"] else given), what
        assert gains is None or not torch.equal(folded, given)
        assert out.requires_grad is want["requires_grad"], what
        assert isinstance(out, losses._PhotoLossTensor) is want["subclass"], what
        scale = 2.0 if weighted and normalize == "weights" else 1.0
        assert out.item() == LOSS * scale, what
        seen.add(("folded" if want["folded"] else "given", tuple(k for k, v in want["keywords"].items() if v and k != "weights")))
        if not want["requires_grad"]:
            continue
        out.backward()
        leaves = dict(x=x, photos=photos, scenes=scenes, gains=gains)
        for name, leaf in leaves.items():
            if leaf is not None:
                assert (leaf.grad is not None) is want["leaves"][name], (what, name)
        if want["leaves"]["x"]:
            assert torch.equal(x.grad, torch.full(x.shape, G_INPUT * scale)), what
        if want["leaves"]["photos"]:
            assert torch.equal(photos.grad, torch.full(photos.shape, G_PHOTOS * scale)), what
        if want["leaves"]["scenes"]:
            # through the fold: the colour columns' gradient times the gains, the gains' times the colours
            colour = 1.0 if not want["folded"] else gains.detach()
            assert torch.equal(scenes.grad, torch.cat((torch.full((B, S, 6), G_SCENES * scale),
                                                       G_SCENES * scale * colour * torch.ones(B, S, 3)), dim=-1)), what
        if want["leaves"]["gains"]:
            if want["chained"]:
                assert torch.equal(gains.grad, G_SCENES * scale * given[..., 6:]), what
            else:
                assert torch.equal(gains.grad, torch.full((B, S, 3), G_EXPOSURE * scale)), what
    # every route was driven: the composed definition, the four modes, a fold in front of three of them
    modes = {m for _, m in (s for s in seen if s != "composed")}
    assert "composed" in seen and {(), ("want_grad",), ("exposure", "want_grad", "want_exposure_grad"),
                                   ("want_grad", "want_scene_grad"), ("want_grad", "want_photo_grad"),
                                   ("want_photo_grad",)} <= modes, modes
    assert {("folded", ()), ("folded", ("want_grad", "want_scene_grad")), ("folded", ("want_grad", "want_photo_grad"))} <= seen


def test_a_retained_graph_keeps_the_buffers_and_a_second_plain_backward_fails(stand_ins):
    """the hand-over's contract on the stand-in: under retain_graph every backward receives a scaled copy, a plain one
    takes the buffers, and the backward after it raises the second-time error"""
    from svbrdf_estimation_amd import losses, renderers
    x, photos, scenes, _, gains = _operands(False, False, "grad", "constant", False, True)
    out = losses.PhotoLoss(renderers.LocalRenderer())(x, photos, scenes, None, gains)
    (out * 3.0).backward(retain_graph=True)
    assert torch.equal(x.grad, torch.full(x.shape, G_INPUT * 3.0)) and torch.equal(gains.grad, torch.full((B, S, 3), G_EXPOSURE * 3.0))
    x.grad = gains.grad = None
    out.backward()
    assert torch.equal(x.grad, torch.full(x.shape, G_INPUT)) and torch.equal(gains.grad, torch.full((B, S, 3), G_EXPOSURE))
    with pytest.raises(RuntimeError, match="Trying to backward through the fused photo loss a second time"):
        out.backward()
