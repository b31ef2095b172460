"""The gradient of the photo losses towards the photographs, without a GPU: the comparison values the GPU tests
(tests/test_gpu_photo_grad.py) rely on, the definition against torch autograd, the modules' routing and the entry points'
argument checks.  tests/photo_grad_checks.py holds the restatement of the magnitude and the cases."""
import ctypes
import os

import numpy as np
import pytest
import torch

import photo_grad_checks as pg
import tolerances

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = pg.EPS


# ------------------------------------------------------------------------------------------------ caps by the oracle alone

def test_gpu_cases_stay_inside_the_caps_by_the_comparison_values_alone():
    """every (case, layout, maps / head) the GPU parity test runs: at most MAX_TIE_PIXELS tie pixels (0 are expected: a
    changed generator fails here and not on the GPU) and no sign flip of the float32 oracle against float64 outside ties"""
    smallest = (np.inf, None)
    for name, layout, head in pg.PARAMS:
        c = pg.comparison(name, layout, head)
        assert c.tie_pixels() <= tolerances.MAX_TIE_PIXELS, (name, layout, head, c.tie_pixels())
        decided = ~c.structural & ~c.tie_terms
        flips = int((np.sign(c.delta32[decided]) != np.sign(c.delta64[decided])).sum())
        assert flips == 0, (name, layout, head, flips)
        assert decided.any() and np.isfinite(c.value64).all() and np.isfinite(c.m32).all()
        # the restatement against the float64 value on the case's own terms
        live = decided & (c.m32 > 0)
        rel = np.abs(c.m32[live].astype(np.float64) - np.abs(c.value64[live])) / np.abs(c.value64[live])
        assert rel.max() <= (pg.ROUNDINGS + 1) * 2.0 ** -24, (name, layout, head, rel.max())
        smallest = min(smallest, (c.smallest_delta(), "%s %s %s" % (name, layout, "head" if head else "maps")))
        print("[photo-grad] %s %s %s: %d tie pixels, smallest non-structural |delta64| %.3g" % (
            name, layout, "head" if head else "maps", c.tie_pixels(), c.smallest_delta()))
    print("[photo-grad] smallest non-structural |delta64| over all cases: %.3g at %s" % smallest)


def test_restatement_is_within_its_roundings_of_the_float64_magnitude():
    """(R + 1) 2^-24 relative on 10^6 random (w, p): R individually rounded operations, each within 2^-24 relative (half an
    ULP is at most 2^-24 of the value), and one more for the products of the (1 + d) factors"""
    rng = np.random.default_rng(2600)
    n = 10 ** 6
    w = rng.random(n, dtype=np.float32)
    w[w == 0] = 1.0
    p = (rng.random(n, dtype=np.float32) * np.float32(1.25)).astype(np.float32)
    p[: n // 8] = (rng.random(n // 8, dtype=np.float32) * np.float32(1e-3)).astype(np.float32)      # dark values, where eps rules
    worst = 0.0
    for count in (3, 2 * 9 * 3 * 45 * 45, 8 * 9 * 3 * 256 * 256, 3 * (1 << 25) * 7):
        m = pg.restated_magnitude(p, w, EPS, count)
        exact = w.astype(np.float64) / (float(count) * (p.astype(np.float64) + np.float64(np.float32(EPS))))
        rel = np.abs(m.astype(np.float64) - exact) / exact
        worst = max(worst, float(rel.max()))
        assert rel.max() <= (pg.ROUNDINGS + 1) * 2.0 ** -24, (count, rel.max() * 2.0 ** 24)
    print("[photo-grad] restatement vs float64 on 1e6 (w, p): largest %.2f x 2^-24 (bound %d)" % (worst * 2.0 ** 24, pg.ROUNDINGS + 1))
    # unweighted: the same formula with w = 1 (the multiply is exact)
    assert np.array_equal(pg.restated_magnitude(p, None, EPS, 1234), pg.restated_magnitude(p, np.ones_like(p), EPS, 1234))


# ------------------------------------------------------------------------------------------------ torch autograd agreement

class _ToyRenderer:
    """a plugin: any object with render(scene, svbrdf [12,H,W] or [1,12,H,W]) -> [1,3,H,W]; differentiable torch ops"""

    def render(self, scene, svbrdf):
        m = svbrdf if svbrdf.dim() == 4 else svbrdf.unsqueeze(0)
        cam = torch.as_tensor(scene.camera.pos, dtype=m.dtype).view(1, 3, 1, 1)
        col = torch.as_tensor(scene.light.color, dtype=m.dtype).view(1, 3, 1, 1)
        lz = float(torch.as_tensor(scene.light.pos)[2])
        return (m[:, 3:6] * col * 0.01 + m[:, 9:12] * torch.clamp((m[:, 0:3] * cam).sum(1, keepdim=True), min=0.0) ** 2
                + m[:, 6:9] * lz * 0.1)


def _toy_problem(dtype=torch.float64, B=2, S=3, H=6, seed=5):
    from svbrdf_estimation_amd import environment
    g = torch.Generator().manual_seed(seed)
    maps = torch.rand((B, 12, H, H), generator=g, dtype=torch.float64).to(dtype)
    photos = torch.rand((B, S, 3, H, H), generator=g, dtype=torch.float64).to(dtype)
    torch.manual_seed(seed)
    table = torch.stack([environment.scene_table(1, S - 1) for _ in range(B)])
    weights = torch.rand((B, S, H, H), generator=g, dtype=torch.float64).to(torch.float32)
    weights[weights < 0.25] = 0.0
    weights[weights > 0.75] = 1.0
    return maps, photos, table, weights


def _toy_rendered(maps, table):
    from svbrdf_estimation_amd import environment
    R = _ToyRenderer()
    return torch.stack([torch.cat([R.render(sc, maps[b]) for sc in environment.scenes_from_table(table[b])], dim=0)
                        for b in range(maps.shape[0])], dim=0)


def _value64(rendered, photos, eps, weights):
    """the float64 comparison value, the formula of photo_grad_checks.Comparison.value64"""
    w = torch.ones(photos.shape[:2] + photos.shape[3:], dtype=torch.float64) if weights is None else \
        weights.to(torch.float64).expand(photos.shape[:2] + photos.shape[3:])
    w = w.unsqueeze(2)
    p = torch.where(w > 0, photos, torch.zeros((), dtype=photos.dtype))
    delta = torch.log(rendered + eps) - torch.log(p + eps)
    return -w * torch.sign(delta) / (photos.numel() * (p + eps))


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_comparison_value_is_torch_autograd_of_the_definition(weighted):
    from svbrdf_estimation_amd import losses
    maps, photos, table, weights = _toy_problem()
    rendered = _toy_rendered(maps, table)
    w = weights if weighted else None
    leaf = photos.clone().requires_grad_(True)
    loss = losses.weighted_log_l1(rendered, leaf, 0.05, w) if weighted else \
        torch.nn.functional.l1_loss(torch.log(rendered + 0.05), torch.log(leaf + 0.05))
    loss.backward()
    want = _value64(rendered, photos, 0.05, w)
    assert want.abs().max() > 0
    assert (leaf.grad - want).abs().max() <= 1e-12 * want.abs().max()
    if weighted:
        assert not leaf.grad[(weights == 0).unsqueeze(2).expand_as(leaf.grad)].any()


def test_zero_weights_over_nan_photos_give_exactly_zero_in_torch_too():
    from svbrdf_estimation_amd import losses
    maps, photos, table, weights = _toy_problem()
    spoiled = photos.clone()
    dead = (weights == 0).unsqueeze(2).expand_as(photos)
    assert dead.any()
    spoiled[dead] = float("nan")
    leaf = spoiled.clone().requires_grad_(True)
    loss = losses.weighted_log_l1(_toy_rendered(maps, table), leaf, 0.05, weights)
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(leaf.grad).all() and not leaf.grad[dead].any() and leaf.grad[~dead].any()
    clean = photos.clone().requires_grad_(True)
    losses.weighted_log_l1(_toy_rendered(maps, table), clean, 0.05, weights).backward()
    assert torch.equal(clean.grad, leaf.grad)


# ------------------------------------------------------------------------------------------------ routing on the host

@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_differentiable_photos_with_a_plugin_renderer_is_the_torch_gradient(weighted):
    from svbrdf_estimation_amd import losses
    for dtype in (torch.float32, torch.float64):
        maps, photos, table, weights = _toy_problem(dtype)
        w = weights if weighted else None
        fn = losses.PhotoLoss(_ToyRenderer(), eps=0.05, differentiable_photos=True)
        assert not fn.uses_fused_kernel() and fn.differentiable_photos
        leaf, x = photos.clone().requires_grad_(True), maps.clone().requires_grad_(True)
        loss = fn(x, leaf, table, w)
        loss.backward()
        ref_leaf = photos.clone().requires_grad_(True)
        rendered = _toy_rendered(maps, table)
        ref = losses.weighted_log_l1(rendered, ref_leaf, 0.05, w) if weighted else \
            torch.nn.functional.l1_loss(torch.log(rendered + 0.05), torch.log(ref_leaf + 0.05))
        ref.backward()
        assert torch.equal(loss.detach(), ref.detach()) and torch.equal(leaf.grad, ref_leaf.grad) and x.grad is not None
        if dtype == torch.float64:
            want = _value64(rendered, photos, 0.05, w)
            assert (leaf.grad - want).abs().max() <= 1e-12 * want.abs().max()


def test_default_constructor_still_refuses_photos_that_require_grad():
    from svbrdf_estimation_amd import losses, renderers
    maps, photos, table, _ = _toy_problem(torch.float32)
    for fn in (losses.PhotoLoss(_ToyRenderer()), losses.PhotoLoss(renderers.LocalRenderer()),
               losses.PhotoLoss(_ToyRenderer(), differentiable_photos=False)):
        assert fn.differentiable_photos is False
        with pytest.raises(RuntimeError, match="no gradient w.r.t. the photos"):
            fn(maps, photos.clone().requires_grad_(True), table)
    with pytest.raises(RuntimeError, match="no gradient w.r.t. the photos"):
        losses.HeadPhotoLoss(renderers.LocalRenderer())(maps[:, :9], photos.clone().requires_grad_(True), table)
    assert losses.HeadPhotoLoss(renderers.LocalRenderer(), differentiable_photos=True).differentiable_photos is True


def test_binding_refuses_the_photo_gradient_beside_exposure_or_scene_gradient():
    from svbrdf_estimation_amd import _native
    maps, photos, table, _ = _toy_problem(torch.float32)
    with pytest.raises(ValueError, match="want_photo_grad"):
        _native.photo_loss(maps, photos, table, want_photo_grad=True, exposure=torch.ones(2, 3, 3))
    with pytest.raises(ValueError, match="want_photo_grad"):
        _native.photo_loss(maps, photos, table, want_photo_grad=True, want_scene_grad=True)
    with pytest.raises(_native.NativeLibraryError):         # host tensors: no CPU fallback
        _native.photo_loss(maps, photos, table, want_photo_grad=True)


@pytest.fixture(scope="module")
def lib():
    from svbrdf_estimation_amd import _native
    return _native._load()


def test_entries_are_exported_declared_and_bound(lib):
    from svbrdf_estimation_amd import _native
    header = open(os.path.join(ROOT, "include", "svbrdf_hip.h")).read()
    for name in pg.ENTRIES:
        assert hasattr(lib, name), name
        assert "SVBRDF_API int %s(" % name in header
        declared = header.split("SVBRDF_API int %s(" % name)[1].split(");")[0]
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == 17 == declared.count(",") + 1
    assert "svbrdf_[head_]photo_loss_photo_grad_fwd_bwd" in header and "ADDED TO ABI VERSION 8 WITHOUT A BUMP" in header
    assert lib.svbrdf_abi_version() == 8


@pytest.mark.parametrize("entry", pg.ENTRIES)
def test_argument_errors_come_before_any_launch(lib, entry):
    """-1 null pointers (grad_photos included; grad_input and weights may be null), -2 dims, eps, a weight_planes that does
    not fit `weights`, S beyond 1706 without the map gradient; -3 misaligned; -4 workspace too small.  Host buffers stand in
    for device memory: nothing is enqueued."""
    fn = getattr(lib, entry)
    B, S, H = 1, 9, 8
    buf = (ctypes.c_float * 28672)()
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 63) & ~63
    need = lib.svbrdf_rendering_loss_workspace_bytes(B, S, H, H)
    assert need == 65 * 8

    def call(input=p, photos=p + 256, weights=p + 16384, planes=S, scenes=p + 512, xrow=p + 1024, eps=0.1, loss=p + 2048,
             grad=p + 4096, grad_p=p + 24000, ws=p + 8192, ws_bytes=need, B=B, S=S, H=H, W=H):
        return fn(input, photos, weights, planes, scenes, xrow, ctypes.c_float(eps), loss, grad, grad_p, ws, ws_bytes, B, S, H, W,
                  None)

    launches = lib.svbrdf_debug_launch_count()
    for name in ("input", "photos", "scenes", "xrow", "loss", "grad_p", "ws"):
        assert call(**{name: None}) == -1, name
        assert lib.svbrdf_last_error()
        assert call(**{name: None}, grad=None) == -1, name
    for planes in (0, 2, S + 1, -1):
        assert call(planes=planes) == -2, planes
        assert b"weight_planes" in lib.svbrdf_last_error()
    for planes in (1, S, 2):                                        # no weights: only 0 planes
        assert call(weights=None, planes=planes) == -2, planes
        assert b"weight_planes" in lib.svbrdf_last_error()
    assert call(W=H + 1) == -2 and call(B=0) == -2 and call(S=0, planes=1) == -2 and call(eps=0.0) == -2
    assert call(photos=p + 258) == -3 and call(grad=p + 4098) == -3 and call(scenes=p + 514) == -3
    assert call(weights=p + 16386) == -3 and call(grad_p=p + 24002) == -3 and call(ws=p + 8196) == -3
    assert call(ws_bytes=need - 8) == -4
    assert call(S=1707, planes=1707, grad=None, ws_bytes=1 << 20) == -2     # forward only: the item's table is staged in LDS
    assert b"1706" in lib.svbrdf_last_error()
    assert lib.svbrdf_debug_launch_count() == launches              # failed calls enqueue and count nothing
