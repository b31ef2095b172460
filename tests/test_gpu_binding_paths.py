"""Every form in which the ctypes binding (svbrdf_estimation_amd/_native.py) takes a scene table reaches the same result.

A table may arrive on the device, on the host small enough to ride in the launch's kernel-argument block, or on the host
and larger than that (then the binding uploads it); K1 / K2 also take ONE host table [S,9] shared by every map.  Each entry
family is called with the table in each form it accepts and must give bitwise the same outputs (the kernels share their
bodies: no tolerance), enqueue exactly one kernel, and enter ``upload_scene_table`` exactly when the form says so.  The
upload is forced at these small shapes by setting the row limit the binding caches (``_host_rows``) to 1.  The shared forms
are compared with the device call on the same rows repeated per map.  ``render_fwd`` on the device table is held to the
oracle, which anchors the whole comparison.

Shapes: B = 2, S = 3, H = W = 12 (vector width 4) and H = W = 7 (width 1, a partial last workgroup) -- the smallest that
reach both vector paths and a ragged workgroup.  Only public functions of the binding and ``_host_rows`` are used.
"""
import numpy as np
import pytest
import torch

import photo_checks
import synth
import tolerances

pytestmark = pytest.mark.gpu

B, S = 2, 3
PER_MAP = ("device", "host", "upload")                  # [B,S,9]
SHARED = ("device", "shared", "shared_upload")          # [S,9] on the host; "device": the same rows repeated per map


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X (select CPU tests with -m 'not gpu')"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def native():
    from svbrdf_estimation_amd import _native
    _native._load()
    return _native


@pytest.fixture(scope="module", params=[12, 7], ids=["12x12", "7x7"])
def case(request, dev, native):
    """the inputs of one size, made once and never written"""
    H = request.param
    c = {"H": H, "maps_np": synth.make_maps(61, B, H, tiled_roughness=False)}
    c["maps"] = photo_checks.to_device(c["maps_np"], dev)
    c["target"] = photo_checks.to_device(synth.make_maps(62, B, H), dev)
    c["enc9"] = photo_checks.to_device(synth.make_maps(63, B, H)[:, 3:12] * 2 - 1, dev)      # a head output in [-1, 1)
    c["scenes"] = torch.from_numpy(photo_checks.scene_table(B, 17, n_random=1, n_specular=2))
    assert tuple(c["scenes"].shape) == (B, S, 9) and B * S <= native.host_scenes_max_rows()
    c["repeated"] = c["scenes"][0:1].expand(B, S, 9).contiguous()
    c["cot"] = photo_checks.to_device(synth.uniform01(64, (B, S, 3, H, H)) - np.float32(0.5), dev)
    c["photos"] = native.render_fwd(c["target"], c["scenes"].to(dev)).clamp(0.0, 1.0)
    c["weights"] = photo_checks.to_device(synth.uniform01(65, (B, S, H, H)), dev)
    c["noise"] = torch.from_numpy(synth.uniform01(66, (B, S)) * np.float32(0.05))
    torch.cuda.synchronize()
    return c


def _same(a, b):
    return (a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b))


def _all_forms_agree(native, monkeypatch, dev, call, scenes, forms, uploads=1, what=""):
    """``call(table) -> tuple of tensors (or None)`` with ``scenes`` (host [B,S,9]) in each of ``forms``: one launch each,
    ``uploads`` entries into upload_scene_table in the forms that upload and none in the others, every output bitwise
    that of the first form.  -> the first form's outputs"""
    entered = []
    real = native.upload_scene_table

    def counting(table, device):
        entered.append(tuple(table.shape))
        return real(table, device)

    monkeypatch.setattr(native, "upload_scene_table", counting)
    results = {}
    for form in forms:
        with monkeypatch.context() as m:
            if form.endswith("upload"):
                m.setattr(native, "_host_rows", 1)
            table = scenes.to(dev) if form == "device" else scenes[0].clone() if form.startswith("shared") else scenes.clone()
            del entered[:]
            before = native.launch_count()
            results[form] = call(table, form)
            launches = native.launch_count() - before
        print("%s %-13s launches %d, uploads %r" % (what, form, launches, entered))
        assert launches == 1, (what, form, launches)
        assert len(entered) == (uploads if form.endswith("upload") else 0), (what, form, entered)
    torch.cuda.synchronize()
    first = results[forms[0]]
    for form in forms[1:]:
        assert len(results[form]) == len(first)
        for i, (a, b) in enumerate(zip(results[form], first)):
            assert _same(a, b), "%s: output %d of form %r differs from form %r" % (what, i, form, forms[0])
    return first


def test_render_fwd_and_bwd(case, dev, native, oracle, monkeypatch):
    maps, cot = case["maps"], case["cot"]
    for scenes, forms in ((case["scenes"], PER_MAP), (case["repeated"], SHARED)):
        out, = _all_forms_agree(native, monkeypatch, dev, lambda t, f: (native.render_fwd(maps, t),), scenes, forms,
                                what="render_fwd")
        assert out.dtype == torch.float32 and tuple(out.shape) == (B, S, 3, case["H"], case["H"])
        tolerances.assert_render_strict(photo_checks.to_numpy(out), oracle.render_fwd(case["maps_np"], scenes.numpy()),
                                        "render_fwd, device table")
        grad, = _all_forms_agree(native, monkeypatch, dev, lambda t, f: (native.render_bwd(maps, t, cot),), scenes, forms,
                                 what="render_bwd")
        assert grad.shape == maps.shape and torch.isfinite(grad).all() and grad.abs().sum() > 0


def test_render_fwd_and_bwd_float64(case, dev, native, monkeypatch):
    """float64 maps: the table always ends on the device, by a plain copy -- the pinned ring is never entered"""
    maps, cot = case["maps"].double(), case["cot"].double()
    for scenes, forms in ((case["scenes"], PER_MAP), (case["repeated"], SHARED)):
        out, = _all_forms_agree(native, monkeypatch, dev, lambda t, f: (native.render_fwd(maps, t),), scenes, forms,
                                uploads=0, what="render_fwd f64")
        assert out.dtype == torch.float64 and tuple(out.shape) == (B, S, 3, case["H"], case["H"])
        assert torch.isfinite(out).all() and out.abs().sum() > 0
        grad, = _all_forms_agree(native, monkeypatch, dev, lambda t, f: (native.render_bwd(maps, t, cot),), scenes, forms,
                                 uploads=0, what="render_bwd f64")
        assert grad.dtype == torch.float64 and grad.shape == maps.shape and torch.isfinite(grad).all()


def test_render_inputs(case, dev, native, monkeypatch):
    maps, noise = case["maps"], case["noise"]
    clean, = _all_forms_agree(native, monkeypatch, dev, lambda t, f: (native.render_inputs(maps, t),), case["scenes"], PER_MAP,
                              what="render_inputs")
    assert tuple(clean.shape) == (B, S, 3, case["H"], case["H"]) and 0.0 <= clean.min() and clean.max() <= 1.0
    # the noise levels travel with the scenes: on the device with a device table, on the host with a host table, and
    # through the upload as a pair
    noisy, = _all_forms_agree(native, monkeypatch, dev,
                              lambda t, f: (native.render_inputs(maps, t, noise.to(dev) if f == "device" else noise.clone(),
                                                                 seed=5, offset=8),),
                              case["scenes"], PER_MAP, uploads=2, what="render_inputs + noise")
    assert not torch.equal(noisy, clean) and 0.0 <= noisy.min() and noisy.max() <= 1.0


@pytest.mark.parametrize("want_grad", [True, False], ids=["grad", "forward_only"])
@pytest.mark.parametrize("options", [{}, {"l1_weight": 0.1}, {"head": True}], ids=["plain", "l1", "head"])
def test_rendering_loss(case, options, want_grad, dev, native, monkeypatch):
    x = case["enc9"] if options.get("head") else case["maps"]
    loss, grad = _all_forms_agree(
        native, monkeypatch, dev, lambda t, f: native.rendering_loss(x, case["target"], t, want_grad=want_grad, **options),
        case["scenes"], PER_MAP, what="rendering_loss %r" % (options,))
    assert tuple(loss.shape) == (1,) and np.isfinite(loss.item()) and loss.item() > 0
    assert (grad.shape == x.shape and torch.isfinite(grad).all()) if want_grad else grad is None
    photo_checks.assert_scratch_is_zero(native)


@pytest.mark.parametrize("options", [{}, {"head": True}, {"weights": True}], ids=["plain", "head", "weights"])
def test_photo_loss(case, options, dev, native, monkeypatch):
    x = case["enc9"] if options.get("head") else case["maps"]
    if "weights" in options:
        options = dict(options, weights=case["weights"])
    loss, grad = _all_forms_agree(native, monkeypatch, dev, lambda t, f: native.photo_loss(x, case["photos"], t, **options),
                                  case["scenes"], PER_MAP, what="photo_loss %s" % sorted(options))
    assert tuple(loss.shape) == (1,) and np.isfinite(loss.item()) and loss.item() > 0
    assert grad.shape == x.shape and torch.isfinite(grad).all()
    photo_checks.assert_scratch_is_zero(native)


def test_rendering_loss_module_uploads_a_large_table_once(case, dev, native, monkeypatch):
    """losses.RenderingLoss on the ctypes path, both gradients wanted: two launches (the target's gradient is the same
    kernel with the roles swapped) on ONE hand-over of the table -- no upload by value, exactly one above the limit -- and
    bitwise the same loss and gradients either way"""
    from svbrdf_estimation_amd import _hostext, losses, renderers
    fn = losses.RenderingLoss(renderers.LocalRenderer())
    fn.random_configuration_count, fn.specular_configuration_count = 1, 2
    monkeypatch.setattr(_hostext, "_disabled", True)
    entered = []
    real = native.upload_scene_table

    def counting(table, device):
        entered.append(tuple(table.shape))
        return real(table, device)

    monkeypatch.setattr(native, "upload_scene_table", counting)
    results = []
    for limit, uploads in ((None, 0), (1, 1)):
        with monkeypatch.context() as m:
            if limit is not None:
                m.setattr(native, "_host_rows", limit)
            x, t = case["maps"].clone().requires_grad_(True), case["target"].clone().requires_grad_(True)
            torch.manual_seed(17)
            del entered[:]
            before = native.launch_count()
            loss = fn(x, t)
            launches = native.launch_count() - before
            loss.backward()
        print("RenderingLoss, row limit %s: launches %d, uploads %r" % (limit, launches, entered))
        assert launches == 2 and len(entered) == uploads, (limit, launches, entered)
        results.append((loss.detach(), x.grad, t.grad))
    torch.cuda.synchronize()
    for a, b in zip(*results):
        assert _same(a, b) and torch.isfinite(a).all()
    assert results[0][1].abs().sum() > 0 and results[0][2].abs().sum() > 0
