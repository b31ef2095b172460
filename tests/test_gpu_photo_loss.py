"""The fused photo loss on the device (csrc/svbrdf_photo_loss.hip, losses.PhotoLoss):

    L = mean | log(render(scene[b,s], input[b]) + eps) - log(photo[b,s] + eps) |

against the reference (tests/golden/g18_photo_loss.npz, written by tests/golden/make_golden_photo.py) and against the C
oracle's composition (tests/photo_checks.py), through PhotoLoss and through the C ABI, with the scene table in device memory
and by value in the kernel arguments.  Bounds: tests/tolerances.py -- loss 1e-6 relative; gradient 1e-4 |b| + 1e-5 max|b|,
widened by 2 |b - f64| for at most MAX_WIDENED_GRAD elements; tie pixels (photo_checks: a non-structural term with
|delta_f64| < TIE_LEVEL) left out of the element-wise comparison, within TIE_SLACK max|g|, at most MAX_TIE_PIXELS = 8 of
them, max(8, 2e-6 terms) at size.  The inputs were chosen with the oracle alone so that the caps hold (counts: 0 for the three
seeded cases, raw and clamped photos; 1 for the 48 x 48 case; 13 at 512 x 512 with 32 scenes, cap 50; 14 at B = 8,
256 x 256, cap 28).

Speed (test_photo_loss_is_no_slower_than_k3, figures of the last run on an MI355X in profiles/r09_photo_loss.txt): median of
event-timed launches at the configuration-2 shape, batches rotating beyond the Infinity Cache, same process, same box: the
photo loss takes no longer per launch than K3's rendering loss on the same maps.
"""
import os

import numpy as np
import pytest
import torch

import photo_checks
import synth
import tolerances
from photo_checks import assert_scratch_is_zero as _scratch_is_zero, scene_table as _table, to_device as _t, to_numpy as _np

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 0.1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X (select CPU tests with -m 'not gpu')"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def native():
    from svbrdf_estimation_amd import _native
    _native._load()
    return _native


@pytest.fixture(scope="module")
def photo_loss():
    from svbrdf_estimation_amd import losses, renderers
    fn = losses.PhotoLoss(renderers.LocalRenderer())
    assert fn.uses_fused_kernel() and fn.eps == EPS
    return fn


def _edge_maps(seed):
    """roughness below the clamp (rows 0-3 of item 0: zero roughness gradient) and normals facing away from every light
    (rows 5-8 of item 1: n.wi < 0, radiance exactly 0)"""
    m = synth.make_maps(seed, 2, 64)
    m[0, 6:9, :4, :] = 0.0004
    m[1, 0:3, 5:9, :] = np.array([0.0, 0.0, -1.0], np.float32)[:, None, None]      # every light is above the patch
    return m


def _case(name, oracle):
    """-> input, photos, scenes (numpy), cap on tie pixels"""
    cap = tolerances.MAX_TIE_PIXELS
    if name.startswith("seeded"):
        a, b, seed = {"seeded_123": (1, 2, 123), "seeded_7": (3, 4, 7), "seeded_11": (5, 6, 11)}[name.split("-")[0]]
        inp, tgt, sc = synth.make_maps(a, 2, 64), synth.make_maps(b, 2, 64), _table(2, seed)
        ph = oracle.render_fwd(tgt, sc)
        return inp, (np.clip(ph, 0.0, 1.0) if name.endswith("-clamped") else ph), sc, cap
    if name == "one_scene":
        inp, tgt, sc = synth.make_maps(21, 2, 64), synth.make_maps(22, 2, 64), _table(2, 31, 1, 0)
    elif name == "size_48":
        inp, tgt, sc = synth.make_maps(23, 2, 48), synth.make_maps(24, 2, 48), _table(2, 33)
    elif name == "untied_roughness":
        inp, tgt = synth.make_maps(25, 2, 64, tiled_roughness=False), synth.make_maps(26, 2, 64, tiled_roughness=False)
        sc = _table(2, 35)
    elif name == "clamps":
        inp, tgt, sc = _edge_maps(27), _edge_maps(28), _table(2, 37)
    elif name == "512_s32":
        inp, tgt, sc = synth.make_maps(29, 1, 512), synth.make_maps(30, 1, 512), _table(1, 39, 11, 21)
        cap = max(cap, int(2e-6 * 32 * 3 * 512 * 512))
    elif name == "at_size":
        inp, tgt, sc = synth.make_maps(11, 8, 256), synth.make_maps(12, 8, 256), _table(8, 313)
        return inp, oracle.render_fwd(tgt, sc), sc, max(cap, int(2e-6 * 8 * 9 * 3 * 256 * 256))
    else:
        raise KeyError(name)
    return inp, np.clip(oracle.render_fwd(tgt, sc), 0.0, 1.0), sc, cap


def _check_against(native, dev, what, inp, ph, sc, ref_loss, ref_grad, f64_grad, delta64, cap, photo_loss=None):
    """device table and by-value table, C ABI and (photo_loss given) PhotoLoss: each within the bounds of `ref`"""
    tmap = photo_checks.tie_map(inp, ph, sc, delta64)
    d_in, d_ph, d_sc, h_sc = _t(inp, dev), _t(ph, dev), _t(sc, dev), torch.from_numpy(np.ascontiguousarray(sc))
    results = {}
    for form, table in (("device table", d_sc), ("by-value table", h_sc)):
        loss, grad = native.photo_loss(d_in, d_ph, table, EPS)
        results["C ABI, " + form] = (loss.item(), _np(grad))
        if photo_loss is not None:
            x = d_in.clone().requires_grad_(True)
            l = photo_loss(x, d_ph, table)
            assert l.dim() == 0
            l.backward()
            results["PhotoLoss, " + form] = (l.item(), _np(x.grad))
    for how, (loss, grad) in results.items():
        print("[photo-loss] %s, %s: loss %.9g (ref %.9g), max|g| %.4e" % (what, how, loss, ref_loss, np.abs(grad).max()))
        tolerances.assert_loss_close(loss, ref_loss, "%s %s loss" % (what, how))
        photo_checks.assert_photo_grad_close(grad, ref_grad, f64_grad, tmap, "%s %s" % (what, how), max_ties=cap)
    first = results["C ABI, device table"]
    for how, (loss, grad) in results.items():       # one arithmetic, four ways in: the same bits
        assert loss == first[0] and np.array_equal(grad, first[1]), "%s: %s differs from the device-table C ABI call" % (what, how)
    _scratch_is_zero(native)
    return first


def test_reference_fixture(dev, native, photo_loss, golden):
    g = golden("g18_photo_loss.npz")
    inp = synth.make_maps(int(g["input_seed"]), int(g["B"]), int(g["H"]))
    assert synth.checksum(inp) == str(g["input_sha256"])
    _, _, delta64 = photo_checks.oracle_photo_loss(inp, g["photos"], g["scenes"], EPS, f64=True, want_grad=False)
    _check_against(native, dev, "g18 vs the reference", inp, g["photos"], g["scenes"], float(g["loss"]), g["grad_input"],
                   g["grad_input_f64"], delta64, tolerances.MAX_TIE_PIXELS, photo_loss)
    # ... and against the oracle's composition on the same inputs
    l32, g32, _ = photo_checks.oracle_photo_loss(inp, g["photos"], g["scenes"], EPS)
    _, g64, _ = photo_checks.oracle_photo_loss(inp, g["photos"], g["scenes"], EPS, f64=True)
    _check_against(native, dev, "g18 vs the oracle", inp, g["photos"], g["scenes"], l32, g32, g64, delta64,
                   tolerances.MAX_TIE_PIXELS)


@pytest.mark.parametrize("name", ["seeded_123", "seeded_123-clamped", "seeded_7", "seeded_7-clamped", "seeded_11",
                                  "seeded_11-clamped", "one_scene", "size_48", "untied_roughness", "clamps", "512_s32"])
def test_against_the_oracle(dev, native, photo_loss, oracle, name):
    inp, ph, sc, cap = _case(name, oracle)
    l32, g32, _ = photo_checks.oracle_photo_loss(inp, ph, sc, EPS)
    _, g64, delta64 = photo_checks.oracle_photo_loss(inp, ph, sc, EPS, f64=True)
    loss, grad = _check_against(native, dev, name, inp, ph, sc, l32, g32, g64, delta64, cap,
                                photo_loss if name != "512_s32" else None)
    d_in, d_ph, d_sc = _t(inp, dev), _t(ph, dev), _t(sc, dev)
    # forward only: the same loss bit for bit, both table forms; nothing left in the scratch
    for table in (d_sc, torch.from_numpy(sc)):
        l, g = native.photo_loss(d_in, d_ph, table, EPS, want_grad=False)
        assert g is None and l.item() == loss, (name, l.item(), loss)
    _scratch_is_zero(native)
    if name == "one_scene":         # [B,3,H,W] photos mean S = 1
        x = d_in.clone().requires_grad_(True)
        l = photo_loss(x, d_ph[:, 0], d_sc)
        l.backward()
        assert l.item() == loss and np.array_equal(_np(x.grad), grad)
    if name == "clamps":
        assert not grad[0, 6:9, :4, :].any(), "roughness below the clamp must have zero gradient"
        # both sides of a term exactly eps where the light is behind the surface and the photo is 0: no gradient at all
        assert (ph[1, :, :, 5:9, :] == 0.0).all() and not grad[1, :, 5:9, :].any()
    if name == "seeded_123":
        # a misaligned pointer (4-byte aligned only): the same one-pixel-per-lane path, the same bits
        def off(t):
            flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
            view = flat[1:].view(t.shape)
            view.copy_(t)
            assert view.data_ptr() % 16 == 4
            return view
        l, g = native.photo_loss(off(d_in), off(d_ph), off(d_sc), EPS)
        assert l.item() == loss and np.array_equal(_np(g), grad)
        # Scene objects instead of a table
        from svbrdf_estimation_amd import environment
        x = d_in.clone().requires_grad_(True)
        l = photo_loss(x, d_ph, [environment.scenes_from_table(torch.from_numpy(sc[b])) for b in range(sc.shape[0])])
        l.backward()
        assert l.item() == loss and np.array_equal(_np(x.grad), grad)


def test_at_size_against_the_oracle_all_pixels(dev, native, oracle):
    inp, ph, sc, cap = _case("at_size", oracle)
    l32, g32, _ = photo_checks.oracle_photo_loss(inp, ph, sc, EPS)
    _, g64, delta64 = photo_checks.oracle_photo_loss(inp, ph, sc, EPS, f64=True)
    print("[photo-loss] at size: cap on tie pixels %d" % cap)
    _check_against(native, dev, "B=8 256x256 S=9", inp, ph, sc, l32, g32, g64, delta64, cap)


def test_photos_from_synthesis_are_accepted_end_to_end(dev, native, photo_loss):
    """photos and scene table as synthesis.render_inputs makes them (its table is drawn from torch's global generator:
    the same seed gives it again), fitted maps differ from the photographed ones"""
    from svbrdf_estimation_amd import synthesis
    B, count, H = 2, 5, 64
    truth, start = _t(synth.make_maps(41, B, H), dev), synth.make_maps(42, B, H)
    torch.manual_seed(77)
    photos = synthesis.render_inputs(truth, count, use_augmentation=True, noise=None)
    torch.manual_seed(77)
    table = torch.stack([synthesis.input_scene_table(count, True) for _ in range(B)], dim=0)
    assert photos.shape == (B, count, 3, H, H) and table.shape == (B, count, 9)
    x = _t(start, dev).requires_grad_(True)
    loss = photo_loss(x, photos, table)
    loss.backward()
    ph = _np(photos)
    l32, g32, _ = photo_checks.oracle_photo_loss(start, ph, table.numpy(), EPS)
    _, g64, d64 = photo_checks.oracle_photo_loss(start, ph, table.numpy(), EPS, f64=True)
    tolerances.assert_loss_close(loss.item(), l32, "synthesis photos")
    photo_checks.assert_photo_grad_close(_np(x.grad), g32, g64, photo_checks.tie_map(start, ph, table.numpy(), d64),
                                         "synthesis photos")
    # the photographed maps themselves fit their own noise-free photos, up to the photos' clamp to [0, 1]: every term
    # whose photo value is below 1 is exactly 0 (K1 and the loss kernel shade alike)
    at_truth = photo_loss(truth, photos, table).item()
    print("[photo-loss] synthesis photos: loss %.6f at the start maps, %.6f at the photographed maps" % (loss.item(), at_truth))
    assert at_truth < loss.item()
    unclamped = (photos < 1.0).all(dim=2, keepdim=True).expand_as(photos)
    rendered = native.render_fwd(truth, table)
    assert torch.equal(rendered[unclamped], photos[unclamped])


def test_gradient_of_each_map_in_isolation(dev, photo_loss, oracle):
    from svbrdf_estimation_amd import utils
    inp, ph, sc, _ = _case("seeded_7-clamped", oracle)
    d_ph, d_sc = _t(ph, dev), _t(sc, dev)
    x = _t(inp, dev).requires_grad_(True)
    photo_loss(x, d_ph, d_sc).backward()
    full = x.grad
    for k, name in enumerate(("normals", "diffuse", "roughness", "specular")):
        parts = [t.clone() for t in torch.split(_t(inp, dev), (3, 3, 3, 3), dim=1)]
        parts[k].requires_grad_(True)
        photo_loss(utils.pack_svbrdf(*parts), d_ph, d_sc).backward()
        assert torch.equal(parts[k].grad, full[:, 3 * k:3 * k + 3]), name
        assert all(p.grad is None for i, p in enumerate(parts) if i != k)


def test_launch_count_reproducibility_scratch_and_non_finite_inputs(dev, native, photo_loss, oracle):
    inp, ph, sc, _ = _case("seeded_11", oracle)
    d_in, d_ph, d_sc = _t(inp, dev), _t(ph, dev), _t(sc, dev)
    runs = []
    for scale in (None, 1.0, 2.5):
        x = d_in.clone().requires_grad_(True)
        torch.cuda.synchronize()
        n0 = native.launch_count()
        loss = photo_loss(x, d_ph, d_sc)
        if scale is None:
            loss.backward()                         # upstream gradient 1.0: the kernel's buffer is the gradient
        else:
            (loss * scale).backward()               # an upstream gradient autograd made: applied by svbrdf_scale_inplace
        torch.cuda.synchronize()
        launches = native.launch_count() - n0
        assert launches == (1 if scale is None else 2), (scale, launches)
        runs.append((loss.item(), _np(x.grad)))
        _scratch_is_zero(native)
    assert runs[0][0] == runs[1][0] == runs[2][0]
    assert np.array_equal(runs[0][1], runs[1][1])                               # two runs: bitwise equal
    assert np.array_equal(runs[2][1], runs[0][1] * np.float32(2.5))
    with torch.no_grad():                           # no gradient wanted: the forward-only kernel, one launch
        n0 = native.launch_count()
        assert photo_loss(d_in, d_ph, d_sc).item() == runs[0][0] and native.launch_count() - n0 == 1
    # NaN / inf in the maps or the photos, a photo value below -eps: NaN loss, scratch left zeroed, nothing sticks
    def poisoned(a, idx, v):
        b = a.copy()
        b[idx] = v
        return _t(b, dev)
    cases = [(poisoned(inp, (-1, 4, -1, -1), np.nan), d_ph), (poisoned(inp, (0, 0, 3, 3), np.inf), d_ph),
             (poisoned(inp, (1, 7, 9, 9), np.nan), d_ph), (d_in, poisoned(ph, (1, 8, 2, 63, 63), np.nan)),
             (d_in, poisoned(ph, (0, 0, 0, 0, 0), np.inf)), (d_in, poisoned(ph, (0, 4, 1, 5, 5), -0.5))]
    for bad_in, bad_ph in cases:
        for want_grad in (True, False):
            l, _ = native.photo_loss(bad_in, bad_ph, d_sc, EPS, want_grad=want_grad)
            assert np.isnan(l.item())
            _scratch_is_zero(native)
    l, g = native.photo_loss(d_in, d_ph, d_sc, EPS)
    assert l.item() == runs[0][0] and np.array_equal(_np(g), runs[0][1])
    _scratch_is_zero(native)


def test_float64_and_second_order_take_the_composed_definition(dev, photo_loss, oracle):
    inp, ph, sc, _ = _case("seeded_123-clamped", oracle)
    d_ph, d_sc = _t(ph, dev), _t(sc, dev)
    x = _t(inp, dev).requires_grad_(True)
    fused = photo_loss(x, d_ph, d_sc)
    fused.backward()
    x64 = _t(inp, dev).double().requires_grad_(True)
    composed = photo_loss(x64, d_ph, d_sc)
    assert composed.dtype == torch.float64
    composed.backward()
    _, g64, d64 = photo_checks.oracle_photo_loss(inp, ph, sc, EPS, f64=True)
    tolerances.assert_loss_close(fused.item(), composed.item(), "fused vs float64 composed")
    # the float64 composed gradient is the comparison value here; its own error is its distance from the oracle's float64
    photo_checks.assert_photo_grad_close(_np(x.grad), _np(x64.grad), g64, photo_checks.tie_map(inp, ph, sc, d64),
                                         "fused vs float64 composed")
    # create_graph=True: differentiable, and the first-order values are the composed ones
    x2 = _t(inp, dev).requires_grad_(True)
    g, = torch.autograd.grad(photo_loss(x2, d_ph, d_sc), x2, create_graph=True)
    assert g.requires_grad and g.dtype == torch.float32
    photo_checks.assert_photo_grad_close(_np(g), _np(x64.grad), g64, photo_checks.tie_map(inp, ph, sc, d64),
                                         "create_graph gradient vs float64 composed")
    g.square().sum().backward()
    assert x2.grad is not None and torch.isfinite(x2.grad).all() and x2.grad.abs().max() > 0


def test_fifty_adam_steps_lower_the_loss(dev, photo_loss, oracle):
    B, H = 2, 64
    truth = synth.make_maps(51, B, H)
    sc = _table(B, 53)
    photos = _t(np.clip(oracle.render_fwd(truth, sc), 0.0, 1.0), dev)
    start = truth.copy()
    start[:, 3:] = np.clip(start[:, 3:] + 0.15 * (synth.uniform01(55, start[:, 3:].shape) - 0.5), 0.02, 0.98)
    x = _t(start, dev).requires_grad_(True)
    opt = torch.optim.Adam([x], lr=0.01)
    d_sc = _t(sc, dev)
    history = []
    for _ in range(50):
        opt.zero_grad(set_to_none=True)
        loss = photo_loss(x, photos, d_sc)
        loss.backward()
        opt.step()
        with torch.no_grad():
            x[:, 3:].clamp_(0.0, 1.0)
        history.append(loss.item())
    print("[photo-loss] 50 Adam steps: %.6f -> %.6f" % (history[0], history[-1]))
    assert np.isfinite(history).all() and history[-1] < history[0]


def test_photo_loss_is_no_slower_than_k3(dev, native):
    """K3 is the parent's unchanged kernel and does strictly more arithmetic per pixel-render (two shadings, where this
    kernel has one shading and three loads): no margin."""
    res = photo_checks.measure_photo_loss_against_k3(dev, native)
    print("[photo-loss] config-2 shape, median us per launch: photo loss %.2f, K3 rendering loss %.2f (rounds %s); "
          "%.3f of 8 TB/s at the algorithmic bytes" % (res["photo_loss_us"], res["k3_us"], res["rounds"],
                                                      res["photo_loss_frac_of_8TBps"]))
    out = os.environ.get("SVBRDF_RESULTS_DIR")      # where a measurement run keeps its figures (profiles/r09_photo_loss.txt)
    with open(os.path.join(out, "photo_loss_vs_k3.txt") if out else os.devnull, "w") as f:
        f.write("# tests/test_gpu_photo_loss.py::test_photo_loss_is_no_slower_than_k3 on %s\n" % res["device"])
        f.write("photo loss %.2f us per launch, K3 rendering loss %.2f us per launch (medians of event-timed launches; "
                "per round %s)\n" % (res["photo_loss_us"], res["k3_us"], res["rounds"]))
    assert res["photo_loss_us"] <= res["k3_us"], res
