"""The head-fused photo loss on the device (csrc/svbrdf_photo_loss.hip: k_head_photo*, losses.HeadPhotoLoss):

    L = PhotoLoss(renderer, eps)(losses.decode_head(encoded9), photos, scenes)     in ONE launch, gradient w.r.t. encoded9

against the reference (tests/golden/g20_head_photo_loss.npz, written by tests/golden/make_golden_head_photo.py) and against
the C oracle's composition (tests/head_photo_checks.py), through HeadPhotoLoss and through the C ABI, with the scene table in
device memory and by value in the kernel arguments.  Bounds: tests/tolerances.py unchanged -- loss 1e-6 relative; gradient
1e-4 |b| + 1e-5 max|b|, widened by 2 |b - f64| for at most MAX_WIDENED_GRAD elements; tie pixels left out of the
element-wise comparison, within TIE_SLACK max|g|, at most MAX_TIE_PIXELS = 8 of them.  The inputs stay inside those caps
by the comparison values alone (tests/test_head_photo_loss_cpu.py: 0 tie pixels everywhere but sweep 2: 1, sweep 11: 6,
sweep 23: 1, the 256 x 256 case: 1, the fixture: 3).

Speed (test_fused_is_no_slower_than_the_unfused_composition; the figures of the last run on an MI355X are in
profiles/r11_head_photo_loss.txt): medians of event-timed steps at the configuration-2 shape, batches rotating through HBM,
one process.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import head_checks
import head_photo_checks as hp
import photo_checks
import synth
import tolerances
from photo_checks import assert_scratch_is_zero as _scratch_is_zero, to_device as _t, to_numpy as _np

pytestmark = pytest.mark.gpu
EPS = hp.EPS


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
def head_photo_loss():
    from svbrdf_estimation_amd import losses, renderers
    fn = losses.HeadPhotoLoss(renderers.LocalRenderer())
    assert fn.uses_fused_kernel() and fn.eps == EPS
    return fn


def _table(sc, host, dev):
    return torch.from_numpy(np.ascontiguousarray(sc, np.float32)) if host else _t(sc, dev)


def _call_abi(native, enc, photos, scenes, want_grad=True):
    return photo_checks.call_abi(native, enc, photos, scenes, EPS, want_grad, head=True)


def _four_ways(native, dev, head_photo_loss, enc, ph, sc):
    """C ABI / HeadPhotoLoss x device table / by-value table -> {how: (loss, grad)}, all four asserted bitwise equal"""
    d_enc, d_ph = _t(enc, dev), _t(ph, dev)
    results = {}
    for form, host in (("device table", False), ("by-value table", True)):
        table = _table(sc, host, dev)
        results["C ABI, " + form] = _call_abi(native, d_enc, d_ph, table)
        x = d_enc.clone().requires_grad_(True)
        l = head_photo_loss(x, d_ph, table)
        assert l.dim() == 0
        l.backward()
        results["HeadPhotoLoss, " + form] = (l.item(), _np(x.grad))
    first = results["C ABI, device table"]
    for how, (loss, grad) in results.items():       # one arithmetic, four ways in: the same bits
        assert loss == first[0] and np.array_equal(grad, first[1]), "%s differs from the device-table C ABI call" % how
    _scratch_is_zero(native)
    return results


def test_reference_fixture(dev, native, head_photo_loss, golden):
    g = golden("g20_head_photo_loss.npz")
    enc = head_checks.fixture_input(int(g["enc_seed"]), int(g["B"]), int(g["H"]))
    assert synth.checksum(enc) == str(g["enc_sha256"])
    ref = photo_checks.Reference(enc, g["photos"], g["scenes"], EPS, head=True)
    results = _four_ways(native, dev, head_photo_loss, enc, g["photos"], g["scenes"])
    print("[head-photo] g20: four ways in, bitwise equal: yes")
    for how, (loss, grad) in results.items():
        print("[head-photo] g20 %s: loss %.9g (reference %.9g, oracle %.9g), max|g| %.4e" % (
            how, loss, float(g["loss"]), ref.loss, np.abs(grad).max()))
        assert grad.shape == enc.shape
        tolerances.assert_loss_close(loss, g["loss"], "g20 %s vs the reference" % how)
        photo_checks.assert_photo_grad_close(grad, g["grad9"], g["grad9_f64"], ref.tie, "g20 %s vs the reference" % how)
        ref.assert_close(loss, grad, "g20 %s vs the oracle" % how)


def test_seeded_sweep_against_the_oracle(dev, native):
    cases = head_checks.sweep_cases()
    assert len(cases) == 24 and {c["H"] for c in cases} == set(head_checks.SWEEP_SIZES)
    for c in cases:
        enc, ph, sc = hp.sweep_inputs(c)
        what = "photo " + head_checks.sweep_name(c)
        ref = photo_checks.Reference(enc, ph, sc, head=True)
        d_enc, d_ph = _t(enc, dev), _t(ph, dev)
        loss, grad = _call_abi(native, d_enc, d_ph, _table(sc, c["host_table"], dev))
        assert grad.shape == enc.shape
        ref.assert_close(loss, grad, what)
        for host in (False, True):      # forward only: the same loss bit for bit, both table forms
            fwd, none = _call_abi(native, d_enc, d_ph, _table(sc, host, dev), want_grad=False)
            assert none is None and fwd == loss, (what, host, fwd, loss)
        _scratch_is_zero(native)
    print("[head-photo] sweep: forward-only loss bitwise equal to forward + adjoint in both table forms: yes (24 cases)")


@pytest.mark.parametrize("name", [c[0] for c in head_checks.POW2_CASES] + [hp.RAW_POW2 + "-raw"])
def test_power_of_two_widths_every_pixel(dev, native, oracle, name):
    raw = name.endswith("-raw")
    base = name[:-4] if raw else name
    _, B, H, nr, ns, host, _ = head_checks.POW2_CASES[[c[0] for c in head_checks.POW2_CASES].index(base)]
    assert H & (H - 1) == 0 and nr + ns == 9
    oracle.set_threads(min(16, oracle.max_threads()))
    enc, ph, sc = hp.pow2_inputs(base, raw=raw)
    if raw:
        assert ph.max() > 1.0, "the raw photographs should hold values the clamp would have cut"
    ref = photo_checks.Reference(enc, ph, sc, head=True)
    loss, grad = _call_abi(native, _t(enc, dev), _t(ph, dev), _table(sc, host, dev))
    ref.assert_close(loss, grad, "photo head pow2 " + name)
    _scratch_is_zero(native)


def _off(t, dev):
    """a copy of `t` whose storage starts 4 bytes behind a 16-byte boundary (tests/test_gpu_photo_loss.py)"""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    view = flat[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


def _raw_call(native, dev, entry, enc, ph, scenes, xrow, loss, grad):
    """the C ABI with buffers of the caller's, of exactly the element counts the kernel addresses"""
    B, _, H, W = enc.shape
    S = ph.shape[1]
    assert enc.numel() == B * 9 * H * W and grad.numel() == enc.numel() and ph.numel() == B * S * 3 * H * W
    assert scenes.numel() == B * S * 9 and xrow.numel() == W and loss.numel() == 1
    assert all(t.is_contiguous() for t in (enc, ph, scenes, xrow, grad))
    lib = native._load()
    ws = native._workspace(dev, lib.svbrdf_rendering_loss_workspace_bytes(B, S, H, W))
    rc = getattr(lib, entry)(enc.data_ptr(), ph.data_ptr(), scenes.data_ptr(), xrow.data_ptr(), ctypes.c_float(EPS),
                             loss.data_ptr(), grad.data_ptr(), ws.data_ptr(), ws.numel() * 8, B, S, H, W, native._stream(dev))
    assert rc == 0, lib.svbrdf_last_error()
    torch.cuda.synchronize()
    return loss.item(), _np(grad)


@pytest.mark.parametrize("H", [13, 17])
def test_every_device_pointer_four_bytes_off_alignment(dev, native, H):
    enc, ph, sc = hp.alignment_inputs(H)
    ref = photo_checks.Reference(enc, ph, sc, head=True)
    d_enc, d_ph, d_sc = _t(enc, dev), _t(ph, dev), _t(sc, dev)
    loss, grad = _call_abi(native, d_enc, d_ph, d_sc)
    ref.assert_close(loss, grad, "photo head alignment %d" % H)
    xr = native.xrow(dev, H)
    l_al, g_al = _raw_call(native, dev, hp.ENTRIES[0], d_enc, d_ph, d_sc, xr, torch.empty(1, device=dev), torch.empty_like(d_enc))
    assert l_al == loss and np.array_equal(g_al, grad)
    # every device pointer but the 8-byte-aligned scratch moved: the same one-pixel-per-lane path, the same bits
    l_off, g_off = _raw_call(native, dev, hp.ENTRIES[0], _off(d_enc, dev), _off(d_ph, dev), _off(d_sc, dev), _off(xr, dev),
                             _off(torch.zeros(1, device=dev), dev), _off(torch.zeros_like(d_enc), dev))
    assert l_off == loss and np.array_equal(g_off, grad)
    # ... and the by-value entry (its table is host memory)
    l_inl, g_inl = _raw_call(native, dev, hp.ENTRIES[1], _off(d_enc, dev), _off(d_ph, dev), torch.from_numpy(sc).contiguous(),
                             _off(xr, dev), _off(torch.zeros(1, device=dev), dev), _off(torch.zeros_like(d_enc), dev))
    assert l_inl == loss and np.array_equal(g_inl, grad)
    print("[head-photo] alignment %d: pointers 4 bytes off 16-byte alignment, bitwise equal to the aligned call: yes" % H)
    _scratch_is_zero(native)


def test_launch_count_reproducibility_scratch_and_non_finite_inputs(dev, native, head_photo_loss):
    enc, ph, sc = hp.argument_inputs()
    d_enc, d_ph, d_sc = _t(enc, dev), _t(ph, dev), _t(sc, dev)
    runs = []
    for scale in (None, 1.0, 2.5):
        x = d_enc.clone().requires_grad_(True)
        torch.cuda.synchronize()
        n0 = native.launch_count()
        loss = head_photo_loss(x, d_ph, d_sc)
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
    photo_checks.Reference(enc, ph, sc, head=True).assert_close(runs[0][0], runs[0][1], "photo head arguments case")
    with torch.no_grad():                           # no gradient wanted: the forward-only kernel, one launch
        n0 = native.launch_count()
        assert head_photo_loss(d_enc, d_ph, d_sc).item() == runs[0][0] and native.launch_count() - n0 == 1
    print("[head-photo] launches: backward() 1, (loss * 2.5).backward() 2, no_grad 1; two runs bitwise equal: yes")

    # NaN / +inf in one channel of every encoded group, NaN / inf / a value below -eps in the photos: NaN loss from both
    # kernels, scratch left zeroed, nothing sticks
    def poisoned(a, idx, v):
        b = a.copy()
        b[idx] = v
        return _t(b, dev)
    cases = []
    for ch, pix in ((0, (3, 3)), (1, (16, 2)), (3, (5, 11)), (5, (9, 9)), (8, (16, 16))):   # normal x, y, diffuse, roughness, specular
        for v in (np.nan, np.inf):
            cases.append(("enc[%d] = %s" % (ch, v), poisoned(enc, (ch % 2, ch) + pix, v), d_ph))
    cases += [("photo NaN", d_enc, poisoned(ph, (1, 4, 2, 16, 16), np.nan)), ("photo inf", d_enc, poisoned(ph, (0, 0, 0, 0, 0), np.inf)),
              ("photo < -eps", d_enc, poisoned(ph, (0, 3, 1, 5, 5), -0.5))]
    for what, bad_enc, bad_ph in cases:
        for want_grad in (True, False):
            l, _ = _call_abi(native, bad_enc, bad_ph, d_sc, want_grad=want_grad)
            assert np.isnan(l), (what, want_grad, l)
            _scratch_is_zero(native)
    l, g = _call_abi(native, d_enc, d_ph, d_sc)
    assert l == runs[0][0] and np.array_equal(g, runs[0][1])
    _scratch_is_zero(native)
    print("[head-photo] %d non-finite cases x 2 kernels: NaN loss, scratch zero, the next clean call bitwise as before: yes" % len(cases))


def test_gradient_of_each_encoded_group_in_isolation(dev, head_photo_loss):
    B, H = 2, 16
    enc = head_checks.interior(7350, B, H)
    sc = head_checks.scene_table(675, B, 2, 3)
    d_ph, d_sc = _t(hp.photographs(synth.make_maps(7351, B, H), sc), dev), _t(sc, dev)
    x = _t(enc, dev).requires_grad_(True)
    head_photo_loss(x, d_ph, d_sc).backward()
    full = x.grad
    assert full.abs().max() > 0
    order = ("normal", "diffuse", "roughness", "specular")
    sizes = [head_checks.GROUPS[n].stop - head_checks.GROUPS[n].start for n in order]
    assert sizes == [2, 3, 1, 3]
    for k, name in enumerate(order):
        parts = [t.clone() for t in torch.split(_t(enc, dev), sizes, dim=1)]
        parts[k].requires_grad_(True)
        head_photo_loss(torch.cat(parts, dim=1), d_ph, d_sc).backward()
        assert torch.equal(parts[k].grad, full[:, head_checks.GROUPS[name]]), name
        assert all(p.grad is None for i, p in enumerate(parts) if i != k)


def test_against_the_unfused_composition(dev, native, head_photo_loss):
    from svbrdf_estimation_amd import losses, renderers
    enc, ph, sc = hp.pow2_inputs("64_host")
    ref = photo_checks.Reference(enc, ph, sc, head=True)
    d_ph, table = _t(ph, dev), _table(sc, True, dev)
    x = _t(enc, dev).requires_grad_(True)
    fused = head_photo_loss(x, d_ph, table)
    fused.backward()
    x2 = _t(enc, dev).requires_grad_(True)
    unfused = losses.PhotoLoss(renderers.LocalRenderer(), EPS)(losses.decode_head(x2), d_ph, table)
    unfused.backward()
    print("[head-photo] fused %.9g, unfused composition %.9g, oracle %.9g" % (fused.item(), unfused.item(), ref.loss))
    ref.assert_close(fused.item(), _np(x.grad), "fused head photo loss 64_host")
    ref.assert_close(unfused.item(), _np(x2.grad), "unfused composition 64_host")
    tolerances.assert_loss_close(fused.item(), unfused.item(), "fused vs unfused composition")     # (not bitwise: torch's
    _scratch_is_zero(native)                                                                       # decode rounds differently)


def test_float64_and_second_order_take_the_composed_definition(dev, head_photo_loss):
    enc, ph, sc = hp.pow2_inputs("16_host")
    ref = photo_checks.Reference(enc, ph, sc, head=True)
    d_ph, d_sc = _t(ph, dev), _t(sc, dev)
    x64 = _t(enc, dev).double().requires_grad_(True)
    composed = head_photo_loss(x64, d_ph, d_sc)
    assert composed.dtype == torch.float64
    composed.backward()
    assert x64.grad.dtype == torch.float64
    tolerances.assert_loss_close(composed.item(), ref.loss64, "float64 composed vs the oracle's f64")
    photo_checks.assert_photo_grad_close(_np(x64.grad), ref.grad64, None, ref.tie, "float64 composed vs the oracle's f64")
    assert head_photo_loss(_t(enc, dev), d_ph.double(), d_sc).dtype == torch.float64       # double on either side
    # create_graph=True: differentiable, float32, and the first-order values are within the bounds
    x2 = _t(enc, dev).requires_grad_(True)
    g, = torch.autograd.grad(head_photo_loss(x2, d_ph, d_sc), x2, create_graph=True)
    assert g.requires_grad and g.dtype == torch.float32 and g.shape == x2.shape
    photo_checks.assert_photo_grad_close(_np(g), ref.grad, ref.grad64, ref.tie, "create_graph gradient vs the oracle")
    g.square().sum().backward()
    assert x2.grad is not None and torch.isfinite(x2.grad).all() and x2.grad.abs().max() > 0


def test_thirty_adam_steps_of_a_small_network(dev, native, head_photo_loss):
    """photos -> Conv2d(3, 9, 3) -> tanh -> HeadPhotoLoss against the same photos: self-supervised training on the input
    photos, one library launch per step"""
    from svbrdf_estimation_amd import synthesis
    B, count, H = 2, 5, 32
    truth = _t(synth.make_maps(61, B, H), dev)
    torch.manual_seed(79)
    photos = synthesis.render_inputs(truth, count, use_augmentation=True, noise=None)
    torch.manual_seed(79)
    table = torch.stack([synthesis.input_scene_table(count, True) for _ in range(B)], dim=0)
    assert photos.shape == (B, count, 3, H, H) and table.shape == (B, count, 9)
    torch.manual_seed(3)
    net = torch.nn.Conv2d(3, 9, 3, padding=1).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=0.01)
    first = photos[:, 0].contiguous()
    history = []
    for _ in range(30):
        opt.zero_grad(set_to_none=True)
        y = torch.tanh(net(first))
        torch.cuda.synchronize()
        n0 = native.launch_count()
        loss = head_photo_loss(y, photos, table)
        loss.backward()
        torch.cuda.synchronize()
        assert native.launch_count() - n0 == 1
        opt.step()
        history.append(loss.item())
    print("[head-photo] 30 Adam steps of Conv2d(3, 9, 3) + tanh: %.6f -> %.6f, one launch per step" % (history[0], history[-1]))
    assert np.isfinite(history).all() and history[-1] < history[0]
    _scratch_is_zero(native)


def test_fused_is_no_slower_than_the_unfused_composition(dev, native):
    """The unfused composition runs the 12-channel photo kernel -- the same scene loop -- plus the decode's elementwise
    passes and their backward: no margin.  The 12-channel kernel alone is reported, not compared (K3's head variant is
    slower than plain K3, README)."""
    res = hp.measure_head_photo_loss(dev, native)
    line = ("fused head photo loss %.2f us per step, unfused composition PhotoLoss(decode_head(x)) forward + backward %.2f us "
            "per step, 12-channel photo kernel alone %.2f us per launch (medians of event-timed steps; per round %s); fused at "
            "%.3f of 8 TB/s at the algorithmic bytes" % (res["head_photo_us"], res["composition_us"], res["photo12_us"],
                                                        res["rounds"], res["head_photo_frac_of_8TBps"]))
    print("[head-photo] config-2 shape (B = 8, 256 x 256, S = 9, by-value table, %d rotating batches): %s" % (res["sets"], line))
    out = os.environ.get("SVBRDF_RESULTS_DIR")      # where a measurement run keeps its figures (profiles/r11_head_photo_loss.txt)
    with open(os.path.join(out, "head_photo_loss.txt") if out else os.devnull, "w") as f:
        f.write("# tests/test_gpu_head_photo_loss.py::test_fused_is_no_slower_than_the_unfused_composition on %s\n" % res["device"])
        f.write(line + "\n")
    assert res["head_photo_us"] <= res["composition_us"], res
