"""The smoothness prior across pixels of the photo fit (csrc/svbrdf_photo_fit_smooth.hip: k_smooth_step*, k_smooth_joint*;
svbrdf_photo_fit_smooth_adam_step[_scene_grad]; fitting.smoothness, composed_step(smooth=), PhotoFit(smooth=)), everything
that needs no GPU:

  * fitting.smoothness against a hand-written double sum, and its autograd gradient against the test oracle's c k;
  * composed_step(smooth=) in float64 is Adam applied by hand to (photo gradient + prior gradient); None and all zeros are
    today's composed_step bit for bit; a pixel no photograph sees stays bit for bit without the prior and moves with it;
    the hole experiment with the toy renderer;
  * argument validation; header, library and binding agree; every bad argument of both entries is rejected before anything
    is launched, the buffers untouched;
  * the four kernels compiled with the Makefile's flags: no scratch, no packed fp32, at most 128 VGPRs, the update's 12
    divisions and 12 square roots, 48 neighbour loads behind wave-uniform branches.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import photo_fit_checks as fc
import photo_fit_pose_checks as jc
import photo_fit_smooth_checks as sm
import synth
import unit_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = "svbrdf_photo_fit_smooth"
needs_hipcc = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs /opt/rocm/bin/hipcc (cross-compiles gfx950)")
OTHER_KERNELS = ("k_fit_maps", "k_fit_run", "k_joint_fit", "k_pose", "k_exposure", "k_photo_loss", "k_head_photo", "wphoto")


@pytest.fixture(scope="module")
def lib():
    from svbrdf_estimation_amd import _native
    return _native._load()


# ------------------------------------------------------------------------------------------------ smoothness, the specification

def _hand_sum(x, lam):
    """R(x) written out: Python floats, one term at a time"""
    B, C, H, W = x.shape
    total = 0.0
    for ch in range(C):
        tv = 0.0
        for b in range(B):
            for i in range(H):
                for j in range(W):
                    if j + 1 < W:
                        tv += abs(float(x[b, ch, i, j + 1]) - float(x[b, ch, i, j]))
                    if i + 1 < H:
                        tv += abs(float(x[b, ch, i + 1, j]) - float(x[b, ch, i, j]))
        total += float(lam[ch]) * tv / (B * H * W)
    return total


@pytest.mark.parametrize("B,H,W", ((1, 1, 1), (2, 2, 2), (2, 3, 5)))
def test_smoothness_is_the_hand_written_sum(B, H, W):
    from svbrdf_estimation_amd import fitting
    x = synth.uniform01(300 + H * W, (B, 12, H, W)).astype(np.float64)
    lam = np.linspace(0.0, 1.1, 12)
    got = fitting.smoothness(torch.from_numpy(x), lam)
    assert got.dim() == 0 and got.dtype == torch.float64
    want = _hand_sum(x, lam)
    assert abs(got.item() - want) <= 1e-14 * max(want, 1.0), (got.item(), want)
    if H * W == 1:
        assert got.item() == 0.0                                    # no neighbours
    # four values: one per map group, expanded x 3
    four = fitting.smoothness(torch.from_numpy(x), [0.0, 0.5, 0.25, 1.0])
    assert abs(four.item() - _hand_sum(x, np.repeat([0.0, 0.5, 0.25, 1.0], 3))) <= 1e-14
    # no wrap-around and no coupling between items: items reversed, rows and columns flipped, the value stands
    again = fitting.smoothness(torch.from_numpy(x[::-1, :, ::-1, ::-1].copy()), lam)
    assert abs(again.item() - want) <= 1e-14 * max(want, 1.0)


def test_smoothness_gradient_is_the_oracles_c_k():
    """autograd through the stock ops against the restatement's c k on float32 maps with ties (multiples of 1/8 on half of
    the planes): within 2^-22 relative -- a partial sum of +-c rounds once, at 3 c (autograd adds the four contributions one
    by one; 2 c and 4 c are exact), 2^-24; the product c k rounds once, 2^-24; the rest is margin.  Where k = 0 the oracle
    has an exact 0 and so must autograd: +c - c."""
    from svbrdf_estimation_amd import fitting
    B, H, W = 2, 9, 11
    x = synth.uniform01(41, (B, 12, H, W)).astype(np.float32)
    x[:, ::2] = np.round(x[:, ::2] * np.float32(8)) / np.float32(8)
    lam = sm.LAMBDA
    c, k, t = sm.prior_term(x, lam)
    assert set(np.unique(k[:, lam != 0]).astype(int)) == set(range(-4, 5))
    leaf = torch.from_numpy(x).requires_grad_(True)
    fitting.smoothness(leaf, lam).backward()
    got = leaf.grad.numpy()
    assert got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - t.astype(np.float64))
    assert (err <= 2.0 ** -22 * np.abs(t.astype(np.float64))).all(), (err / np.maximum(np.abs(t), 1e-30)).max()
    assert (got[k == 0] == 0).all() and (got[:, lam == 0] == 0).all()
    print("[smooth] autograd vs c k: worst relative error %.3g (bound 2^-22 = %.3g)" % (
        (err[t != 0] / np.abs(t[t != 0])).max(), 2.0 ** -22))


def test_oracle_sign_sum_rules():
    """the restatement itself on a hand-made plane: borders contribute 0, ties 0, a NaN makes its four neighbours' k NaN, two
    equal infinities give 0, and nothing couples two items or two channels"""
    from svbrdf_estimation_amd import fitting
    x = np.zeros((2, 12, 3, 3), np.float32)
    x[0, 4] = [[1, 2, 3], [4, 5, 6], [7, 8, 9]]
    k = sm.sign_sum(x)
    assert (k[0, 4] == [[-2, -1, 0], [-1, 0, 1], [0, 1, 2]]).all() and not k[1].any() and not k[0, :4].any()
    # and the specification says the same: with lambda = B H W = 18 on every plane its gradient IS k
    leaf = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    fitting.smoothness(leaf, [18.0] * 12).backward()
    assert (leaf.grad.numpy() == k).all()
    x[0, 4, 1, 1] = np.nan
    k = sm.sign_sum(x)
    assert np.isnan(k[0, 4, 1, 1]) and np.isnan(k[0, 4, 0, 1]) and np.isnan(k[0, 4, 1, 0]) and np.isnan(k[0, 4, 1, 2]) and np.isnan(k[0, 4, 2, 1])
    assert np.isnan(k).sum() == 5
    x[0, 4] = np.inf
    assert not sm.sign_sum(x).any()
    g = synth.uniform01(3, x.shape).astype(np.float32) - np.float32(0.5)
    g[0, 0, 0, 0] = -0.0
    lam = np.zeros(12, np.float32)
    assert fc.same_bits(sm.smooth_gradient(g, x, lam), g) and np.signbit(sm.smooth_gradient(g, x, lam)[0, 0, 0, 0])


# ------------------------------------------------------------------------------------------------ composed_step, PhotoFit

def _toy_problem(dtype, H=8):
    from svbrdf_estimation_amd import environment
    B, S = 2, 3
    maps = torch.from_numpy(synth.make_maps(41, B, H)).to(dtype)
    torch.manual_seed(5)
    table = torch.stack([environment.scene_table(1, S - 1) for _ in range(B)])
    photos = (torch.rand(B, S, 3, H, H) * 0.2).to(dtype)
    weights = torch.from_numpy(fc.wp.weight_field(77, B, S, H))
    return maps, photos, table, weights


def test_composed_step_in_float64_is_adam_by_hand_on_both_gradients():
    from svbrdf_estimation_amd import fitting, losses
    maps, photos, table, weights = _toy_problem(torch.float64)
    lam = [0.0, 0.02, 0.3, 0.05]
    lr, b1, b2, eps = 0.05, 0.9, 0.999, 1e-8
    u = synth.uniform01(9, (2,) + tuple(maps.shape)).astype(np.float64)
    m0, v0 = torch.from_numpy((u[0] - 0.5) * 2e-3), torch.from_numpy(u[1] * 1e-5)
    for t in (1, 3):
        x = maps.clone().requires_grad_(True)
        photo = losses.PhotoLoss(fc.ToyRenderer())(x, photos, table, weights)
        g, = torch.autograd.grad(photo, x)
        p, = torch.autograd.grad(fitting.smoothness(x, lam), x)
        assert p[:, :3].abs().max() == 0 and p[:, 3:].abs().max() > 0
        g = g + p
        m = b1 * m0 + (1 - b1) * g
        v = b2 * v0 + (1 - b2) * g * g
        want = maps - (lr / (1 - b1 ** t)) * m / (v.sqrt() / np.sqrt(1 - b2 ** t) + eps)
        want[:, 3:] = want[:, 3:].clamp(0.0, 1.0)
        xm, em, ev = maps.clone(), m0.clone(), v0.clone()
        loss = fitting.composed_step(xm, em, ev, t, photos, table, weights, lr=lr, betas=(b1, b2), eps=eps, bounds=fc.BOUNDS_FIT,
                                     renderer=fc.ToyRenderer(), smooth=lam)
        assert torch.equal(loss, photo.detach())                    # the loss returned is the photo term
        for got, exp in ((xm, want), (em, m), (ev, v)):
            assert (got - exp).abs().max().item() <= 1e-14, t


def test_no_prior_and_all_zeros_are_todays_composed_step_bit_for_bit():
    from svbrdf_estimation_amd import fitting
    maps, photos, table, weights = _toy_problem(torch.float32)
    outs = []
    for smooth in ("absent", None, [0.0] * 4, np.zeros(12)):
        x, m, v = maps.clone(), torch.zeros_like(maps), torch.zeros_like(maps)
        kw = {} if isinstance(smooth, str) else dict(smooth=smooth)
        for t in (1, 2):
            loss = fitting.composed_step(x, m, v, t, photos, table, weights, lr=fc.LR, bounds=fc.BOUNDS_FIT, renderer=fc.ToyRenderer(), **kw)
        outs.append((loss, x, m, v))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert fc.same_bits(a.numpy(), b.numpy())
    # and PhotoFit: None and zeros take the path without the prior
    for smooth in (None, [0.0] * 12):
        fit = fitting.PhotoFit(maps.clone(), lr=fc.LR, bounds=fc.BOUNDS_FIT, renderer=fc.ToyRenderer(), smooth=smooth)
        assert fit._smooth_c is None
        fit.step(photos, table, weights)
        fit.step(photos, table, weights)
        assert fc.same_bits(fit.maps.numpy(), outs[0][1].numpy())


def test_a_pixel_no_photograph_sees_stays_without_the_prior_and_moves_with_it():
    from svbrdf_estimation_amd import fitting
    maps, photos, table, weights = _toy_problem(torch.float32)
    weights = weights.clone()
    weights[:, :, 3, 4] = 0.0
    for i, j in ((2, 4), (4, 4), (3, 3), (3, 5)):
        maps[:, 3:, i, j] = 0.25
    maps[:, 3:, 3, 4] = 0.5                                         # above its four neighbours in d, r, s: k = +4, no tie
    without = fitting.PhotoFit(maps.clone(), lr=fc.LR, bounds=fc.BOUNDS_FIT, renderer=fc.ToyRenderer())
    with_prior = fitting.PhotoFit(maps.clone(), lr=fc.LR, bounds=fc.BOUNDS_FIT, renderer=fc.ToyRenderer(), smooth=[0.0, 0.01, 0.01, 0.01])
    for _ in range(3):
        without.step(photos, table, weights)
        with_prior.step(photos, table, weights)
    assert fc.same_bits(without.maps[:, :, 3, 4].numpy(), maps[:, :, 3, 4].numpy())       # g = 0, m = 0: bit for bit
    assert not without.exp_avg[:, :, 3, 4].any()
    assert (with_prior.maps[:, 3:, 3, 4] != maps[:, 3:, 3, 4]).all()                       # d, r, s moved
    assert fc.same_bits(with_prior.maps[:, :3, 3, 4].numpy(), maps[:, :3, 3, 4].numpy())   # lambda = 0 on the normals
    seen = (weights.amin(dim=1, keepdim=True) > 0).expand(-1, 9, -1, -1)
    assert seen.any() and (without.maps[:, 3:] != maps[:, 3:])[seen].any()                 # the seen pixels move either way


def test_hole_experiment_with_the_toy_renderer():
    """The experiment of the feature on the CPU: 16 x 16, truth in constant 8 x 8 cells, weights 0 on [2:6, 2:6] in all 5
    photos, start = truth + jitter, Adam lr 0.01, 200 steps, float32.  Without the prior the hole stays at its start
    value; with lambda = 0.01 on d, r, s its error is strictly below that."""
    from svbrdf_estimation_amd import environment, fitting
    H, S = 16, 5
    truth, start, weights, mask = sm.hole_problem(H, 8, (2, 6), S)
    torch.manual_seed(5)
    table = torch.stack([environment.scene_table(2, 3)])
    tt, w = torch.from_numpy(truth), torch.from_numpy(weights)
    toy = fc.ToyRenderer()
    scenes = environment.scenes_from_table(table[0])
    photos = torch.stack([toy.render(s, tt)[0] for s in scenes]).unsqueeze(0)
    errs = {}
    for name, lam in (("without", None), ("with", [0.0, 0.01, 0.01, 0.01])):
        fit = fitting.PhotoFit(torch.from_numpy(start.copy()), lr=0.01, bounds=fc.BOUNDS_FIT, renderer=toy, smooth=lam)
        for _ in range(200):
            fit.step(photos, table, w)
        errs[name] = sm.hole_errors(fit.maps.numpy(), truth, mask)
        if lam is None:
            assert fc.same_bits(fit.maps.numpy()[..., mask], start[..., mask])
    at_start = sm.hole_errors(start, truth, mask)
    print("[smooth] toy hole experiment, mean |d,r,s - truth| (hole, seen): start %.4f %.4f; without the prior %.4f %.4f; "
          "with lambda 0.01 %.4f %.4f" % (at_start + errs["without"] + errs["with"]))
    assert errs["without"][0] == at_start[0]
    assert errs["with"][0] < errs["without"][0]


def test_argument_validation():
    from svbrdf_estimation_amd import fitting
    maps, photos, table, weights = _toy_problem(torch.float32)
    nan, inf = float("nan"), float("inf")
    for bad in ([0.1] * 3, [0.1] * 5, [0.1] * 11, [0.1] * 13, [nan] + [0.0] * 3, [0.0] * 11 + [-1e-3], [inf] * 4, [0.0, -0.0, -1.0, 0.0]):
        with pytest.raises(ValueError):
            fitting.PhotoFit(maps.clone(), smooth=bad)
        with pytest.raises(ValueError):
            fitting.smoothness(maps, bad)
        with pytest.raises(ValueError):
            fitting.composed_step(maps.clone(), torch.zeros_like(maps), torch.zeros_like(maps), 1, photos, table, smooth=bad,
                                  renderer=fc.ToyRenderer())
    with pytest.raises(ValueError):
        fitting.smoothness(maps[:, :9], [0.1] * 4)
    fit = fitting.PhotoFit(maps.clone(), smooth=[0.0, 0.1, 0.2, 0.3])
    assert fit.smooth.tolist() == [0.0] * 3 + [0.1] * 3 + [0.2] * 3 + [0.3] * 3
    assert [round(v, 6) for v in fit._smooth_c] == [round(float(np.float32(v)), 6) for v in fit.smooth.tolist()]
    fit.smooth = None                                               # reassignable, like bounds
    assert fit.smooth is None and fit._smooth_c is None
    fit.smooth = np.arange(12) / 100.0
    assert fit.smooth.shape == (12,) and fit._smooth_c is not None
    with pytest.raises(ValueError):
        fit.smooth = [-1.0] * 4
    assert fit.smooth.shape == (12,)                                # a refused value leaves the old one


def test_photofit_with_a_prior_never_falls_back_on_the_cpu():
    """this package's renderer computes on a ROCm device only: CPU float32 maps are an error with the prior too"""
    from svbrdf_estimation_amd import _native, fitting
    x, photos = torch.rand(1, 12, 8, 8), torch.rand(1, 2, 3, 8, 8)
    fit = fitting.PhotoFit(x.clone(), smooth=[0.0, 0.01, 0.01, 0.01])
    with pytest.raises(_native.NativeLibraryError):
        fit.step(photos, torch.rand(1, 2, 9) + 0.5)
    assert fit.state["step"] == 0 and torch.equal(fit.maps, x)
    with pytest.raises(_native.NativeLibraryError):
        _native.photo_fit_smooth_adam_step(x, x.clone(), x.clone(), x.clone(), photos, torch.rand(1, 2, 9) + 0.5, 1,
                                           (ctypes.c_float * 12)())


# ------------------------------------------------------------------------------------------------ the C ABI

def test_library_exports_the_entries_without_an_abi_bump(lib):
    from svbrdf_estimation_amd import _native
    assert lib.svbrdf_abi_version() == 8 and _native.ABI_VERSION == 8
    with open(os.path.join(ROOT, "include", "svbrdf_hip.h")) as f:
        header = f.read()
    names = lambda text: [a.split()[-1].lstrip("*") for a in text.replace("\n", " ").split(",")]
    for entry, twin, count in ((sm.STEP_ENTRY, fc.STEP_ENTRY, 26), (sm.JOINT_ENTRY, jc.JOINT_ENTRY, 27)):
        assert hasattr(lib, entry), entry
        declared = header.split("SVBRDF_API int %s(" % entry)[1].split(");")[0]
        assert entry in _native.SIGNATURES and len(_native.SIGNATURES[entry][1]) == count == declared.count(",") + 1
        # the twin's list with maps_in / maps_out for maps and smooth_host in front of bounds_host
        t = names(header.split("SVBRDF_API int %s(" % twin)[1].split(");")[0])
        assert names(declared) == ["maps_in", "maps_out"] + t[1:9] + ["smooth_host"] + t[9:]
        assert "const float *maps_in" in declared and "const float *smooth_host" in declared
    assert "MUST NOT OVERLAP" in header and "PHOTO TERM alone" in header and "torch.sign(inf - inf)" in header


@pytest.mark.parametrize("joint", (False, True), ids=("maps", "joint"))
def test_argument_errors_come_before_any_launch_and_touch_nothing(lib, joint):
    """The entry's own checks first -- smooth_host NULL, a lambda that is NaN, negative or infinite, maps_in and maps_out
    overlapping: -2 -- then the twin's in its order: -1 null pointers (maps_out is required; weights, bounds and grad_out may
    be null), -2 dims, eps, weight_planes, step, lr, betas, adam_eps, bounds, -3 misaligned, -4 workspace too small.  Host
    buffers stand in for device memory: nothing is enqueued, and not a byte of them changes."""
    fn = getattr(lib, sm.JOINT_ENTRY if joint else sm.STEP_ENTRY)
    B, S, H = 1, 9, 8
    buf = (ctypes.c_float * 32768)()
    for i in range(len(buf)):
        buf[i] = float(i % 251)
    snapshot = bytes(buf)
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 63) & ~63
    need = getattr(lib, jc.WORKSPACE_BYTES)(B, S, H, H) if joint else lib.svbrdf_rendering_loss_workspace_bytes(B, S, H, H)
    good = np.array([[0.0, 1.0]] * 12, dtype=np.float32)
    lam = np.full(12, 0.01, np.float32)
    nan, inf = float("nan"), float("inf")
    n_maps = B * 12 * H * H * 4                                     # 3072 bytes

    def call(maps=p, out=p + 45056, m=p + 4096, v=p + 8192, photos=p + 12288, weights=p + 20480, planes=S, scenes=p + 24576,
             xrow=p + 25600, eps=0.1, smooth=lam, bounds=good, lr=1e-2, b1=0.9, b2=0.999, ae=1e-8, step=1, loss=p + 26624,
             grad=p + 28672, grad_s=p + 36864, ws=p + 40960, ws_bytes=need, B=B, S=S, H=H, W=H):
        barr = None if bounds is None else (ctypes.c_float * 24)(*np.asarray(bounds, np.float32).reshape(-1).tolist())
        sarr = None if smooth is None else (ctypes.c_float * 12)(*np.asarray(smooth, np.float32).tolist())
        f = ctypes.c_float
        return fn(maps, out, m, v, photos, weights, planes, scenes, xrow, f(eps), sarr, barr, f(lr), f(b1), f(b2), f(ae), step,
                  loss, grad, *((grad_s,) if joint else ()), ws, ws_bytes, B, S, H, W, None)

    launches = lib.svbrdf_debug_launch_count()
    # the entry's own, in front of everything else: even with a null pointer elsewhere the answer is theirs
    assert call(smooth=None) == -2 and b"smooth_host" in lib.svbrdf_last_error()
    assert call(smooth=None, photos=None) == -2
    for k, value in ((0, nan), (5, -1e-3), (11, inf), (3, -inf)):
        bad = lam.copy()
        bad[k] = value
        assert call(smooth=bad) == -2, (k, value)
        assert b"smooth_host" in lib.svbrdf_last_error()
    for maps, out in ((p, p), (p, p + 4), (p, p + n_maps - 4), (p + 45056 + n_maps - 4, p + 45056)):
        assert call(maps=maps, out=out) == -2, (maps - p, out - p)
        assert b"overlap" in lib.svbrdf_last_error()
    assert call(out=p + 2, photos=None) == -2                       # overlapping AND misaligned AND a null: the overlap
    assert call(maps=p + 45056 + n_maps, ws_bytes=need - 8) == -4   # adjacent buffers do not overlap: the next failure
    assert call(smooth=np.zeros(12, np.float32), ws_bytes=need - 8) == -4          # all-zero lambda is valid
    # then the twin's
    for name in ("maps", "out", "m", "v", "photos", "scenes", "xrow", "loss", "ws") + (("grad_s",) if joint else ()):
        assert call(**{name: None}) == -1, name
    for planes in (0, 2, S + 1, -1):
        assert call(planes=planes) == -2, planes
        assert b"weight_planes" in lib.svbrdf_last_error()
    for planes in (1, S):
        assert call(weights=None, planes=planes) == -2, planes
    assert call(W=H + 1) == -2 and call(B=0) == -2 and call(S=0, planes=1) == -2 and call(eps=0.0) == -2
    for bad in (dict(step=0), dict(step=-3), dict(lr=-1e-2), dict(lr=nan), dict(lr=inf), dict(ae=-1e-8), dict(ae=nan),
                dict(ae=inf), dict(b1=1.0), dict(b1=-0.1), dict(b1=nan), dict(b2=1.0), dict(b2=-0.5), dict(b2=nan)):
        assert call(**bad) == -2, bad
    for k, pair in ((0, (nan, 1.0)), (5, (0.0, nan)), (11, (1.0, 0.0)), (3, (inf, -inf))):
        b = good.copy()
        b[k] = pair
        assert call(bounds=b) == -2, (k, pair)
        assert b"bounds" in lib.svbrdf_last_error()
    assert call(maps=p + 2, out=p + 45058) == -3 and call(out=p + 45058) == -3 and call(m=p + 4098) == -3 and call(v=p + 8194) == -3
    assert call(photos=p + 12290) == -3 and call(weights=p + 20482) == -3 and call(grad=p + 28674) == -3
    assert call(scenes=p + 24578) == -3 and call(ws=p + 40964) == -3
    assert call(ws_bytes=need - 8) == -4
    if joint:
        assert call(grad_s=p + 36866) == -3
        assert call(ws_bytes=lib.svbrdf_rendering_loss_workspace_bytes(B, S, H, H)) == -4
        for big in (426, 384):
            assert call(S=big, planes=big, ws_bytes=1 << 20) == -2, big
            assert b"too many scenes" in lib.svbrdf_last_error()
    assert call(grad=None, weights=None, planes=0, bounds=None, ws_bytes=need - 1) == -4      # what may be null, may
    assert lib.svbrdf_debug_launch_count() == launches              # failed calls enqueue and count nothing
    assert bytes(buf) == snapshot


# ------------------------------------------------------------------------------------------------ the kernels

def _isa_stats():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_stats
    return isa_stats


@pytest.fixture(scope="module")
def smooth_asm(tmp_path_factory):
    return unit_build.compile_unit_asm(tmp_path_factory.mktemp("isa_smooth"), UNIT, "SCHED_PHOTO")


@needs_hipcc
def test_smooth_kernels_resources_and_update(smooth_asm):
    isa_stats = _isa_stats()
    names = sorted(k for k in isa_stats.kernels(smooth_asm) if "__hip_cuid" not in k)
    assert len(names) == 4, names                                   # maps-only and joint, unweighted and weighted; nothing else
    assert sum("k_smooth_step" in k for k in names) == 2 and sum("k_smooth_joint" in k for k in names) == 2
    assert not [k for k in names if any(s in k for s in OTHER_KERNELS)], names
    for k in names:
        _, meta, whole, loops, ins, rng = isa_stats.analyse(smooth_asm, k)
        print("%s\n   VGPRs %s, SGPRs %s, occupancy %s, LDS %s bytes, scratch %s, %d instructions" % (
            k, meta["NumVgprs"], meta.get("NumSgprs", meta.get("next_free_sgpr", "?")), meta["Occupancy"], meta["LDSByteSize"], meta["ScratchSize"], whole["total"]))
        assert int(meta["NumVgprs"]) <= 128 and int(meta["NumAgprs"]) == 0 and int(meta["Occupancy"]) == 4, (k, meta)
        assert int(meta["ScratchSize"]) == 0 and whole["scratch"] == 0, (k, meta)
        assert whole["v_pk"] == 0, (k, whole)
        mns = [mn for _, _, mn, _ in ins if mn]
        assert not [mn for mn in mns if mn.startswith("flat_")], k
        # the update behind the loops: 12 IEEE divisions and 12 square roots, as the twins'
        assert mns.count("v_div_fixup_f32") == 12 and mns.count("v_div_fmas_f32") == 12, k
        assert sum(1 for mn in mns if mn.startswith("v_sqrt_f32")) == 12, k
        # 12 gradient stores (skipped without grad_out) and the 36 of maps and state, all with the gradient stores' policy
        stores = [ops for _, _, mn, ops in ins if mn and mn.startswith("buffer_store_dword")]
        assert len(stores) == 48 and all("sc0 sc1" in s for s in stores), (k, len(stores))
        # the prior: 48 neighbour loads more than the twin's plane loads, one unordered compare per neighbour
        loads = sum(1 for mn in mns if mn.startswith("buffer_load_dword"))
        unordered = sum(1 for mn in mns if mn.startswith("v_cmp_u_f32"))
        print("   %d buffer loads, %d unordered compares, %d LDS instructions" % (
            loads, unordered, sum(1 for mn in mns if mn.startswith("ds_"))))
        assert unordered == 48, (k, unordered)


@needs_hipcc
def test_makefile_builds_the_unit_into_the_library():
    unit_build.assert_makefile_builds(UNIT, "SCHED_PHOTO")
    assert "-ffp-contract=off" in unit_build.make_var("HIPFLAGS")


def test_source_reuses_the_two_flows_and_holds_one_update():
    """no inline assembly with instructions, no cooperative launch, no fma; the scene loops and the launch tails are the fit
    and the joint unit's own -- shared through headers that hold no kernel and no entry point -- and the update with the
    prior's term stands once"""
    src = unit_build.read_csrc(UNIT + ".hip")        # (the unit owns no header)
    for m in re.finditer(r'asm\s+volatile\s*\(\s*"([^"]*)"', src):
        assert m.group(1) == "", "inline asm with instructions: %r" % m.group(1)
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert "Cooperative" not in code and "grid_group" not in code and "fma" not in code and "sqrtf" not in code
    joint = unit_build.assert_includes_shared_header(UNIT, "svbrdf_photo_fit_pose_device.h")
    assert "void joint_body(" in joint and '#include "svbrdf_photo_fit_device.h"' in joint
    assert "void fit_body(" in unit_build.assert_includes_shared_header("svbrdf_photo_fit", "svbrdf_photo_fit_device.h")
    for used in ("fit_body<WEIGHTED>(", "joint_body<WEIGHTED>(", "adam_channel(", "adam_args(who,", "weights_check(who,",
                 "plan_sums(who,", "plan_loss(who,", "fail_as(who,"):
        assert used in code, used
    assert len(re.findall(r"\bvoid smooth_epilogue\(", code)) == 1 and code.count("smooth_epilogue(") == 2
    assert code.count("adam_channel(") == 1 and "photo_scene_loop" not in code and "pose_scene_loop" not in code
    assert re.findall(r"SVBRDF_SMOOTH_(?:FIT|JOINT)_KERNEL\((k_\w+),", code) == [
        "k_smooth_step", "k_smooth_step_weighted", "k_smooth_joint", "k_smooth_joint_weighted"]
