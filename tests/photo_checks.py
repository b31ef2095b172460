"""Shared by the photo-loss tests (tests/test_*photo_loss*.py), their fixture generators and tools/photo_loss_bench.py: the
ORACLE's photo loss in its four forms, the tie rule, the comparison values of one case and the event-timed measurement.

The C oracle needs no photo loss of its own -- it is the composition

    rad   = c_oracle.render_fwd(input, scenes)
    delta = log(rad + eps) - log(photo + eps)
    loss  = sum(w |delta|) / N
    g     = w sign(delta) / (N (rad + eps))
    grad  = c_oracle.render_bwd(input, scenes, g)

with N = B S 3 H W and w = 1 (with photo = render_fwd(target) it then reproduces c_oracle.rendering_loss: loss to 7 digits,
gradient to 1.1e-7 of its maximum).  With confidence weights w[b,s,i,j] in [0, 1] ([B,S,H,W], or [B,1,H,W] shared by the
item's photos) the photo is first REPLACED under a zero weight, never multiplied: photo = where(w > 0, photo, 0).  f64=True
evaluates everything in double on the same float32 inputs: the comparison value's own error.  For the head losses the
12-channel gradient goes through chain9 at the float32-decoded maps (class Reference with head=True).

Ties.  A term (b, s, c, i, j) whose |delta| in float64 is below tolerances.TIE_LEVEL has an undetermined sign in any fp32
evaluation, the reference's included -- unless it is STRUCTURAL: the photo value is exactly 0 and the light is behind the
surface (unclamped n.wi < -1e-6, computed here in float64 from the scene row and the pixel grid), where both sides are
exactly eps in every evaluation and the term is exactly 0 with gradient 0.  A term under a weight of exactly 0 is structural
as well: exactly 0 with gradient exactly 0 in every evaluation, whatever its delta.  A tie pixel has a non-structural tied
term.  Tie pixels are left out of the element-wise comparison, must stay within TIE_SLACK * max|g| and are counted against a
cap.
"""
import ctypes

import numpy as np
import torch

import tolerances
from oracle import c_oracle

EPS = 0.1


def broadcast_weights(weights, S):
    """[B,S,H,W] float32 from [B,S,H,W] or [B,1,H,W]"""
    w = np.asarray(weights, np.float32)
    assert w.ndim == 4 and w.shape[1] in (1, S), w.shape
    return np.ascontiguousarray(np.broadcast_to(w, (w.shape[0], S) + w.shape[2:]))


def excused_photos(photos, weights):
    """p' = where(w > 0, photo, 0): [B,S,3,H,W] float32"""
    photos = np.asarray(photos, np.float32)
    w = broadcast_weights(weights, photos.shape[1])
    return np.where((w > 0)[:, :, None], photos, np.float32(0.0)).astype(np.float32)


def oracle_photo_loss(inp, photos, scenes, eps=EPS, f64=False, want_grad=True, weights=None):
    """-> (loss: float, grad [B,12,H,W] float32 / float64 or None, delta [B,S,3,H,W]; with `weights`: of the excused photos)"""
    inp = np.ascontiguousarray(inp, np.float32)
    scenes = np.ascontiguousarray(scenes, np.float32)
    if weights is None:
        photos, w = np.asarray(photos, np.float32), 1.0
    else:
        photos = excused_photos(photos, weights)
        w = broadcast_weights(weights, photos.shape[1]).astype(np.float64)[:, :, None]
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
    loss = float((w * np.abs(delta.astype(np.float64))).sum() / float(delta.size))
    if not want_grad:
        return loss, None, delta
    g = (w * np.sign(delta).astype(np.float64) / (float(delta.size) * a.astype(np.float64))).astype(np.float32)
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


def tie_map(inp, photos, scenes, delta_f64, weights=None):
    """[B,H,W] float64: smallest |delta_f64| over the pixel's NON-structural terms (inf where all are structural); with
    `weights` the rule holds for the excused photos, and a weight of exactly 0 is structural too"""
    if weights is not None:
        photos = excused_photos(photos, weights)
    structural = (np.asarray(photos) == 0.0) & (unclamped_n_dot_wi(inp, scenes) < -1e-6)[:, :, None]
    if weights is not None:
        structural |= (broadcast_weights(weights, photos.shape[1]) == 0.0)[:, :, None]
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


def chain9(enc, maps, g12, n=None):
    """d loss / d encoded9 [B,9,H,W] float64 from d loss / d maps [B,12,H,W]: the chain rule through the head decode in
    float64 (head_checks.head_loss_f64_on_f32_decode).  `n`: the unit normal the Jacobian is taken at, default the
    float32-decoded one of `maps`."""
    enc = np.asarray(enc, np.float32)
    g12 = np.asarray(g12, np.float64)
    n = np.asarray(maps)[:, 0:3].astype(np.float64) if n is None else np.asarray(n, np.float64)
    ex, ey = 3.0 * enc[:, 0].astype(np.float64), 3.0 * enc[:, 1].astype(np.float64)
    k = 3.0 / np.sqrt(ex * ex + ey * ey + 1.0)
    ng = (n * g12[:, 0:3]).sum(axis=1)
    g9 = np.empty(enc.shape, np.float64)
    g9[:, 0] = k * (g12[:, 0] - n[:, 0] * ng)
    g9[:, 1] = k * (g12[:, 1] - n[:, 1] * ng)
    g9[:, 2:5] = 0.5 * g12[:, 3:6]
    g9[:, 5] = 0.5 * (g12[:, 6] + g12[:, 7] + g12[:, 8])
    g9[:, 6:9] = 0.5 * g12[:, 9:12]
    return g9


class Reference:
    """the oracle's values of one case, computed once: fp32 and fp64 loss and gradient, tie map.  `x`: the 12 maps, or with
    head=True the encoded [B,9,H,W] tensor -- `maps` is then its float32 decode (c_oracle.head_decode: the reference's
    rounding), `grad` and `grad64` its 9-channel gradient (float64 arrays) and `grad12_64` the one w.r.t. the maps"""

    def __init__(self, x, photos, scenes, eps=EPS, head=False, weights=None):
        self.x, self.head = np.ascontiguousarray(x, np.float32), bool(head)
        self.maps = c_oracle.head_decode(self.x) if head else self.x
        self.loss, g32, _ = oracle_photo_loss(self.maps, photos, scenes, eps, weights=weights)
        self.loss64, g64, self.delta64 = oracle_photo_loss(self.maps, photos, scenes, eps, f64=True, weights=weights)
        self.grad12_64 = np.asarray(g64, np.float64)
        if head:
            self.grad, self.grad64 = chain9(self.x, self.maps, g32), chain9(self.x, self.maps, g64)
        else:
            self.grad, self.grad64 = np.asarray(g32), self.grad12_64
        self.tie = tie_map(self.maps, photos, scenes, self.delta64, weights)

    def n_ties(self):
        return int((self.tie < tolerances.TIE_LEVEL).sum())

    def n_widened(self):
        """elements, tie pixels excluded, where the fp32 oracle is outside the strict bound against the fp64 oracle"""
        strict = tolerances.GRAD_RTOL * np.abs(self.grad64) + tolerances.GRAD_ATOL_FRAC * np.abs(self.grad64).max()
        ties = np.broadcast_to((self.tie < tolerances.TIE_LEVEL)[:, None], self.grad64.shape)
        return int(((np.abs(self.grad - self.grad64) > strict) & ~ties).sum())

    def assert_close(self, loss, grad, what, max_ties=tolerances.MAX_TIE_PIXELS):
        tolerances.assert_loss_close(loss, self.loss, what + " loss")
        return assert_photo_grad_close(grad, self.grad, self.grad64, self.tie, what + (" grad9" if self.head else " grad"),
                                       max_ties=max_ties)


def scene_table(B, seed, n_random=3, n_specular=6):
    """[B,S,9] host table: what RenderingLoss draws after torch.manual_seed(seed)"""
    from svbrdf_estimation_amd import losses, renderers
    fn = losses.RenderingLoss(renderers.LocalRenderer())
    fn.random_configuration_count, fn.specular_configuration_count = n_random, n_specular
    torch.manual_seed(seed)
    return fn.sample_scene_table(B).numpy().copy()


# ------------------------------------------------------------------------------------------------ the device side

def to_device(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def to_numpy(t):
    return t.detach().cpu().numpy()


def assert_scratch_is_zero(native):
    torch.cuda.synchronize()
    assert native._workspace_cache, "no call has allocated the scratch yet"
    for ws in native._workspace_cache.values():
        assert ws.numel() * 8 >= 65 * 8
        assert not ws.any().item(), "scratch left dirty: %s" % (ws.cpu().numpy()[:65],)


def call_abi(native, x, photos, scenes, eps=EPS, want_grad=True, head=False, weights=None):
    """the C ABI through the binding: scenes on the device -> the device-table entry, on the host -> the by-value entry
    -> (loss: float, gradient as numpy float32 or None)"""
    loss, grad = native.photo_loss(x, photos, scenes, eps, want_grad=want_grad, head=head, weights=weights)
    return loss.item(), (None if grad is None else to_numpy(grad))


# ------------------------------------------------------------------------------------------------ the speed measurements

def event_timed_median(enqueue, n, block, dev):
    """median over n steps of the time between the events recorded around each; the steps are enqueued while the device
    is held by `block()` (a spinning wave), so the stream runs them back to back whatever the host's pace"""
    stream = torch.cuda.current_stream(dev)
    for i in range(16):
        enqueue(i)                                   # warm: code objects loaded, clocks up
    torch.cuda.synchronize(dev)
    block()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    ev[0].record(stream)
    for i in range(n):
        enqueue(i)
        ev[i + 1].record(stream)
    torch.cuda.synchronize(dev)
    return float(np.median([ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(n)]))


def spinning_wave(native, dev):
    """-> block(): one wave spins for 8 ms on the stream, the timed steps queue up behind it"""
    clk = torch.zeros(2, dtype=torch.int64, device=dev)
    return lambda: native.clock_probe(clk, ticks=800000)


def timed_legs(legs, n, rounds, block, dev):
    """`legs` ((name, enqueue), ...) alternating round by round in one process -> ({name: median of its rounds},
    {name: [event_timed_median of each round]})"""
    res = {name: [] for name, _ in legs}
    for _ in range(rounds):
        for name, fn in legs:
            res[name].append(event_timed_median(fn, n, block, dev))
    return {name: float(np.median(v)) for name, v in res.items()}, res


def measure_photo_loss_against_k3(dev, native, sets=6, n=60, rounds=3):
    """-> dict of medians (us per launch) at the configuration-2 shape, B = 8, 256 x 256, S = 9, by-value scene table,
    `sets` rotating batches (642 MB for the photo loss, 453 MB for K3: beyond the 256 MB Infinity Cache); the two kernels
    alternate round by round in one process"""
    from bench import synthetic_maps
    from svbrdf_estimation_amd import environment
    B, H, S = 8, 256, 9
    lib = native._load()
    gen = torch.Generator().manual_seed(5)
    torch.manual_seed(11)
    table = environment.BatchSceneSampler(B, 3, 6).sample().contiguous()
    ins = [synthetic_maps(gen, B, H, tied=True).to(dev) for _ in range(sets)]
    tgs = [synthetic_maps(gen, B, H, tied=True).to(dev) for _ in range(sets)]
    photos = [native.render_fwd(t, table).clamp_(0.0, 1.0) for t in tgs]          # photographs of the target maps
    grads = [torch.empty_like(a) for a in ins]
    xr = native.xrow(dev, H)
    ws = torch.zeros(65, dtype=torch.int64, device=dev)
    loss = torch.empty(1, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def photo(i):
        k = i % sets
        rc = lib.svbrdf_photo_loss_fwd_bwd_host_scenes(ins[k].data_ptr(), photos[k].data_ptr(), table.data_ptr(), xr.data_ptr(),
                                                       ctypes.c_float(EPS), loss.data_ptr(), grads[k].data_ptr(), ws.data_ptr(),
                                                       ws.numel() * 8, B, S, H, H, st)
        assert rc == 0, lib.svbrdf_last_error()

    def k3(i):
        k = i % sets
        rc = lib.svbrdf_mixed_loss_fwd_bwd_host_scenes(ins[k].data_ptr(), tgs[k].data_ptr(), table.data_ptr(), xr.data_ptr(),
                                                       ctypes.c_float(EPS), ctypes.c_float(0.0), ctypes.c_float(0.01),
                                                       loss.data_ptr(), grads[k].data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                                       B, S, H, H, st)
        assert rc == 0, lib.svbrdf_last_error()

    out, res = timed_legs((("photo_loss_us", photo), ("k3_us", k3)), n, rounds, spinning_wave(native, dev), dev)
    out.update(rounds=res, device=torch.cuda.get_device_name(dev), launches_per_round=n, sets=sets)
    out["photo_loss_frac_of_8TBps"] = (12 + 3 * S + 12) * 4 * H * H * B / (out["photo_loss_us"] * 1e-6) / 8.0e12
    return out
