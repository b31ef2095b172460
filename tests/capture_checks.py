"""The checker of svbrdf_estimation_amd.capture (csrc/svbrdf_capture.hip: k_rectify; svbrdf_rectify_photos):

  * ``restatement``: the definition of include/svbrdf_hip.h in numpy, one individually rounded operation per statement.  In
    float32 it is THE oracle of the GPU tests: the kernel equals it bit for bit, values and weights, no tolerance.  The same
    statements in float64 (``dtype=np.float64``) are what the float32 ones are held against on the CPU;
  * ``torch_composition``: the independent check, and the composed form the speed test times the one launch against --
    ``grid_sample(mode="bilinear", padding_mode="zeros", align_corners=True)`` on 2u/(Ws-1) - 1 behind a table gather and a
    permute, with the validity and clip masks as separate passes;
  * matrices and sources for the tests, deterministic (tests/synth.py's generator).
"""
import numpy as np
import torch

import synth

F32_PLANAR, U8_INTERLEAVED = 0, 1

# float32 restatement against the float64 one, at pixels where validity and all tap indices agree:
#   err <= F32_ERROR_FACTOR * (2^-23 max(Hs, Ws) tap_spread + 2^-22 |value|)
# A coordinate u <= max(Hs, Ws) carries a few roundings of 2^-24 u from X, Z and the quotient; the value moves by that
# times the local slope, at most the spread of the four taps, and the three interpolation steps add roundings of the value
# itself.  Measured on uniform-random sources through the `mild` and `outside` matrices (test_capture_cpu.py prints it):
# worst ratio 0.876 at 97x131 -> 32x32, 1.183 at 480x640 -> 64x64, 1.481 at 1200x1600 -> 256x256 (errors 9.6e-6, 6.7e-5,
# 2.2e-4; 1 of 2048, 1 of 8192 and 13 of 131072 pixels excluded).  The bound is twice the largest.
F32_ERROR_MEASURED = 1.481
F32_ERROR_FACTOR = 2.0 * F32_ERROR_MEASURED
MAX_EXCLUDED_SHARE = 1e-3       # pixels whose validity or tap indices differ between the two precisions


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def count_differing(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def restatement(src, matrices, size, k=1, lut=None, clip=None, dtype=np.float32, detail=False):
    """src: float32 [P,3,Hs,Ws] or uint8 [P,Hs,Ws,3]; matrices float32 [P,9] (or [P,3,3]); size (Hd, Wd); k in {1,2,4}; lut
    float32 [256] for uint8; clip (lo, hi) or None -> (values [P,3,Hd,Wd], weights [P,Hd,Wd]) of `dtype`.  detail=True adds a
    dict: "valid" [P,k*k,Hd,Wd] geometric validity, "x0", "y0" the tap indices, "spread" [P,Hd,Wd] the largest
    max - min over a sub-sample's four taps and the three channels."""
    f = dtype
    src = np.asarray(src)
    u8 = src.dtype == np.uint8
    P = src.shape[0]
    Hs, Ws = (src.shape[1], src.shape[2]) if u8 else (src.shape[2], src.shape[3])
    Hd, Wd = size
    M = np.asarray(matrices, np.float32).reshape(P, 9).astype(f)
    if u8:
        table = np.asarray(lut, np.float32).astype(f)
        lo, hi = (-1, 256) if clip is None else (int(np.floor(max(-1.0, min(256.0, clip[0])))), int(np.ceil(max(-1.0, min(256.0, clip[1])))))
    else:
        lo, hi = (f(-np.inf), f(np.inf)) if clip is None else (f(np.float32(clip[0])), f(np.float32(clip[1])))
    wmax, hmax, zero = f(Ws - 1), f(Hs - 1), f(0.0)
    xg = np.broadcast_to(np.arange(Wd, dtype=f)[None, :], (Hd, Wd))
    yg = np.broadcast_to(np.arange(Hd, dtype=f)[:, None], (Hd, Wd))
    values = np.zeros((P, 3, Hd, Wd), f)
    weights = np.zeros((P, Hd, Wd), f)
    info = dict(valid=np.zeros((P, k * k, Hd, Wd), bool), x0=np.zeros((P, k * k, Hd, Wd), np.int64),
                y0=np.zeros((P, k * k, Hd, Wd), np.int64), spread=np.zeros((P, Hd, Wd), f))
    with np.errstate(all="ignore"):
        for p in range(P):
            m = M[p]
            ok = np.ones((Hd, Wd), bool)
            acc = [None, None, None]
            for j in range(k):
                for i in range(k):
                    xs = xg + f((i + 0.5) / k - 0.5)
                    ys = yg + f((j + 0.5) / k - 0.5)
                    X = (m[0] * xs + m[1] * ys) + m[2]
                    Y = (m[3] * xs + m[4] * ys) + m[5]
                    Z = (m[6] * xs + m[7] * ys) + m[8]
                    u, v = X / Z, Y / Z
                    valid = (Z > zero) & (u >= zero) & (u <= wmax) & (v >= zero) & (v <= hmax)
                    ok &= valid
                    u, v = np.where(valid, u, zero), np.where(valid, v, zero)
                    u, v = np.fmin(np.fmax(u, zero), wmax), np.fmin(np.fmax(v, zero), hmax)
                    x0f, y0f = np.floor(u), np.floor(v)
                    fx, fy = u - x0f, v - y0f
                    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
                    x1, y1 = np.minimum(x0 + 1, Ws - 1), np.minimum(y0 + 1, Hs - 1)
                    info["valid"][p, j * k + i], info["x0"][p, j * k + i], info["y0"][p, j * k + i] = valid, x0, y0
                    for ch in range(3):
                        taps = []
                        for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)):
                            if u8:
                                code = src[p, yy, xx, ch].astype(np.int64)
                                ok &= (code > lo) & (code < hi)
                                taps.append(table[code])
                            else:
                                t = src[p, ch, yy, xx].astype(f)
                                ok &= (t > lo) & (t < hi) & (np.abs(t) < f(np.inf))
                                taps.append(t)
                        a, b, c, d = taps
                        top = a + fx * (b - a)
                        bot = c + fx * (d - c)
                        val = top + fy * (bot - top)
                        acc[ch] = val if acc[ch] is None else acc[ch] + val
                        info["spread"][p] = np.maximum(info["spread"][p], np.where(
                            np.isfinite(a + b + c + d), np.maximum.reduce(taps) - np.minimum.reduce(taps), zero))
            scale = f(1.0 / (k * k))
            for ch in range(3):
                values[p, ch] = np.where(ok, acc[ch] * scale, zero)
            weights[p] = np.where(ok, f(1.0), zero)
    assert values.dtype == f and weights.dtype == f
    return (values, weights, info) if detail else (values, weights)


def torch_composition(src, matrices, size, lut=None, clip=None, dtype=torch.float32):
    """The composed form in torch ops, k = 1, on the device of `src`: to float, table gather, permute, grid_sample
    (bilinear, zeros, align_corners=True) on 2u/(Ws-1) - 1, the geometric and tap masks, where.  src: uint8 [P,Hs,Ws,3] or
    float [P,3,Hs,Ws] tensor; matrices [P,9] -> (values [P,3,Hd,Wd], weights [P,Hd,Wd]) of `dtype`."""
    Hd, Wd = size
    dev = src.device
    u8 = src.dtype == torch.uint8
    P = src.shape[0]
    if u8:
        Hs, Ws = src.shape[1], src.shape[2]
        img = lut.to(device=dev, dtype=dtype)[src.long()].permute(0, 3, 1, 2).contiguous()
        lo, hi = (-1, 256) if clip is None else clip
        bad = ((src <= lo) | (src >= hi)).any(dim=-1)
    else:
        Hs, Ws = src.shape[2], src.shape[3]
        img = src.to(dtype)
        lo, hi = (-float("inf"), float("inf")) if clip is None else clip
        bad = (~torch.isfinite(src) | (src <= lo) | (src >= hi)).any(dim=1)
    m = matrices.to(device=dev, dtype=dtype).reshape(P, 9, 1, 1)
    xs = torch.arange(Wd, device=dev, dtype=dtype).view(1, 1, Wd).expand(P, Hd, Wd)
    ys = torch.arange(Hd, device=dev, dtype=dtype).view(1, Hd, 1).expand(P, Hd, Wd)
    X = (m[:, 0] * xs + m[:, 1] * ys) + m[:, 2]
    Y = (m[:, 3] * xs + m[:, 4] * ys) + m[:, 5]
    Z = (m[:, 6] * xs + m[:, 7] * ys) + m[:, 8]
    u, v = X / Z, Y / Z
    valid = (Z > 0) & (u >= 0) & (u <= Ws - 1) & (v >= 0) & (v <= Hs - 1)
    u, v = torch.where(valid, u, torch.zeros_like(u)), torch.where(valid, v, torch.zeros_like(v))
    grid = torch.stack((2.0 * u / max(Ws - 1, 1) - 1.0, 2.0 * v / max(Hs - 1, 1) - 1.0), dim=-1)
    clean = torch.where(bad[:, None], torch.zeros_like(img), img) if not u8 else img      # (0 * NaN would spoil a neighbour)
    val = torch.nn.functional.grid_sample(clean, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    # a pixel is refused if any of its four taps is: the bad-texel mask spread over each 2x2 footprint, read at (y0, x0)
    padded = torch.nn.functional.pad(bad[:, None].to(dtype), (0, 1, 0, 1), mode="replicate")
    spread = torch.nn.functional.max_pool2d(padded, kernel_size=2, stride=1)[:, 0]
    x0, y0 = u.floor().long().clamp_(0, Ws - 1), v.floor().long().clamp_(0, Hs - 1)
    touched = spread.reshape(P, -1).gather(1, (y0 * Ws + x0).reshape(P, -1)).reshape(P, Hd, Wd) > 0
    ok = valid & ~touched
    return torch.where(ok[:, None], val, torch.zeros_like(val)), ok.to(dtype)


# ------------------------------------------------------------------------------------------------ inputs

KINDS = ("mild", "outside", "horizon", "identity", "translation")


def matrix(kind, src_size, dst_size, p=0):
    """float32 [9]: destination pixel -> source pixel, for photo `p` of a batch (every photo its own matrix).
    mild: a perspective view of an inner part of the source, every pixel valid.  outside: the same with the corners partly
    beyond the image.  horizon: Z falls through 0 at 0.6 of the destination's width.  identity.  translation: by (2, -1)."""
    (Hs, Ws), (Hd, Wd) = src_size, dst_size
    if kind == "identity":
        return np.eye(3, dtype=np.float32).reshape(9)
    if kind == "translation":
        return np.array([1, 0, 2 + p, 0, 1, -1 - p, 0, 0, 1], np.float32)
    sx, sy = (Ws - 1.0) / max(Wd - 1.0, 1.0), (Hs - 1.0) / max(Hd - 1.0, 1.0)
    j = 0.01 * (p % 8)
    if kind == "outside":
        A = [1.09 * sx, 0.02 * sx * Wd / Hd, (-0.04 - j) * (Ws - 1.0), -0.03 * sy * Hd / Wd, 1.08 * sy, (-0.02 + j) * (Hs - 1.0)]
        persp = [0.02 / Wd, 0.01 / Hd, 1.0]
    else:
        A = [0.9 * sx, 0.03 * sx * Wd / Hd, (0.05 + j) * (Ws - 1.0), 0.02 * sy * Hd / Wd, 0.9 * sy, (0.06 - j) * (Hs - 1.0)]
        persp = [0.2 / Wd, 0.1 / Hd, 1.0 + j]
        if kind == "horizon":
            persp = [-1.0 / (0.6 * Wd + p), 0.05 / Hd, 1.0]
    if kind == "mild":          # X / Z must stay inside: Z >= 1 only shrinks it, and the numerator tops out at 0.98 (Ws - 1)
        pass
    return np.array(A + persp, np.float32)


def matrices(kind, src_size, dst_size, P):
    return np.stack([matrix(kind, src_size, dst_size, p) for p in range(P)])


def float_source(seed, P, Hs, Ws):
    """float32 [P,3,Hs,Ws], uniform in [0, 1)"""
    return synth.uniform01(seed, (P, 3, Hs, Ws)).astype(np.float32)


def u8_source(seed, P, Hs, Ws, blobs=False):
    """uint8 [P,Hs,Ws,3], uniform codes; blobs=True: mid-grey codes 20..235 with saturated (255) and black (0) discs"""
    u = synth.uniform01(seed, (P, Hs, Ws, 3))
    if not blobs:
        return np.minimum(u * 256.0, 255.0).astype(np.uint8)
    img = (20.0 + u * 215.0).astype(np.uint8)
    yy, xx = np.mgrid[0:Hs, 0:Ws]
    for n, (cy, cx, r, code) in enumerate(((0.3, 0.3, 0.12, 255), (0.7, 0.6, 0.08, 255), (0.5, 0.85, 0.06, 0), (0.15, 0.7, 0.05, 252))):
        disc = (yy - cy * Hs) ** 2 + (xx - cx * Ws) ** 2 <= (r * min(Hs, Ws)) ** 2
        img[:, disc, n % 3] = code          # one channel is enough to refuse the tap
    return img


# ------------------------------------------------------------------------------------------------ on the device

def abi_rectify(native, dev, src, matrices, size, k=1, lut=None, clip=None, src_offset=0, dst_offset=0, want_weights=True):
    """svbrdf_rectify_photos called with raw device pointers.  src: numpy uint8 [P,Hs,Ws,3] or float32 [P,3,Hs,Ws];
    `src_offset` / `dst_offset`: ELEMENTS by which the source / the two outputs are moved off their allocation's alignment
    (1 float = 4 bytes, 1 code = 1 byte).  The outputs sit between canaries.
    -> dict(values, weights or None, canaries_intact, launches)"""
    import ctypes
    lib = native._load()
    src = np.ascontiguousarray(src)
    u8 = src.dtype == np.uint8
    P = src.shape[0]
    Hs, Ws = (src.shape[1], src.shape[2]) if u8 else (src.shape[2], src.shape[3])
    Hd, Wd = size
    pad, canary = 64, -7.0
    sbuf = torch.zeros(src.size + src_offset + 16, dtype=torch.uint8 if u8 else torch.float32, device=dev)
    sview = sbuf[src_offset:src_offset + src.size]
    sview.copy_(torch.from_numpy(src.reshape(-1)))
    mats = torch.from_numpy(np.ascontiguousarray(matrices, np.float32).reshape(P, 9)).to(dev)
    table = None if lut is None else torch.as_tensor(lut, dtype=torch.float32).to(dev)
    n_out, n_w = P * 3 * Hd * Wd, P * Hd * Wd
    obuf = torch.full((n_out + 2 * pad + dst_offset,), canary, dtype=torch.float32, device=dev)
    wbuf = torch.full((n_w + 2 * pad + dst_offset,), canary, dtype=torch.float32, device=dev)
    o0, w0 = pad + dst_offset, pad + dst_offset
    lo, hi = (-np.inf, np.inf) if clip is None else clip
    before = native.launch_count()
    rc = lib.svbrdf_rectify_photos(sview.data_ptr(), U8_INTERLEAVED if u8 else F32_PLANAR, P, Hs, Ws, mats.data_ptr(), Hd, Wd, k,
                                   None if table is None else table.data_ptr(), ctypes.c_float(lo), ctypes.c_float(hi),
                                   obuf[o0:].data_ptr(), wbuf[w0:].data_ptr() if want_weights else None,
                                   ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0, (rc, lib.svbrdf_last_error())
    torch.cuda.synchronize(dev)
    o, w = obuf.cpu().numpy(), wbuf.cpu().numpy()
    intact = (o[:o0] == canary).all() and (o[o0 + n_out:] == canary).all() and (w[:w0] == canary).all() \
        and (w[w0 + n_w:] == canary).all() and (want_weights or (w == canary).all())
    return dict(values=o[o0:o0 + n_out].reshape(P, 3, Hd, Wd), weights=w[w0:w0 + n_w].reshape(P, Hd, Wd) if want_weights else None,
                canaries_intact=bool(intact), launches=native.launch_count() - before,
                src_ptr=sview.data_ptr(), out_ptr=obuf[o0:].data_ptr())


def measure_capture(dev, native, P=8, src_size=(480, 640), dst_size=(256, 256), k=1, u8=True, clip=(5, 250), sets=4, n=30,
                    rounds=3, composed=True):
    """-> dict of medians (us per call): "fused_us", the one launch of capture.rectify, and "composed_us", torch_composition
    on the same data (k = 1 only: to float, table gather, permute, grid_sample, validity and clip masks, where) -- one
    process, `sets` rotating source batches, the legs alternating round by round (photo_checks.timed_legs)."""
    import photo_checks
    from svbrdf_estimation_amd import capture
    Hs, Ws = src_size
    lut = capture.gamma_lut().to(dev) if u8 else None
    if not u8:
        clip = (0.02, 0.98) if clip is not None else None
    M = torch.from_numpy(matrices("outside", src_size, dst_size, P)).to(dev)
    if u8:
        srcs = [torch.randint(0, 256, (P, Hs, Ws, 3), dtype=torch.uint8, device=dev, generator=None) for _ in range(sets)]
    else:
        srcs = [torch.rand((P, 3, Hs, Ws), dtype=torch.float32, device=dev) for _ in range(sets)]

    def fused(i):
        capture.rectify(srcs[i % sets], M, dst_size, lut=lut, clip=clip, samples=k)

    def comp(i):
        torch_composition(srcs[i % sets], M, dst_size, lut=lut, clip=clip)

    legs = (("fused_us", fused),) + ((("composed_us", comp),) if composed and k == 1 else ())
    out, res = photo_checks.timed_legs(legs, n, rounds, photo_checks.spinning_wave(native, dev), dev)
    got = capture.rectify(srcs[0], M, dst_size, lut=lut, clip=clip, samples=k)
    out.update(rounds=res, device=torch.cuda.get_device_name(dev), P=P, src_size=src_size, dst_size=dst_size, k=k,
               source="uint8" if u8 else "float32", zero_weight_share=float((got[1] == 0).float().mean().item()),
               source_bytes=srcs[0].numel() * srcs[0].element_size(), output_bytes=P * 4 * dst_size[0] * dst_size[1] * 4)
    if "composed_us" in out:
        ref = torch_composition(srcs[0], M, dst_size, lut=lut, clip=clip)
        same_w = (ref[1] == got[1])
        out["weights_differing_from_composed"] = int((~same_w).sum().item())
        out["max_abs_diff_from_composed"] = float((ref[0] - got[0]).abs()[same_w[:, None].expand_as(ref[0])].max().item())
        out["fused_over_composed"] = out["fused_us"] / out["composed_us"]
    return out
