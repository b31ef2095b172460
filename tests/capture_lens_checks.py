"""The checker of capture.rectify(..., lens=) (csrc/svbrdf_capture_lens.hip: k_lens_rectify, svbrdf_rectify_photos_lens;
csrc/svbrdf_capture_lens_grad.hip: k_lens_grad, svbrdf_rectify_photos_lens_grad):

  * ``restatement`` and ``grad_terms``: the definitions of include/svbrdf_hip.h in numpy, one individually rounded operation
    per statement, line for line.  In float32 they are THE oracle of the GPU tests: the forward equals the restatement bit
    for bit, and the gradient's terms are these planes, so what is left between the kernel's sums and the exact sum of the
    planes is the kernel's additions (capture_grad_checks.bound).  The same statements in float64, on the float32 run's
    cells, are held against torch's float64 autograd on the CPU;
  * ``torch_forward``: the forward composed of differentiable torch ops, with the tap cell, ``valid`` and ``ok`` given as
    constants -- what autograd differentiates towards all 18 inputs;
  * ``torch_composition``: the composed form on the device (the polynomial in torch ops, then grid_sample and masks): the
    independent check and the speed test's other leg;
  * ``abi_rectify_lens`` / ``abi_lens_grad``: the C entries called with raw device pointers, outputs between canaries;
  * the lens sets of the tests, and the refinement loop of the dry run.
The reference has no lens model: there is no reference-written fixture.
"""
import ctypes

import numpy as np
import torch

import capture_checks as cc
import capture_grad_checks as gc

# float32 restatement against the float64 one, capture_checks.F32_ERROR_MEASURED's form and reasoning:
#   err <= F32_LENS_ERROR_FACTOR * (2^-23 max(Hs, Ws) tap_spread + 2^-22 |value|)
# at pixels where validity and all tap cells agree.  The lens map adds some twenty roundings between the quotient and the
# cell, each at most 2^-24 of a coordinate.  Measured on uniform-random sources through `mild` and `outside` with `barrel`
# and `pincushion` (test_capture_lens_cpu.py prints it): worst ratio 1.043 at 97x131 -> 32x32, 1.483 at 480x640 -> 64x64,
# 2.037 at 1200x1600 -> 256x256 (errors 1.4e-5, 9.5e-5, 3.0e-4; 0 of 4096, 1 of 16384 and 28 of 262144 pixels excluded, a
# share of 1.07e-4 at most).  The bound is twice the largest.
F32_LENS_ERROR_MEASURED = 2.037
F32_LENS_ERROR_FACTOR = 2.0 * F32_LENS_ERROR_MEASURED

NULL = np.array([1, 1, 0, 0, 0, 0, 0, 0, 0], np.float32)


def lens(kind, src_size, p=0):
    """float32 [9] fx, fy, cx, cy, k1, k2, p1, p2, k3 for photo `p` (every photo its own principal point)"""
    Hs, Ws = src_size
    f, cx, cy = 0.8 * Ws, (Ws - 1) / 2.0 + 3.0 + 0.25 * p, (Hs - 1) / 2.0 - 2.0 - 0.5 * p
    if kind == "null":
        return NULL.copy()
    if kind == "barrel":
        return np.array([f, f, cx, cy, -0.22, 0.05, 1e-3, -7e-4, 0.0], np.float32)
    if kind == "pincushion":
        return np.array([f, f, cx, cy, 0.12, -0.02, -5e-4, 4e-4, 0.003], np.float32)
    if kind == "folding":       # r rad(r) turns back at r = 1 / sqrt(2.7) = 0.61, i.e. 0.18 Ws from the principal point
        return np.array([0.3 * Ws, 0.3 * Ws, cx, cy, -0.9, 0.0, 0.0, 0.0, 0.0], np.float32)
    raise ValueError(kind)


def lenses(kind, src_size, P):
    return np.stack([lens(kind, src_size, p) for p in range(P)])


LENS_KINDS = ("null", "barrel", "pincushion", "folding")


def hostile_lenses(src_size):
    """name -> float32 [9]: rows under which no sub-sample may be valid and every address must stay inside the source"""
    good = lens("barrel", src_size)

    def with_(**kw):
        row = good.copy()
        for name, value in kw.items():
            row["fx fy cx cy k1 k2 p1 p2 k3".split().index(name)] = value
        return row
    return {
        "all NaN": np.full(9, np.nan, np.float32),
        "k1 = NaN": with_(k1=np.nan),
        "cx = +inf": with_(cx=np.inf),
        "cy = -inf": with_(cy=-np.inf),
        "fx = +inf": with_(fx=np.inf),
        "k2 = -inf": with_(k2=-np.inf),
        "fx = 0": with_(fx=0.0),
        "fy = 0": with_(fy=0.0),
        "fx < 0": with_(fx=-good[0]),
        "fx, fy < 0, no distortion": np.array([-1, -1, 0, 0, 0, 0, 0, 0, 0], np.float32),
        "1e30 everywhere": np.full(9, 1e30, np.float32),
        "cx = 1e30": with_(cx=1e30),
        "k1 = 1e30": with_(k1=1e30),
        "p1 = 1e30": with_(p1=1e30),
    }


# ------------------------------------------------------------------------------------------------ the two restatements

def _decode(src, lut, clip, f):
    u8 = src.dtype == np.uint8
    if u8:
        table = np.asarray(lut, np.float32).astype(f)
        lo, hi = (-1, 256) if clip is None else (int(np.floor(max(-1.0, min(256.0, clip[0])))), int(np.ceil(max(-1.0, min(256.0, clip[1])))))
    else:
        table = None
        lo, hi = (f(-np.inf), f(np.inf)) if clip is None else (f(np.float32(clip[0])), f(np.float32(clip[1])))
    return u8, table, lo, hi


def _lens_map(m, L, xs, ys, f):
    """the header's lines from X to (ud, vd), one rounded operation each -> dict"""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = L
    one, two = f(1.0), f(2.0)
    X = (m[0] * xs + m[1] * ys) + m[2]
    Y = (m[3] * xs + m[4] * ys) + m[5]
    Z = (m[6] * xs + m[7] * ys) + m[8]
    u, v = X / Z, Y / Z
    xn = (u - cx) / fx
    yn = (v - cy) / fy
    xx = xn * xn
    yy = yn * yn
    xy = xn * yn
    r2 = xx + yy
    rad = one + r2 * (k1 + r2 * (k2 + r2 * k3))
    mono = one + r2 * ((f(3.0) * k1) + r2 * ((f(5.0) * k2) + r2 * (f(7.0) * k3)))
    t = two * xy
    xx2 = two * xx
    yy2 = two * yy
    tx = (p1 * t) + (p2 * (r2 + xx2))
    ty = (p1 * (r2 + yy2)) + (p2 * t)
    xd = (xn * rad) + tx
    yd = (yn * rad) + ty
    ud = (xd * fx) + cx
    vd = (yd * fy) + cy
    return dict(Z=Z, u=u, v=v, xn=xn, yn=yn, xx=xx, yy=yy, xx2=xx2, yy2=yy2, r2=r2, rad=rad, mono=mono, t=t, xd=xd, yd=yd,
                ud=ud, vd=vd)


def _walk(src, matrices, lens_rows, size, k, lut, clip, f, cells):
    """For every photo p and sub-sample s = j k + i: the lens map, the cell and the twelve taps, by the header's lines.
    Yields (p, s, xs, ys, g, taps) with g the map's dict plus valid, fx, fy, x0f, y0f, and taps[ch] = (a, b, c, d); after a
    photo's last sub-sample yields (p, None, ok)."""
    src = np.asarray(src)
    u8, table, lo, hi = _decode(src, lut, clip, f)
    P = src.shape[0]
    Hs, Ws = (src.shape[1], src.shape[2]) if u8 else (src.shape[2], src.shape[3])
    Hd, Wd = size
    M = np.asarray(matrices, np.float32).reshape(P, 9).astype(f)
    Ls = np.asarray(lens_rows, np.float32).reshape(P, 9).astype(f)
    wmax, hmax, zero = f(Ws - 1), f(Hs - 1), f(0.0)
    xg = np.broadcast_to(np.arange(Wd, dtype=f)[None, :], (Hd, Wd))
    yg = np.broadcast_to(np.arange(Hd, dtype=f)[:, None], (Hd, Wd))
    for p in range(P):
        m, L = M[p], Ls[p]
        ok = np.ones((Hd, Wd), bool)
        for j in range(k):
            for i in range(k):
                s = j * k + i
                xs = xg + f((i + 0.5) / k - 0.5)
                ys = yg + f((j + 0.5) / k - 0.5)
                g = _lens_map(m, L, xs, ys, f)
                valid = (g["Z"] > zero) & (L[0] > zero) & (L[1] > zero) & (g["mono"] > zero) & (g["ud"] >= zero) \
                    & (g["ud"] <= wmax) & (g["vd"] >= zero) & (g["vd"] <= hmax)
                if cells is not None:
                    valid = cells["valid"][p, s]
                ok &= valid
                uc, vc = np.where(valid, g["ud"], zero), np.where(valid, g["vd"], zero)
                uc, vc = np.fmin(np.fmax(uc, zero), wmax), np.fmin(np.fmax(vc, zero), hmax)
                x0f, y0f = np.floor(uc), np.floor(vc)
                if cells is not None:
                    x0f, y0f = cells["x0f"][p, s].astype(f), cells["y0f"][p, s].astype(f)
                x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
                x1, y1 = np.minimum(x0 + 1, Ws - 1), np.minimum(y0 + 1, Hs - 1)
                g.update(valid=valid, fx=uc - x0f, fy=vc - y0f, x0f=x0f, y0f=y0f)
                taps = []
                for ch in range(3):
                    four = []
                    for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)):
                        if u8:
                            code = src[p, yy, xx, ch].astype(np.int64)
                            ok &= (code > lo) & (code < hi)
                            four.append(table[code])
                        else:
                            t = src[p, ch, yy, xx].astype(f)
                            ok &= (t > lo) & (t < hi) & (np.abs(t) < f(np.inf))
                            four.append(t)
                    taps.append(four)
                yield p, s, xs, ys, g, taps
        if cells is not None:
            ok = cells["ok"][p]
        yield p, None, ok


def restatement(src, matrices, lens_rows, size, k=1, lut=None, clip=None, dtype=np.float32, detail=False):
    """src: float32 [P,3,Hs,Ws] or uint8 [P,Hs,Ws,3]; matrices float32 [P,9]; lens_rows float32 [P,9]; size (Hd, Wd) ->
    (values [P,3,Hd,Wd], weights [P,Hd,Wd]) of `dtype`; detail=True adds capture_checks.restatement's dict (valid, x0, y0,
    spread) with "mono_refused" [P,k*k,Hd,Wd]: sub-samples invalid by mono alone."""
    f = dtype
    P, (Hd, Wd) = np.asarray(src).shape[0], size
    values, weights = np.zeros((P, 3, Hd, Wd), f), np.zeros((P, Hd, Wd), f)
    info = dict(valid=np.zeros((P, k * k, Hd, Wd), bool), x0=np.zeros((P, k * k, Hd, Wd), np.int64),
                y0=np.zeros((P, k * k, Hd, Wd), np.int64), spread=np.zeros((P, Hd, Wd), f),
                mono_refused=np.zeros((P, k * k, Hd, Wd), bool))
    zero, scale = f(0.0), f(1.0 / (k * k))
    acc = [None, None, None]
    with np.errstate(all="ignore"):
        for item in _walk(src, matrices, lens_rows, size, k, lut, clip, f, None):
            if item[1] is None:
                p, _, ok = item
                for ch in range(3):
                    values[p, ch] = np.where(ok, acc[ch] * scale, zero)
                weights[p] = np.where(ok, f(1.0), zero)
                acc = [None, None, None]
                continue
            p, s, xs, ys, g, taps = item
            info["valid"][p, s], info["x0"][p, s], info["y0"][p, s] = g["valid"], g["x0f"].astype(np.int64), g["y0f"].astype(np.int64)
            Hs, Ws = (src.shape[1], src.shape[2]) if np.asarray(src).dtype == np.uint8 else (src.shape[2], src.shape[3])
            info["mono_refused"][p, s] = (g["Z"] > 0) & (g["ud"] >= 0) & (g["ud"] <= Ws - 1) & (g["vd"] >= 0) \
                & (g["vd"] <= Hs - 1) & ~(g["mono"] > 0)
            for ch in range(3):
                a, b, c, d = taps[ch]
                top = a + g["fx"] * (b - a)
                bot = c + g["fx"] * (d - c)
                val = top + g["fy"] * (bot - top)
                acc[ch] = val if acc[ch] is None else acc[ch] + val
                info["spread"][p] = np.maximum(info["spread"][p], np.where(
                    np.isfinite(a + b + c + d), np.maximum.reduce(taps[ch]) - np.minimum.reduce(taps[ch]), zero))
    assert values.dtype == f and weights.dtype == f
    return (values, weights, info) if detail else (values, weights)


def grad_terms(src, matrices, lens_rows, size, grad_values, k=1, lut=None, clip=None, dtype=np.float32, cells=None):
    """-> (terms [P,k*k,18,Hd,Wd] of `dtype`: the nine matrix terms, then the nine lens terms in the lens's order, 0 where the
    pixel's `ok` is false; ok [P,Hd,Wd] bool; cells).  `cells`: the dict a float32 run returned -- valid, x0f, y0f per
    sub-sample and ok -- to be held constant by a float64 run (None: the run's own)."""
    f = dtype
    P, (Hd, Wd) = np.asarray(src).shape[0], size
    G = np.asarray(grad_values).astype(f)
    Ls = np.asarray(lens_rows, np.float32).reshape(P, 9).astype(f)
    terms = np.zeros((P, k * k, 18, Hd, Wd), f)
    oks = np.zeros((P, Hd, Wd), bool)
    own = dict(valid=np.zeros((P, k * k, Hd, Wd), bool), x0f=np.zeros((P, k * k, Hd, Wd), np.float64),
               y0f=np.zeros((P, k * k, Hd, Wd), np.float64), ok=oks)
    zero, one, scale = f(0.0), f(1.0), f(1.0 / (k * k))
    with np.errstate(all="ignore"):
        for item in _walk(src, matrices, lens_rows, size, k, lut, clip, f, cells):
            if item[1] is None:
                p, _, ok = item
                oks[p] = ok
                terms[p] = np.where(ok[None, None], terms[p], zero)     # a select
                continue
            p, s, xs, ys, c, taps = item
            own["valid"][p, s], own["x0f"][p, s], own["y0f"][p, s] = c["valid"], c["x0f"], c["y0f"]
            fx, fy, cx, cy, k1, k2, p1, p2, k3 = Ls[p]
            du, dv = [], []
            for ch in range(3):
                ta, tb, tc, td = taps[ch]
                ba = tb - ta
                dc = td - tc
                du.append(ba + c["fy"] * (dc - ba))
                top = ta + c["fx"] * ba
                bot = tc + c["fx"] * dc
                dv.append(bot - top)
            g = G[p]
            gud = ((g[0] * du[0] + g[1] * du[1]) + g[2] * du[2]) * scale
            gvd = ((g[0] * dv[0] + g[1] * dv[1]) + g[2] * dv[2]) * scale
            a = gud * fx
            b = gvd * fy
            k2_2, k3_3 = f(2.0) * k2, f(3.0) * k3
            p1_2, p1_6, p2_2, p2_6 = f(2.0) * p1, f(6.0) * p1, f(2.0) * p2, f(6.0) * p2
            r2, xn, yn, rad, t, xx2, yy2 = c["r2"], c["xn"], c["yn"], c["rad"], c["t"], c["xx2"], c["yy2"]
            q = k1 + (r2 * (k2_2 + (k3_3 * r2)))
            jxx = ((rad + (xx2 * q)) + (p1_2 * yn)) + (p2_6 * xn)
            jxy = ((t * q) + (p1_2 * xn)) + (p2_2 * yn)
            jyy = ((rad + (yy2 * q)) + (p1_6 * yn)) + (p2_2 * xn)
            gxn = (a * jxx) + (b * jxy)
            gyn = (a * jxy) + (b * jyy)
            gu = gxn / fx
            gv = gyn / fy
            rz = one / c["Z"]
            pu = gu * rz
            pv = gv * rz
            pz = -((pu * c["u"]) + (pv * c["v"]))
            sx = (a * xn) + (b * yn)
            s1 = sx * r2
            s2 = s1 * r2
            s3 = s2 * r2
            planes = (pu * xs, pu * ys, pu, pv * xs, pv * ys, pv, pz * xs, pz * ys, pz,
                      (gud * c["xd"]) - (gu * xn), (gvd * c["yd"]) - (gv * yn), gud - gu, gvd - gv, s1, s2,
                      (a * t) + (b * (r2 + yy2)), (a * (r2 + xx2)) + (b * t), s3)
            for n, plane in enumerate(planes):
                terms[p, s, n] = plane
    assert terms.dtype == f
    return terms, oks, own


def sums(terms):
    """-> (ref [P,18], A [P,18]): the float64 sum of the term planes and of their absolute values"""
    t = terms.astype(np.float64)
    return t.sum(axis=(1, 3, 4)), np.abs(t).sum(axis=(1, 3, 4))


# ------------------------------------------------------------------------------------------------ torch

def torch_lens_map(u, v, L):
    """(ud, vd, mono) of the polynomial in torch ops; L: sequence of nine tensors or numbers broadcastable against u"""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = L
    xn, yn = (u - cx) / fx, (v - cy) / fy
    xx, yy, xy = xn * xn, yn * yn, xn * yn
    r2 = xx + yy
    rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    mono = 1.0 + r2 * (3.0 * k1 + r2 * (5.0 * k2 + r2 * (7.0 * k3)))
    xd = xn * rad + (p1 * (2.0 * xy) + p2 * (r2 + 2.0 * xx))
    yd = yn * rad + (p1 * (r2 + 2.0 * yy) + p2 * (2.0 * xy))
    return xd * fx + cx, yd * fy + cy, mono


def torch_forward(img, M, L, size, k, cells):
    """The forward's values [P,3,Hd,Wd] in torch ops of M's dtype (float64), differentiable towards M [P,9] and L [P,9]; img
    [P,3,Hs,Ws] the decoded source; the cell (x0f, y0f), `valid` and `ok` are the constants of `cells`."""
    P, _, Hs, Ws = img.shape
    Hd, Wd = size
    dt = M.dtype
    xg = torch.arange(Wd, dtype=dt).view(1, 1, Wd).expand(P, Hd, Wd)
    yg = torch.arange(Hd, dtype=dt).view(1, Hd, 1).expand(P, Hd, Wd)
    m = M.reshape(P, 9, 1, 1)
    rows = [L.reshape(P, 9)[:, n].view(P, 1, 1) for n in range(9)]
    ok = torch.from_numpy(cells["ok"])
    pidx = torch.arange(P).view(P, 1, 1, 1)
    cidx = torch.arange(3).view(1, 3, 1, 1)
    acc = None
    for j in range(k):
        for i in range(k):
            s = j * k + i
            xs, ys = xg + ((i + 0.5) / k - 0.5), yg + ((j + 0.5) / k - 0.5)
            X = (m[:, 0] * xs + m[:, 1] * ys) + m[:, 2]
            Y = (m[:, 3] * xs + m[:, 4] * ys) + m[:, 5]
            Z = (m[:, 6] * xs + m[:, 7] * ys) + m[:, 8]
            valid = torch.from_numpy(cells["valid"][:, s])
            ud, vd, _ = torch_lens_map(X / Z, Y / Z, rows)
            u = torch.where(valid, ud, torch.zeros_like(X))
            v = torch.where(valid, vd, torch.zeros_like(Y))
            x0f, y0f = torch.from_numpy(cells["x0f"][:, s]).to(dt), torch.from_numpy(cells["y0f"][:, s]).to(dt)
            fx, fy = (u - x0f)[:, None], (v - y0f)[:, None]
            x0, y0 = x0f.long()[:, None], y0f.long()[:, None]
            x1, y1 = (x0 + 1).clamp(max=Ws - 1), (y0 + 1).clamp(max=Hs - 1)
            a, b, c, d = img[pidx, cidx, y0, x0], img[pidx, cidx, y0, x1], img[pidx, cidx, y1, x0], img[pidx, cidx, y1, x1]
            top = a + fx * (b - a)
            bot = c + fx * (d - c)
            val = top + fy * (bot - top)
            acc = val if acc is None else acc + val
    return torch.where(ok[:, None], acc * (1.0 / (k * k)), torch.zeros_like(acc))


def autograd_grad(src, matrices, lens_rows, size, grad_values, k, lut, cells):
    """float64 [P,18]: torch autograd of sum(grad_values * torch_forward) towards the matrices and the lens rows"""
    M = torch.from_numpy(np.asarray(matrices, np.float32).reshape(-1, 9).astype(np.float64)).requires_grad_(True)
    L = torch.from_numpy(np.asarray(lens_rows, np.float32).reshape(-1, 9).astype(np.float64)).requires_grad_(True)
    val = torch_forward(gc.decoded(src, lut), M, L, size, k, cells)
    G = torch.from_numpy(np.asarray(grad_values, np.float64))
    (torch.where(torch.from_numpy(cells["ok"])[:, None], G, torch.zeros_like(G)) * val).sum().backward()
    return np.concatenate((M.grad.numpy(), L.grad.numpy()), axis=1)


def torch_composition(src, matrices, lens_rows, size, lut=None, clip=None, dtype=torch.float32):
    """capture_checks.torch_composition with the lens polynomial in torch ops between the quotient and grid_sample, k = 1, on
    the device of `src`; matrices [P,9], lens_rows [P,9] (either may require grad) -> (values [P,3,Hd,Wd], weights)."""
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
    L = lens_rows.to(device=dev, dtype=dtype).reshape(P, 9, 1, 1)
    xs = torch.arange(Wd, device=dev, dtype=dtype).view(1, 1, Wd).expand(P, Hd, Wd)
    ys = torch.arange(Hd, device=dev, dtype=dtype).view(1, Hd, 1).expand(P, Hd, Wd)
    X = (m[:, 0] * xs + m[:, 1] * ys) + m[:, 2]
    Y = (m[:, 3] * xs + m[:, 4] * ys) + m[:, 5]
    Z = (m[:, 6] * xs + m[:, 7] * ys) + m[:, 8]
    u, v, mono = torch_lens_map(X / Z, Y / Z, [L[:, n] for n in range(9)])
    valid = (Z > 0) & (L[:, 0] > 0) & (L[:, 1] > 0) & (mono > 0) & (u >= 0) & (u <= Ws - 1) & (v >= 0) & (v <= Hs - 1)
    u, v = torch.where(valid, u, torch.zeros_like(u)), torch.where(valid, v, torch.zeros_like(v))
    grid = torch.stack((2.0 * u / max(Ws - 1, 1) - 1.0, 2.0 * v / max(Hs - 1, 1) - 1.0), dim=-1)
    clean = torch.where(bad[:, None], torch.zeros_like(img), img) if not u8 else img
    val = torch.nn.functional.grid_sample(clean, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    padded = torch.nn.functional.pad(bad[:, None].to(dtype), (0, 1, 0, 1), mode="replicate")
    spread = torch.nn.functional.max_pool2d(padded, kernel_size=2, stride=1)[:, 0]
    x0, y0 = u.detach().floor().long().clamp_(0, Ws - 1), v.detach().floor().long().clamp_(0, Hs - 1)
    touched = spread.reshape(P, -1).gather(1, (y0 * Ws + x0).reshape(P, -1)).reshape(P, Hd, Wd) > 0
    ok = valid & ~touched
    return torch.where(ok[:, None], val, torch.zeros_like(val)), ok.to(dtype)


# ------------------------------------------------------------------------------------------------ on the device

def _device_source(src, dev, src_offset):
    src = np.ascontiguousarray(src)
    u8 = src.dtype == np.uint8
    sbuf = torch.zeros(src.size + src_offset + 16, dtype=torch.uint8 if u8 else torch.float32, device=dev)
    sview = sbuf[src_offset:src_offset + src.size]
    sview.copy_(torch.from_numpy(src.reshape(-1)))
    Hs, Ws = (src.shape[1], src.shape[2]) if u8 else (src.shape[2], src.shape[3])
    return sview, u8, src.shape[0], Hs, Ws


def _device_floats(values, dev, offset):
    values = np.ascontiguousarray(values, np.float32).reshape(-1)
    buf = torch.zeros(values.size + offset, dtype=torch.float32, device=dev)
    buf[offset:].copy_(torch.from_numpy(values))
    return buf[offset:]


def abi_rectify_lens(native, dev, src, matrices, lens_rows, size, k=1, lut=None, clip=None, src_offset=0, ptr_offset=0,
                     want_weights=True):
    """svbrdf_rectify_photos_lens called with raw device pointers; `src_offset`: ELEMENTS by which the source is moved off its
    allocation's alignment, `ptr_offset`: floats by which matrices, lens and the two outputs are.  The outputs sit between
    canaries.  -> dict(values, weights or None, canaries_intact, launches)"""
    lib = native._load()
    sview, u8, P, Hs, Ws = _device_source(src, dev, src_offset)
    Hd, Wd = size
    pad, canary = 64, -7.0
    mats, rows = _device_floats(matrices, dev, ptr_offset), _device_floats(lens_rows, dev, ptr_offset)
    assert mats.numel() == P * 9 == rows.numel()
    table = None if lut is None else torch.as_tensor(lut, dtype=torch.float32).to(dev)
    n_out, n_w = P * 3 * Hd * Wd, P * Hd * Wd
    obuf = torch.full((n_out + 2 * pad + ptr_offset,), canary, dtype=torch.float32, device=dev)
    wbuf = torch.full((n_w + 2 * pad + ptr_offset,), canary, dtype=torch.float32, device=dev)
    o0 = pad + ptr_offset
    lo, hi = (-np.inf, np.inf) if clip is None else clip
    before = native.launch_count()
    rc = lib.svbrdf_rectify_photos_lens(sview.data_ptr(), cc.U8_INTERLEAVED if u8 else cc.F32_PLANAR, P, Hs, Ws, mats.data_ptr(),
                                        rows.data_ptr(), Hd, Wd, k, None if table is None else table.data_ptr(),
                                        ctypes.c_float(lo), ctypes.c_float(hi), obuf[o0:].data_ptr(),
                                        wbuf[o0:].data_ptr() if want_weights else None,
                                        ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0, (rc, lib.svbrdf_last_error())
    torch.cuda.synchronize(dev)
    o, w = obuf.cpu().numpy(), wbuf.cpu().numpy()
    intact = (o[:o0] == canary).all() and (o[o0 + n_out:] == canary).all() and (w[:o0] == canary).all() \
        and (w[o0 + n_w:] == canary).all() and (want_weights or (w == canary).all())
    return dict(values=o[o0:o0 + n_out].reshape(P, 3, Hd, Wd), weights=w[o0:o0 + n_w].reshape(P, Hd, Wd) if want_weights else None,
                canaries_intact=bool(intact), launches=native.launch_count() - before)


def abi_lens_grad(native, dev, src, matrices, lens_rows, size, grad_values, k=1, lut=None, clip=None, src_offset=0,
                  ptr_offset=0, workspace=None):
    """svbrdf_rectify_photos_lens_grad called with raw device pointers (offsets as abi_rectify_lens; grad_values and the two
    results are moved by `ptr_offset` as well).  The results sit between canaries.  `workspace`: an int64 tensor to reuse
    (None: a fresh zeroed one).  -> dict(grad [P,18]: matrices then lens, canaries_intact, launches, workspace, workspace_zero)"""
    lib = native._load()
    sview, u8, P, Hs, Ws = _device_source(src, dev, src_offset)
    Hd, Wd = size
    pad, canary = 16, -7.0
    mats, rows = _device_floats(matrices, dev, ptr_offset), _device_floats(lens_rows, dev, ptr_offset)
    assert mats.numel() == P * 9 == rows.numel()
    gv = np.ascontiguousarray(grad_values, np.float32)
    assert gv.shape == (P, 3, Hd, Wd)
    gbuf = _device_floats(gv, dev, ptr_offset)
    table = None if lut is None else torch.as_tensor(lut, dtype=torch.float32).to(dev)
    bufs = [torch.full((P * 9 + 2 * pad + ptr_offset,), canary, dtype=torch.float32, device=dev) for _ in range(2)]
    o0 = pad + ptr_offset
    nbytes = lib.svbrdf_rectify_lens_grad_workspace_bytes(P, Hd, Wd)
    assert nbytes >= 4 * P + 72 * P * ((Wd + 63) // 64) * ((Hd + 3) // 4)
    if workspace is None:
        workspace = torch.zeros((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    assert workspace.numel() * 8 >= nbytes
    lo, hi = (-np.inf, np.inf) if clip is None else clip
    before = native.launch_count()
    rc = lib.svbrdf_rectify_photos_lens_grad(
        sview.data_ptr(), cc.U8_INTERLEAVED if u8 else cc.F32_PLANAR, P, Hs, Ws, mats.data_ptr(), rows.data_ptr(), Hd, Wd, k,
        None if table is None else table.data_ptr(), ctypes.c_float(lo), ctypes.c_float(hi), gbuf.data_ptr(),
        bufs[0][o0:].data_ptr(), bufs[1][o0:].data_ptr(), workspace.data_ptr(), workspace.numel() * 8,
        ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0, (rc, lib.svbrdf_last_error())
    torch.cuda.synchronize(dev)
    outs = [b.cpu().numpy() for b in bufs]
    intact = all((o[:o0] == canary).all() and (o[o0 + P * 9:] == canary).all() for o in outs)
    grad = np.concatenate([o[o0:o0 + P * 9].reshape(P, 9) for o in outs], axis=1)
    return dict(grad=grad, canaries_intact=bool(intact), launches=native.launch_count() - before, workspace=workspace,
                workspace_zero=not bool(workspace.any().item()))


def measure_lens(dev, native, P=8, src_size=(480, 640), dst_size=(256, 256), k=1, sets=4, n=30, rounds=3):
    """-> dict of medians (us per call), timed as capture_checks.measure_capture times: one process, `sets` rotating uint8
    source batches, the legs alternating round by round.  "lens_us" / "pinhole_us": the two forward launches;
    "composed_us": torch_composition; "lens_grad_us" / "pinhole_grad_us": the two gradient launches; "composed_grad_us": the
    backward of torch_composition towards matrices and lens (its forward built once per batch, outside the timing)."""
    import photo_checks
    from svbrdf_estimation_amd import capture
    Hs, Ws = src_size
    lut = capture.gamma_lut().to(dev)
    clip = (5, 250)
    M = torch.from_numpy(cc.matrices("outside", src_size, dst_size, P)).to(dev)
    L = torch.from_numpy(lenses("barrel", src_size, P)).to(dev)
    srcs = [torch.randint(0, 256, (P, Hs, Ws, 3), dtype=torch.uint8, device=dev) for _ in range(sets)]
    G = torch.randn((P, 3) + tuple(dst_size), device=dev)
    head = (cc.U8_INTERLEAVED, P, Hs, Ws, M)
    tail = (dst_size[0], dst_size[1], k, lut, float(clip[0]), float(clip[1]), G)
    Mreq, Lreq = M.clone().requires_grad_(True), L.clone().requires_grad_(True)
    graphs = [torch_composition(s, Mreq, Lreq, dst_size, lut=lut, clip=clip)[0] for s in srcs]
    legs = (
        ("lens_us", lambda i: capture.rectify(srcs[i % sets], M, dst_size, lut=lut, clip=clip, samples=k, lens=L)),
        ("pinhole_us", lambda i: capture.rectify(srcs[i % sets], M, dst_size, lut=lut, clip=clip, samples=k)),
        ("composed_us", lambda i: torch_composition(srcs[i % sets], M, L, dst_size, lut=lut, clip=clip)),
        ("lens_grad_us", lambda i: native.rectify_lens_grad(srcs[i % sets], *head, L, *tail)),
        ("pinhole_grad_us", lambda i: native.rectify_grad_matrices(srcs[i % sets], *head, *tail)),
        ("composed_grad_us", lambda i: torch.autograd.grad(graphs[i % sets], (Mreq, Lreq), G, retain_graph=True)),
    )
    out, res = photo_checks.timed_legs(legs, n, rounds, photo_checks.spinning_wave(native, dev), dev)
    out.update(rounds=res, device=torch.cuda.get_device_name(dev), P=P, src_size=src_size, dst_size=dst_size, k=k)
    return out


# ------------------------------------------------------------------------------------------------ refinement

REF_K1, REF_K2, REF_FOCAL, REF_LR_K1 = -0.18, 0.04, 0.8, 0.01


def reference_lens(k1=REF_K1, k2=REF_K2):
    """float64 [9]: the dry run's lens on capture_grad_checks' 96 x 128 source"""
    Hs, Ws = gc.REG_SRC
    return np.array([REF_FOCAL * Ws, REF_FOCAL * Ws, (Ws - 1) / 2.0, (Hs - 1) / 2.0, k1, k2, 0.0, 0.0, 0.0])


def refinement_loop(rectify, target, target_w, corners0=None, steps=gc.REG_STEPS, k1_start=0.0):
    """Adam on k1 (its own group, lr REF_LR_K1) and, if `corners0` is given, on the eight corner coordinates (lr REG_LR);
    rectify(M [1,3,3] float64, lens [9] float64) -> (values [1,3,H,W], weights [1,H,W]); the loss is
    capture_grad_checks.registration_loop's squared log difference.  -> (k1, corners [4,2])"""
    from svbrdf_estimation_amd import capture
    base = torch.from_numpy(reference_lens(0.0, REF_K2))
    k1 = torch.tensor(k1_start, dtype=torch.float64, requires_grad=True)
    fit_corners = corners0 is not None
    corners = torch.tensor((corners0 if fit_corners else gc.REG_CORNERS)[None], dtype=torch.float64, requires_grad=fit_corners)
    groups = [dict(params=[k1], lr=REF_LR_K1)] + ([dict(params=[corners], lr=gc.REG_LR)] if fit_corners else [])
    opt = torch.optim.Adam(groups)
    logt = (target + gc.REG_EPS).log()
    pick = torch.zeros(9, dtype=torch.float64)
    pick[4] = 1.0
    for _ in range(steps):
        opt.zero_grad()
        vals, w = rectify(capture.corner_matrices(corners, gc.REG_GRID), base + pick * k1)
        w = (w * target_w).detach()
        loss = (w[:, None] * ((vals + gc.REG_EPS).log() - logt) ** 2).sum() / (3.0 * w.sum())
        loss.backward()
        opt.step()
    return float(k1.detach()), corners.detach()[0]


def cpu_float64_rectify(src):
    """rectify(M, lens) for refinement_loop on the CPU in float64: torch_forward on the cells of the float64 forward itself
    (capture_grad_checks.cpu_float64_rectify's way: the cells are taken under the inputs rounded to float32)"""
    img = torch.from_numpy(src.astype(np.float64))
    gz = np.zeros((1, 3) + gc.REG_GRID)

    def rectify(M, L):
        _, ok, cells = grad_terms(src, M.detach().numpy().astype(np.float32), L.detach().numpy().astype(np.float32), gc.REG_GRID,
                                  gz, dtype=np.float64)
        return torch_forward(img, M.reshape(1, 9), L.reshape(1, 9), gc.REG_GRID, 1, cells), torch.from_numpy(ok.astype(np.float64))
    return rectify
