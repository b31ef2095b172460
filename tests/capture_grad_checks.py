"""The checker of the gradient of svbrdf_estimation_amd.capture.rectify towards its matrices (csrc/svbrdf_capture_grad.hip:
k_homography_grad; svbrdf_rectify_photos_grad_matrices):

  * ``grad_terms``: the definition of include/svbrdf_hip.h in numpy, one individually rounded operation per statement -> the
    nine terms of every sub-sample as planes.  In float32 it is the oracle of the GPU tests: the kernel's terms are these bit
    for bit, and what is left between the kernel's sums and the exact sum of the planes is the kernel's additions, bounded
    by ``bound``.  The same statements in float64 (``dtype=np.float64``), on the float32 run's cells, are held against
    torch's float64 autograd on the CPU;
  * ``torch_forward``: the forward composed of differentiable torch ops, any k, with the tap cell given as a constant
    (``floor().detach()``) -- what autograd differentiates;
  * ``abi_grad``: the C entry called with raw device pointers;
  * the registration loop of the tests and of its CPU dry run, and its band-limited source.
"""
import ctypes

import numpy as np
import torch

import capture_checks as cc


def depth():
    """D: the float32 additions one term passes through at most (the binding's constant)"""
    from svbrdf_estimation_amd import _native
    return _native.RECTIFY_GRAD_DEPTH


def bound(A, extra=0):
    """|got_n - ref_n| <= (D + 2) 2^-24 A_n: D float32 additions, the term's own last rounding, the final rounding"""
    return (depth() + 2 + extra) * 2.0 ** -24 * A


def grad_terms(src, matrices, size, grad_values, k=1, lut=None, clip=None, dtype=np.float32, cells=None):
    """src: float32 [P,3,Hs,Ws] or uint8 [P,Hs,Ws,3]; matrices float32 [P,9]; size (Hd, Wd); grad_values [P,3,Hd,Wd];
    k in {1,2,4} -> (terms [P,k*k,9,Hd,Wd] of `dtype`, 0 where the pixel's `ok` is false; ok [P,Hd,Wd] bool; cells).
    `cells`: the dict a float32 run returned -- valid, x0f, y0f per sub-sample and ok -- to be held constant by a float64
    run (None: the run's own)."""
    f = dtype
    src = np.asarray(src)
    u8 = src.dtype == np.uint8
    P = src.shape[0]
    Hs, Ws = (src.shape[1], src.shape[2]) if u8 else (src.shape[2], src.shape[3])
    Hd, Wd = size
    M = np.asarray(matrices, np.float32).reshape(P, 9).astype(f)
    G = np.asarray(grad_values).astype(f)
    if u8:
        table = np.asarray(lut, np.float32).astype(f)
        lo, hi = (-1, 256) if clip is None else (int(np.floor(max(-1.0, min(256.0, clip[0])))), int(np.ceil(max(-1.0, min(256.0, clip[1])))))
    else:
        lo, hi = (f(-np.inf), f(np.inf)) if clip is None else (f(np.float32(clip[0])), f(np.float32(clip[1])))
    wmax, hmax, zero, one = f(Ws - 1), f(Hs - 1), f(0.0), f(1.0)
    xg = np.broadcast_to(np.arange(Wd, dtype=f)[None, :], (Hd, Wd))
    yg = np.broadcast_to(np.arange(Hd, dtype=f)[:, None], (Hd, Wd))
    terms = np.zeros((P, k * k, 9, Hd, Wd), f)
    oks = np.zeros((P, Hd, Wd), bool)
    own = dict(valid=np.zeros((P, k * k, Hd, Wd), bool), x0f=np.zeros((P, k * k, Hd, Wd), np.float64),
               y0f=np.zeros((P, k * k, Hd, Wd), np.float64), ok=oks)
    scale = f(1.0 / (k * k))
    with np.errstate(all="ignore"):
        for p in range(P):
            m = M[p]
            ok = np.ones((Hd, Wd), bool)
            for j in range(k):
                for i in range(k):
                    s = j * k + i
                    xs = xg + f((i + 0.5) / k - 0.5)
                    ys = yg + f((j + 0.5) / k - 0.5)
                    X = (m[0] * xs + m[1] * ys) + m[2]
                    Y = (m[3] * xs + m[4] * ys) + m[5]
                    Z = (m[6] * xs + m[7] * ys) + m[8]
                    u, v = X / Z, Y / Z
                    valid = (Z > zero) & (u >= zero) & (u <= wmax) & (v >= zero) & (v <= hmax)
                    if cells is not None:
                        valid = cells["valid"][p, s]
                    ok &= valid
                    uc, vc = np.where(valid, u, zero), np.where(valid, v, zero)
                    uc, vc = np.fmin(np.fmax(uc, zero), wmax), np.fmin(np.fmax(vc, zero), hmax)
                    x0f, y0f = np.floor(uc), np.floor(vc)
                    if cells is not None:
                        x0f, y0f = cells["x0f"][p, s].astype(f), cells["y0f"][p, s].astype(f)
                    fx, fy = uc - x0f, vc - y0f
                    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
                    x1, y1 = np.minimum(x0 + 1, Ws - 1), np.minimum(y0 + 1, Hs - 1)
                    own["valid"][p, s], own["x0f"][p, s], own["y0f"][p, s] = valid, x0f, y0f
                    du, dv = [], []
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
                        ba = b - a
                        dc = d - c
                        du.append(ba + fy * (dc - ba))
                        top = a + fx * ba
                        bot = c + fx * dc
                        dv.append(bot - top)
                    g = G[p]
                    gu = ((g[0] * du[0] + g[1] * du[1]) + g[2] * du[2]) * scale
                    gv = ((g[0] * dv[0] + g[1] * dv[1]) + g[2] * dv[2]) * scale
                    rz = one / Z
                    pu = gu * rz
                    pv = gv * rz
                    pz = -((pu * u) + (pv * v))
                    for n, t in enumerate((pu * xs, pu * ys, pu, pv * xs, pv * ys, pv, pz * xs, pz * ys, pz)):
                        terms[p, s, n] = t
            if cells is not None:
                ok = cells["ok"][p]
            oks[p] = ok
            terms[p] = np.where(ok[None, None], terms[p], zero)     # a select: whatever stood under a refused pixel is gone
    assert terms.dtype == f
    return terms, oks, own


def sums(terms):
    """-> (ref [P,9], A [P,9]): the float64 sum of the term planes and of their absolute values"""
    t = terms.astype(np.float64)
    return t.sum(axis=(1, 3, 4)), np.abs(t).sum(axis=(1, 3, 4))


def torch_forward(img, M, size, k, cells):
    """The forward's values [P,3,Hd,Wd] in torch ops of M's dtype (float64), differentiable towards M [P,9]; img [P,3,Hs,Ws]
    the decoded source; the cell (x0f, y0f), `valid` and `ok` are the constants of `cells` (a grad_terms run's)."""
    P, _, Hs, Ws = img.shape
    Hd, Wd = size
    dt = M.dtype
    xg = torch.arange(Wd, dtype=dt).view(1, 1, Wd).expand(P, Hd, Wd)
    yg = torch.arange(Hd, dtype=dt).view(1, Hd, 1).expand(P, Hd, Wd)
    m = M.reshape(P, 9, 1, 1)
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
            u = torch.where(valid, X / Z, torch.zeros_like(X))
            v = torch.where(valid, Y / Z, torch.zeros_like(Y))
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


def decoded(src, lut=None):
    """numpy source of either format -> float64 torch [P,3,Hs,Ws], NaN and infinities replaced by 0 (they sit under refused
    pixels only, and 0 * NaN would spoil the sum)"""
    src = np.asarray(src)
    if src.dtype == np.uint8:
        img = np.asarray(lut, np.float64)[src.astype(np.int64)].transpose(0, 3, 1, 2)
    else:
        img = src.astype(np.float64)
    return torch.from_numpy(np.ascontiguousarray(np.where(np.isfinite(img), img, 0.0)))


def autograd_grad(src, matrices, size, grad_values, k, lut, cells):
    """float64 [P,9]: torch autograd of sum(grad_values * torch_forward) towards the matrices"""
    M = torch.from_numpy(np.asarray(matrices, np.float32).reshape(-1, 9).astype(np.float64)).requires_grad_(True)
    val = torch_forward(decoded(src, lut), M, size, k, cells)
    G = torch.from_numpy(np.asarray(grad_values, np.float64))
    (torch.where(torch.from_numpy(cells["ok"])[:, None], G, torch.zeros_like(G)) * val).sum().backward()
    return M.grad.numpy()


# ------------------------------------------------------------------------------------------------ on the device

def abi_grad(native, dev, src, matrices, size, grad_values, k=1, lut=None, clip=None, src_offset=0, ptr_offset=0, workspace=None):
    """svbrdf_rectify_photos_grad_matrices called with raw device pointers.  `src_offset`: ELEMENTS by which the source is
    moved off its allocation's alignment; `ptr_offset`: floats by which matrices, grad_values and grad_matrices are.  The
    result sits between canaries.  `workspace`: an int64 tensor to reuse (None: a fresh zeroed one).
    -> dict(grad [P,9], canaries_intact, launches, workspace, workspace_zero: the scratch was left zeroed)"""
    lib = native._load()
    src = np.ascontiguousarray(src)
    u8 = src.dtype == np.uint8
    P = src.shape[0]
    Hs, Ws = (src.shape[1], src.shape[2]) if u8 else (src.shape[2], src.shape[3])
    Hd, Wd = size
    pad, canary = 16, -7.0
    sbuf = torch.zeros(src.size + src_offset + 16, dtype=torch.uint8 if u8 else torch.float32, device=dev)
    sview = sbuf[src_offset:src_offset + src.size]
    sview.copy_(torch.from_numpy(src.reshape(-1)))
    mbuf = torch.zeros(P * 9 + ptr_offset, dtype=torch.float32, device=dev)
    mbuf[ptr_offset:].copy_(torch.from_numpy(np.ascontiguousarray(matrices, np.float32).reshape(-1)))
    gv = np.ascontiguousarray(grad_values, np.float32)
    assert gv.shape == (P, 3, Hd, Wd)
    gbuf = torch.zeros(gv.size + ptr_offset, dtype=torch.float32, device=dev)
    gbuf[ptr_offset:].copy_(torch.from_numpy(gv.reshape(-1)))
    table = None if lut is None else torch.as_tensor(lut, dtype=torch.float32).to(dev)
    obuf = torch.full((P * 9 + 2 * pad + ptr_offset,), canary, dtype=torch.float32, device=dev)
    o0 = pad + ptr_offset
    nbytes = lib.svbrdf_rectify_grad_workspace_bytes(P, Hd, Wd)
    assert nbytes >= 4 * P + 36 * P * ((Wd + 63) // 64) * ((Hd + 3) // 4)
    if workspace is None:
        workspace = torch.zeros((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    assert workspace.numel() * 8 >= nbytes
    lo, hi = (-np.inf, np.inf) if clip is None else clip
    before = native.launch_count()
    rc = lib.svbrdf_rectify_photos_grad_matrices(
        sview.data_ptr(), cc.U8_INTERLEAVED if u8 else cc.F32_PLANAR, P, Hs, Ws, mbuf[ptr_offset:].data_ptr(), Hd, Wd, k,
        None if table is None else table.data_ptr(), ctypes.c_float(lo), ctypes.c_float(hi), gbuf[ptr_offset:].data_ptr(),
        obuf[o0:].data_ptr(), workspace.data_ptr(), workspace.numel() * 8,
        ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0, (rc, lib.svbrdf_last_error())
    torch.cuda.synchronize(dev)
    o = obuf.cpu().numpy()
    intact = (o[:o0] == canary).all() and (o[o0 + P * 9:] == canary).all()
    return dict(grad=o[o0:o0 + P * 9].reshape(P, 9), canaries_intact=bool(intact), launches=native.launch_count() - before,
                workspace=workspace, workspace_zero=not bool(workspace.any().item()))


def measure_grad(dev, native, P=8, src_size=(480, 640), dst_size=(256, 256), k=1, sets=4, n=30, rounds=3, composed=True):
    """-> dict of medians (us per call), timed as capture_checks.measure_capture times: one process, `sets` rotating uint8
    source batches, the legs alternating round by round.  "fused_us": the one launch of the gradient; "forward_us": the
    forward's launch; "composed_us": the BACKWARD of capture_checks.torch_composition towards the matrices (grid_sample's
    backward and the chain to M; its forward is built once per batch, outside the timing, and its graph kept)."""
    import photo_checks
    from svbrdf_estimation_amd import capture
    Hs, Ws = src_size
    lut = capture.gamma_lut().to(dev)
    clip = (5, 250)
    M = torch.from_numpy(cc.matrices("outside", src_size, dst_size, P)).to(dev)
    srcs = [torch.randint(0, 256, (P, Hs, Ws, 3), dtype=torch.uint8, device=dev) for _ in range(sets)]
    G = torch.randn((P, 3) + tuple(dst_size), device=dev)
    args = (cc.U8_INTERLEAVED, P, Hs, Ws, M, dst_size[0], dst_size[1], k, lut, float(clip[0]), float(clip[1]), G)

    def fused(i):
        native.rectify_grad_matrices(srcs[i % sets], *args)

    def forward(i):
        capture.rectify(srcs[i % sets], M, dst_size, lut=lut, clip=clip, samples=k)

    legs = [("fused_us", fused), ("forward_us", forward)]
    if composed and k == 1:
        Mreq = M.clone().requires_grad_(True)
        graphs = [cc.torch_composition(s, Mreq, dst_size, lut=lut, clip=clip)[0] for s in srcs]

        def comp(i):
            torch.autograd.grad(graphs[i % sets], Mreq, G, retain_graph=True)

        legs.append(("composed_us", comp))
    out, res = photo_checks.timed_legs(tuple(legs), n, rounds, photo_checks.spinning_wave(native, dev), dev)
    out.update(rounds=res, device=torch.cuda.get_device_name(dev), P=P, src_size=src_size, dst_size=dst_size, k=k)
    return out


# ------------------------------------------------------------------------------------------------ the bits of the four entries

BITS_P, BITS_SRC, BITS_DST = 3, (37, 53), (9, 70)      # two tile columns (the second ragged) x three tile rows (the last ragged)
BITS_CASES = tuple((fmt, k) for fmt in ("uint8", "float32") for k in (1, 2, 4))


def record_bits(native, dev):
    """The four rectify entries of the loaded library on seeded inputs, 24 launches (and each gradient launch once more on
    the workspace its first call left): P = 3, source 37 x 53, destination 9 x 70 -- six tiles per photo, so a photo's last
    workgroup adds more than one partial; `outside` matrices, `barrel` lens rows with photo 2's replaced by a hostile one
    (k1 = NaN), uint8 sources under clip (5, 250) and float32 sources without a clip, k = 1, 2, 4.
    -> (bits, facts): bits maps "<fmt>_k<k>_<values|weights|grad_matrices|lens_values|lens_weights|lens_grad>" to float32
    arrays (lens_grad: [P,18], matrices then lens); facts maps the same case names to
    (canaries intact, one launch each, workspace zero after both calls, the second call's bits equal the first's)."""
    import capture_lens_checks as lc
    import synth
    from svbrdf_estimation_amd import capture
    M = cc.matrices("outside", BITS_SRC, BITS_DST, BITS_P)
    L = lc.lenses("barrel", BITS_SRC, BITS_P)
    L[2] = lc.hostile_lenses(BITS_SRC)["k1 = NaN"]
    G = synth.uniform01(71, (BITS_P, 3) + BITS_DST).astype(np.float32) * 2.0 - 1.0
    bits, facts = {}, {}
    for fmt, k in BITS_CASES:
        u8 = fmt == "uint8"
        src = cc.u8_source(72, BITS_P, *BITS_SRC, blobs=True) if u8 else cc.float_source(73, BITS_P, *BITS_SRC)
        kw = dict(k=k, lut=capture.gamma_lut().numpy() if u8 else None, clip=(5, 250) if u8 else None)
        name = "%s_k%d_" % (fmt, k)
        fwd = cc.abi_rectify(native, dev, src, M, BITS_DST, **kw)
        lens = lc.abi_rectify_lens(native, dev, src, M, L, BITS_DST, **kw)
        grad = abi_grad(native, dev, src, M, BITS_DST, G, **kw)
        grad2 = abi_grad(native, dev, src, M, BITS_DST, G, workspace=grad["workspace"], **kw)
        lgrad = lc.abi_lens_grad(native, dev, src, M, L, BITS_DST, G, **kw)
        lgrad2 = lc.abi_lens_grad(native, dev, src, M, L, BITS_DST, G, workspace=lgrad["workspace"], **kw)
        bits.update({name + "values": fwd["values"], name + "weights": fwd["weights"], name + "grad_matrices": grad["grad"],
                     name + "lens_values": lens["values"], name + "lens_weights": lens["weights"], name + "lens_grad": lgrad["grad"]})
        runs = (fwd, lens, grad, grad2, lgrad, lgrad2)
        facts[name] = (all(r["canaries_intact"] for r in runs), all(r["launches"] == 1 for r in runs),
                       all(r["workspace_zero"] for r in runs[2:]),
                       cc.same_bits(grad2["grad"], grad["grad"]) and cc.same_bits(lgrad2["grad"], lgrad["grad"]))
    return bits, facts


# ------------------------------------------------------------------------------------------------ registration

REG_SRC, REG_GRID, REG_STEPS, REG_LR, REG_OFF, REG_EPS = (96, 128), (32, 32), 150, 0.2, 3.0, 0.01
REG_SEED = 2
REG_CORNERS = np.array([[20.5, 14.25], [14.0, 80.5], [109.25, 84.0], [101.5, 10.75]])     # the patch in the 96 x 128 source


def band_limited_source(seed, Hs, Ws, waves=24, longest=0.5, shortest=12.0):
    """float32 [1,3,Hs,Ws] in (0, 1): per channel a sum of `waves` sinusoids with wavelengths between `shortest` pixels and
    `longest` of the image -- nothing a bilinear tap at one sample per 3 to 4 source pixels aliases badly"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:Hs, 0:Ws].astype(np.float64)
    img = np.zeros((3, Hs, Ws))
    for ch in range(3):
        for _ in range(waves):
            lam = np.exp(rng.uniform(np.log(shortest), np.log(longest * max(Hs, Ws))))
            th, ph = rng.uniform(0, 2 * np.pi, 2)
            img[ch] += rng.uniform(0.3, 1.0) * np.sin(2 * np.pi * (np.cos(th) * xx + np.sin(th) * yy) / lam + ph)
        img[ch] = 0.1 + 0.8 * (img[ch] - img[ch].min()) / (img[ch].max() - img[ch].min())
    return img[None].astype(np.float32)


def start_corners(seed, true=REG_CORNERS, off=REG_OFF):
    """every corner `off` source pixels from its place, in a direction drawn from `seed`"""
    ang = np.random.RandomState(seed).uniform(0, 2 * np.pi, 4)
    return true + off * np.stack((np.cos(ang), np.sin(ang)), axis=1)


def corner_error(corners, true=REG_CORNERS):
    c = corners.detach().cpu().numpy() if isinstance(corners, torch.Tensor) else np.asarray(corners)
    return float(np.sqrt(((c.reshape(4, 2) - true) ** 2).sum(axis=1)).mean())


def registration_loop(rectify, target, target_w, corners0, device, steps=REG_STEPS, lr=REG_LR, history=None, power=2):
    """Adam on the eight corner coordinates (float64 [1,4,2] on the host); rectify(M [1,3,3] float64 with grad) ->
    (values [1,3,H,W], weights [1,H,W]) on `device`; the loss is mean w |log(rect + eps) - log(target + eps)|^power with
    w = the product of the two weight planes.  power = 2 is the tests' loss: its gradient vanishes at the optimum, so the
    end of the loop is a place; with power = 1 (the loss of tools/fit_photos.py --fit-registration, robust against
    highlights) the gradient keeps its size, Adam at a fixed lr ends in a jitter of 0.01 to 0.07 px, and WHERE in it step 150
    falls turns on roundings (see test_gpu_capture_grad.py).  -> the final corners [4,2] (`history`: a list that receives the mean corner
    error before every step)"""
    from svbrdf_estimation_amd import capture
    corners = torch.tensor(corners0[None], dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([corners], lr=lr)
    logt = (target + REG_EPS).log()
    for _ in range(steps):
        if history is not None:
            history.append(corner_error(corners[0]))
        opt.zero_grad()
        vals, w = rectify(capture.corner_matrices(corners, REG_GRID))
        w = (w * target_w).detach()
        loss = (w[:, None] * ((vals + REG_EPS).log() - logt).abs() ** power).sum() / (3.0 * w.sum())
        loss.backward()
        opt.step()
    return corners.detach()[0]


def cpu_float64_rectify(src):
    """rectify(M) for registration_loop on the CPU in float64: torch_forward on the cells of the float64 forward itself"""
    img = torch.from_numpy(src.astype(np.float64))
    gz = np.zeros((1, 3) + REG_GRID)

    def rectify(M):
        _, ok, cells = grad_terms(src, M.detach().numpy().astype(np.float32), REG_GRID, gz, dtype=np.float64)
        return torch_forward(img, M.reshape(1, 9), REG_GRID, 1, cells), torch.from_numpy(ok.astype(np.float64))
    return rectify
