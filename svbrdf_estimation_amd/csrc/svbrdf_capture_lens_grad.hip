// svbrdf_capture_lens_grad.hip -- translation unit of libsvbrdf_hip.so: the gradient of svbrdf_rectify_photos_lens' values
// towards the 3x3 matrices, THROUGH the lens's Jacobian, and towards the nine lens entries, ONE launch (ABI version 8).
//
// Refining a registration photometrically under a lens needs d loss / d M through the distortion, and a lens coefficient can
// be refined the same way (one coefficient per stage: k1 and k2 trade off against each other on a patch that covers the
// middle of the frame).  k_lens_grad repeats the forward's gather (svbrdf_capture_lens_device.h: the
// same geometry, lens map, clamped addressing and tap rule) and reduces eighteen terms per sub-sample to eighteen floats
// per photo.
//
// Definition (include/svbrdf_hip.h has it in full; tests/capture_lens_checks.py restates it in numpy float32).  Everything
// up to the taps and the pixel's `ok` is the forward's.  The gradient is that of the forward's expression with the cell,
// `valid` (mono's sign included) and `ok` held constant.  With g_ch = grad_values[p, ch, y, x], per sub-sample, every line
// ONE individually rounded float32 operation (HIPFLAGS: -ffp-contract=off; no fused multiply-add written; IEEE `/`):
//     gud, gvd: svbrdf_capture_grad.hip's gu, gv, formed at the cell of (ud, vd)
//     a = gud fx;  b = gvd fy;  q = k1 + (r2 ((2 k2) + ((3 k3) r2)))
//     jxx = ((rad + ((2 xx) q)) + ((2 p1) yn)) + ((6 p2) xn)
//     jxy = ((t q) + ((2 p1) xn)) + ((2 p2) yn)
//     jyy = ((rad + ((2 yy) q)) + ((6 p1) yn)) + ((2 p2) xn)
//     gxn = (a jxx) + (b jxy);  gyn = (a jxy) + (b jyy);  gu = gxn / fx;  gv = gyn / fy
//     rz = 1 / Z;  pu = gu rz;  pv = gv rz;  pz = -((pu u) + (pv v))
//     matrix terms:  pu xs, pu ys, pu,  pv xs, pv ys, pv,  pz xs, pz ys, pz
//     s = (a xn) + (b yn);  s1 = s r2;  s2 = s1 r2;  s3 = s2 r2
//     lens terms:    (gud xd) - (gu xn),  (gvd yd) - (gv yn),  gud - gu,  gvd - gv,  s1,  s2,
//                    (a t) + (b (r2 + (2 yy))),  (a (r2 + (2 xx))) + (b t),  s3            (fx fy cx cy k1 k2 p1 p2 k3)
//
// The reduction is k_homography_grad's with eighteen words per workgroup instead of nine: K^2 - 1 thread additions, the
// 64-lane butterfly, (w0 + w1) + (w2 + w3) through LDS, write-through stores of the workgroup's words, a drain, the
// per-photo integer ticket; the last workgroup acquires, adds the partials in float64 in index order, rounds once and
// leaves the workspace zeroed.  No float atomic, no release fence; SVBRDF_RECTIFY_GRAD_DEPTH bounds this sum as the other.
#include "svbrdf_host.h"
#include "svbrdf_capture_device.h"
#include "svbrdf_capture_lens_device.h"

namespace {

static_assert(4 * 4 - 1 + 6 + 2 <= SVBRDF_RECTIFY_GRAD_DEPTH, "float32 additions a term passes through: thread, wave, waves");
constexpr int kLensGradWords = 18;                  // nine matrix terms, nine lens terms
constexpr int kLensGradTicketBytes = 256;           // the counters' block is padded to a multiple of this

inline size_t lens_grad_ticket_bytes(int P)
{
    return ((size_t)P * sizeof(unsigned) + kLensGradTicketBytes - 1) / kLensGradTicketBytes * kLensGradTicketBytes;
}

inline size_t lens_grad_tiles(int Hd, int Wd)
{
    return (size_t)((Wd + kRectifyTileW - 1) / kRectifyTileW) * (size_t)((Hd + kRectifyTileH - 1) / kRectifyTileH);
}

__device__ __forceinline__ double lens_shfl_xor_f64(double v, int mask)
{
    const unsigned long long bits = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)bits, mask, 64);
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(bits >> 32), mask, 64);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

template <bool U8, int K>
__global__ __launch_bounds__(kRectifyTileW * kRectifyTileH) void k_lens_grad(
    const void *__restrict__ src, const float *__restrict__ matrices, const float *__restrict__ lens,
    const float *__restrict__ lut, RectifyClip clip, const float *__restrict__ grad_values, float *__restrict__ grad_matrices,
    float *__restrict__ grad_lens, unsigned *tickets, float *partials, int Hs, int Ws, int Hd, int Wd)
{
    constexpr int N = kLensGradWords;
    constexpr int kLut = U8 ? 256 : 0;
    __shared__ float s_words[kLut + kRectifyTileH * N];     // the table, then the four waves' eighteen sums
    float *s_lut = s_words, *s_sums = s_words + kLut;
    if (U8) {
        s_lut[threadIdx.x] = lut[threadIdx.x];      // 256 threads, 256 entries
        __syncthreads();
    }
    const int p = blockIdx.z;
    const int lane = threadIdx.x & (kRectifyTileW - 1), wave = threadIdx.x / kRectifyTileW;
    const int x = blockIdx.x * kRectifyTileW + lane;
    const int y = blockIdx.y * kRectifyTileH + wave;
    const bool live = x < Wd && y < Hd;             // a thread beyond the destination adds exact zeros
    float m[9];
#pragma unroll
    for (int n = 0; n < 9; ++n) m[n] = matrices[(size_t)p * 9 + n];
    const RectifyLens L = rectify_lens_row(lens, p);
    const float k2_2 = 2.0f * L.k2, k3_3 = 3.0f * L.k3;
    const float p1_2 = 2.0f * L.p1, p1_6 = 6.0f * L.p1, p2_2 = 2.0f * L.p2, p2_6 = 6.0f * L.p2;
    const size_t plane = (size_t)Hs * Ws;
    const size_t base = (size_t)p * 3 * plane;      // first element of photo p in either layout
    const size_t dplane = (size_t)Hd * Wd;
    float g[3] = {0.0f, 0.0f, 0.0f};
    if (live) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) g[ch] = grad_values[((size_t)p * 3 + ch) * dplane + (size_t)y * Wd + x];
    }
    float acc[N];
    bool ok = live;
#pragma unroll
    for (int j = 0; j < K; ++j) {
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const float xs = (float)x + ((i + 0.5f) / K - 0.5f);        // the offset is a compile-time constant, exact
            const float ys = (float)y + ((j + 0.5f) / K - 0.5f);
            const RectifyLensCell c = rectify_lens_cell(m, L, xs, ys, Hs, Ws);
            ok = ok && c.valid;
            float du[3], dv[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float ta = rectify_tap<U8>(src, rectify_index<U8>(base, plane, Ws, c.y0, c.x0, ch), s_lut, clip, ok);
                const float tb = rectify_tap<U8>(src, rectify_index<U8>(base, plane, Ws, c.y0, c.x1, ch), s_lut, clip, ok);
                const float tc = rectify_tap<U8>(src, rectify_index<U8>(base, plane, Ws, c.y1, c.x0, ch), s_lut, clip, ok);
                const float td = rectify_tap<U8>(src, rectify_index<U8>(base, plane, Ws, c.y1, c.x1, ch), s_lut, clip, ok);
                const float ba = tb - ta;
                const float dc = td - tc;
                du[ch] = ba + c.fy * (dc - ba);
                const float top = ta + c.fx * ba;
                const float bot = tc + c.fx * dc;
                dv[ch] = bot - top;
            }
            const float gud = ((g[0] * du[0] + g[1] * du[1]) + g[2] * du[2]) * (1.0f / (K * K));
            const float gvd = ((g[0] * dv[0] + g[1] * dv[1]) + g[2] * dv[2]) * (1.0f / (K * K));
            const float a = gud * L.fx;
            const float b = gvd * L.fy;
            const float q = L.k1 + (c.r2 * (k2_2 + (k3_3 * c.r2)));
            const float xx2 = 2.0f * c.xx, yy2 = 2.0f * c.yy;
            const float jxx = ((c.rad + (xx2 * q)) + (p1_2 * c.yn)) + (p2_6 * c.xn);
            const float jxy = ((c.t * q) + (p1_2 * c.xn)) + (p2_2 * c.yn);
            const float jyy = ((c.rad + (yy2 * q)) + (p1_6 * c.yn)) + (p2_2 * c.xn);
            const float gxn = (a * jxx) + (b * jxy);
            const float gyn = (a * jxy) + (b * jyy);
            const float gu = gxn / L.fx;
            const float gv = gyn / L.fy;
            const float rz = 1.0f / c.Z;
            const float pu = gu * rz;
            const float pv = gv * rz;
            const float pz = -((pu * c.u) + (pv * c.v));
            const float s = (a * c.xn) + (b * c.yn);
            const float s1 = s * c.r2;
            const float s2 = s1 * c.r2;
            const float s3 = s2 * c.r2;
            const float t[N] = {pu * xs, pu * ys, pu, pv * xs, pv * ys, pv, pz * xs, pz * ys, pz,
                                (gud * c.xd) - (gu * c.xn), (gvd * c.yd) - (gv * c.yn), gud - gu, gvd - gv, s1, s2,
                                (a * c.t) + (b * (c.r2 + yy2)), (a * (c.r2 + xx2)) + (b * c.t), s3};
#pragma unroll
            for (int n = 0; n < N; ++n) acc[n] = (i == 0 && j == 0) ? t[n] : acc[n] + t[n];
        }
    }
#pragma unroll
    for (int n = 0; n < N; ++n) {
        float v = ok ? acc[n] : 0.0f;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        acc[n] = v;
    }
    if (lane == 0) {
#pragma unroll
        for (int n = 0; n < N; ++n) s_sums[wave * N + n] = acc[n];
    }
    __syncthreads();
    if (wave != 0) return;
    const size_t tiles = (size_t)gridDim.x * gridDim.y;
    const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    float *mine = partials + ((size_t)p * tiles + tile) * N;
    // the eighteen words go out WRITE-THROUGH (a relaxed agent-scope store), so no release fence is needed: drained, they
    // are in memory before the ticket is drawn
    if (lane < N) {
        const float v = (s_sums[lane] + s_sums[N + lane]) + (s_sums[2 * N + lane] + s_sums[3 * N + lane]);
        __hip_atomic_store(reinterpret_cast<unsigned *>(mine) + lane, __builtin_bit_cast(unsigned, v), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    unsigned ticket = 0;
    if (lane == 0) ticket = __hip_atomic_fetch_add(tickets + p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ticket = (unsigned)__builtin_amdgcn_readfirstlane((int)ticket);
    if ((size_t)ticket + 1 != tiles) return;
    // the photo's last workgroup: every other one's partial was in memory before its ticket was drawn
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    float *all = partials + (size_t)p * tiles * N;
    double sum[N];
#pragma unroll
    for (int n = 0; n < N; ++n) sum[n] = 0.0;
    for (size_t t = lane; t < tiles; t += 64) {
#pragma unroll
        for (int n = 0; n < N; ++n) {
            sum[n] += (double)all[t * N + n];
            all[t * N + n] = 0.0f;          // left zeroed
        }
    }
#pragma unroll
    for (int n = 0; n < N; ++n) {
        double v = sum[n];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += lens_shfl_xor_f64(v, off);
        sum[n] = v;
    }
    if (lane == 0) {
#pragma unroll
        for (int n = 0; n < 9; ++n) {
            grad_matrices[(size_t)p * 9 + n] = (float)sum[n];
            grad_lens[(size_t)p * 9 + n] = (float)sum[9 + n];
        }
        __hip_atomic_store(tickets + p, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <bool U8>
void launch_lens_grad(int k, dim3 grid, hipStream_t st, const void *src, const float *matrices, const float *lens,
                      const float *lut, RectifyClip clip, const float *grad_values, float *grad_matrices, float *grad_lens,
                      unsigned *tickets, float *partials, int Hs, int Ws, int Hd, int Wd)
{
    const dim3 block(kRectifyTileW * kRectifyTileH);
    if (k == 1)
        k_lens_grad<U8, 1><<<grid, block, 0, st>>>(src, matrices, lens, lut, clip, grad_values, grad_matrices, grad_lens, tickets,
                                                   partials, Hs, Ws, Hd, Wd);
    else if (k == 2)
        k_lens_grad<U8, 2><<<grid, block, 0, st>>>(src, matrices, lens, lut, clip, grad_values, grad_matrices, grad_lens, tickets,
                                                   partials, Hs, Ws, Hd, Wd);
    else
        k_lens_grad<U8, 4><<<grid, block, 0, st>>>(src, matrices, lens, lut, clip, grad_values, grad_matrices, grad_lens, tickets,
                                                   partials, Hs, Ws, Hd, Wd);
}

}  // namespace

extern "C" {

size_t svbrdf_rectify_lens_grad_workspace_bytes(int P, int Hd, int Wd)
{
    if (P < 1 || Hd < 1 || Wd < 1 || P > 65535 || Hd > kRectifyMaxDim || Wd > kRectifyMaxDim) return 0;
    return lens_grad_ticket_bytes(P) + (size_t)P * lens_grad_tiles(Hd, Wd) * kLensGradWords * sizeof(float);
}

int svbrdf_rectify_photos_lens_grad(const void *src, int src_format, int P, int Hs, int Ws, const float *matrices,
                                    const float *lens, int Hd, int Wd, int k, const float *lut, float clip_lo, float clip_hi,
                                    const float *grad_values, float *grad_matrices, float *grad_lens, void *workspace,
                                    size_t workspace_bytes, void *stream)
{
    const char *who = "svbrdf_rectify_photos_lens_grad";
    int rc = rectify_check(who, "grad_matrices", src, src_format, P, Hs, Ws, matrices, Hd, Wd, k, lut, clip_lo, clip_hi,
                           grad_matrices, grad_values);
    if (rc) return rc;
    rc = rectify_lens_check(who, lens);
    if (rc) return rc;
    char text[200];
    const auto bad = [&](int code, const char *what) {
        std::snprintf(text, sizeof(text), "%s: %s", who, what);
        return fail(code, text);
    };
    if (!grad_values || !grad_lens || !workspace) return bad(SVBRDF_ERR_NULL, "grad_values, grad_lens and workspace are required");
    if (!aligned(grad_lens, 4)) return bad(SVBRDF_ERR_ALIGN, "grad_lens must be 4-byte aligned");
    if (!aligned(workspace, 8)) return bad(SVBRDF_ERR_ALIGN, "workspace must be 8-byte aligned");
    if (workspace_bytes < svbrdf_rectify_lens_grad_workspace_bytes(P, Hd, Wd))
        return bad(SVBRDF_ERR_WORKSPACE, "workspace is smaller than svbrdf_rectify_lens_grad_workspace_bytes(P, Hd, Wd)");
    const bool u8 = src_format == SVBRDF_RECTIFY_U8_INTERLEAVED;
    const RectifyClip clip = rectify_clip(clip_lo, clip_hi);
    const dim3 grid = rectify_grid(P, Hd, Wd);
    unsigned *tickets = static_cast<unsigned *>(workspace);
    float *partials = reinterpret_cast<float *>(static_cast<char *>(workspace) + lens_grad_ticket_bytes(P));
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (u8)
        launch_lens_grad<true>(k, grid, st, src, matrices, lens, lut, clip, grad_values, grad_matrices, grad_lens, tickets,
                               partials, Hs, Ws, Hd, Wd);
    else
        launch_lens_grad<false>(k, grid, st, src, matrices, lens, lut, clip, grad_values, grad_matrices, grad_lens, tickets,
                                partials, Hs, Ws, Hd, Wd);
    return launch_status(who);
}

}  // extern "C"
