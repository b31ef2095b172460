// svbrdf_capture_grad.hip -- translation unit of libsvbrdf_hip.so: the gradient of svbrdf_rectify_photos' values towards the
// 3x3 matrices, ONE launch (ABI version 8).
//
// Photometric refinement of a registration moves a photograph's four corners until its rectification agrees with a
// rendering; that needs d loss / d M for every photograph, reduced over all grid pixels and sub-samples.  k_homography_grad
// repeats the forward's gather (svbrdf_capture_device.h: the same geometry, the same clamped addressing, the same tap rule)
// and reduces nine terms per sub-sample to nine floats per photo.
//
// Definition (include/svbrdf_hip.h has it in full; tests/capture_grad_checks.py restates it in numpy float32).  Everything up
// to the taps a, b, c, d and the pixel's `ok` is the forward's.  The gradient is that of the forward's expression with the
// cell (x0, y0), `valid` and `ok` held constant.  With g_ch = grad_values[p, ch, y, x], per sub-sample, every line ONE
// individually rounded float32 operation (HIPFLAGS: -ffp-contract=off; no fmaf(); the quotient is the language's IEEE `/`):
//     per channel:  ba = b - a;  dc = d - c;  du = ba + fy (dc - ba);  dv = bot - top
//     gu = ((g0 du0 + g1 du1) + g2 du2) (1/K^2);   gv likewise with dv
//     rz = 1 / Z;   pu = gu rz;   pv = gv rz;   pz = -((pu u) + (pv v))
//     the nine terms:  pu xs, pu ys, pu,   pv xs, pv ys, pv,   pz xs, pz ys, pz
// grad_matrices[p, n] is the sum of term n over the sub-samples of the pixels whose `ok` holds -- a select, so whatever
// grad_values holds under a zero-weight pixel is never looked at.
//
// The sum is the same bits in every launch and takes no float atomic.  A workgroup is the forward's 64 x 4 tile.
//   1. a thread adds its K^2 sub-samples in (j, i) order into nine float32 accumulators (K^2 - 1 additions), and replaces
//      them by +0 unless its pixel exists and is ok;
//   2. a butterfly over the wave's 64 lanes (lane ^ 32, 16, 8, 4, 2, 1: 6 additions; a + b = b + a, so all lanes hold the
//      same bits), then (w0 + w1) + (w2 + w3) over the four waves through LDS (2 additions);
//   3. the workgroup's nine words go to its slot of the workspace with write-through vector stores (sc1; a release fence
//      per workgroup instead costs 11 us per photo of 256 workgroups: profiles/r23_capture_grad.txt);
//   4. wave 0 drains its stores (s_waitcnt vmcnt(0)) and draws a ticket from the photo's counter (an integer atomic);
//   5. the wave that draws the last ticket acquires at agent scope and adds the photo's partials in float64: lane l takes
//      the workgroups l, l + 64, ... in index order, the 64 lane sums meet in the same butterfly in float64, and the sum
//      is rounded to float32 once.  It stores zeros over the partials it read and over the counter: the workspace is
//      zeroed once by the caller and left zeroed by every completed call.
// SVBRDF_RECTIFY_GRAD_DEPTH = 24 (include/svbrdf_hip.h) bounds the float32 additions any single term passes through: K^2 - 1 <= 15, 6 and 2 make 23.
// No float32 sum crosses a workgroup.  Which workgroup finishes depends on timing; what it computes does not.
// svbrdf_capture_grad_device.h holds du .. gv and steps 2 to 5 as functions (rectify_grad_taps, rectify_grad_reduce<N>), which
// k_lens_grad calls, and the host side of both gradient entries: the workspace's size and split and the second-stage checks.
#include "svbrdf_host.h"
#include "svbrdf_capture_device.h"
#include "svbrdf_capture_grad_device.h"

namespace {

// k_homography_grad keeps the body it had before the capture units were put on shared device functions, with its own cell and
// reduction: on the shared ones its uint8 k = 1 launch was 0.28 us above the criterion of profiles/r27_capture_refactor.txt.
// A change to rectify_cell or rectify_grad_reduce (the shared headers) has to be made here as well.
//
// One sub-sample at (xs, ys) through m0..m8: the forward's statements from X to the tap cell, one rounded float32 operation
// each, in its order.  u and v are the quotients as they are; the cell and the fractions come from their clamped copies, so
// every index lies in the source whatever the matrix holds.
struct HomographyCell {
    float Z, u, v, fx, fy;
    int x0, y0, x1, y1;
    bool valid;
};

__device__ __forceinline__ HomographyCell homography_cell(const float m[9], float xs, float ys, int Hs, int Ws)
{
    const float wmax = (float)(Ws - 1), hmax = (float)(Hs - 1);
    HomographyCell g;
    const float X = (m[0] * xs + m[1] * ys) + m[2];
    const float Y = (m[3] * xs + m[4] * ys) + m[5];
    g.Z = (m[6] * xs + m[7] * ys) + m[8];
    g.u = X / g.Z;
    g.v = Y / g.Z;
    g.valid = g.Z > 0.0f && g.u >= 0.0f && g.u <= wmax && g.v >= 0.0f && g.v <= hmax;
    float u = g.valid ? g.u : 0.0f;
    float v = g.valid ? g.v : 0.0f;
    u = fminf(fmaxf(u, 0.0f), wmax);        // in float, before the conversion: NaN and +-inf cannot reach it
    v = fminf(fmaxf(v, 0.0f), hmax);
    const float x0f = floorf(u), y0f = floorf(v);
    g.fx = u - x0f;
    g.fy = v - y0f;
    g.x0 = (int)x0f;
    g.y0 = (int)y0f;
    g.x1 = min(g.x0 + 1, Ws - 1);
    g.y1 = min(g.y0 + 1, Hs - 1);
    return g;
}

template <bool U8, int K>
__global__ __launch_bounds__(kRectifyTileW * kRectifyTileH) void k_homography_grad(
    const void *__restrict__ src, const float *__restrict__ matrices, const float *__restrict__ lut, RectifyClip clip,
    const float *__restrict__ grad_values, float *__restrict__ grad_matrices, unsigned *tickets, float *partials, int Hs,
    int Ws, int Hd, int Wd)
{
    constexpr int kLut = U8 ? 256 : 0;
    __shared__ float s_words[kLut + kRectifyTileH * 9];     // the table, then the four waves' nine sums
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
    const size_t plane = (size_t)Hs * Ws;
    const size_t base = (size_t)p * 3 * plane;      // first element of photo p in either layout
    const size_t dplane = (size_t)Hd * Wd;
    float g[3] = {0.0f, 0.0f, 0.0f};
    if (live) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) g[ch] = grad_values[((size_t)p * 3 + ch) * dplane + (size_t)y * Wd + x];
    }
    float acc[9];
    bool ok = live;
#pragma unroll
    for (int j = 0; j < K; ++j) {
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const float xs = (float)x + ((i + 0.5f) / K - 0.5f);        // the offset is a compile-time constant, exact
            const float ys = (float)y + ((j + 0.5f) / K - 0.5f);
            const HomographyCell c = homography_cell(m, xs, ys, Hs, Ws);
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
            const float gu = ((g[0] * du[0] + g[1] * du[1]) + g[2] * du[2]) * (1.0f / (K * K));
            const float gv = ((g[0] * dv[0] + g[1] * dv[1]) + g[2] * dv[2]) * (1.0f / (K * K));
            const float rz = 1.0f / c.Z;
            const float pu = gu * rz;
            const float pv = gv * rz;
            const float pz = -((pu * c.u) + (pv * c.v));
            const float t[9] = {pu * xs, pu * ys, pu, pv * xs, pv * ys, pv, pz * xs, pz * ys, pz};
#pragma unroll
            for (int n = 0; n < 9; ++n) acc[n] = (i == 0 && j == 0) ? t[n] : acc[n] + t[n];
        }
    }
#pragma unroll
    for (int n = 0; n < 9; ++n) {
        float v = ok ? acc[n] : 0.0f;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        acc[n] = v;
    }
    if (lane == 0) {
#pragma unroll
        for (int n = 0; n < 9; ++n) s_sums[wave * 9 + n] = acc[n];
    }
    __syncthreads();
    if (wave != 0) return;
    const size_t tiles = (size_t)gridDim.x * gridDim.y;
    const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    float *mine = partials + ((size_t)p * tiles + tile) * 9;
    // the nine words go out WRITE-THROUGH (a relaxed agent-scope store: global_store_dword sc1), so no release fence -- it
    // would write the whole L2 back, once per workgroup -- is needed: drained, they are in memory before the ticket is drawn
    if (lane < 9) {
        const float v = (s_sums[lane] + s_sums[9 + lane]) + (s_sums[18 + lane] + s_sums[27 + lane]);
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
    float *all = partials + (size_t)p * tiles * 9;
    double sum[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (size_t t = lane; t < tiles; t += 64) {
#pragma unroll
        for (int n = 0; n < 9; ++n) {
            sum[n] += (double)all[t * 9 + n];
            all[t * 9 + n] = 0.0f;          // left zeroed
        }
    }
#pragma unroll
    for (int n = 0; n < 9; ++n) {
        double v = sum[n];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += shfl_xor_f64(v, off);
        sum[n] = v;
    }
    if (lane == 0) {
#pragma unroll
        for (int n = 0; n < 9; ++n) grad_matrices[(size_t)p * 9 + n] = (float)sum[n];
        __hip_atomic_store(tickets + p, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace

extern "C" {

size_t svbrdf_rectify_grad_workspace_bytes(int P, int Hd, int Wd) { return rectify_grad_workspace_bytes(P, Hd, Wd, 9); }

int svbrdf_rectify_photos_grad_matrices(const void *src, int src_format, int P, int Hs, int Ws, const float *matrices,
                                        int Hd, int Wd, int k, const float *lut, float clip_lo, float clip_hi,
                                        const float *grad_values, float *grad_matrices, void *workspace,
                                        size_t workspace_bytes, void *stream)
{
    const char *who = "svbrdf_rectify_photos_grad_matrices";
    int rc = rectify_check(who, "grad_matrices", src, src_format, P, Hs, Ws, matrices, Hd, Wd, k, lut, clip_lo, clip_hi,
                           grad_matrices, grad_values);
    if (rc) return rc;
    rc = rectify_grad_check(who, "svbrdf_rectify_grad_workspace_bytes", false, P, Hd, Wd, 9, grad_values, nullptr, workspace,
                            workspace_bytes);
    if (rc) return rc;
    const RectifyClip clip = rectify_clip(clip_lo, clip_hi);
    const dim3 grid = rectify_grid(P, Hd, Wd);
    unsigned *tickets = rectify_grad_tickets(workspace);
    float *partials = rectify_grad_partials(workspace, P);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    rectify_dispatch(src_format, k, [&](auto u8, auto kk) {
        k_homography_grad<decltype(u8)::value, decltype(kk)::value><<<grid, kRectifyBlock, 0, st>>>(
            src, matrices, lut, clip, grad_values, grad_matrices, tickets, partials, Hs, Ws, Hd, Wd);
    });
    return launch_status(who);
}

}  // extern "C"
