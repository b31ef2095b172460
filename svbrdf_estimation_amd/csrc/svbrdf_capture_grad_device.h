// svbrdf_capture_grad_device.h -- what the two gradient units share: svbrdf_capture_grad.hip (k_homography_grad, nine words
// per workgroup) and svbrdf_capture_lens_grad.hip (k_lens_grad, eighteen).  On the host the workspace's size and split and
// the second stage of the two entries' argument checks; on the device shfl_xor_f64 and, as functions templated on the word
// count, the pixel's grad_values, the gradient's tap block (du, dv per channel, and from them gu, gv) and the reduction from
// a thread's N sums to N floats per photo, which orders memory between workgroups (k_lens_grad calls them;
// k_homography_grad keeps its old body's copy, svbrdf_capture_grad.hip says why).  svbrdf_capture_grad.hip's header describes the reduction; include/svbrdf_hip.h has the
// definition.  No kernel and no entry point.  The including unit has svbrdf_host.h and svbrdf_capture_device.h in front.
#ifndef SVBRDF_CAPTURE_GRAD_DEVICE_H
#define SVBRDF_CAPTURE_GRAD_DEVICE_H

namespace {

static_assert(4 * 4 - 1 + 6 + 2 <= SVBRDF_RECTIFY_GRAD_DEPTH, "float32 additions a term passes through: thread, wave, waves");
constexpr int kRectifyGradTicketBytes = 256;        // the counters' block is padded to a multiple of this

inline size_t rectify_grad_ticket_bytes(int P)
{
    return ((size_t)P * sizeof(unsigned) + kRectifyGradTicketBytes - 1) / kRectifyGradTicketBytes * kRectifyGradTicketBytes;
}

inline size_t rectify_grad_tiles(int Hd, int Wd)
{
    return (size_t)((Wd + kRectifyTileW - 1) / kRectifyTileW) * (size_t)((Hd + kRectifyTileH - 1) / kRectifyTileH);
}

// the workspace of a gradient entry with `words` sums per workgroup: the photos' tickets, then a partial per workgroup; 0
// outside the limits
inline size_t rectify_grad_workspace_bytes(int P, int Hd, int Wd, int words)
{
    if (P < 1 || Hd < 1 || Wd < 1 || P > 65535 || Hd > kRectifyMaxDim || Wd > kRectifyMaxDim) return 0;
    return rectify_grad_ticket_bytes(P) + (size_t)P * rectify_grad_tiles(Hd, Wd) * words * sizeof(float);
}

inline unsigned *rectify_grad_tickets(void *workspace) { return static_cast<unsigned *>(workspace); }

inline float *rectify_grad_partials(void *workspace, int P)
{
    return reinterpret_cast<float *>(static_cast<char *>(workspace) + rectify_grad_ticket_bytes(P));
}

// The second stage of the two gradient entries' checks, behind rectify_check's (and the lens's): grad_values, the
// workspace and -- for the lens entry, `query` names its size function -- grad_lens.  0, or the error code with its text set.
inline int rectify_grad_check(const char *who, const char *query, bool lens, int P, int Hd, int Wd, int words,
                              const float *grad_values, const float *grad_lens, const void *workspace, size_t workspace_bytes)
{
    char text[200];
    const auto bad = [&](int code, const char *what) {
        std::snprintf(text, sizeof(text), "%s: %s", who, what);
        return fail(code, text);
    };
    if (!grad_values || (lens && !grad_lens) || !workspace)
        return bad(SVBRDF_ERR_NULL, lens ? "grad_values, grad_lens and workspace are required" : "grad_values and workspace are required");
    if (!aligned(grad_lens, 4)) return bad(SVBRDF_ERR_ALIGN, "grad_lens must be 4-byte aligned");
    if (!aligned(workspace, 8)) return bad(SVBRDF_ERR_ALIGN, "workspace must be 8-byte aligned");
    if (workspace_bytes < rectify_grad_workspace_bytes(P, Hd, Wd, words)) {
        char what[120];
        std::snprintf(what, sizeof(what), "workspace is smaller than %s(P, Hd, Wd)", query);
        return bad(SVBRDF_ERR_WORKSPACE, what);
    }
    return 0;
}

__device__ __forceinline__ double shfl_xor_f64(double v, int mask)
{
    const unsigned long long bits = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)bits, mask, 64);
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(bits >> 32), mask, 64);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// the pixel's three grad_values; a thread beyond the destination holds zeros
__device__ __forceinline__ void rectify_grad_values(const RectifyTile &t, const float *__restrict__ grad_values, int Hd, int Wd,
                                                    float (&g)[3])
{
    const size_t dplane = (size_t)Hd * Wd;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) g[ch] = t.live ? grad_values[((size_t)t.p * 3 + ch) * dplane + (size_t)t.y * Wd + t.x] : 0.0f;
}

// The gradient's tap block: per channel the bilinear value's slopes du, dv along the cell's axes, and with the pixel's
// g their sums gu, gv times 1/K^2 -- the gradient towards the coordinates the cell was taken at.
template <bool U8, int K>
__device__ __forceinline__ void rectify_grad_taps(const RectifySource &s, const RectifyCell &c, const float (&g)[3], bool &ok,
                                                  float &gu, float &gv)
{
    ok = ok && c.valid;
    float du[3], dv[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float ta, tb, tc, td;
        rectify_taps<U8>(s, c, ch, ok, ta, tb, tc, td);
        const float ba = tb - ta;
        const float dc = td - tc;
        du[ch] = ba + c.fy * (dc - ba);
        const float top = ta + c.fx * ba;
        const float bot = tc + c.fx * dc;
        dv[ch] = bot - top;
    }
    gu = ((g[0] * du[0] + g[1] * du[1]) + g[2] * du[2]) * (1.0f / (K * K));
    gv = ((g[0] * dv[0] + g[1] * dv[1]) + g[2] * dv[2]) * (1.0f / (K * K));
}

// The reduction's tail: a thread's N sums `acc` (replaced by +0 unless `ok`) -> N floats per photo, rows[r][p * 9 + n] for
// the N / 9 rows of nine.  `s_sums`: kRectifyTileH * N floats of LDS.  Every wave but wave 0 ends at the barrier.
template <int N>
__device__ __forceinline__ void rectify_grad_reduce(const RectifyTile &t, bool ok, float (&acc)[N], float *s_sums,
                                                    float *const (&rows)[N / 9], unsigned *tickets, float *partials)
{
    static_assert(N % 9 == 0 && N <= kRectifyTileW, "rows of nine, a word per lane of wave 0");
    const int p = t.p, lane = t.lane, wave = t.wave;
    // the butterfly over the wave's 64 lanes: a + b = b + a, so all lanes hold the same bits
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
    // the N words go out WRITE-THROUGH (a relaxed agent-scope store: global_store_dword sc1), so no release fence -- it
    // would write the whole L2 back, once per workgroup -- is needed: drained, they are in memory before the ticket is drawn
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
    // lane l adds the workgroups l, l + 64, ... in index order, in float64; the 64 lane sums meet in the same butterfly
    float *all = partials + (size_t)p * tiles * N;
    double sum[N];
#pragma unroll
    for (int n = 0; n < N; ++n) sum[n] = 0.0;
    for (size_t w = lane; w < tiles; w += 64) {
#pragma unroll
        for (int n = 0; n < N; ++n) {
            sum[n] += (double)all[w * N + n];
            all[w * N + n] = 0.0f;          // left zeroed
        }
    }
#pragma unroll
    for (int n = 0; n < N; ++n) {
        double v = sum[n];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += shfl_xor_f64(v, off);
        sum[n] = v;
    }
    // rounded to float32 once; the ticket goes back to 0: the workspace is zeroed once by the caller and left zeroed by
    // every completed call
    if (lane == 0) {
#pragma unroll
        for (int n = 0; n < N; ++n) rows[n / 9][(size_t)p * 9 + n % 9] = (float)sum[n];
        __hip_atomic_store(tickets + p, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace

#endif  // SVBRDF_CAPTURE_GRAD_DEVICE_H
