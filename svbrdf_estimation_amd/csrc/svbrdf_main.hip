// svbrdf_main.hip -- the main unit of libsvbrdf_hip.so: the C ABI declared in include/svbrdf_hip.h (every entry point but
// those of the float64, photo and capture units), the kernels only it launches -- K1 render_fwd, K2 render_bwd, K4
// mix_materials, the forward-only K3 variants, the copy and clock probes -- and the error text and launch counter that
// every unit reports through.  The device code of K1-K3 is in svbrdf_device.h; the forward+adjoint K3 kernels are in
// svbrdf_k3_adjoint{,_extra}.hip, reached through the two hidden launchers of svbrdf_k3_kernels.h.  Built with the
// bottom-up post-RA scheduler (csrc/Makefile: SCHED_MAIN; the adjoint units' sets cost K2 13 %).
#include "svbrdf_host.h"
#include "svbrdf_k3_kernels.h"

namespace {

// K1 (render_fwd_body, svbrdf_device.h)
template <int VEC>
__global__ __launch_bounds__(kThreads) void k_render_fwd(const float *__restrict__ maps,
                                                         const float *__restrict__ scenes,
                                                         const float *__restrict__ xrow,
                                                         float *__restrict__ out, const int *__restrict__ offsets,
                                                         int shared, int S, int H, int W)
{
    render_fwd_body<VEC>(maps, scenes, xrow, out, offsets, shared != 0, S, H, W);
}

// scene rows BY VALUE in the kernel-argument block (see SceneBlock, svbrdf_device.h: the table is the first argument and is
// read through the kernarg segment pointer with the same wave-uniform scalar loads).  A reference-shaped
// `render(scene, svbrdf)` call (renderers.py:67-104: three synchronous H2D copies per call, :79,91,98) is then ONE
// dispatch with no copy command in front of it.
template <int VEC>
__global__ __launch_bounds__(kThreads) void k_render_fwd_inl([[maybe_unused]] const SceneBlock table,
                                                             const float *__restrict__ maps,
                                                             const float *__restrict__ xrow, float *__restrict__ out,
                                                             int shared, int S, int H, int W)
{
    const float *__restrict__ rows = (const float *)__builtin_amdgcn_kernarg_segment_ptr();
    render_fwd_body<VEC>(maps, rows, xrow, out, nullptr, shared != 0, S, H, W);
}

// K1 with the sensor-noise epilogue (render_inputs, dataset.py:206-219): EPI = 1 clamp, 2 noise + clamp.  The noise levels
// (one per render) come from a device table, or ride behind the scene rows in the argument block.
#ifndef SVBRDF_PHOTO_MIN_WAVES
#define SVBRDF_PHOTO_MIN_WAVES 4    // the Philox state next to four pixels' shading: 137 VGPRs (3 waves/SIMD) left to itself
#endif
#define SVBRDF_PHOTO_ATTRS __attribute__((amdgpu_waves_per_eu(SVBRDF_PHOTO_MIN_WAVES, 8)))
struct PhotoBlock {
    float v[SVBRDF_HOST_SCENES_MAX_ROWS * 9];
    float sigma[SVBRDF_HOST_SCENES_MAX_ROWS];
};

template <int VEC, int EPI>
__global__ __launch_bounds__(kThreads) SVBRDF_PHOTO_ATTRS void k_render_inputs(const float *__restrict__ maps,
                                                            const float *__restrict__ scenes,
                                                            const float *__restrict__ sigma, PhiloxKey key,
                                                            const float *__restrict__ xrow, float *__restrict__ out,
                                                            int S, int H, int W)
{
    render_fwd_body<VEC, EPI>(maps, scenes, xrow, out, nullptr, false, S, H, W, Epilogue{sigma, key});
}

template <int VEC, int EPI>
__global__ __launch_bounds__(kThreads) SVBRDF_PHOTO_ATTRS void k_render_inputs_inl([[maybe_unused]] const PhotoBlock table, PhiloxKey key,
                                                                const float *__restrict__ maps,
                                                                const float *__restrict__ xrow, float *__restrict__ out,
                                                                int S, int H, int W)
{
    const float *__restrict__ rows = (const float *)__builtin_amdgcn_kernarg_segment_ptr();
    render_fwd_body<VEC, EPI>(maps, rows, xrow, out, nullptr, false, S, H, W,
                              Epilogue{rows + SVBRDF_HOST_SCENES_MAX_ROWS * 9, key});
}

// K2 (render_bwd_body, svbrdf_device.h)
template <int VEC>
__global__ __launch_bounds__(kThreads) void k_render_bwd(const float *__restrict__ maps,
                                                         const float *__restrict__ scenes,
                                                         const float *__restrict__ xrow,
                                                         const float *__restrict__ grad_out,
                                                         float *__restrict__ grad_maps, const int *__restrict__ offsets,
                                                         int shared, int S, int H, int W)
{
    render_bwd_body<VEC>(maps, scenes, xrow, grad_out, grad_maps, offsets, shared != 0, S, H, W);
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void k_render_bwd_inl([[maybe_unused]] const SceneBlock table,
                                                             const float *__restrict__ maps,
                                                             const float *__restrict__ xrow,
                                                             const float *__restrict__ grad_out,
                                                             float *__restrict__ grad_maps, int shared, int S, int H, int W)
{
    const float *__restrict__ rows = (const float *)__builtin_amdgcn_kernarg_segment_ptr();
    render_bwd_body<VEC>(maps, rows, xrow, grad_out, grad_maps, nullptr, shared != 0, S, H, W);
}

// data[i] *= *scale, skipped entirely (no memory traffic) when *scale == 1: lets the autograd
// wrapper apply an upstream gradient that lives on the device without a host sync.
__global__ __launch_bounds__(kThreads) void k_scale_inplace(float *__restrict__ data, const float *__restrict__ scale,
                                                            size_t n)
{
    const float s = scale[0];
    if (s == 1.0f) return;
    const size_t stride = (size_t)gridDim.x * kThreads;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) data[i] *= s;
}

// ------------------------------------------------------------------------------------------
// arithmetic self-check: div_rn / sqrt_rn against the compiler's IEEE `/` and sqrtf
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned hash32(unsigned x)
{
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}

__global__ __launch_bounds__(kThreads) void k_check_arith(unsigned long long n, unsigned seed, float lo, float hi,
                                                          unsigned long long *__restrict__ counts)
{
    unsigned long long bad_div = 0, bad_sqrt = 0;
    const unsigned long long stride = (unsigned long long)gridDim.x * kThreads;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
        const unsigned h0 = hash32((unsigned)i * 2654435761U + seed), h1 = hash32(h0 ^ (unsigned)(i >> 32) ^ 0x9e3779b9U);
        // denominators log-uniform in [lo, hi], numerators uniform in [-hi, hi] with random mantissas
        const float u0 = (float)(h0 >> 8) * (1.0f / 16777216.0f), u1 = (float)(h1 >> 8) * (1.0f / 16777216.0f);
        const float b = lo * exp2f(u0 * log2f(hi / lo));
        const float a = (2.0f * u1 - 1.0f) * hi;
        // b plays the squared length: the kernels divide by sqrt(b)
        float seed;
        const Recip r = length_rn(b, seed);
        const float len = sqrtf(b);
        if (r.b != len) ++bad_sqrt;
        if (div_rn(a, r) != a / len) ++bad_div;
    }
    if (bad_div) atomicAdd(&counts[0], bad_div);
    if (bad_sqrt) atomicAdd(&counts[1], bad_sqrt);
}

// ------------------------------------------------------------------------------------------
// K4: material mixing (dataset.py:142-160 SvbrdfDataset.mix), one pass over two SVBRDFs:
//   normals projected to z = 1 (n / max(0.01, n.z)), blended, renormalised; diffuse / roughness / specular blended;
//   weights alpha and fp32(1 - alpha) per batch item.  HBM-bound (24 planes in, 12 out = 144 B per pixel, ~40 flop).
// Operation order and roundings are the reference's: every product rounded on its own (-ffp-contract=off), the
// squared length summed (p0 + p1) + p2 like torch.sum over the channel axis, IEEE division and square root.
// ------------------------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(kThreads) void k_mix_materials(const float *__restrict__ m0, const float *__restrict__ m1,
                                                            const float *__restrict__ alpha, float *__restrict__ out,
                                                            size_t plane)
{
    const size_t pix = ((size_t)blockIdx.x * kThreads + threadIdx.x) * VEC;
    const int b = blockIdx.y;
    if (pix >= plane) return;
    const float a = alpha[b], oma = 1.0f - a;
    const float *__restrict__ p0 = m0 + (size_t)b * 12 * plane + pix;
    const float *__restrict__ p1 = m1 + (size_t)b * 12 * plane + pix;
    float *__restrict__ po = out + (size_t)b * 12 * plane + pix;
    float n0[3][VEC], n1[3][VEC], nm[3][VEC];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        load_vec<VEC, true>(p0 + (size_t)k * plane, n0[k]);
        load_vec<VEC, true>(p1 + (size_t)k * plane, n1[k]);
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        const float z0 = fmaxf(0.01f, n0[2][v]), z1 = fmaxf(0.01f, n1[2][v]);
#pragma unroll
        for (int k = 0; k < 3; ++k) nm[k][v] = a * (n0[k][v] / z0) + oma * (n1[k][v] / z1);
        const float len = sqrtf((nm[0][v] * nm[0][v] + nm[1][v] * nm[1][v]) + nm[2][v] * nm[2][v]);
#pragma unroll
        for (int k = 0; k < 3; ++k) nm[k][v] = nm[k][v] / len;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) store_vec<VEC, true>(po + (size_t)k * plane, nm[k]);
#pragma unroll
    for (int k = 3; k < 12; ++k) {
        float x0[VEC], x1[VEC], y[VEC];
        load_vec<VEC, true>(p0 + (size_t)k * plane, x0);
        load_vec<VEC, true>(p1 + (size_t)k * plane, x1);
#pragma unroll
        for (int v = 0; v < VEC; ++v) y[v] = a * x0[v] + oma * x1[v];
        store_vec<VEC, true>(po + (size_t)k * plane, y);
    }
}

// ------------------------------------------------------------------------------------------
// measurement aid: the shader clock the chip holds while other kernels run.  One wave spins for `ticks` ticks of
// the constant 100 MHz counter (s_memrealtime) and reports how many shader cycles (s_memtime) went by: launched
// on a stream of its own beside the fused loss it reads the clock under THAT load (DVFS lowers it under VALU-dense
// kernels); one wave on one SIMD does not disturb the measured kernels.  out[0] = shader cycles, out[1] = ticks.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_clock_probe(unsigned long long *__restrict__ out, unsigned long long ticks)
{
    if (threadIdx.x != 0) return;
    const unsigned long long r0 = wall_clock64(), c0 = clock64();
    unsigned long long r1 = r0;
    while (r1 - r0 < ticks) {
        __builtin_amdgcn_s_sleep(32);
        r1 = wall_clock64();
    }
    const unsigned long long c1 = clock64();
    out[0] = c1 - c0;
    out[1] = r1 - r0;
}

// ------------------------------------------------------------------------------------------
// measurement aid: the HBM copy rate of THIS box ("fraction of both nominal and measured-copy peak").  A plain
// streaming copy, 16 bytes per lane and access, non-temporal both ways, UNROLL independent loads in flight per lane
// before the first store; a workgroup owns one contiguous UNROLL x 4 KiB chunk.  Bytes moved = 2 x n x 4.
// SVBRDF_COPY_UNROLL / SVBRDF_COPY_NT select the A/B variants of tools/copy_peak.py.  Shipped: UNROLL = 1, non-temporal --
// 6.55-6.59 TB/s on 1 and 4 GiB (profiles/r06_copy_peak.txt; unroll 2: 6.1-6.2, 4: 6.3, 8: 4.4-4.5; plain accesses
// 0.3-0.6 TB/s lower at every unroll; hipMemcpyAsync device-to-device 5.0-5.2; the guide quotes 6.29 for a float4 copy).
// ------------------------------------------------------------------------------------------
template <int UNROLL, bool NT>
__global__ __launch_bounds__(kThreads) void k_copy_vec4(vec4f *__restrict__ dst, const vec4f *__restrict__ src, size_t n4)
{
    const size_t base = (size_t)blockIdx.x * (kThreads * UNROLL) + threadIdx.x;
    vec4f v[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
        const size_t i = base + (size_t)u * kThreads;
        if (i < n4) v[u] = NT ? __builtin_nontemporal_load(src + i) : src[i];
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
        const size_t i = base + (size_t)u * kThreads;
        if (i < n4) {
            if (NT) __builtin_nontemporal_store(v[u], dst + i);
            else dst[i] = v[u];
        }
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
thread_local char g_err[256] = "";
std::atomic<unsigned long long> g_launches{0};      // svbrdf_debug_launch_count()

}  // namespace

int svbrdf_internal_fail(int code, const char *what)
{
    std::snprintf(g_err, sizeof(g_err), "%s", what);
    return code;
}
int svbrdf_internal_launch_status(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        std::snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
        return (int)e;
    }
    g_launches.fetch_add(1, std::memory_order_relaxed);      // every entry point enqueues exactly one kernel and ends here
    return 0;
}

extern "C" {

int svbrdf_abi_version(void) { return SVBRDF_ABI_VERSION; }

const char *svbrdf_last_error(void) { return g_err; }

int svbrdf_make_xrow(float *xrow_host, int W)
{
    if (!xrow_host) return fail(SVBRDF_ERR_NULL, "xrow_host is null");
    if (W <= 0) return fail(SVBRDF_ERR_DIMS, "W must be positive");
    if (W == 1) { xrow_host[0] = -1.0f; return 0; }
    // torch.linspace(-1, 1, W) on the reference's CPU path: symmetric halves, one FMA each
    const float step = 2.0f / (float)(W - 1);
    for (int i = 0; i < W; ++i)
        xrow_host[i] = (i < W / 2) ? std::fmaf(step, (float)i, -1.0f) : std::fmaf(-step, (float)(W - 1 - i), 1.0f);
    return 0;
}

// `host_rows` > 0: `scenes` is a HOST table of that many rows and travels by value in the argument block
static int render_fwd_impl(const float *maps, const float *scenes, const float *xrow, float *out, const int *offsets,
                           int shared, int host_rows, int B, int S, int H, int W, void *stream)
{
    if (!maps || !scenes || !xrow || !out) return fail(SVBRDF_ERR_NULL, "render_fwd: null pointer");
    if (int e = check_dims(B, S, H, W)) return e;
    if (!aligned(maps, 4) || !aligned(scenes, 4) || !aligned(xrow, 4) || !aligned(out, 4) || !aligned(offsets, 4))
        return fail(SVBRDF_ERR_ALIGN, "render_fwd: pointers must be 4-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int vec = pick_vec(env_vec("SVBRDF_K1_VEC", 4), W, {maps, xrow, out});
    const dim3 grid = grid_for(B, H, W, vec), block(kThreads);
    if (host_rows > 0) {
        SceneBlock block_arg;      // only the first host_rows rows are ever read
        std::memcpy(block_arg.v, scenes, (size_t)host_rows * 9 * sizeof(float));
        if (vec == 4) hipLaunchKernelGGL(k_render_fwd_inl<4>, grid, block, 0, st, block_arg, maps, xrow, out, shared, S, H, W);
        else if (vec == 2) hipLaunchKernelGGL(k_render_fwd_inl<2>, grid, block, 0, st, block_arg, maps, xrow, out, shared, S, H, W);
        else hipLaunchKernelGGL(k_render_fwd_inl<1>, grid, block, 0, st, block_arg, maps, xrow, out, shared, S, H, W);
        return launch_status("render_fwd_host_scenes launch");
    }
    if (vec == 4) hipLaunchKernelGGL(k_render_fwd<4>, grid, block, 0, st, maps, scenes, xrow, out, offsets, shared, S, H, W);
    else if (vec == 2) hipLaunchKernelGGL(k_render_fwd<2>, grid, block, 0, st, maps, scenes, xrow, out, offsets, shared, S, H, W);
    else hipLaunchKernelGGL(k_render_fwd<1>, grid, block, 0, st, maps, scenes, xrow, out, offsets, shared, S, H, W);
    return launch_status("render_fwd launch");
}

static int host_rows_for(const char *who, int scenes_shared, int B, int S, int *rows)
{
    const long long n = scenes_shared ? (long long)S : (long long)B * S;
    if (n > SVBRDF_HOST_SCENES_MAX_ROWS)
        return fail(SVBRDF_ERR_DIMS, who);
    *rows = (int)n;
    return 0;
}

int svbrdf_render_fwd(const float *maps, const float *scenes, const float *xrow, float *out,
                      int B, int S, int H, int W, void *stream)
{
    return render_fwd_impl(maps, scenes, xrow, out, nullptr, 0, 0, B, S, H, W, stream);
}

int svbrdf_render_fwd_host_scenes(const float *maps, const float *scenes_host, int scenes_shared, const float *xrow,
                                  float *out, int B, int S, int H, int W, void *stream)
{
    if (int e = check_dims(B, S, H, W)) return e;
    int rows = 0;
    if (int e = host_rows_for("render_fwd_host_scenes: the table exceeds SVBRDF_HOST_SCENES_MAX_ROWS (upload it and use "
                              "svbrdf_render_fwd)", scenes_shared, B, S, &rows)) return e;
    return render_fwd_impl(maps, scenes_host, xrow, out, nullptr, scenes_shared != 0, rows, B, S, H, W, stream);
}

int svbrdf_render_fwd_ragged(const float *maps, const float *scenes, const int *offsets, const float *xrow, float *out,
                             int B, int R, int H, int W, void *stream)
{
    if (!offsets) return fail(SVBRDF_ERR_NULL, "render_fwd_ragged: offsets is null");
    if (R < 0) return fail(SVBRDF_ERR_DIMS, "render_fwd_ragged: R must be >= 0");
    if (R == 0) return check_dims(B, 1, H, W);          // nothing to render
    return render_fwd_impl(maps, scenes, xrow, out, offsets, 0, 0, B, 1, H, W, stream);
}

// K1 + sensor-noise epilogue (render_inputs, dataset.py:206-219).  `sigma` null: clamp only.
static int render_inputs_impl(const char *who, bool on_host, const float *maps, const float *scenes, const float *sigma,
                              unsigned long long seed, unsigned long long offset, const float *xrow, float *out,
                              int B, int S, int H, int W, void *stream)
{
    if (!maps || !scenes || !xrow || !out) return fail(SVBRDF_ERR_NULL, "render_inputs: null pointer");
    if (int e = check_dims(B, S, H, W)) return e;
    if (on_host && (long long)B * S > SVBRDF_HOST_SCENES_MAX_ROWS)
        return fail(SVBRDF_ERR_DIMS, "render_inputs_host_scenes: the table exceeds SVBRDF_HOST_SCENES_MAX_ROWS (upload scenes "
                                     "and noise levels and use svbrdf_render_inputs)");
    if (!aligned(maps, 4) || !aligned(scenes, 4) || !aligned(sigma, 4) || !aligned(xrow, 4) || !aligned(out, 4))
        return fail(SVBRDF_ERR_ALIGN, "render_inputs: pointers must be 4-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int vec = pick_vec(env_vec("SVBRDF_K1_VEC", 4), W, {maps, xrow, out});
    const dim3 grid = grid_for(B, H, W, vec), block(kThreads);
    const PhiloxKey key{(unsigned)seed, (unsigned)(seed >> 32), (unsigned)offset, (unsigned)(offset >> 32)};
#define SVBRDF_LAUNCH_PHOTOS(V, E)                                                                                     \
    do {                                                                                                               \
        if (on_host)                                                                                                   \
            hipLaunchKernelGGL((k_render_inputs_inl<V, E>), grid, block, 0, st, block_arg, key, maps, xrow, out, S, H, W); \
        else                                                                                                           \
            hipLaunchKernelGGL((k_render_inputs<V, E>), grid, block, 0, st, maps, scenes, sigma, key, xrow, out, S, H, W); \
    } while (0)
    PhotoBlock block_arg;          // only the first B*S rows / levels are ever read
    if (on_host) {
        std::memcpy(block_arg.v, scenes, (size_t)B * S * 9 * sizeof(float));
        if (sigma) std::memcpy(block_arg.sigma, sigma, (size_t)B * S * sizeof(float));
    }
    if (sigma) {
        if (vec == 4) SVBRDF_LAUNCH_PHOTOS(4, 2); else if (vec == 2) SVBRDF_LAUNCH_PHOTOS(2, 2); else SVBRDF_LAUNCH_PHOTOS(1, 2);
    } else {
        if (vec == 4) SVBRDF_LAUNCH_PHOTOS(4, 1); else if (vec == 2) SVBRDF_LAUNCH_PHOTOS(2, 1); else SVBRDF_LAUNCH_PHOTOS(1, 1);
    }
#undef SVBRDF_LAUNCH_PHOTOS
    return launch_status(who);
}

int svbrdf_render_inputs(const float *maps, const float *scenes, const float *noise_std, unsigned long long seed,
                         unsigned long long offset, const float *xrow, float *out, int B, int S, int H, int W, void *stream)
{
    return render_inputs_impl("render_inputs launch", false, maps, scenes, noise_std, seed, offset, xrow, out, B, S, H, W,
                              stream);
}

int svbrdf_render_inputs_host_scenes(const float *maps, const float *scenes_host, const float *noise_std_host,
                                     unsigned long long seed, unsigned long long offset, const float *xrow, float *out,
                                     int B, int S, int H, int W, void *stream)
{
    return render_inputs_impl("render_inputs_host_scenes launch", true, maps, scenes_host, noise_std_host, seed, offset,
                              xrow, out, B, S, H, W, stream);
}

static int render_bwd_impl(const float *maps, const float *scenes, const float *xrow, const float *grad_out,
                           float *grad_maps, const int *offsets, int shared, int host_rows, int B, int S, int H, int W,
                           void *stream)
{
    if (!maps || !scenes || !xrow || !grad_out || !grad_maps) return fail(SVBRDF_ERR_NULL, "render_bwd: null pointer");
    if (int e = check_dims(B, S, H, W)) return e;
    if (!aligned(maps, 4) || !aligned(scenes, 4) || !aligned(xrow, 4) || !aligned(grad_out, 4) || !aligned(grad_maps, 4) ||
        !aligned(offsets, 4))
        return fail(SVBRDF_ERR_ALIGN, "render_bwd: pointers must be 4-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int vec = pick_vec(env_vec("SVBRDF_K2_VEC", 2), W, {maps, xrow, grad_out, grad_maps});
    const dim3 grid = grid_for(B, H, W, vec), block(kThreads);
    if (host_rows > 0) {
        SceneBlock block_arg;
        std::memcpy(block_arg.v, scenes, (size_t)host_rows * 9 * sizeof(float));
        if (vec == 4) hipLaunchKernelGGL(k_render_bwd_inl<4>, grid, block, 0, st, block_arg, maps, xrow, grad_out, grad_maps, shared, S, H, W);
        else if (vec == 2) hipLaunchKernelGGL(k_render_bwd_inl<2>, grid, block, 0, st, block_arg, maps, xrow, grad_out, grad_maps, shared, S, H, W);
        else hipLaunchKernelGGL(k_render_bwd_inl<1>, grid, block, 0, st, block_arg, maps, xrow, grad_out, grad_maps, shared, S, H, W);
        return launch_status("render_bwd_host_scenes launch");
    }
    if (vec == 4) hipLaunchKernelGGL(k_render_bwd<4>, grid, block, 0, st, maps, scenes, xrow, grad_out, grad_maps, offsets, shared, S, H, W);
    else if (vec == 2) hipLaunchKernelGGL(k_render_bwd<2>, grid, block, 0, st, maps, scenes, xrow, grad_out, grad_maps, offsets, shared, S, H, W);
    else hipLaunchKernelGGL(k_render_bwd<1>, grid, block, 0, st, maps, scenes, xrow, grad_out, grad_maps, offsets, shared, S, H, W);
    return launch_status("render_bwd launch");
}

int svbrdf_render_bwd(const float *maps, const float *scenes, const float *xrow, const float *grad_out,
                      float *grad_maps, int B, int S, int H, int W, void *stream)
{
    return render_bwd_impl(maps, scenes, xrow, grad_out, grad_maps, nullptr, 0, 0, B, S, H, W, stream);
}

int svbrdf_render_bwd_host_scenes(const float *maps, const float *scenes_host, int scenes_shared, const float *xrow,
                                  const float *grad_out, float *grad_maps, int B, int S, int H, int W, void *stream)
{
    if (int e = check_dims(B, S, H, W)) return e;
    int rows = 0;
    if (int e = host_rows_for("render_bwd_host_scenes: the table exceeds SVBRDF_HOST_SCENES_MAX_ROWS (upload it and use "
                              "svbrdf_render_bwd)", scenes_shared, B, S, &rows)) return e;
    return render_bwd_impl(maps, scenes_host, xrow, grad_out, grad_maps, nullptr, scenes_shared != 0, rows, B, S, H, W, stream);
}

int svbrdf_render_bwd_ragged(const float *maps, const float *scenes, const int *offsets, const float *xrow,
                             const float *grad_out, float *grad_maps, int B, int R, int H, int W, void *stream)
{
    if (!offsets) return fail(SVBRDF_ERR_NULL, "render_bwd_ragged: offsets is null");
    if (R < 0) return fail(SVBRDF_ERR_DIMS, "render_bwd_ragged: R must be >= 0");
    // R == 0 still launches: every map's gradient is written (zeros)
    const float *go = (R == 0 && !grad_out) ? maps : grad_out, *sc = (R == 0 && !scenes) ? maps : scenes;
    return render_bwd_impl(maps, sc, xrow, go, grad_maps, offsets, 0, 0, B, 1, H, W, stream);
}

size_t svbrdf_rendering_loss_workspace_bytes(int B, int S, int H, int W)
{
    if (B <= 0 || S <= 0 || H <= 0 || W <= 0) return 0;
    return (kLossSlots + 1) * sizeof(unsigned long long);   // sharded fixed-point accumulators + tail word
}

static int loss_impl(const char *who, bool head, bool scenes_on_host, const float *input, const float *target,
                     const float *scenes, const float *xrow, float eps, float l1_weight, float eps_l1,
                     float *loss_out, float *grad_input, void *workspace, size_t workspace_bytes, int B, int S,
                     int H, int W, void *stream)
{
    LossPlan p;
    if (int e = plan_loss(who, scenes_on_host, {input, target, scenes, xrow, loss_out}, grad_input, workspace,
                          workspace_bytes, "eps_render", eps, l1_weight, B, S, H, W, &p)) return e;
    const long long plane = (long long)H * W;
    const L1Params l1{l1_weight * (float)S, (float)((double)l1_weight / ((double)B * 3.0 * (double)plane)), eps_l1};
    const float *rows = scenes_on_host ? scenes : nullptr;
    if (grad_input)
        (l1_weight != 0.0f || head ? svbrdf_internal_launch_k3_adjoint_extra : svbrdf_internal_launch_k3_adjoint_plain)(
            l1_weight != 0.0f, head, rows, p.grid.x, p.grid.y, p.lds_bytes, stream, input, target, scenes, xrow, eps,
            p.inv_count, p.loss_scale, p.fixed_scale, l1.sum_scale, l1.grad_scale, l1.eps, grad_input, p.ws, loss_out, B, S,
            H, W);
    else      // forward only: all four variants are this unit's, picked as above
        (l1_weight != 0.0f || head ? launch_k3<false, 1> : launch_k3<false, 0>)(
            l1_weight != 0.0f, head, rows, p.grid, p.lds_bytes, static_cast<hipStream_t>(stream), input, target, scenes,
            xrow, eps, p.inv_count, p.loss_scale, p.fixed_scale, l1, grad_input, p.ws, loss_out, B, S, H, W);
    return launch_status(who);
}

int svbrdf_rendering_loss_fwd_bwd(const float *input, const float *target, const float *scenes,
                                  const float *xrow, float eps, float *loss_out, float *grad_input,
                                  void *workspace, size_t workspace_bytes, int B, int S, int H, int W,
                                  void *stream)
{
    return loss_impl("rendering_loss", false, false, input, target, scenes, xrow, eps, 0.0f, 0.01f, loss_out, grad_input,
                     workspace, workspace_bytes, B, S, H, W, stream);
}

int svbrdf_mixed_loss_fwd_bwd(const float *input, const float *target, const float *scenes, const float *xrow,
                              float eps_render, float l1_weight, float eps_l1, float *loss_out,
                              float *grad_input, void *workspace, size_t workspace_bytes, int B, int S, int H,
                              int W, void *stream)
{
    return loss_impl("mixed_loss", false, false, input, target, scenes, xrow, eps_render, l1_weight, eps_l1, loss_out,
                     grad_input, workspace, workspace_bytes, B, S, H, W, stream);
}

int svbrdf_head_loss_fwd_bwd(const float *encoded9, const float *target, const float *scenes, const float *xrow,
                             float eps_render, float l1_weight, float eps_l1, float *loss_out, float *grad_encoded9,
                             void *workspace, size_t workspace_bytes, int B, int S, int H, int W, void *stream)
{
    return loss_impl("head_loss", true, false, encoded9, target, scenes, xrow, eps_render, l1_weight, eps_l1, loss_out,
                     grad_encoded9, workspace, workspace_bytes, B, S, H, W, stream);
}

int svbrdf_host_scenes_max_rows(void) { return SVBRDF_HOST_SCENES_MAX_ROWS; }

int svbrdf_mixed_loss_fwd_bwd_host_scenes(const float *input, const float *target, const float *scenes_host,
                                          const float *xrow, float eps_render, float l1_weight, float eps_l1,
                                          float *loss_out, float *grad_input, void *workspace, size_t workspace_bytes,
                                          int B, int S, int H, int W, void *stream)
{
    return loss_impl("mixed_loss_host_scenes", false, true, input, target, scenes_host, xrow, eps_render, l1_weight,
                     eps_l1, loss_out, grad_input, workspace, workspace_bytes, B, S, H, W, stream);
}

int svbrdf_head_loss_fwd_bwd_host_scenes(const float *encoded9, const float *target, const float *scenes_host,
                                         const float *xrow, float eps_render, float l1_weight, float eps_l1,
                                         float *loss_out, float *grad_encoded9, void *workspace, size_t workspace_bytes,
                                         int B, int S, int H, int W, void *stream)
{
    return loss_impl("head_loss_host_scenes", true, true, encoded9, target, scenes_host, xrow, eps_render, l1_weight,
                     eps_l1, loss_out, grad_encoded9, workspace, workspace_bytes, B, S, H, W, stream);
}

int svbrdf_scale_inplace(float *data, const float *scale_dev, size_t n, void *stream)
{
    // The common case (upstream gradient 1) exits at once, so the launch itself is the cost: 1024 workgroups
    // (4 per CU, grid-stride) still stream at HBM rate when the scale is not 1 and dispatch in a third of the
    // time of 4096.
    constexpr size_t kScaleBlocks = SVBRDF_SCALE_BLOCKS;
    if (!data || !scale_dev) return fail(SVBRDF_ERR_NULL, "scale_inplace: null pointer");
    if (n == 0) return 0;
    const size_t blocks = (n + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(k_scale_inplace, dim3((unsigned)(blocks < kScaleBlocks ? blocks : kScaleBlocks)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), data, scale_dev, n);
    return launch_status("scale_inplace launch");
}

int svbrdf_debug_check_arith(unsigned long long n, unsigned seed, float lo, float hi,
                             unsigned long long *counts_dev, void *stream)
{
    if (!counts_dev) return fail(SVBRDF_ERR_NULL, "check_arith: null pointer");
    if (!(lo > 0.0f) || !(hi > lo)) return fail(SVBRDF_ERR_DIMS, "check_arith: need 0 < lo < hi");
    hipLaunchKernelGGL(k_check_arith, dim3(2048), dim3(kThreads), 0, static_cast<hipStream_t>(stream), n, seed, lo, hi,
                       counts_dev);
    return launch_status("check_arith launch");
}

int svbrdf_mix_materials(const float *svbrdf0, const float *svbrdf1, const float *alpha, float *out, int B, int H, int W,
                         void *stream)
{
    if (!svbrdf0 || !svbrdf1 || !alpha || !out) return fail(SVBRDF_ERR_NULL, "mix_materials: null pointer");
    if (B <= 0 || H <= 0 || W <= 0 || B > 65535 || (long long)H * W > (1LL << 30))
        return fail(SVBRDF_ERR_DIMS, "mix_materials: bad dimensions");
    if (!aligned(svbrdf0, 4) || !aligned(svbrdf1, 4) || !aligned(alpha, 4) || !aligned(out, 4))
        return fail(SVBRDF_ERR_ALIGN, "mix_materials: pointers must be 4-byte aligned");
    const size_t plane = (size_t)H * W;
    int vec = 4;            // whole planes are contiguous here: the vector width only needs H*W and the bases to agree
    while (vec > 1 && !((plane % vec) == 0 && aligned(svbrdf0, 4 * vec) && aligned(svbrdf1, 4 * vec) && aligned(out, 4 * vec))) vec >>= 1;
    const dim3 grid((unsigned)((plane + (size_t)kThreads * vec - 1) / ((size_t)kThreads * vec)), (unsigned)B, 1), block(kThreads);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (vec == 4) hipLaunchKernelGGL(k_mix_materials<4>, grid, block, 0, st, svbrdf0, svbrdf1, alpha, out, plane);
    else if (vec == 2) hipLaunchKernelGGL(k_mix_materials<2>, grid, block, 0, st, svbrdf0, svbrdf1, alpha, out, plane);
    else hipLaunchKernelGGL(k_mix_materials<1>, grid, block, 0, st, svbrdf0, svbrdf1, alpha, out, plane);
    return launch_status("mix_materials launch");
}

int svbrdf_debug_copy(float *dst, const float *src, size_t n, void *stream)
{
    if (!dst || !src) return fail(SVBRDF_ERR_NULL, "debug_copy: null pointer");
    if (n == 0 || (n & 3) != 0) return fail(SVBRDF_ERR_DIMS, "debug_copy: n must be a positive multiple of 4 floats");
    if (!aligned(dst, 16) || !aligned(src, 16)) return fail(SVBRDF_ERR_ALIGN, "debug_copy: pointers must be 16-byte aligned");
    const int unroll = [] { const char *e = std::getenv("SVBRDF_COPY_UNROLL"); const int v = e ? std::atoi(e) : 0;
                            return (v == 1 || v == 2 || v == 4 || v == 8) ? v : 1; }();
    const bool nt = [] { const char *e = std::getenv("SVBRDF_COPY_NT"); return !(e && e[0] == '0'); }();
    const size_t n4 = n / 4, per_block = (size_t)kThreads * unroll, blocks = (n4 + per_block - 1) / per_block;
    if (blocks > 0x7fffffffULL) return fail(SVBRDF_ERR_DIMS, "debug_copy: n too large");
    const dim3 grid((unsigned)blocks), block(kThreads);
    hipStream_t st = static_cast<hipStream_t>(stream);
    vec4f *d = reinterpret_cast<vec4f *>(dst);
    const vec4f *sp = reinterpret_cast<const vec4f *>(src);
#define SVBRDF_COPY(U)                                                                            \
    do {                                                                                          \
        if (nt) hipLaunchKernelGGL((k_copy_vec4<U, true>), grid, block, 0, st, d, sp, n4);        \
        else hipLaunchKernelGGL((k_copy_vec4<U, false>), grid, block, 0, st, d, sp, n4);          \
    } while (0)
    if (unroll == 8) SVBRDF_COPY(8); else if (unroll == 4) SVBRDF_COPY(4); else if (unroll == 2) SVBRDF_COPY(2); else SVBRDF_COPY(1);
#undef SVBRDF_COPY
    return launch_status("debug_copy launch");
}

unsigned long long svbrdf_debug_launch_count(void) { return g_launches.load(std::memory_order_relaxed); }

int svbrdf_debug_clock_probe(unsigned long long *out_dev, unsigned long long ticks_100mhz, void *stream)
{
    if (!out_dev) return fail(SVBRDF_ERR_NULL, "clock_probe: null pointer");
    if (ticks_100mhz == 0 || ticks_100mhz > 100000000ULL) return fail(SVBRDF_ERR_DIMS, "clock_probe: 0 < ticks <= 1e8 (1 s)");
    hipLaunchKernelGGL(k_clock_probe, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), out_dev, ticks_100mhz);
    return launch_status("clock_probe launch");
}

}  // extern "C"
