// svbrdf_photo_fit.hip -- translation unit of libsvbrdf_hip.so: one STEP of a fit of SVBRDF maps to photographs -- the
// photo loss, its gradient and the Adam update of the maps -- in the one launch (added to ABI version 8 without a bump).
//
//   g  = d/d maps of (1/N) sum w | log(render(scene[b,s], maps[b]) + eps) - log(p' + eps) |      (never written, unless asked for)
//   m' = (beta1 m) + (c1 g)                    c1 = 1 - beta1
//   v' = (beta2 v) + ((c2 g) g)                c2 = 1 - beta2
//   x' = clamp(x - step_size (m' / ((sqrt(v') rsb2) + adam_eps)), lo[ch], hi[ch])
//                                              step_size = lr / (1 - beta1^t), rsb2 = 1 / sqrt(1 - beta2^t)
//
// The loop a user of PhotoLoss runs is loss, backward, torch.optim.Adam.step, clamp_: the first two are one launch, the other
// two are several more passes over the same [B,12,H,W] tensors.  A thread of the photo kernels owns one pixel and all S
// renders of it, and behind the scene loop it holds that pixel's complete gradient in 12 registers, 1/N folded in; Adam is
// element-wise.  So the thread applies the update itself: 24 state values in, 36 out, the gradient stays in registers.
//
// Two kernels, unweighted and weighted, forward + adjoint, scene table in device memory.  The flow is
// svbrdf_photo_loss.hip's, included below without its kernels, launcher and entry points: the set-up of a pixel
// (wave_pixel_setup), the scene loop (photo_scene_loop, tied / three-lobe chosen per wave as k_photo_loss / k_wphoto
// choose it), the loss reduction (loss_arrive, same 65-word scratch).  The loss and the gradient are therefore bit for bit
// those of svbrdf_photo_loss[_weighted]_fwd_bwd: the same statements, and float arithmetic without contraction does not
// depend on how the compiler schedules it.  What differs:
//   * the diffuse and roughness planes of the pixel as stored (the set-up keeps only what it derives from them; normal and
//     specular survive in MapK as loaded) wait in LDS across the scene loop: the loop has no six registers to spare;
//   * behind the loop, when the shading temporaries are dead: the 24 state loads back to back, the five lines above per
//     channel -- every operation an individually rounded float32 one (this unit is built with -ffp-contract=off and the
//     lines hold no fma), IEEE division and square root -- and 36 stores with the gradient stores' cache policy;
//   * the clamp is two compares and selects: a NaN stays a NaN (v_max / v_min would return the bound), +-inf bounds never
//     select.
#define SVBRDF_PHOTO_SHARED_ONLY
#include "svbrdf_photo_loss.hip"

namespace {

// What the update needs, by value in the kernel-argument block (scalar loads, wave-uniform)
struct AdamArgs {
    float beta1, c1, beta2, c2, step_size, rsb2, adam_eps;
    float lo[12], hi[12];
};

// plane order of a [12,H,W] SVBRDF: normal 0:3, diffuse 3:6, roughness 6:9, specular 9:12
__device__ __forceinline__ float fit_stash(int k, float put, bool take)
{
    __shared__ float words[6 * kLossThreads];
    int i = k * kLossThreads + (int)threadIdx.x;
    if (!take) {
        words[i] = put;
        return put;
    }
    asm volatile("" : "+v"(i));     // (expo_stash: the compiler would otherwise forward the stored registers and keep them)
    return words[i];
}

__device__ __forceinline__ float adam_channel(const AdamArgs &a, int ch, float x, float g, float &m, float &v)
{
    m = (a.beta1 * m) + (a.c1 * g);
    v = (a.beta2 * v) + ((a.c2 * g) * g);
    const float den = (sqrtf(v) * a.rsb2) + a.adam_eps;
    float xn = x - (a.step_size * (m / den));
    xn = xn < a.lo[ch] ? a.lo[ch] : xn;         // false for NaN: it stays
    xn = xn > a.hi[ch] ? a.hi[ch] : xn;
    return xn;
}

// One thread = one pixel, all S renders of it and its 36 values of maps and state; workgroup = 256 pixels of one item, as
// photo_loss_body<true, false, false, WEIGHTED>.
template <bool WEIGHTED>
__device__ __forceinline__ void fit_body(float *maps, float *exp_avg, float *exp_avg_sq, const float *__restrict__ photos,
                                         const float *__restrict__ weights, int weight_planes,
                                         const float *__restrict__ scenes, const float *__restrict__ xrow, float eps,
                                         float inv_count, double loss_scale, float fixed_scale, const AdamArgs &adam,
                                         float *grad_out, unsigned long long *__restrict__ ws,
                                         float *__restrict__ loss_out, int S, int H, int W)
{
    const size_t plane = (size_t)H * W;
    const size_t pix = (size_t)blockIdx.x * kLossThreads + threadIdx.x;
    const int b = blockIdx.y;
    float lsum = 0.0f;
    if (pix < plane) {
        {
            // diffuse and roughness as stored, to LDS (the same six loads wave_pixel_setup issues: one access each)
            const PlaneBuf xb = plane_buf(maps + (size_t)b * 12 * plane, 12, plane, pix);
#pragma unroll
            for (int k = 0; k < 6; ++k) fit_stash(k, plane_load(xb, 3 + k), false);
        }
        PixelSetup ps = wave_pixel_setup<false, WEIGHTED>(maps, xrow, b, plane, pix, W);
        const float *__restrict__ scp = scenes + (size_t)b * S * 9;
        const float *__restrict__ pp = photos + (size_t)b * S * 3 * plane;
        const float *__restrict__ wp = WEIGHTED ? weights + (size_t)b * weight_planes * plane : nullptr;
        const size_t wstride = weight_planes == 1 ? 0 : plane;
        if (__all(ps.tied))         // wave-uniform
            lsum = photo_scene_loop<1, true, 7, WEIGHTED>(ps.mi, ps.x, ps.y, scp, nullptr, pp, plane, pix, S, eps, inv_count,
                                                          ps.acc, wp, wstride, ps.poison);
        else
            lsum = photo_scene_loop<3, true, 3, WEIGHTED>(ps.mi, ps.x, ps.y, scp, nullptr, pp, plane, pix, S, eps, inv_count,
                                                          ps.acc, wp, wstride, ps.poison);
        if (grad_out) store_grads_k3(grad_out + (size_t)b * 12 * plane, plane, pix, ps.acc);
        const PlaneBuf xb = plane_buf(maps + (size_t)b * 12 * plane, 12, plane, pix);
        const PlaneBuf mb = plane_buf(exp_avg + (size_t)b * 12 * plane, 12, plane, pix);
        const PlaneBuf vb = plane_buf(exp_avg_sq + (size_t)b * 12 * plane, 12, plane, pix);
        float m[12], v[12], x[12], g[12];
        __builtin_amdgcn_sched_barrier(0);      // the three resources stand: the 24 state loads back to back
#pragma unroll
        for (int k = 0; k < 12; ++k) m[k] = plane_load(mb, k);
#pragma unroll
        for (int k = 0; k < 12; ++k) v[k] = plane_load(vb, k);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            x[0 + k] = ps.mi.n[k];
            x[3 + k] = fit_stash(k, 0.0f, true);
            x[6 + k] = fit_stash(3 + k, 0.0f, true);
            x[9 + k] = ps.mi.s[k];
            g[0 + k] = ps.acc.n[k];
            g[3 + k] = ps.acc.d[k];
            g[6 + k] = ps.acc.r[k];
            g[9 + k] = ps.acc.s[k];
        }
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            const float xn = adam_channel(adam, k, x[k], g[k], m[k], v[k]);
            plane_store(xb, k, xn);
            plane_store(mb, k, m[k]);
            plane_store(vb, k, v[k]);
        }
    }
    {
        __shared__ float wave_part[kLossThreads / 64];
        lsum = wave_sum(lsum);
        if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = lsum;
        __syncthreads();
        if (threadIdx.x == 0) {
            float t = 0.0f;
#pragma unroll
            for (int w = 0; w < kLossThreads / 64; ++w) t += wave_part[w];
            loss_arrive(t, fixed_scale, loss_scale, ws, loss_out);
        }
    }
}

#define SVBRDF_FIT_KERNEL(NAME, WEIGHTED)                                                                             \
    __global__ SVBRDF_PHOTO_LOSS_ATTRS void NAME(float *maps, float *exp_avg, float *exp_avg_sq,                      \
                                                 const float *__restrict__ photos, const float *__restrict__ weights, \
                                                 int weight_planes, const float *__restrict__ scenes,                 \
                                                 const float *__restrict__ xrow, float eps, float inv_count,          \
                                                 double loss_scale, float fixed_scale, const AdamArgs adam,           \
                                                 float *grad_out, unsigned long long *__restrict__ ws,                \
                                                 float *__restrict__ loss_out, int S, int H, int W)                   \
    {                                                                                                                 \
        fit_body<WEIGHTED>(maps, exp_avg, exp_avg_sq, photos, weights, weight_planes, scenes, xrow, eps, inv_count,   \
                           loss_scale, fixed_scale, adam, grad_out, ws, loss_out, S, H, W);                           \
    }
// (names that hold none of "k_photo_loss", "k_head_photo", "wphoto", "k_exposure", "k_pose": the other photo kernels are
// counted by those)
SVBRDF_FIT_KERNEL(k_fit_maps, false)
SVBRDF_FIT_KERNEL(k_fit_maps_weighted, true)
#undef SVBRDF_FIT_KERNEL

// The four scalars of a step, in double from the float arguments the step entry takes, each rounded once to float.
// -> false: the arguments are not an Adam step's.
bool adam_scalars(float lr, float beta1, float beta2, int step, float out[4])
{
    if (step < 1 || !(lr >= 0.0f) || !std::isfinite(lr) || !(beta1 >= 0.0f && beta1 < 1.0f) || !(beta2 >= 0.0f && beta2 < 1.0f))
        return false;
    const double b1 = beta1, b2 = beta2;
    out[0] = (float)(1.0 - b1);
    out[1] = (float)(1.0 - b2);
    out[2] = (float)((double)lr / (1.0 - std::pow(b1, (double)step)));
    out[3] = (float)(1.0 / std::sqrt(1.0 - std::pow(b2, (double)step)));
    return true;
}

}  // namespace

extern "C" {

int svbrdf_photo_fit_adam_scalars(float lr, float beta1, float beta2, int step, float *out4)
{
    if (!out4) return fail(SVBRDF_ERR_NULL, "photo_fit_adam_scalars");
    if (!adam_scalars(lr, beta1, beta2, step, out4))
        return fail(SVBRDF_ERR_DIMS, "photo_fit_adam_scalars: step >= 1, a finite lr >= 0 and betas in [0, 1) are required");
    return 0;
}

int svbrdf_photo_fit_adam_step(float *maps, float *exp_avg, float *exp_avg_sq, const float *photos, const float *weights,
                               int weight_planes, const float *scenes, const float *xrow, float eps,
                               const float *bounds_host, float lr, float beta1, float beta2, float adam_eps, int step,
                               float *loss_out, float *grad_out, void *workspace, size_t workspace_bytes, int B, int S, int H,
                               int W, void *stream)
{
    const char *who = "photo_fit_adam_step";
    char text[200];
    const auto bad = [&](int code, const char *what) {
        std::snprintf(text, sizeof(text), "%s: %s", who, what);
        return fail(code, text);
    };
    LossPlan p;
    // (grad_out may be null and the kernels are forward + adjoint whatever it is: the plan is the one with a gradient)
    if (int e = plan_loss(who, false, {maps, exp_avg, exp_avg_sq, photos, scenes, xrow, loss_out}, grad_out ? grad_out : maps,
                          workspace, workspace_bytes, "eps", eps, 0.0f, B, S, H, W, &p)) return e;
    if (!aligned(weights, 4)) return bad(SVBRDF_ERR_ALIGN, "pointers must be 4-byte aligned");
    if (weights ? (weight_planes != 1 && weight_planes != S) : weight_planes != 0)
        return bad(SVBRDF_ERR_DIMS, "weight_planes must be 1 (one plane per item) or S (one per photo) with weights, 0 without");
    AdamArgs a;
    float sc[4];
    if (!adam_scalars(lr, beta1, beta2, step, sc))
        return bad(SVBRDF_ERR_DIMS, "step >= 1, a finite lr >= 0 and betas in [0, 1) are required");
    if (!(adam_eps >= 0.0f) || !std::isfinite(adam_eps)) return bad(SVBRDF_ERR_DIMS, "adam_eps must be finite and >= 0");
    a.beta1 = beta1; a.c1 = sc[0]; a.beta2 = beta2; a.c2 = sc[1]; a.step_size = sc[2]; a.rsb2 = sc[3]; a.adam_eps = adam_eps;
    for (int k = 0; k < 12; ++k) {
        a.lo[k] = bounds_host ? bounds_host[2 * k] : -__builtin_inff();
        a.hi[k] = bounds_host ? bounds_host[2 * k + 1] : __builtin_inff();
        if (!(a.lo[k] <= a.hi[k])) return bad(SVBRDF_ERR_DIMS, "bounds must hold lo <= hi for every channel, and no NaN");
    }
    hipLaunchKernelGGL(weights ? k_fit_maps_weighted : k_fit_maps, p.grid, dim3(kLossThreads), 0,
                       static_cast<hipStream_t>(stream), maps, exp_avg, exp_avg_sq, photos, weights, weight_planes, scenes,
                       xrow, eps, p.inv_count, p.loss_scale, p.fixed_scale, a, grad_out, p.ws, loss_out, S, H, W);
    return launch_status(who);
}

}  // extern "C"
