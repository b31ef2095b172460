// svbrdf_photo_fit_device.h -- the Adam update of a pixel behind the scene loop, the fit step's body and the host helpers
// of the fit entries, shared by svbrdf_photo_fit.hip (which describes them) and, through svbrdf_photo_fit_pose_device.h,
// the joint and the smooth units.
#ifndef SVBRDF_PHOTO_FIT_DEVICE_H
#define SVBRDF_PHOTO_FIT_DEVICE_H
#include "svbrdf_photo_loss_device.h"

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

// The single step's update of the pixel `pix` of item b, behind the scene loop: the 24 state loads back to back, the pixel's
// 12 values (normal and specular from `mi` as loaded, diffuse and roughness from fit_stash) and its gradient `acc`,
// adam_channel per channel, 36 stores.  The one copy: fit_body and joint_body (svbrdf_photo_fit_pose_device.h) call it.
__device__ __forceinline__ void adam_epilogue(float *maps, float *exp_avg, float *exp_avg_sq, int b, size_t plane, size_t pix,
                                              const PixelSetup &ps, const AdamArgs &adam)
{
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

// What fit_body and joint_body do with a pixel behind the scene loop.  This one: the gradient to grad_out if given, then
// adam_epilogue on `maps` itself.  A unit that includes this header may pass an update of its own, called as
// update(b, plane, pix, ps) and then in charge of grad_out too (svbrdf_photo_fit_smooth.hip: `maps` is then only read).
struct UpdateInPlace {
    static constexpr bool in_place = true;
};

// One thread = one pixel, all S renders of it and its 36 values of maps and state; workgroup = 256 pixels of one item, as
// photo_loss_body<true, false, false, WEIGHTED>.
template <bool WEIGHTED, typename Update = UpdateInPlace>
__device__ __forceinline__ void fit_body(float *maps, float *exp_avg, float *exp_avg_sq, const float *__restrict__ photos,
                                         const float *__restrict__ weights, int weight_planes,
                                         const float *__restrict__ scenes, const float *__restrict__ xrow, float eps,
                                         float inv_count, double loss_scale, float fixed_scale, const AdamArgs &adam,
                                         float *grad_out, unsigned long long *__restrict__ ws,
                                         float *__restrict__ loss_out, int S, int H, int W, const Update &update = {})
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
        if constexpr (Update::in_place) {
            if (grad_out) store_grads_k3(grad_out + (size_t)b * 12 * plane, plane, pix, ps.acc);
            adam_epilogue(maps, exp_avg, exp_avg_sq, b, plane, pix, ps, adam);
        } else {
            update(b, plane, pix, ps);
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

// What the fit entries check and fill alike, each in its own order -> 0, or the error reported (fail_as).  Their weights:
// weights_check of svbrdf_photo_loss_device.h, called by the entry or by its plan_sums.
// The update's arguments of Adam's step `step`: the scalars (`scalars_rule`: the entry's wording of what they require),
// adam_eps, the seven scalars, then the 12 bounds -- +-inf without bounds_host
int adam_args(const char *who, const char *scalars_rule, const float *bounds_host, float lr, float beta1, float beta2,
              float adam_eps, int step, AdamArgs *a)
{
    float sc[4];
    if (!adam_scalars(lr, beta1, beta2, step, sc)) return fail_as(who, SVBRDF_ERR_DIMS, scalars_rule);
    if (!(adam_eps >= 0.0f) || !std::isfinite(adam_eps))
        return fail_as(who, SVBRDF_ERR_DIMS, "adam_eps must be finite and >= 0");
    a->beta1 = beta1; a->c1 = sc[0]; a->beta2 = beta2; a->c2 = sc[1]; a->step_size = sc[2]; a->rsb2 = sc[3]; a->adam_eps = adam_eps;
    for (int k = 0; k < 12; ++k) {
        a->lo[k] = bounds_host ? bounds_host[2 * k] : -__builtin_inff();
        a->hi[k] = bounds_host ? bounds_host[2 * k + 1] : __builtin_inff();
        if (!(a->lo[k] <= a->hi[k]))
            return fail_as(who, SVBRDF_ERR_DIMS, "bounds must hold lo <= hi for every channel, and no NaN");
    }
    return 0;
}
constexpr const char *kStepRule = "step >= 1, a finite lr >= 0 and betas in [0, 1) are required";

}  // namespace

#endif  // SVBRDF_PHOTO_FIT_DEVICE_H
