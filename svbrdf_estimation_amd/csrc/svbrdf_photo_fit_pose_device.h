// svbrdf_photo_fit_pose_device.h -- joint_body, the fit step with the gradient towards the scene table: the pose header's
// scene loop and the fit header's update.  Shared by svbrdf_photo_fit_pose.hip (which describes it) and
// svbrdf_photo_fit_smooth.hip.
#ifndef SVBRDF_PHOTO_FIT_POSE_DEVICE_H
#define SVBRDF_PHOTO_FIT_POSE_DEVICE_H
#include "svbrdf_photo_pose_device.h"
#include "svbrdf_photo_fit_device.h"

namespace {

// (`update`: what a live lane does with its pixel behind the loop, UpdateInPlace of svbrdf_photo_fit_device.h unless a unit that
// includes this header passes its own)
template <bool WEIGHTED, typename Update = UpdateInPlace>
__device__ __forceinline__ void joint_body(float *maps, float *exp_avg, float *exp_avg_sq, const float *__restrict__ photos,
                                           const float *__restrict__ weights, int weight_planes,
                                           const float *__restrict__ scenes, const float *__restrict__ xrow, float eps,
                                           float inv_count, double loss_scale, float fixed_scale, double grad_scale,
                                           float per_count, const AdamArgs &adam, float *grad_out,
                                           float *__restrict__ grad_scenes, unsigned long long *__restrict__ ws,
                                           float *__restrict__ loss_out, int S, int H, int W,
                                           const Update &update = {})
{
    float *sums = pose_lds();
    const size_t plane = (size_t)H * W;
    const int b = blockIdx.y;
    const int n_sums = 9 * S;
    const WaveIndex wi = wave_index(plane, kPoseSpill + n_sums);
    float lsum = 0.0f;
    if (!wi.wave_live) {
        for (int i = threadIdx.x & 63; i < n_sums; i += 64) sums[wi.row + kPoseSpill + i] = 0.0f;     // a wave without pixels
    } else {
        {
            // diffuse and roughness as stored, to LDS (fit_body; a lane without a pixel stashes the last pixel's, unread)
            const PlaneBuf xb = plane_buf(maps + (size_t)b * 12 * plane, 12, plane, wi.pix);
#pragma unroll
            for (int k = 0; k < 6; ++k) fit_stash(k, plane_load(xb, 3 + k), false);
        }
        PixelSetup ps = wave_pixel_setup<false, WEIGHTED>(maps, xrow, b, plane, wi.pix, W);
        const float *__restrict__ scp = scenes + (size_t)b * n_sums;
        const float *__restrict__ pp = photos + (size_t)b * S * 3 * plane;
        const float *__restrict__ wp = WEIGHTED ? weights + (size_t)b * weight_planes * plane : nullptr;
        const size_t wstride = weight_planes == 1 ? 0 : plane;
#pragma unroll
        for (int k = 0; k < 3; ++k) expo_stash(k, ps.mi.r4m[k], false);
        if (__builtin_amdgcn_readfirstlane((int)__all(ps.tied)))      // wave-uniform, and known to be
            lsum = pose_scene_loop<1, WEIGHTED>(ps.mi, ps.x, ps.y, scp, pp, plane, wi.pix, S, eps, inv_count, ps.acc, wp,
                                                wstride, ps.poison, wi.row, wi.live);
        else
            lsum = pose_scene_loop<3, WEIGHTED>(ps.mi, ps.x, ps.y, scp, pp, plane, wi.pix, S, eps, inv_count, ps.acc, wp,
                                                wstride, ps.poison, wi.row, wi.live);
        positive_check(scp, 9, 6, S, lsum);         // the item's light colours
        if (wi.live) {
            // the fit step's update, for the lanes that own a pixel ONLY
            if constexpr (Update::in_place) {
                if (grad_out) store_grads_k3(grad_out + (size_t)b * 12 * plane, plane, wi.pix, ps.acc);
                adam_epilogue(maps, exp_avg, exp_avg_sq, b, plane, wi.pix, ps, adam);
            } else {
                update(b, plane, wi.pix, ps);
            }
        } else {
            lsum -= lsum;       // +0; a NaN stays
        }
    }
    photo_sums_finish<true>(
        lsum, b, n_sums, fixed_scale, loss_scale, ws, loss_out,
        [&](int i, bool &sane) {        // the waves' floats, each checked against kPoseWaveLimit, to fixed point (pose_body)
            long long sum = 0;
#pragma unroll
            for (int w = 0; w < kPoseWaves; ++w) {
                const float v = sums[w * (kPoseSpill + n_sums) + kPoseSpill + i] * per_count;
                const bool ok = fabsf(v) <= kPoseWaveLimit;         // false for NaN
                sane = sane && ok;
                sum += ok ? (long long)v : 0LL;
            }
            return sum;
        },
        [&](int i, long long sum, bool nan) {
            float gr = (float)((double)sum * grad_scale);
            if (i % 9 >= 6) gr *= rcp_(scenes[i]);       // the colour columns hold sum(Q): d / d colour = Q / colour
            grad_scenes[i] = nan ? __builtin_nanf("") : gr;
        });
}

}  // namespace

#endif  // SVBRDF_PHOTO_FIT_POSE_DEVICE_H
