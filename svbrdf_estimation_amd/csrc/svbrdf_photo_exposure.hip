// svbrdf_photo_exposure.hip -- translation unit of libsvbrdf_hip.so: the fused photo losses with a PER-PHOTO EXPOSURE and
// its gradient in the one launch (added to ABI version 8 without a bump).
//
//   L = (1/N) sum w | log(render(scene[b,s] with light colour fl32(colour_c e[b,s,c]), input[b]) + eps) - log(p' + eps) |
//   dL/de[b,s,c] = sum_{i,j} w sign(delta) rad_c / (N (rad_c + eps) e_c)
//
// Every captured photograph has an unknown radiometric scale (flash power, shutter, ISO, white balance); without a
// gradient towards it a wrong flash intensity is absorbed into the albedos.  The gain enters as ONE float32 multiply of the
// scene row's colour in front of the falloff, so the loss and the map gradient are bit for bit those of the existing
// kernels on a table whose colour columns were multiplied by e in float32 (all-ones e: the existing results).  The gradient
// towards light and camera positions is svbrdf_photo_pose.hip's.
//
// Four kernels, {maps, head} x {unweighted, weighted}, forward + adjoint, scene table in device memory.  They are
// svbrdf_photo_loss.hip's flow -- the per-render device functions of svbrdf_photo_loss_device.h with EXPO set -- plus:
//   * per item and wave: the 3 S gains are checked once, a lane each; one that is NaN, infinite or <= 0 poisons the
//     loss the way a bad weight does;
//   * per render: the gains (wave-uniform loads) scale the colour (expo_scale); q = w sign(delta)
//     (1 - ec / b) per channel from registers the loss already holds (no new transcendental, no division) is summed over
//     the wave and stored, as a fixed-point integer, in the wave's row of the [waves][kExpoSpill + 3 S] LDS sums by one lane (expo_collect);
//   * behind the loop the launch ends as photo_sums_finish (svbrdf_photo_loss_device.h, where the hand-off is explained) ends
//     it: the four waves' integers added to the B S 3 accumulator words of the workspace, the arrival, and the finisher
//     writes grad_exposure = sum / (2^24 N e), or NaN everywhere when the loss is NaN.
// Integer sums from the wave on: bitwise reproducible.
// (The alternative, a per-workgroup slab of sums written with sc1 stores and added up by the finisher, needs
// grid x 3 S words of workspace, more than the 65 + B S 3 words of the C ABI, and a finisher that reads all of them: not
// built, and unmeasured.  What the tail of this variant costs is measured: DESIGN.md section 4.5, round 16.)
// The wave-whole indexing, the set-up of a pixel, the end of the launch and the launcher's checks are shared with
// svbrdf_photo_pose.hip through svbrdf_photo_loss_device.h (wave_index, wave_pixel_setup, photo_sums_finish, plan_sums).
#include "svbrdf_photo_loss_device.h"

namespace {

// One thread = one pixel, all S renders of it; workgroup = 256 pixels of one item, as photo_loss_body<true, false, HEAD,
// WEIGHTED>.  The difference in shape: a wave that holds at least one pixel runs WHOLE (wave_index), so that the wave sums
// of expo_collect never read a disabled lane.
template <bool HEAD, bool WEIGHTED>
__device__ __forceinline__ void exposure_body(const float *__restrict__ input, const float *__restrict__ photos,
                                              const float *__restrict__ weights, int weight_planes,
                                              const float *__restrict__ exposure, const float *__restrict__ scenes,
                                              const float *__restrict__ xrow, float eps, float inv_count, double loss_scale,
                                              float fixed_scale, double grad_scale, float per_weight,
                                              float *__restrict__ grad_input,
                                              float *__restrict__ grad_exposure, unsigned long long *__restrict__ ws,
                                              float *__restrict__ loss_out, int S, int H, int W)
{
    int *q_lds = expo_lds();        // [waves][kExpoSpill + 3 S]: see ExpoLoop
    const size_t plane = (size_t)H * W;
    const int b = blockIdx.y;
    const int n_sums = 3 * S;
    // (no barrier in front of the scene loop: behind one, the wave-uniform loads of the scene rows and the gains would no
    // longer be scalar loads)
    const WaveIndex wi = wave_index(plane, kExpoSpill + n_sums);
    float lsum = 0.0f;
    int *wave_sums = q_lds + wi.row + kExpoSpill;       // (through the pointer: the indexed form costs the weighted maps
                                                        // kernel a fifth spilled SGPR)
    if (!wi.wave_live) {
        for (int i = threadIdx.x & 63; i < n_sums; i += 64) wave_sums[i] = 0;      // a wave without pixels: its row of zeros
    } else {
        PixelSetup ps = wave_pixel_setup<HEAD, WEIGHTED>(input, xrow, b, plane, wi.pix, W);
        const float *__restrict__ scp = scenes + (size_t)b * S * 9;
        const float *__restrict__ pp = photos + (size_t)b * S * 3 * plane;
        const float *__restrict__ wp = WEIGHTED ? weights + (size_t)b * weight_planes * plane : nullptr;
        const size_t wstride = weight_planes == 1 ? 0 : plane;
        const ExpoLoop xl{wi.row, wi.live, per_weight};
#pragma unroll
        for (int k = 0; k < 3; ++k) expo_stash(k, ps.mi.r4m[k], false);
        const float *__restrict__ gain = exposure + (size_t)b * n_sums;
        if (HEAD || __builtin_amdgcn_readfirstlane((int)__all(ps.tied)))      // wave-uniform, and known to be
            lsum = photo_scene_loop<1, true, 7, WEIGHTED, true>(ps.mi, ps.x, ps.y, scp, nullptr, pp, plane, wi.pix, S, eps,
                                                                inv_count, ps.acc, wp, wstride, ps.poison, &xl, gain);
        else
            lsum = photo_scene_loop<3, true, 3, WEIGHTED, true>(ps.mi, ps.x, ps.y, scp, nullptr, pp, plane, wi.pix, S, eps,
                                                                inv_count, ps.acc, wp, wstride, ps.poison, &xl, gain);
        // the item's gains.  (Behind the scene loop: in front of it these vector loads keep the loop's own loads of the gains
        // from being scalar loads.)
        positive_check(gain, 3, 0, S, lsum);
        if (wi.live) {
            if (HEAD) store_pixel_grad<true>(ps.head, ps.acc, grad_input, b, plane, wi.pix);
            else store_grads_k3(grad_input + (size_t)b * 12 * plane, plane, wi.pix, ps.acc);
        } else {
            lsum -= lsum;       // +0; a NaN stays (expo_collect's poison sits in lane 63, a bad gain's in every lane)
        }
    }
    photo_sums_finish<false>(
        lsum, b, n_sums, fixed_scale, loss_scale, ws, loss_out,
        [&](int i, bool &) {        // the waves' integers: nothing to check
            long long sum = 0;
#pragma unroll
            for (int w = 0; w < kLossThreads / 64; ++w) sum += q_lds[w * (kExpoSpill + n_sums) + kExpoSpill + i];
            return sum;
        },
        [&](int i, long long sum, bool nan) {       // grad_exposure = sum / (2^24 N e)
            if (grad_exposure) {
                const float g = (float)((double)sum * grad_scale) * rcp_(exposure[i]);
                grad_exposure[i] = nan ? __builtin_nanf("") : g;
            }
        });
}

#define SVBRDF_EXPOSURE_KERNEL(NAME, HEAD, WEIGHTED)                                                                  \
    __global__ SVBRDF_PHOTO_LOSS_ATTRS void NAME(const float *__restrict__ input, const float *__restrict__ photos,   \
                                                 const float *__restrict__ weights, int weight_planes,                \
                                                 const float *__restrict__ exposure, const float *__restrict__ scenes, \
                                                 const float *__restrict__ xrow, float eps, float inv_count,          \
                                                 double loss_scale, float fixed_scale, double grad_scale,             \
                                                 float per_weight,                                                    \
                                                 float *__restrict__ grad_input, float *__restrict__ grad_exposure,   \
                                                 unsigned long long *__restrict__ ws, float *__restrict__ loss_out,   \
                                                 int S, int H, int W)                                                 \
    {                                                                                                                 \
        exposure_body<HEAD, WEIGHTED>(input, photos, weights, weight_planes, exposure, scenes, xrow, eps, inv_count,  \
                                      loss_scale, fixed_scale, grad_scale, per_weight, grad_input, grad_exposure, ws,  \
                                      loss_out, S,                                                                    \
                                      H, W);                                                                          \
    }
// (names that hold none of "k_photo_loss", "k_head_photo", "wphoto": the other photo kernels are counted by those)
SVBRDF_EXPOSURE_KERNEL(k_exposure_maps, false, false)
SVBRDF_EXPOSURE_KERNEL(k_exposure_maps_weighted, false, true)
SVBRDF_EXPOSURE_KERNEL(k_exposure_head, true, false)
SVBRDF_EXPOSURE_KERNEL(k_exposure_head_weighted, true, true)
#undef SVBRDF_EXPOSURE_KERNEL

// The argument checks, the grid and the scales (plan_sums), the launch.
int exposure_impl(const char *who, bool head, const float *input, const float *photos, const float *weights,
                  int weight_planes, const float *exposure, const float *scenes, const float *xrow, float eps,
                  float *loss_out, float *grad_input, float *grad_exposure, void *workspace, size_t workspace_bytes, int B,
                  int S, int H, int W, void *stream)
{
    LossPlan p;
    double units;       // N 2^24
    if (int e = plan_sums(who, {input, photos, exposure, scenes, xrow, loss_out}, weights, weight_planes, grad_exposure, eps,
                          grad_input, workspace, workspace_bytes, 3, kExpoSpill, B, S, H, W, &p, &units)) return e;
    const auto kernel = head ? (weights ? k_exposure_head_weighted : k_exposure_head)
                             : (weights ? k_exposure_maps_weighted : k_exposure_maps);
    hipLaunchKernelGGL(kernel, p.grid, dim3(kLossThreads), p.lds_bytes, static_cast<hipStream_t>(stream), input, photos,
                       weights, weight_planes, exposure, scenes, xrow, eps, p.inv_count, p.loss_scale, p.fixed_scale,
                       1.0 / units, (float)units, grad_input, grad_exposure, p.ws, loss_out, S, H, W);
    return launch_status(who);
}

}  // namespace

extern "C" {

size_t svbrdf_photo_exposure_workspace_bytes(int B, int S, int H, int W)
{
    return sums_workspace_bytes(3, B, S, H, W);
}

int svbrdf_photo_loss_exposure_fwd_bwd(const float *input, const float *photos, const float *weights, int weight_planes,
                                       const float *exposure, const float *scenes, const float *xrow, float eps,
                                       float *loss_out, float *grad_input, float *grad_exposure, void *workspace,
                                       size_t workspace_bytes, int B, int S, int H, int W, void *stream)
{
    return exposure_impl("photo_loss_exposure", false, input, photos, weights, weight_planes, exposure, scenes, xrow, eps,
                         loss_out, grad_input, grad_exposure, workspace, workspace_bytes, B, S, H, W, stream);
}

int svbrdf_head_photo_loss_exposure_fwd_bwd(const float *encoded9, const float *photos, const float *weights,
                                            int weight_planes, const float *exposure, const float *scenes,
                                            const float *xrow, float eps, float *loss_out, float *grad_encoded9,
                                            float *grad_exposure, void *workspace, size_t workspace_bytes, int B, int S,
                                            int H, int W, void *stream)
{
    return exposure_impl("head_photo_loss_exposure", true, encoded9, photos, weights, weight_planes, exposure, scenes, xrow,
                         eps, loss_out, grad_encoded9, grad_exposure, workspace, workspace_bytes, B, S, H, W, stream);
}

}  // extern "C"
