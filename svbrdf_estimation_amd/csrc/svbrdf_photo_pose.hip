// svbrdf_photo_pose.hip -- translation unit of libsvbrdf_hip.so: the fused photo losses with the gradient towards the
// SCENE TABLE -- camera position, light position, light colour of every photo -- in the one launch (added to ABI version 8
// without a bump).
//
//   L = (1/N) sum w | log(render(scene[b,s], input[b]) + eps) - log(p' + eps) |
//   grad_scenes[b,s,0:3] = dL/d camera, [3:6] = dL/d light position, [6:9] = dL/d light colour
//
// A captured flash photograph comes with a camera position estimated from a homography and a flash "somewhere next to the
// lens"; with the table frozen a light that is a few centimetres off is absorbed into the normals and the roughness.  The
// loss and the map gradient are bit for bit those of the existing entries on the same table, by construction: the forward
// and the map adjoint are svbrdf_photo_loss_device.h's per-render functions (photo_pixel_scene, photo_pixel_scene_by_channel)
// with POSE set, which adds statements behind theirs and changes none, and float arithmetic without contraction does not
// depend on how the compiler schedules it.
//
// Four kernels, {maps, head} x {unweighted, weighted}, forward + adjoint, scene table in device memory.  The shape is the
// exposure kernels' (svbrdf_photo_exposure.hip) and so are its parts, shared through svbrdf_photo_loss_device.h: a wave that
// holds at least one pixel runs WHOLE (wave_index), the set-up of a pixel (wave_pixel_setup), per-wave rows of sums in
// LDS, the end of the launch (photo_sums_finish), the launcher's checks (plan_sums).  What differs:
//   * per render the adjoint continues behind the bars shade_bwd forms (NH, VN, LN, LN+): the bars of p = (1 - VH)^5 and of
//     the falloff, then back through the normalisations of h, wo and wi to camera - P and light - P (pose_bwd): 9 values per
//     (pixel, render), consumed at once -- summed over the wave in float (DPP, fixed lanes, fixed order) and stored in the
//     wave's row of LDS by its last lane;
//   * the position terms are not bounded by 1 as the exposure's are: the wave sums stay FLOAT in LDS, and behind the loop
//     9 S lanes check each against kPoseWaveLimit, convert to 64-bit fixed point (unit 2^-24 / N) and add the four waves'
//     values to the accumulator.  A wave sum that is NaN or beyond the limit makes the loss NaN (and with it every
//     gradient): 2^19 waves per item (plan_loss: H W <= 2^25) times 2^43 cannot wrap 63 bits;
//   * the scene loop is the plain one (geometry, shading, adjoint of render s; the photo of render s + 1 loaded ahead), not
//     the two-pass software pipeline of the kernels without a scene gradient: this loop already stands at 122 / 125 of 128
//     VGPRs (maps), and the pipelined form, which holds a second geometry, was not built and is unmeasured.  It is the one
//     piece of the flow that stands beside photo_scene_loop instead of inside it.
// The scene loop and the body (pose_scene_loop, pose_body) are in svbrdf_photo_pose_device.h, which the joint fit units
// include too; this file holds the four kernels, their launcher and their entry points.
#include "svbrdf_photo_pose_device.h"

namespace {

#define SVBRDF_POSE_KERNEL(NAME, HEAD, WEIGHTED)                                                                      \
    __global__ SVBRDF_PHOTO_LOSS_ATTRS void NAME(const float *__restrict__ input, const float *__restrict__ photos,   \
                                                 const float *__restrict__ weights, int weight_planes,                \
                                                 const float *__restrict__ scenes, const float *__restrict__ xrow,    \
                                                 float eps, float inv_count, double loss_scale, float fixed_scale,    \
                                                 double grad_scale, float per_count, float *__restrict__ grad_input,  \
                                                 float *__restrict__ grad_scenes, unsigned long long *__restrict__ ws, \
                                                 float *__restrict__ loss_out, int S, int H, int W)                   \
    {                                                                                                                 \
        pose_body<HEAD, WEIGHTED>(input, photos, weights, weight_planes, scenes, xrow, eps, inv_count, loss_scale,    \
                                  fixed_scale, grad_scale, per_count, grad_input, grad_scenes, ws, loss_out, S, H, W); \
    }
// (names that hold none of "k_photo_loss", "k_head_photo", "wphoto", "k_exposure": the other photo kernels are counted by those)
SVBRDF_POSE_KERNEL(k_pose_maps, false, false)
SVBRDF_POSE_KERNEL(k_pose_maps_weighted, false, true)
SVBRDF_POSE_KERNEL(k_pose_head, true, false)
SVBRDF_POSE_KERNEL(k_pose_head_weighted, true, true)
#undef SVBRDF_POSE_KERNEL

// The argument checks, the grid and the scales (plan_sums: the exposure entries' order and codes), the launch.
int pose_impl(const char *who, bool head, const float *input, const float *photos, const float *weights, int weight_planes,
              const float *scenes, const float *xrow, float eps, float *loss_out, float *grad_input, float *grad_scenes,
              void *workspace, size_t workspace_bytes, int B, int S, int H, int W, void *stream)
{
    LossPlan p;
    double units;       // N 2^24
    if (int e = plan_sums(who, {input, photos, grad_scenes, scenes, xrow, loss_out}, weights, weight_planes, nullptr, eps,
                          grad_input, workspace, workspace_bytes, 9, kPoseSpill, B, S, H, W, &p, &units)) return e;
    const auto kernel = head ? (weights ? k_pose_head_weighted : k_pose_head) : (weights ? k_pose_maps_weighted : k_pose_maps);
    hipLaunchKernelGGL(kernel, p.grid, dim3(kLossThreads), p.lds_bytes, static_cast<hipStream_t>(stream), input, photos,
                       weights, weight_planes, scenes, xrow, eps, p.inv_count, p.loss_scale, p.fixed_scale, 1.0 / units,
                       (float)units, grad_input, grad_scenes, p.ws, loss_out, S, H, W);
    return launch_status(who);
}

}  // namespace

extern "C" {

size_t svbrdf_photo_scene_grad_workspace_bytes(int B, int S, int H, int W)
{
    return sums_workspace_bytes(9, B, S, H, W);
}

int svbrdf_photo_loss_scene_grad_fwd_bwd(const float *input, const float *photos, const float *weights, int weight_planes,
                                         const float *scenes, const float *xrow, float eps, float *loss_out,
                                         float *grad_input, float *grad_scenes, void *workspace, size_t workspace_bytes,
                                         int B, int S, int H, int W, void *stream)
{
    return pose_impl("photo_loss_scene_grad", false, input, photos, weights, weight_planes, scenes, xrow, eps, loss_out,
                     grad_input, grad_scenes, workspace, workspace_bytes, B, S, H, W, stream);
}

int svbrdf_head_photo_loss_scene_grad_fwd_bwd(const float *encoded9, const float *photos, const float *weights,
                                              int weight_planes, const float *scenes, const float *xrow, float eps,
                                              float *loss_out, float *grad_encoded9, float *grad_scenes, void *workspace,
                                              size_t workspace_bytes, int B, int S, int H, int W, void *stream)
{
    return pose_impl("head_photo_loss_scene_grad", true, encoded9, photos, weights, weight_planes, scenes, xrow, eps,
                     loss_out, grad_encoded9, grad_scenes, workspace, workspace_bytes, B, S, H, W, stream);
}

}  // extern "C"
