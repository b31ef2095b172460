// svbrdf_photo_fit_pose.hip -- translation unit of libsvbrdf_hip.so: one step of a fit of SVBRDF maps to photographs
// WITH the gradient towards the scene table -- the photo loss, its gradient towards the maps, the Adam update of the maps,
// and d loss / d (camera, light position, light colour) of every photo -- in the one launch (added to ABI version 8
// without a bump).
//
// A flash photograph never comes with an exact light position or a known gain.  svbrdf_photo_pose.hip returns the
// gradient towards them and leaves the maps to torch.optim.Adam and clamp_, several passes over the [B,12,H,W] tensors;
// svbrdf_photo_fit.hip updates the maps in the launch and holds the table frozen.  This unit is both: the thread of the
// pose loop holds its pixel's complete map gradient in registers behind the loop exactly like the fit kernel's thread.
//
// Two kernels, unweighted and weighted, forward + adjoint, scene table in device memory.  Nothing is computed here that
// the two units do not compute: their device functions come from their headers, and what is written out
// (joint_body, in svbrdf_photo_fit_pose_device.h, which svbrdf_photo_fit_smooth.hip includes too) is the flow alone.
//   * per workgroup pose_body<false, WEIGHTED>'s: a wave that holds a pixel runs whole (wave_index), the per-wave rows of
//     float sums in dynamic LDS, pose_scene_loop<1|3, WEIGHTED> chosen per wave, the colour check, photo_sums_finish<true>
//     with the pose body's two lambdas.  loss_out, grad_out and grad_scenes are therefore bit for bit those of
//     svbrdf_photo_loss_scene_grad_fwd_bwd -- the NaN rules included;
//   * where the pose body stores the gradient of a live lane, the thread stores it if grad_out was given and then calls
//     the fit unit's adam_epilogue, the function fit_body calls: the 24 state loads back to back, adam_channel per channel,
//     36 stores with the gradient stores' cache policy.  Diffuse and roughness as stored wait in LDS across the loop
//     (fit_stash) beside expo_stash's three words.  maps', exp_avg' and exp_avg_sq' are bit for bit
//     svbrdf_photo_fit_adam_step's on the same gradient;
//   * the one place where the two flows disagree: a lane of a whole wave that has no pixel shades the item's LAST pixel
//     with 1/N = 0.  The epilogue runs for live lanes only -- several lanes would otherwise apply the momentum update to
//     that last pixel.
// The map update is applied whatever the loss turns out to be: the thread cannot know the launch's loss.
//
// NOT here, and why:
//   * several steps in one launch.  The table's gradient is a sum over all pixels of an item; a second step would need it
//     reduced and applied between the steps -- a grid barrier, which this project does not build (svbrdf_photo_fit.hip,
//     the section on several steps);
//   * a head (9-channel) variant: PhotoFit fits maps;
//   * the Adam update of the [B,S,9] table and of the gains: a few hundred floats whose parameterisation is the user's
//     (tools/fit_photos.py fits log e, with a learning rate of its own).  A stock torch.optim on them is one or two tiny
//     launches; this kernel's job is everything that is H W-sized.
#include "svbrdf_photo_fit_pose_device.h"

namespace {

#define SVBRDF_JOINT_KERNEL(NAME, WEIGHTED)                                                                           \
    __global__ SVBRDF_PHOTO_LOSS_ATTRS void NAME(float *maps, float *exp_avg, float *exp_avg_sq,                      \
                                                 const float *__restrict__ photos, const float *__restrict__ weights, \
                                                 int weight_planes, const float *__restrict__ scenes,                 \
                                                 const float *__restrict__ xrow, float eps, float inv_count,          \
                                                 double loss_scale, float fixed_scale, double grad_scale,             \
                                                 float per_count, const AdamArgs adam, float *grad_out,               \
                                                 float *__restrict__ grad_scenes, unsigned long long *__restrict__ ws, \
                                                 float *__restrict__ loss_out, int S, int H, int W)                   \
    {                                                                                                                 \
        joint_body<WEIGHTED>(maps, exp_avg, exp_avg_sq, photos, weights, weight_planes, scenes, xrow, eps, inv_count, \
                             loss_scale, fixed_scale, grad_scale, per_count, adam, grad_out, grad_scenes, ws,         \
                             loss_out, S, H, W);                                                                      \
    }
// (names that hold none of the substrings the other photo and fit kernels are counted by)
SVBRDF_JOINT_KERNEL(k_joint_fit, false)
SVBRDF_JOINT_KERNEL(k_joint_fit_weighted, true)
#undef SVBRDF_JOINT_KERNEL

}  // namespace

extern "C" {

int svbrdf_photo_fit_adam_step_scene_grad(float *maps, float *exp_avg, float *exp_avg_sq, const float *photos,
                                          const float *weights, int weight_planes, const float *scenes, const float *xrow,
                                          float eps, const float *bounds_host, float lr, float beta1, float beta2,
                                          float adam_eps, int step, float *loss_out, float *grad_out, float *grad_scenes,
                                          void *workspace, size_t workspace_bytes, int B, int S, int H, int W, void *stream)
{
    const char *who = "photo_fit_adam_step_scene_grad";
    LossPlan p;
    double units;       // N 2^24
    // the scene-gradient entry's checks in its order (grad_out may be null and the kernels are forward + adjoint whatever
    // it is: the plan is the one with a gradient), then the fit entry's (adam_args)
    if (int e = plan_sums(who, {maps, exp_avg, exp_avg_sq, photos, grad_scenes, scenes, xrow, loss_out}, weights,
                          weight_planes, nullptr, eps, grad_out ? grad_out : maps, workspace, workspace_bytes, 9, kPoseSpill,
                          B, S, H, W, &p, &units)) return e;
    // fit_stash's six words per thread stand beside the rows of sums: the workgroup's LDS stays inside what plan_sums
    // allows the scene-gradient kernels (60 KB of rows), S <= 383
    if (p.lds_bytes + 6 * kLossThreads * sizeof(float) > 60 * 1024)
        return fail_as(who, SVBRDF_ERR_DIMS, "too many scenes per item for the LDS sums (max 383)");
    AdamArgs a;
    if (int e = adam_args(who, kStepRule, bounds_host, lr, beta1, beta2, adam_eps, step, &a)) return e;
    hipLaunchKernelGGL(weights ? k_joint_fit_weighted : k_joint_fit, p.grid, dim3(kLossThreads), p.lds_bytes,
                       static_cast<hipStream_t>(stream), maps, exp_avg, exp_avg_sq, photos, weights, weight_planes, scenes,
                       xrow, eps, p.inv_count, p.loss_scale, p.fixed_scale, 1.0 / units, (float)units, a, grad_out,
                       grad_scenes, p.ws, loss_out, S, H, W);
    return launch_status(who);
}

}  // extern "C"
