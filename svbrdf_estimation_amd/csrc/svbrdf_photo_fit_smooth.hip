// svbrdf_photo_fit_smooth.hip -- translation unit of libsvbrdf_hip.so: one step of a fit of SVBRDF maps to photographs
// with a SMOOTHNESS PRIOR ACROSS PIXELS -- the photo loss, its gradient, the gradient of an anisotropic total-variation term
// on the maps, and the Adam update of the maps -- in the one launch, with or without the gradient towards the scene table
// (added to ABI version 8 without a bump).
//
// Every other fit of this library is pixel-local: a pixel no photograph sees (weight 0 in all of them) has an all-zero
// gradient and never moves, and roughness and specular are observed only where a highlight passes.  The objective here is
//
//   photo loss + R(x),   R(x) = sum_ch lambda[ch] / (B H W) sum_b ( sum |x[b,ch,i,j+1] - x[b,ch,i,j]| + sum |x[b,ch,i+1,j] - x[b,ch,i,j]| )
//
// without wrap-around and without coupling between items.  Per element, behind the scene loop, with g the photo gradient
// exactly as the twins hold it:
//
//   s(a, b) = +1 if a > b, -1 if a < b, 0 if a == b, NaN if unordered       compares of the stored values, no subtraction
//   k       = s(x, left) + s(x, right) + s(x, up) + s(x, down)              a neighbour outside the patch contributes 0
//   g'      = g + (c[ch] (float)k)                                          two individually rounded float32 operations
//   c[ch]   = (float)((double)lambda[ch] / ((double)B H W))                 on the host, rounded once
//
// and g' goes through the fit unit's adam_channel unchanged.  Two EQUAL infinite neighbours therefore give 0 where
// torch.sign(inf - inf) gives NaN.  A channel with lambda == 0 skips the term: it reads no neighbour and g' = g, bit for
// bit (g + 0 would turn a -0 into +0); all-zero lambda is the twins' step.  A NaN neighbour makes the term of that channel
// NaN: the NaN spreads by one pixel per step in the channels that have a lambda.
//
// OUT OF PLACE for the maps: the neighbours must be read as they were before the update, and other workgroups own them.
// `maps_in` is only read, `maps_out` only written, and the two must not overlap; the moments are element-wise and stay in
// place.  loss_out is the photo term alone (R is never reduced on the device); grad_out, if given, is g'.
//
// Four kernels: the flow of fit_body (svbrdf_photo_fit.hip) and of joint_body (svbrdf_photo_fit_pose.hip), unweighted and
// weighted, both from svbrdf_photo_fit_pose_device.h and called with this unit's update in the place of
// adam_epilogue.  What is written out here is that update alone (smooth_epilogue, the one copy):
//   * the neighbours come from LOADS, not from cross-lane moves: four clamped offsets per pixel (pix -+ 1 inside the row,
//     pix -+ W inside the item; an absent neighbour loads the pixel itself and is masked), and up to 48 buffer loads on the
//     resource the pixel's own loads used.  Horizontal neighbours are the adjacent lanes' own words, in cache lines the
//     wave has just read; a cross-lane move would serve the inner lanes only when a row is as long as a wave, needs the
//     loads anyway at the wave's two ends and wherever a row ends inside the wave, and in the joint flow the lanes without
//     a pixel hold the item's last pixel, not their neighbour's.  The result is exact either way;
//   * six channels at a time, the loads of every enabled channel are issued first, back to back behind wave-uniform
//     branches on c[ch] != 0, then k and g' per channel; then the twins' sequence: the 24 state loads back to back,
//     adam_channel per channel, 36 stores -- the maps' to maps_out;
//   * what the update alone needs (where it stores, H, W, AdamArgs, c[12]) rides in the argument block and waits in LDS
//     across the scene loop (step_put / step_take): the loops have no scalar registers to spare for it.
// NOT here: several steps in one launch (the second step needs the neighbours' UPDATED values: a grid barrier, which this
// project does not build), a head form, isotropic or Huber variants, R reduced on the device.
#include "svbrdf_photo_fit_pose_device.h"

namespace {

// c[ch], by value in the kernel-argument block (scalar loads, wave-uniform)
struct SmoothArgs {
    float c[12];
};

// What the update alone needs, all of it wave-uniform: where it stores, the patch's size, AdamArgs and c[12].  It WAITS IN LDS
// across the scene loop, 54 words per wave.  Held in scalar registers from the argument block to the update it costs the
// loop registers it does not have -- c[] alone 12: the weighted kernels then spill vector registers to scratch memory, and
// the others keep a dead spill slot for which every launch would set scratch memory up.  Every lane of a wave puts the same
// values in front of the loop and takes them behind it -- the wave's own words, in program order: no barrier -- and
// readfirstlane makes them scalars again: the branches on c[ch] != 0 stay wave-uniform.  The index goes through an empty
// asm the compiler cannot see through (fit_stash: it would otherwise forward the stored registers and keep them).
struct StepArgs {
    float *maps_out, *exp_avg, *exp_avg_sq, *grad_out;
    int H, W;
    AdamArgs adam;
    SmoothArgs smooth;
    int unused;     // (no padding: the struct is copied word by word)
};
constexpr int kStepWords = sizeof(StepArgs) / sizeof(float);
struct StepWords {
    float w[kStepWords];
};
static_assert(sizeof(StepWords) == sizeof(StepArgs) && sizeof(StepArgs) == 4 * 8 + 2 * 4 + sizeof(AdamArgs) + 12 * 4 + 4, "no padding");
__device__ __forceinline__ float *step_words()
{
    __shared__ float words[kLossThreads / 64][kStepWords];
    return words[0];
}
__device__ __forceinline__ void step_put(const StepArgs &args)
{
    float *words = step_words() + (threadIdx.x >> 6) * kStepWords;
    const StepWords a = __builtin_bit_cast(StepWords, args);
#pragma unroll
    for (int k = 0; k < kStepWords; ++k) words[k] = a.w[k];
}
__device__ __forceinline__ StepArgs step_take()
{
    int at = (int)(threadIdx.x >> 6) * kStepWords;
    asm volatile("" : "+v"(at));
    const float *words = step_words() + at;
    StepWords a;
#pragma unroll
    for (int k = 0; k < kStepWords; ++k)
        a.w[k] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, words[k])));
    return __builtin_bit_cast(StepArgs, a);
}

// Where a pixel's four neighbours stand: left, right, up, down -- pix -+ 1 inside the row, pix -+ W inside the item.  An absent
// neighbour loads the pixel itself (inside the item's plane, every one) and is masked.
struct Neighbours {
    PlaneBuf l, r, u, d;
    bool has_l, has_r, has_u, has_d;
};

// The prior's term of the channels FIRST .. FIRST + kSmoothGroup - 1, added to their gradients: the loads of the group's
// enabled channels back to back, then k of the header and g' of each.
constexpr int kSmoothGroup = 6;
template <int FIRST>
__device__ __forceinline__ void smooth_group(const Neighbours &nb, const SmoothArgs &smooth, const float (&x)[12], float (&g)[12])
{
    float c[kSmoothGroup];
#pragma unroll
    for (int i = 0; i < kSmoothGroup; ++i) c[i] = smooth.c[FIRST + i];
    float nl[kSmoothGroup], nr[kSmoothGroup], nu[kSmoothGroup], nd[kSmoothGroup];
#pragma unroll
    for (int i = 0; i < kSmoothGroup; ++i) {
        if (c[i] != 0.0f) {
            nl[i] = plane_load(nb.l, FIRST + i);
            nr[i] = plane_load(nb.r, FIRST + i);
            nu[i] = plane_load(nb.u, FIRST + i);
            nd[i] = plane_load(nb.d, FIRST + i);
        }
    }
#pragma unroll
    for (int i = 0; i < kSmoothGroup; ++i) {
        if (c[i] != 0.0f) {
            // compares of the stored values, counted in an integer
            const float xk = x[FIRST + i];
            const int n = (((int)(nb.has_l & (xk > nl[i])) - (int)(nb.has_l & (xk < nl[i])))
                           + ((int)(nb.has_r & (xk > nr[i])) - (int)(nb.has_r & (xk < nr[i]))))
                          + (((int)(nb.has_u & (xk > nu[i])) - (int)(nb.has_u & (xk < nu[i])))
                             + ((int)(nb.has_d & (xk > nd[i])) - (int)(nb.has_d & (xk < nd[i]))));
            const bool unordered = (nb.has_l & __builtin_isunordered(xk, nl[i])) | (nb.has_r & __builtin_isunordered(xk, nr[i]))
                                   | (nb.has_u & __builtin_isunordered(xk, nu[i])) | (nb.has_d & __builtin_isunordered(xk, nd[i]));
            g[FIRST + i] = g[FIRST + i] + (c[i] * (unordered ? __builtin_nanf("") : (float)n));
        }
    }
}

// The update of the pixel `pix` = (row, col) of item b behind the scene loop: adam_epilogue's with the prior's term added to
// the gradient in front of it, the neighbours read from `maps_in`, the new maps stored to `maps_out`.
__device__ __forceinline__ void smooth_epilogue(const float *maps_in, float *maps_out, float *exp_avg, float *exp_avg_sq,
                                                float *grad_out, int b, size_t plane, size_t pix, int row, int col, int H, int W,
                                                const PixelSetup &ps, const AdamArgs &adam, const SmoothArgs &smooth)
{
    // everything from the lane's byte offset, the one value of the pixel's index that the scene loop keeps in a register
    Neighbours nb;
    const PlaneBuf own = plane_buf(maps_in + (size_t)b * 12 * plane, 12, plane, pix);
    nb.has_l = col > 0, nb.has_r = col + 1 < W, nb.has_u = row > 0, nb.has_d = row + 1 < H;
    nb.l = nb.r = nb.u = nb.d = own;
    nb.l.lane_bytes = nb.has_l ? own.lane_bytes - 4u : own.lane_bytes;
    nb.r.lane_bytes = nb.has_r ? own.lane_bytes + 4u : own.lane_bytes;
    nb.u.lane_bytes = nb.has_u ? own.lane_bytes - (unsigned)W * 4u : own.lane_bytes;
    nb.d.lane_bytes = nb.has_d ? own.lane_bytes + (unsigned)W * 4u : own.lane_bytes;
    float x[12], g[12];
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
    smooth_group<0>(nb, smooth, x, g);
    smooth_group<kSmoothGroup>(nb, smooth, x, g);
    static_assert(2 * kSmoothGroup == 12, "two groups cover the 12 channels");
    const PlaneBuf xb = plane_buf(maps_out + (size_t)b * 12 * plane, 12, plane, pix);
    const PlaneBuf mb = plane_buf(exp_avg + (size_t)b * 12 * plane, 12, plane, pix);
    const PlaneBuf vb = plane_buf(exp_avg_sq + (size_t)b * 12 * plane, 12, plane, pix);
    if (grad_out) {
        const PlaneBuf gb = plane_buf(grad_out + (size_t)b * 12 * plane, 12, plane, pix);
#pragma unroll
        for (int k = 0; k < 12; ++k) plane_store(gb, k, g[k]);
    }
    float m[12], v[12];
    __builtin_amdgcn_sched_barrier(0);      // the 24 state loads back to back, as adam_epilogue's
#pragma unroll
    for (int k = 0; k < 12; ++k) m[k] = plane_load(mb, k);
#pragma unroll
    for (int k = 0; k < 12; ++k) v[k] = plane_load(vb, k);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const float xn = adam_channel(adam, k, x[k], g[k], m[k], v[k]);
        plane_store(xb, k, xn);
        plane_store(mb, k, m[k]);
        plane_store(vb, k, v[k]);
    }
}

// fit_body's and joint_body's `update`: the arguments back from LDS, the pixel's row and column, then smooth_epilogue
struct UpdateSmooth {
    static constexpr bool in_place = false;
    const float *maps_in;
    __device__ __forceinline__ void operator()(int b, size_t plane, size_t pix, const PixelSetup &ps) const
    {
        const StepArgs a = step_take();
        const unsigned bytes = (unsigned)pix * 4u, row_bytes = (unsigned)a.W * 4u;       // (H W <= 2^25)
        const unsigned row = bytes / row_bytes;
        const unsigned col = (bytes - row * row_bytes) >> 2;
        smooth_epilogue(maps_in, a.maps_out, a.exp_avg, a.exp_avg_sq, a.grad_out, b, plane, pix, (int)row, (int)col, a.H, a.W,
                        ps, a.adam, a.smooth);
    }
};

// (the bodies take a `float *maps` because their own update writes it; with UpdateSmooth they only read it)
#define SVBRDF_SMOOTH_FIT_KERNEL(NAME, WEIGHTED)                                                                      \
    __global__ SVBRDF_PHOTO_LOSS_ATTRS void NAME(const float *maps_in, float *maps_out, float *exp_avg,               \
                                                 float *exp_avg_sq, const float *__restrict__ photos,                 \
                                                 const float *__restrict__ weights, int weight_planes,                \
                                                 const float *__restrict__ scenes, const float *__restrict__ xrow,    \
                                                 float eps, float inv_count, double loss_scale, float fixed_scale,    \
                                                 const AdamArgs adam, const SmoothArgs smooth, float *grad_out,       \
                                                 unsigned long long *__restrict__ ws, float *__restrict__ loss_out,   \
                                                 int S, int H, int W)                                                 \
    {                                                                                                                 \
        step_put(StepArgs{maps_out, exp_avg, exp_avg_sq, grad_out, H, W, adam, smooth, 0});                           \
        const UpdateSmooth update{maps_in};                                                                           \
        fit_body<WEIGHTED>(const_cast<float *>(maps_in), exp_avg, exp_avg_sq, photos, weights, weight_planes, scenes, \
                           xrow, eps, inv_count, loss_scale, fixed_scale, adam, grad_out, ws, loss_out, S, H, W,      \
                           update);                                                                                   \
    }
#define SVBRDF_SMOOTH_JOINT_KERNEL(NAME, WEIGHTED)                                                                    \
    __global__ SVBRDF_PHOTO_LOSS_ATTRS void NAME(const float *maps_in, float *maps_out, float *exp_avg,               \
                                                 float *exp_avg_sq, const float *__restrict__ photos,                 \
                                                 const float *__restrict__ weights, int weight_planes,                \
                                                 const float *__restrict__ scenes, const float *__restrict__ xrow,    \
                                                 float eps, float inv_count, double loss_scale, float fixed_scale,    \
                                                 double grad_scale, float per_count, const AdamArgs adam,             \
                                                 const SmoothArgs smooth, float *grad_out,                            \
                                                 float *__restrict__ grad_scenes, unsigned long long *__restrict__ ws, \
                                                 float *__restrict__ loss_out, int S, int H, int W)                   \
    {                                                                                                                 \
        step_put(StepArgs{maps_out, exp_avg, exp_avg_sq, grad_out, H, W, adam, smooth, 0});                           \
        const UpdateSmooth update{maps_in};                                                                           \
        joint_body<WEIGHTED>(const_cast<float *>(maps_in), exp_avg, exp_avg_sq, photos, weights, weight_planes,       \
                             scenes, xrow, eps, inv_count, loss_scale, fixed_scale, grad_scale, per_count, adam,      \
                             grad_out, grad_scenes, ws, loss_out, S, H, W, update);                                   \
    }
// (names that hold none of the substrings the other photo and fit kernels are counted by)
SVBRDF_SMOOTH_FIT_KERNEL(k_smooth_step, false)
SVBRDF_SMOOTH_FIT_KERNEL(k_smooth_step_weighted, true)
SVBRDF_SMOOTH_JOINT_KERNEL(k_smooth_joint, false)
SVBRDF_SMOOTH_JOINT_KERNEL(k_smooth_joint_weighted, true)
#undef SVBRDF_SMOOTH_FIT_KERNEL
#undef SVBRDF_SMOOTH_JOINT_KERNEL

// What the two entries check in front of their twins' checks, and c[ch] -> 0, or the error reported
int smooth_args(const char *who, const float *smooth_host, const float *maps_in, const float *maps_out, int B, int H, int W,
                SmoothArgs *s)
{
    if (!smooth_host) return fail_as(who, SVBRDF_ERR_DIMS, "smooth_host (12 floats on the host) is required");
    for (int k = 0; k < 12; ++k)
        if (!(smooth_host[k] >= 0.0f) || !std::isfinite(smooth_host[k]))
            return fail_as(who, SVBRDF_ERR_DIMS, "smooth_host must hold 12 finite values >= 0");
    if (maps_in && maps_out && B > 0 && H > 0 && W > 0) {
        const unsigned __int128 bytes = (unsigned __int128)B * 12u * (unsigned)H * (unsigned)W * sizeof(float);
        const unsigned long long a = (unsigned long long)(uintptr_t)maps_in, o = (unsigned long long)(uintptr_t)maps_out;
        if ((a > o ? a - o : o - a) < bytes)
            return fail_as(who, SVBRDF_ERR_DIMS, "maps_in and maps_out must not overlap (the step is out of place)");
    }
    const double count = (double)B * (double)H * (double)W;
    for (int k = 0; k < 12; ++k) s->c[k] = count > 0.0 ? (float)((double)smooth_host[k] / count) : 0.0f;
    return 0;
}

}  // namespace

extern "C" {

int svbrdf_photo_fit_smooth_adam_step(const float *maps_in, float *maps_out, float *exp_avg, float *exp_avg_sq,
                                      const float *photos, const float *weights, int weight_planes, const float *scenes,
                                      const float *xrow, float eps, const float *smooth_host, const float *bounds_host,
                                      float lr, float beta1, float beta2, float adam_eps, int step, float *loss_out,
                                      float *grad_out, void *workspace, size_t workspace_bytes, int B, int S, int H, int W,
                                      void *stream)
{
    const char *who = "photo_fit_smooth_adam_step";
    SmoothArgs sm;
    if (int e = smooth_args(who, smooth_host, maps_in, maps_out, B, H, W, &sm)) return e;
    LossPlan p;
    // svbrdf_photo_fit_adam_step's checks in its order
    if (int e = plan_loss(who, false, {maps_in, maps_out, exp_avg, exp_avg_sq, photos, scenes, xrow, loss_out},
                          grad_out ? grad_out : maps_in, workspace, workspace_bytes, "eps", eps, 0.0f, B, S, H, W, &p)) return e;
    if (int e = weights_check(who, weights, weight_planes, S)) return e;
    AdamArgs a;
    if (int e = adam_args(who, kStepRule, bounds_host, lr, beta1, beta2, adam_eps, step, &a)) return e;
    hipLaunchKernelGGL(weights ? k_smooth_step_weighted : k_smooth_step, p.grid, dim3(kLossThreads), 0,
                       static_cast<hipStream_t>(stream), maps_in, maps_out, exp_avg, exp_avg_sq, photos, weights,
                       weight_planes, scenes, xrow, eps, p.inv_count, p.loss_scale, p.fixed_scale, a, sm, grad_out, p.ws,
                       loss_out, S, H, W);
    return launch_status(who);
}

int svbrdf_photo_fit_smooth_adam_step_scene_grad(const float *maps_in, float *maps_out, float *exp_avg, float *exp_avg_sq,
                                                 const float *photos, const float *weights, int weight_planes,
                                                 const float *scenes, const float *xrow, float eps,
                                                 const float *smooth_host, const float *bounds_host, float lr, float beta1,
                                                 float beta2, float adam_eps, int step, float *loss_out, float *grad_out,
                                                 float *grad_scenes, void *workspace, size_t workspace_bytes, int B, int S,
                                                 int H, int W, void *stream)
{
    const char *who = "photo_fit_smooth_adam_step_scene_grad";
    SmoothArgs sm;
    if (int e = smooth_args(who, smooth_host, maps_in, maps_out, B, H, W, &sm)) return e;
    LossPlan p;
    double units;       // N 2^24
    // svbrdf_photo_fit_adam_step_scene_grad's checks in its order
    if (int e = plan_sums(who, {maps_in, maps_out, exp_avg, exp_avg_sq, photos, grad_scenes, scenes, xrow, loss_out}, weights,
                          weight_planes, nullptr, eps, grad_out ? grad_out : maps_in, workspace, workspace_bytes, 9,
                          kPoseSpill, B, S, H, W, &p, &units)) return e;
    if (p.lds_bytes + 6 * kLossThreads * sizeof(float) > 60 * 1024)
        return fail_as(who, SVBRDF_ERR_DIMS, "too many scenes per item for the LDS sums (max 383)");
    AdamArgs a;
    if (int e = adam_args(who, kStepRule, bounds_host, lr, beta1, beta2, adam_eps, step, &a)) return e;
    hipLaunchKernelGGL(weights ? k_smooth_joint_weighted : k_smooth_joint, p.grid, dim3(kLossThreads), p.lds_bytes,
                       static_cast<hipStream_t>(stream), maps_in, maps_out, exp_avg, exp_avg_sq, photos, weights,
                       weight_planes, scenes, xrow, eps, p.inv_count, p.loss_scale, p.fixed_scale, 1.0 / units, (float)units,
                       a, sm, grad_out, grad_scenes, p.ws, loss_out, S, H, W);
    return launch_status(who);
}

}  // extern "C"
