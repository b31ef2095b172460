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
// svbrdf_photo_loss.hip's, from the device functions of svbrdf_photo_loss_device.h: the set-up of a pixel
// (wave_pixel_setup), the scene loop (photo_scene_loop, tied / three-lobe chosen per wave as k_photo_loss / k_wphoto
// choose it), the loss reduction (loss_arrive, same 65-word scratch).  The loss and the gradient are therefore bit for bit
// those of svbrdf_photo_loss[_weighted]_fwd_bwd: the same statements, and float arithmetic without contraction does not
// depend on how the compiler schedules it.  What differs:
//   * the diffuse and roughness planes of the pixel as stored (the set-up keeps only what it derives from them; normal and
//     specular survive in MapK as loaded) wait in LDS across the scene loop: the loop has no six registers to spare;
//   * behind the loop, when the shading temporaries are dead (adam_epilogue, the one copy: the joint step of
//     svbrdf_photo_fit_pose.hip calls it too): the 24 state loads back to back, the five lines above per channel -- every
//     operation an individually rounded float32 one (this unit is built with -ffp-contract=off and the lines hold no
//     fma), IEEE division and square root -- and 36 stores with the gradient stores' cache policy;
//   * the clamp is two compares and selects: a NaN stays a NaN (v_max / v_min would return the bound), +-inf bounds never
//     select.
// The three fit entries -- this unit's two and the joint unit's -- check their weights and turn (bounds, lr, betas, adam_eps,
// step) into AdamArgs through one helper each (weights_check of svbrdf_photo_loss_device.h, adam_args) and report through
// fail_as.  The update, the step's body and adam_args are in svbrdf_photo_fit_device.h, which the joint and the smooth units
// include too; this file holds the kernels of the single step and of several steps, and their entry points.
#include "svbrdf_photo_fit_device.h"

namespace {

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

// ---- Several steps in one launch (svbrdf_photo_fit_adam_steps).  The fit is pixel-local -- a pixel's loss term reads its
// own 12 map values, Adam is element-wise, the loss sum is reported and never fed back -- so the thread that owns a pixel
// runs n consecutive steps on it and no workgroup ever waits for another: no grid barrier, no spinning, no cooperative
// launch.  Maps and state are read from memory once, in front of the first step, and stored once, behind the last.  The
// photographs and weights of the workgroup's 256 pixels are read again in every step ((3 S + P) KB, from L2 after the
// first).  Results EQUAL BIT FOR BIT n launches of k_fit_maps*: the same statements on the same values. ----

// the two scalars of a step that depend on t, one pair per step of the launch, by value in the argument block
struct RunScalars {
    float step_size[SVBRDF_PHOTO_FIT_MAX_STEPS], rsb2[SVBRDF_PHOTO_FIT_MAX_STEPS];
};

// Where a pixel's 36 values of maps and state wait between the steps and across the scene loop (which has no register to
// spare): [k][thread] words of LDS as fit_stash's, no bank conflicts and nobody else's words touched -- no barrier guards
// them.  k = 0..11 the maps, 12..23 exp_avg, 24..35 exp_avg_sq, 36 the pixel's x coordinate as loaded (the guard against
// non-finite maps is added to it anew in every step).  37 KB: four workgroups fit a compute unit's 160 KB.
constexpr int kRunWords = 37;
__device__ __forceinline__ float *run_words()
{
    __shared__ float words[kRunWords * kLossThreads];
    return words;
}
// The thread's index behind an empty asm the compiler cannot see through: a word read through it is LOADED there, where the
// compiler would otherwise forward the registers stored or loaded earlier and keep them across the scene loop (fit_stash).
// One per group of accesses: the words' offsets stay immediates of the LDS instructions.
__device__ __forceinline__ int run_lane()
{
    int t = (int)threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}
__device__ __forceinline__ void run_put(int k, int lane, float v) { run_words()[k * kLossThreads + lane] = v; }
__device__ __forceinline__ float run_take(int k, int lane) { return run_words()[k * kLossThreads + lane]; }

// One thread = one pixel, all S renders of it, n_steps times; workgroup = 256 pixels of one item.  Step k reduces its loss
// through loss_arrive on its own 65 words ws + 65 k into losses_out + k: workgroups are in different steps at the same
// moment.
template <bool WEIGHTED>
__device__ __forceinline__ void fit_run_body(float *maps, float *exp_avg, float *exp_avg_sq, const float *__restrict__ photos,
                                             const float *__restrict__ weights, int weight_planes,
                                             const float *__restrict__ scenes, const float *__restrict__ xrow, float eps,
                                             float inv_count, double loss_scale, float fixed_scale, const AdamArgs &adam,
                                             const RunScalars &steps, int n_steps, unsigned long long *__restrict__ ws,
                                             float *__restrict__ losses_out, int S, int H, int W)
{
    // The waves' partial sums of a step: TWO SETS of words, alternating from step to step, and one barrier per step.  A wave
    // that is a step ahead of lane 0 writes the other set; none gets two steps ahead of lane 0's read of a set, because the
    // barrier of the step between them needs lane 0's wave, which reads (and waits for what it read) in front of it.
    __shared__ float wave_part[2][kLossThreads / 64];
    const size_t plane = (size_t)H * W;
    const size_t pix = (size_t)blockIdx.x * kLossThreads + threadIdx.x;
    const int b = blockIdx.y;
    const bool active = pix < plane;
    float y = 0.0f;
    if (active) {
        const PlaneBuf xb = plane_buf(maps + (size_t)b * 12 * plane, 12, plane, pix);
        const PlaneBuf mb = plane_buf(exp_avg + (size_t)b * 12 * plane, 12, plane, pix);
        const PlaneBuf vb = plane_buf(exp_avg_sq + (size_t)b * 12 * plane, 12, plane, pix);
        const int first = run_lane();
#pragma unroll
        for (int k = 0; k < 12; ++k) run_put(k, first, plane_load(xb, k));
#pragma unroll
        for (int k = 0; k < 12; ++k) run_put(12 + k, first, plane_load(mb, k));
#pragma unroll
        for (int k = 0; k < 12; ++k) run_put(24 + k, first, plane_load(vb, k));
        float x;
        pixel_xy(xrow, pix, W, (W & (W - 1)) == 0, x, y);
        run_put(36, first, x);
    }
#pragma clang loop unroll(disable)
    for (int step = 0; step < n_steps; ++step) {
        float lsum = 0.0f;
        if (active) {
            // the set-up of the pixel from the values as they are now: wave_pixel_setup<false, WEIGHTED>'s statements behind
            // its loads
            Maps in;
            Grad acc;
            float poison = 0.0f;
            const int top = run_lane();
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                in.n[k] = run_take(0 + k, top);
                in.d[k] = run_take(3 + k, top);
                in.r[k] = run_take(6 + k, top);
                in.s[k] = run_take(9 + k, top);
            }
            zero_grad(acc);
            const bool tied = tied_roughness(in);
            MapK mi = prepare<true>(in);
            // dA/dr_hat is used behind the scene loop only (DEFER_R: acc.r *= r4m), and the weighted loops have no three
            // registers to carry it: the loop multiplies by exactly 1 -- the identity, bit for bit -- and the factor is
            // formed behind it, from the roughness that is loaded again there for the update, and applied there
#pragma unroll
            for (int k = 0; k < 3; ++k) mi.r4m[k] = 1.0f;
            float x = run_take(36, top);
            maps_guard<WEIGHTED>(in, x, poison);
            // The scene table through the CONSTANT address space -- no kernel writes it -- so that its wave-uniform loads are
            // scalar loads whatever stands around them.  Through the global one the compiler must first prove that nothing in
            // front of a load clobbers it; with the step loop around the scene loops it gives up, loads the rows of every pass
            // into vector registers, and the loops spill.  (By way of an integer: the compiler drops a plain pair of casts.)
            typedef const float __attribute__((address_space(4))) *ConstTable;
            const float *__restrict__ scp = (const float *)(ConstTable)(unsigned long long)(scenes + (size_t)b * S * 9);
            const float *__restrict__ pp = photos + (size_t)b * S * 3 * plane;
            const float *__restrict__ wp = WEIGHTED ? weights + (size_t)b * weight_planes * plane : nullptr;
            const size_t wstride = weight_planes == 1 ? 0 : plane;
            // per wave AND per step: roughness that starts tied is untied by the first update when the state differs
            // between its three channels
            if (__all(tied))
                lsum = photo_scene_loop<1, true, 7, WEIGHTED>(mi, x, y, scp, nullptr, pp, plane, pix, S, eps, inv_count, acc,
                                                              wp, wstride, poison);
            else
                lsum = photo_scene_loop<3, true, 3, WEIGHTED>(mi, x, y, scp, nullptr, pp, plane, pix, S, eps, inv_count, acc,
                                                              wp, wstride, poison);
            AdamArgs a = adam;
            a.step_size = steps.step_size[step];
            a.rsb2 = steps.rsb2[step];
            const int back = run_lane();        // behind the loop: diffuse, roughness and the state are loaded again
            float xv[12], g[12];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                xv[0 + k] = mi.n[k];
                xv[3 + k] = run_take(3 + k, back);
                xv[6 + k] = run_take(6 + k, back);
                xv[9 + k] = mi.s[k];
                g[0 + k] = acc.n[k];
                g[3 + k] = acc.d[k];
                // prepare()'s r4m: 4 r^3 where r_hat >= kMinRough (and there max(r_hat, kMinRough) is r_hat itself), else 0
                const float rh = xv[6 + k];
                g[6 + k] = acc.r[k] * ((rh >= kMinRough) ? 4.0f * ((rh * rh) * rh) : 0.0f);
                g[9 + k] = acc.s[k];
            }
#pragma unroll
            for (int k = 0; k < 12; ++k) {
                float m = run_take(12 + k, back), v = run_take(24 + k, back);
                run_put(k, back, adam_channel(a, k, xv[k], g[k], m, v));
                run_put(12 + k, back, m);
                run_put(24 + k, back, v);
            }
        }
        lsum = wave_sum(lsum);
        if ((threadIdx.x & 63) == 0) wave_part[step & 1][threadIdx.x >> 6] = lsum;
        __syncthreads();
        if (threadIdx.x == 0) {
            float t = 0.0f;
#pragma unroll
            for (int w = 0; w < kLossThreads / 64; ++w) t += wave_part[step & 1][w];
            loss_arrive(t, fixed_scale, loss_scale, ws + (size_t)step * (kLossSlots + 1), losses_out + step);
        }
    }
    // the 36 values leave once, with the single step's store policy
    if (active) {
        const PlaneBuf xb = plane_buf(maps + (size_t)b * 12 * plane, 12, plane, pix);
        const PlaneBuf mb = plane_buf(exp_avg + (size_t)b * 12 * plane, 12, plane, pix);
        const PlaneBuf vb = plane_buf(exp_avg_sq + (size_t)b * 12 * plane, 12, plane, pix);
        const int last = run_lane();
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            plane_store(xb, k, run_take(k, last));
            plane_store(mb, k, run_take(12 + k, last));
            plane_store(vb, k, run_take(24 + k, last));
        }
    }
}

#define SVBRDF_FIT_RUN_KERNEL(NAME, WEIGHTED)                                                                         \
    __global__ SVBRDF_PHOTO_LOSS_ATTRS void NAME(float *maps, float *exp_avg, float *exp_avg_sq,                      \
                                                 const float *__restrict__ photos, const float *__restrict__ weights, \
                                                 int weight_planes, const float *__restrict__ scenes,                 \
                                                 const float *__restrict__ xrow, float eps, float inv_count,          \
                                                 double loss_scale, float fixed_scale, const AdamArgs adam,           \
                                                 const RunScalars steps, int n_steps,                                 \
                                                 unsigned long long *__restrict__ ws, float *__restrict__ losses_out, \
                                                 int S, int H, int W)                                                 \
    {                                                                                                                 \
        fit_run_body<WEIGHTED>(maps, exp_avg, exp_avg_sq, photos, weights, weight_planes, scenes, xrow, eps,          \
                               inv_count, loss_scale, fixed_scale, adam, steps, n_steps, ws, losses_out, S, H, W);    \
    }
// (names that hold none of the substrings the other fit and photo kernels are counted by)
SVBRDF_FIT_RUN_KERNEL(k_fit_run, false)
SVBRDF_FIT_RUN_KERNEL(k_fit_run_weighted, true)
#undef SVBRDF_FIT_RUN_KERNEL

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
    LossPlan p;
    // (grad_out may be null and the kernels are forward + adjoint whatever it is: the plan is the one with a gradient)
    if (int e = plan_loss(who, false, {maps, exp_avg, exp_avg_sq, photos, scenes, xrow, loss_out}, grad_out ? grad_out : maps,
                          workspace, workspace_bytes, "eps", eps, 0.0f, B, S, H, W, &p)) return e;
    if (int e = weights_check(who, weights, weight_planes, S)) return e;
    AdamArgs a;
    if (int e = adam_args(who, kStepRule, bounds_host, lr, beta1, beta2, adam_eps, step, &a)) return e;
    hipLaunchKernelGGL(weights ? k_fit_maps_weighted : k_fit_maps, p.grid, dim3(kLossThreads), 0,
                       static_cast<hipStream_t>(stream), maps, exp_avg, exp_avg_sq, photos, weights, weight_planes, scenes,
                       xrow, eps, p.inv_count, p.loss_scale, p.fixed_scale, a, grad_out, p.ws, loss_out, S, H, W);
    return launch_status(who);
}

size_t svbrdf_photo_fit_steps_workspace_bytes(int n_steps, int B, int S, int H, int W)
{
    if (n_steps < 1) return 0;
    return (size_t)n_steps * svbrdf_rendering_loss_workspace_bytes(B, S, H, W);
}

int svbrdf_photo_fit_adam_steps(float *maps, float *exp_avg, float *exp_avg_sq, const float *photos, const float *weights,
                                int weight_planes, const float *scenes, const float *xrow, float eps,
                                const float *bounds_host, float lr, float beta1, float beta2, float adam_eps, int first_step,
                                int n_steps, float *losses_out, void *workspace, size_t workspace_bytes, int B, int S, int H,
                                int W, void *stream)
{
    const char *who = "photo_fit_adam_steps";
    const char *rule = "first_step >= 1, a finite lr >= 0 and betas in [0, 1) are required";
    LossPlan p;
    // the single step's checks in its order (a workspace below ONE step's 65 words fails here already)
    if (int e = plan_loss(who, false, {maps, exp_avg, exp_avg_sq, photos, scenes, xrow, losses_out}, maps, workspace,
                          workspace_bytes, "eps", eps, 0.0f, B, S, H, W, &p)) return e;
    if (int e = weights_check(who, weights, weight_planes, S)) return e;
    if (n_steps < 1 || n_steps > SVBRDF_PHOTO_FIT_MAX_STEPS)
        return fail_as(who, SVBRDF_ERR_DIMS, "n_steps must lie in [1, SVBRDF_PHOTO_FIT_MAX_STEPS]");
    AdamArgs a;
    RunScalars run;
    float sc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int k = 0; k < SVBRDF_PHOTO_FIT_MAX_STEPS; ++k) {
        // (first_step + k cannot wrap where it is used: k < n_steps <= 64, and a first_step that close to INT_MAX is no fit's)
        if (k < n_steps && (first_step > 0x7fffffff - k || !adam_scalars(lr, beta1, beta2, first_step + k, sc)))
            return fail_as(who, SVBRDF_ERR_DIMS, rule);
        run.step_size[k] = sc[2];       // (behind n_steps: the last step's, never read)
        run.rsb2[k] = sc[3];
    }
    // everything that does not depend on t (the scalars of first_step passed above); the kernel takes the two that do from `run`
    if (int e = adam_args(who, rule, bounds_host, lr, beta1, beta2, adam_eps, first_step, &a)) return e;
    a.step_size = 0.0f;
    a.rsb2 = 0.0f;
    if (workspace_bytes < svbrdf_photo_fit_steps_workspace_bytes(n_steps, B, S, H, W))
        return fail_as(who, SVBRDF_ERR_WORKSPACE, "workspace too small for n_steps (svbrdf_photo_fit_steps_workspace_bytes)");
    hipLaunchKernelGGL(weights ? k_fit_run_weighted : k_fit_run, p.grid, dim3(kLossThreads), 0,
                       static_cast<hipStream_t>(stream), maps, exp_avg, exp_avg_sq, photos, weights, weight_planes, scenes,
                       xrow, eps, p.inv_count, p.loss_scale, p.fixed_scale, a, run, n_steps, p.ws, losses_out, S, H, W);
    return launch_status(who);
}

}  // extern "C"
