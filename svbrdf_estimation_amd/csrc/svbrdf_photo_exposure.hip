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
// svbrdf_photo_loss.hip's flow -- its per-render device functions with EXPO set, included below without its kernels,
// launcher and entry points -- plus:
//   * per item and wave: the 3 S gains are checked once, a lane each; one that is NaN, infinite or <= 0 poisons the
//     loss the way a bad weight does;
//   * per render: the gains (wave-uniform loads) scale the colour (expo_scale); q = w sign(delta)
//     (1 - ec / b) per channel from registers the loss already holds (no new transcendental, no division) is summed over
//     the wave and stored, as a fixed-point integer, in the wave's row of the [waves][kExpoSpill + 3 S] LDS sums by one lane (expo_collect);
//   * behind the loop and one barrier, 3 S lanes add the four waves' sums to the B S 3 accumulator words of the workspace
//     (behind loss_arrive's 65) with 64-bit agent-scope returning atomics and wait for their return; then the barrier of
//     the loss reduction; then lane 0 arrives (loss_arrive).  Whoever finishes the launch therefore knows every
//     accumulator complete: each workgroup's adds returned before its arrival was counted.
//   * the finisher's wave 0 (told by readfirstlane of loss_arrive's answer: no LDS word, no third barrier, the other three
//     waves have left) fetches and zeroes every accumulator with 64-bit agent-scope atomic exchanges -- 8-byte agent
//     atomics on both sides of the hand-off, no fence; a plain load could be served by this compute unit's L1 or its
//     die's L2 -- and writes grad_exposure = sum / (2^24 N e), or NaN everywhere when the loss is NaN.
// The chain that ends a launch is three dependent round trips here (accumulator adds, slot + tail, exchanges) against two
// in the kernels without exposure, which keep theirs.  Integer sums from the wave on: bitwise reproducible.
// (The alternative, a per-workgroup slab of sums written with sc1 stores and added up by the finisher, needs
// grid x 3 S words of workspace, more than the 65 + B S 3 words of the C ABI, and a finisher that reads all of them: not
// built, and unmeasured.  What the tail of this variant costs is measured: DESIGN.md section 4.5, round 16.)
// exposure_body repeats photo_loss_body's set-up of a pixel (the loads, the non-finite guards, the coordinates) instead of
// sharing it through an inline function: with the shared function six of the eight head kernels of svbrdf_photo_loss.hip came out
// with other machine code (same size, other bytes), which this unit exists to avoid.  A change to those guards is made in
// both bodies.
#define SVBRDF_PHOTO_SHARED_ONLY
#include "svbrdf_photo_loss.hip"

namespace {

constexpr int kExpoWaves = kLossThreads / 64;

// One thread = one pixel, all S renders of it; workgroup = 256 pixels of one item, as photo_loss_body<true, false, HEAD,
// WEIGHTED>, whose statements these are.  The difference in shape: a wave that holds at least one pixel runs WHOLE -- the
// lanes past the item's last pixel shade that last pixel again, deselected from the loss, the sums and the stores -- so
// that the wave sums of expo_collect never read a disabled lane.
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
    const size_t first = (size_t)blockIdx.x * kLossThreads + (threadIdx.x & ~63u);
    const bool live = first + (threadIdx.x & 63) < plane;
    const size_t pix = live ? first + (threadIdx.x & 63) : plane - 1;
    const bool wave_live = __builtin_amdgcn_readfirstlane((int)(first < plane)) != 0;
    const int b = blockIdx.y;
    const int n_sums = 3 * S;
    float lsum = 0.0f;
    // (no barrier in front of the scene loop: behind one, the wave-uniform loads of the scene rows and the gains would no
    // longer be scalar loads)
    const int row_words = kExpoSpill + n_sums;
    const int row = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * row_words;
    int *wave_sums = q_lds + row + kExpoSpill;
    if (!wave_live) {
        for (int i = threadIdx.x & 63; i < n_sums; i += 64) wave_sums[i] = 0;      // a wave without pixels: its row of zeros
    } else {
        Maps in;
        Grad acc;
        [[maybe_unused]] Head head;
        [[maybe_unused]] float head_chk = 0.0f;
        [[maybe_unused]] float poison = 0.0f;
        if (HEAD) {
            float e[9];
            const PlaneBuf pb = plane_buf(input + (size_t)b * 9 * plane, 9, plane, pix);
#pragma unroll
            for (int k = 0; k < 9; ++k) e[k] = plane_load(pb, k);
            head = decode_head(e, in);
            head_chk = ((e[0] - e[0]) + (e[1] - e[1])) + (e[5] - e[5]);
            if (WEIGHTED)
                poison = (((e[2] - e[2]) + (e[3] - e[3])) + ((e[4] - e[4]) + (e[6] - e[6]))) + ((e[7] - e[7]) + (e[8] - e[8]));
        } else {
            load_maps_k3(input + (size_t)b * 12 * plane, plane, pix, in);
        }
        zero_grad(acc);
        const bool tied = HEAD || tied_roughness(in);
        const MapK mi = prepare<true>(in);
        float x[1], y;
        if ((W & (W - 1)) == 0) {
            const unsigned p32 = (unsigned)pix, sh = (unsigned)__builtin_ctz((unsigned)W);
            x[0] = xrow[p32 & (unsigned)(W - 1)];
            y = -xrow[p32 >> sh];
        } else {
            pixel_coords<1>(xrow, pix, W, x, y);
        }
        if (HEAD) {
            x[0] += head_chk;
            if (WEIGHTED) poison += head_chk;
        } else {
            const float chk = ((in.n[0] + in.n[1]) + (in.n[2] + in.r[0])) + (in.r[1] + in.r[2]);
            x[0] += chk - chk;
            if (WEIGHTED) {
                const float ds = ((in.d[0] + in.d[1]) + (in.d[2] + in.s[0])) + (in.s[1] + in.s[2]);
                poison = (chk - chk) + (ds - ds);
            }
        }
        const float *__restrict__ scp = scenes + (size_t)b * S * 9;
        const float *__restrict__ pp = photos + (size_t)b * S * 3 * plane;
        const float *__restrict__ wp = WEIGHTED ? weights + (size_t)b * weight_planes * plane : nullptr;
        const size_t wstride = weight_planes == 1 ? 0 : plane;
        const ExpoLoop xl{row, live, per_weight};
#pragma unroll
        for (int k = 0; k < 3; ++k) expo_stash(k, mi.r4m[k], false);
        const float *__restrict__ gain = exposure + (size_t)b * n_sums;
        if (HEAD || __builtin_amdgcn_readfirstlane((int)__all(tied)))      // wave-uniform, and known to be
            lsum = photo_scene_loop<1, true, 7, WEIGHTED, true>(mi, x[0], y, scp, nullptr, pp, plane, pix, S, eps, inv_count,
                                                                acc, wp, wstride, poison, &xl, gain);
        else
            lsum = photo_scene_loop<3, true, 3, WEIGHTED, true>(mi, x[0], y, scp, nullptr, pp, plane, pix, S, eps, inv_count,
                                                                acc, wp, wstride, poison, &xl, gain);
        // the item's gains, a lane each: one that is NaN, infinite or <= 0 makes the loss sum NaN, whatever the weights.
        // (Behind the scene loop: in front of it these vector loads keep the loop's own loads of the gains from being
        // scalar loads.)
        for (int i = threadIdx.x & 63; i < n_sums; i += 64) {
            const float e = gain[i];
            if (!(e > 0.0f && e < __builtin_inff())) lsum = __builtin_nanf("");
        }
        if (live) {
            if (HEAD) store_pixel_grad<true>(head, acc, grad_input, b, plane, pix);
            else store_grads_k3(grad_input + (size_t)b * 12 * plane, plane, pix, acc);
        } else {
            lsum -= lsum;       // +0; a NaN stays (expo_collect's poison sits in lane 63, a bad gain's in every lane)
        }
    }
    __shared__ float wave_part[kLossThreads / 64];
    lsum = wave_sum(lsum);
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = lsum;
    __syncthreads();        // the workgroup's sums stand in LDS
    unsigned long long *__restrict__ accum = ws + (kLossSlots + 1);
    for (int i = threadIdx.x; i < n_sums; i += kLossThreads) {
        long long sum = 0;
#pragma unroll
        for (int w = 0; w < kExpoWaves; ++w) sum += q_lds[w * row_words + kExpoSpill + i];
        const unsigned long long old = __hip_atomic_fetch_add(&accum[(size_t)b * n_sums + i], (unsigned long long)sum,
                                                              __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // the value is asked for so that the add RETURNS: the wave waits for it here, in front of the barrier
        asm volatile("" ::"v"((unsigned)old), "v"((unsigned)(old >> 32)));
    }
    __syncthreads();        // every add of this workgroup has returned
    if (threadIdx.x >= 64) return;
    int finished = 0;
    if (threadIdx.x == 0) {
        float t = 0.0f;
#pragma unroll
        for (int w = 0; w < kLossThreads / 64; ++w) t += wave_part[w];
        finished = loss_arrive(t, fixed_scale, loss_scale, ws, loss_out);
    }
    finished = __builtin_amdgcn_readfirstlane(finished);
    if (finished == 0) return;
    // the finisher: every workgroup's adds returned before it arrived, and its arrival before the finisher's own returned
    const int n_all = (int)gridDim.y * n_sums;
    for (int i = threadIdx.x; i < n_all; i += 64) {
        const unsigned long long sum = __hip_atomic_exchange(&accum[i], 0ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (grad_exposure) {
            const float g = (float)((double)(long long)sum * grad_scale) * rcp_(exposure[i]);
            grad_exposure[i] = finished == 2 ? __builtin_nanf("") : g;
        }
    }
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

constexpr size_t kExposureLdsMax = 60 * 1024;

// Argument checks (all before the launch), plan_loss's grid and fixed-point scale, the launch.
int exposure_impl(const char *who, bool head, const float *input, const float *photos, const float *weights,
                  int weight_planes, const float *exposure, const float *scenes, const float *xrow, float eps,
                  float *loss_out, float *grad_input, float *grad_exposure, void *workspace, size_t workspace_bytes, int B,
                  int S, int H, int W, void *stream)
{
    char text[200];
    const auto bad = [&](int code, const char *what) {
        std::snprintf(text, sizeof(text), "%s: %s", who, what);
        return fail(code, text);
    };
    LossPlan p;
    if (!grad_input) return fail(SVBRDF_ERR_NULL, who);      // forward + adjoint only
    if (int e = plan_loss(who, false, {input, photos, exposure, scenes, xrow, loss_out}, grad_input, workspace,
                          workspace_bytes, "eps", eps, 0.0f, B, S, H, W, &p)) return e;
    if (!aligned(weights, 4) || !aligned(grad_exposure, 4)) return bad(SVBRDF_ERR_ALIGN, "pointers must be 4-byte aligned");
    if (weights ? (weight_planes != 1 && weight_planes != S) : weight_planes != 0)
        return bad(SVBRDF_ERR_DIMS, "weight_planes must be 1 (one plane per item) or S (one per photo) with weights, 0 without");
    if (workspace_bytes < svbrdf_photo_exposure_workspace_bytes(B, S, H, W)) return bad(SVBRDF_ERR_WORKSPACE, "workspace too small");
    const size_t lds_bytes = (size_t)kExpoWaves * (kExpoSpill + (size_t)S * 3) * sizeof(int);
    if (lds_bytes > kExposureLdsMax) return bad(SVBRDF_ERR_DIMS, "too many scenes per item for the LDS sums (max 1278)");
    const double grad_scale = 1.0 / ((double)B * S * 3.0 * (double)H * W * (double)kExpoFixedScale);       // 1 / (N 2^24)
    const auto kernel = head ? (weights ? k_exposure_head_weighted : k_exposure_head)
                             : (weights ? k_exposure_maps_weighted : k_exposure_maps);
    hipLaunchKernelGGL(kernel, p.grid, dim3(kLossThreads), lds_bytes, static_cast<hipStream_t>(stream), input, photos,
                       weights, weight_planes, exposure, scenes, xrow, eps, p.inv_count, p.loss_scale, p.fixed_scale,
                       grad_scale, (float)((double)B * S * 3.0 * (double)H * W * (double)kExpoFixedScale), grad_input,
                       grad_exposure, p.ws, loss_out, S, H, W);
    return launch_status(who);
}

}  // namespace

extern "C" {

size_t svbrdf_photo_exposure_workspace_bytes(int B, int S, int H, int W)
{
    const size_t sums = (B > 0 && S > 0) ? (size_t)B * (size_t)S * 3 : 0;
    return svbrdf_rendering_loss_workspace_bytes(B, S, H, W) + sums * sizeof(unsigned long long);
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
