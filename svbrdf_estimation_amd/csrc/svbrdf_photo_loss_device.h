// svbrdf_photo_loss_device.h -- what the photo units of libsvbrdf_hip.so share: the per-render device functions, the scene
// loops, the set-up of a pixel, the end of a launch with per-scene sums and the launchers' checks.  svbrdf_photo_loss.hip
// (which describes the flow), svbrdf_photo_exposure.hip and, through the pose and fit headers, every fit unit include it.
//
// K3's own device code comes from svbrdf_device.h and the host-side argument checks from svbrdf_host.h, as for every unit.
#ifndef SVBRDF_PHOTO_LOSS_DEVICE_H
#define SVBRDF_PHOTO_LOSS_DEVICE_H
#include "svbrdf_device.h"
#include "svbrdf_host.h"

namespace {

// (photo + eps) 2^-10 of one term in ONE instruction: fma(photo, 2^-10, eps 2^-10) rounds (photo + eps) 2^-10 once, and a
// power-of-two scale commutes with the rounding: bitwise ldexp(fl(photo + eps), -10), the reference's fp32 photo + eps
// in the loss kernels' units (kLossScaleExp).  A photo value of exactly 0 gives eps 2^-10 exactly -- what shade_loss
// gives for a pixel the light does not reach (LN+ = 0), so such a term is exactly 0 with gradient 0.  A value below -eps
// gives a negative operand and the log of a negative quotient: NaN, as torch.log does.
__device__ __forceinline__ void photo_terms(const float ph[3], float s10, float ec, float bt[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) bt[k] = fma_(ph[k], s10, ec);
}

// The confidence weight of one (pixel, render) of the WEIGHTED kernels, checked once: a weight outside [0, 1] or NaN
// becomes NaN (v_med3 + compare + select) and poisons the loss sum through weighted_term's FMA whatever the term is.
__device__ __forceinline__ float checked_weight(float w)
{
    return (__builtin_amdgcn_fmed3f(w, 0.0f, 1.0f) == w) ? w : __builtin_nanf("");
}

// lsum += w |lg|.  fma(1, x, y) is x + y exactly: weights of all ones give the unweighted kernels' sum bit for bit.
template <bool WEIGHTED>
__device__ __forceinline__ void add_term(float w, float lg, float &lsum)
{
    if (WEIGHTED) lsum = fma_(w, fabsf(lg), lsum);
    else lsum += fabsf(lg);
}

// EXPO (the per-photo exposure kernels of svbrdf_photo_exposure.hip; no kernel of svbrdf_photo_loss.hip sets it): a positive gain per
// photo and colour channel multiplies the light colour, and d loss/d gain[s][c] = sum over the pixels of q / (N gain),
// q = w sign(delta) rad / (rad + eps) = -sign(lg) w (1 - ec / b) from registers the loss already holds.  What the scene
// loop needs for it:
struct ExpoLoop {
    int row;                // this WAVE's row of the dynamic LDS (expo_lds), in words: [kExpoSpill] words that the lanes
                            // which do not hold the wave's sums store theirs to, then [S][3] fixed-point sums of q
    bool live;              // the lane's pixel exists (the whole wave runs the loop); q is in units of live ? 2^-24 : 0
    float per_weight;       // WEIGHTED: N 2^24 -- q from w / N, which the adjoint holds anyway; a missing pixel's weight is 0
};
constexpr int kExpoSpill = 4;
// (LDS by index, not by pointer: a pointer through the struct is a 64-bit generic one, two VGPRs each)
__device__ __forceinline__ int *expo_lds()
{
    extern __shared__ __attribute__((aligned(16))) int expo_words[];
    return expo_words;
}
// dA/dr_hat of the lane's pixel is used behind the scene loop only (DEFER_R), and the exposure loops have no register to
// hold it meanwhile (the three-lobe loop of the weighted kernel spilled 8 VGPRs to scratch around it): it waits here, put
// by exposure_body in front of both loops.  `take` reads through an index the compiler cannot see through (an empty
// asm): it would otherwise forward the stored registers to the load and keep them.
__device__ __forceinline__ float expo_stash(int k, float put, bool take)
{
    __shared__ float words[3 * kLossThreads];
    int i = k * kLossThreads + (int)threadIdx.x;
    if (!take) {
        words[i] = put;
        return put;
    }
    asm volatile("" : "+v"(i));
    return words[i];
}
constexpr float kExpoFixedScale = 16777216.0f;      // 2^24: a wave's sum of q (|q| <= 1 for sane maps) fits 32 bits
// The limit of ONE channel's sum over a row of 16 lanes, in the same units: sane values reach 16 * 2^24 = 2^28, and the four
// row sums of a channel are added in int32 (expo_collect's two row_bcast steps): 4 * 1.5 * 2^28 < 2^31 cannot wrap.
constexpr float kExpoRowLimit = 24.0f * kExpoFixedScale;

// sc[6:9] *= gain, ONE float32 multiply of the colour column in front of the falloff: the rendering is bit for bit that of
// a scene table whose colour columns were multiplied by the gains in float32, and gains of 1 change nothing.  (The gains
// are checked once per item and wave: exposure_body.)
__device__ __forceinline__ void expo_scale(const float gain[3], float sc[9])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) sc[6 + k] *= gain[k];
}

// the three gains of one render: wave-uniform like its scene row, and loaded with it, two passes ahead
__device__ __forceinline__ void load_gain(const float *__restrict__ p, float e[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) e[k] = p[k];
}

// v + (v of the lane DPP control CTRL names), as one instruction.  The integer form with a row mask: rows outside the mask
// add 0.
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v)
{
    return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_add(int v)
{
    return v + __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xf, false);
}

// The four steps of a wave sum that stay inside a row of 16 lanes, N interleaved chains: fixed lanes, fixed order, so
// the sums are the same bits in every launch; every lane then holds its row's N sums.  What crosses the rows is the
// caller's (expo_collect: integers, pose_collect: floats).  Every lane of the wave must be here: DPP does not read a
// disabled lane.
template <int N>
__device__ __forceinline__ void dpp_row_sums(const float v[N], float r[N])
{
#pragma unroll
    for (int k = 0; k < N; ++k) r[k] = dpp_add<0xb1>(v[k]);         // quad_perm [1,0,3,2]
#pragma unroll
    for (int k = 0; k < N; ++k) r[k] = dpp_add<0x4e>(r[k]);         // quad_perm [2,3,0,1]
#pragma unroll
    for (int k = 0; k < N; ++k) r[k] = dpp_add<0x141>(r[k]);        // row_half_mirror
#pragma unroll
    for (int k = 0; k < N; ++k) r[k] = dpp_add<0x140>(r[k]);        // row_mirror
}

__device__ __forceinline__ float expo_unit(const ExpoLoop &xl) { return xl.live ? kExpoFixedScale : 0.0f; }

// The three q of render s (in units of 2^-24: the lane's `unit` is folded into them), summed over the wave -- four float
// steps inside each row of 16 lanes (fixed lanes, fixed order), the row sums converted to integers, then rows 0 -> 1,
// 2 -> 3 and 1 -> 3 -- and stored in the wave's own row of LDS sums by its last lane (a plain store: a wave meets every
// render once; the other lanes store to three words of the wave that nobody reads: a select of the address instead of a
// branch inside the scene loop, which cost 14 VGPRs).  Integer addition from the rows on, so the result does not depend on the order in which waves and workgroups
// arrive.  Every lane of the wave must be here (DPP does not read a disabled lane): the exposure kernels run a partial
// wave's missing pixels on a clamped index with a unit of 0.  A channel's row sum that is NaN or beyond kExpoRowLimit (maps no
// renderer input can produce: rad + eps inside (0, eps / 8) over a whole row) poisons the loss: every gradient is then
// reported as NaN, whatever the saturating conversion made of it, and below the limit the integer adds cannot wrap.
// N channels from channel K0 on: the tied loop collects its three q together (interleaved chains), the three-lobe loop
// each channel's as soon as it is known (one q alive at a time: that loop has no register to spare).
template <int N, int K0>
__device__ __forceinline__ void expo_collect(const ExpoLoop &xl, int s, const float q[N], float &lsum)
{
    float r[N];
    int t[N];
    bool sane = true;
    dpp_row_sums<N>(q, r);
#pragma unroll
    for (int k = 0; k < N; ++k) sane &= fabsf(r[k]) <= kExpoRowLimit;     // per channel, as the integer sums are; false for NaN
    if (!sane) lsum = __builtin_nanf("");
#pragma unroll
    for (int k = 0; k < N; ++k) t[k] = dpp_add<0x142, 0xa>((int)r[k]);      // row_bcast:15 into rows 1 and 3
#pragma unroll
    for (int k = 0; k < N; ++k) t[k] = dpp_add<0x143, 0xc>(t[k]);           // row_bcast:31 into rows 2 and 3
    const int dst = (threadIdx.x & 63) == 63 ? xl.row + kExpoSpill + 3 * s : xl.row;
#pragma unroll
    for (int k = 0; k < N; ++k) expo_lds()[dst + K0 + k] = t[k];
}

// POSE (the scene-gradient kernels of svbrdf_photo_pose.hip; no kernel of svbrdf_photo_loss.hip sets it): the render's scene row, the
// pixel's coordinates and where the 9 values of pose_bwd go.
struct PoseRender {
    const float *sc;
    float x, y;
    float *out;
};

// The adjoint of one render from the bars of its dot products to its scene row, PyTorch's sub-gradient conventions.
//   g_NH, g_VN: d loss / d (n.h), d (n.wo), clamp masks applied;  gl: d loss / d (n.wi), both clamps of it;
//   g_p: d loss / d p, p = (1 - VH)^5;  Q[k] = d loss / d b[k] times (b[k] - ec): the radiance's share, which is
//   d loss / d log colour[k] and d loss / d log falloff.
// With s = wi + wo, h = s / |s| and VH = wo.h = |s| / 2 (unit wo, wi), the bar of s is g_NH (n - (n.h) h) / |s| + g_VH h / 2,
// it joins the bars of wo and wi, and each goes through its normalisation: (bar - (bar.w) w) / |r|.  The falloff 1 / |rl|^2
// adds -2 sum(Q) wi / |rl|.  -> out[0:3] d / d camera, out[3:6] d / d light, out[6:9] = Q (the finisher divides by the colour).
// The lengths are 1-ULP rsq of the sums geometry() forms: the gradient is well conditioned in them.
__device__ __forceinline__ void pose_bwd(const VConst &K, const PoseRender &pr, const Geom &g, const MapK &mi,
                                         const Dots &di, float g_NH, float g_VN, float gl, float g_p, const float Q[3])
{
    const float *sc = pr.sc;
    float *out = pr.out;
    const float rcx = sc[0] - pr.x, rcy = sc[1] - pr.y, rcz = sc[2];
    const float rlx = sc[3] - pr.x, rly = sc[4] - pr.y, rlz = sc[5];
    const float ic = rsq_(dot3(rcx, rcy, rcz, rcx, rcy, rcz));
    const float il = rsq_(dot3(rlx, rly, rlz, rlx, rly, rlz));
    const float sx = g.wix + g.wox, sy = g.wiy + g.woy, sz = g.wiz + g.woz;
    const float ss = dot3(sx, sy, sz, sx, sy, sz);
    const float ih = rsq_(ss);
    const float vh = 0.5f * (ss * ih);
    const float t = 1.0f - vh, t2 = t * t;
    float g_VH = (-5.0f * (t2 * t2)) * g_p;
    if (!(vh >= K.tiny)) g_VH = 0.0f;
    const float a = g_NH * ih;
    const float c = fma_(-a, di.nh_raw, 0.5f * g_VH);       // bar of s = a n + c h
    const float eo = g_VN + a, ei = gl + a;                 // bars of wo, wi = e n + c h
    const float cv = c * vh;                                // h.wo = h.wi = VH
    const float po = fma_(eo, di.vn_raw, cv);
    const float pl = fma_(ei, di.ln_raw, cv) + 2.0f * ((Q[0] + Q[1]) + Q[2]);
    out[0] = fma_(eo, mi.n[0], fma_(c, g.hx, -po * g.wox)) * ic;
    out[1] = fma_(eo, mi.n[1], fma_(c, g.hy, -po * g.woy)) * ic;
    out[2] = fma_(eo, mi.n[2], fma_(c, g.hz, -po * g.woz)) * ic;
    out[3] = fma_(ei, mi.n[0], fma_(c, g.hx, -pl * g.wix)) * il;
    out[4] = fma_(ei, mi.n[1], fma_(c, g.hy, -pl * g.wiy)) * il;
    out[5] = fma_(ei, mi.n[2], fma_(c, g.hz, -pl * g.wiz)) * il;
#pragma unroll
    for (int k = 0; k < 3; ++k) out[6 + k] = Q[k];
}

// PGRAD (the photo-gradient kernels of svbrdf_photo_grad_photos.hip; no kernel of svbrdf_photo_loss.hip sets it):
// d loss / d photo[b,s,c,i,j] = -(w / N) sign(delta) / (photo + eps) for upstream gradient 1, stored where the photo value
// was loaded from, on another base.  The resource of the render whose terms are being formed (photo_scene_loop advances its
// base one pass behind the photos' own); an empty one without PGRAD.
template <bool PGRAD>
__device__ __forceinline__ PlaneBuf photo_grad_buf(float *render_base, size_t plane, size_t pix)
{
    if (PGRAD) return plane_buf(render_base, 3, plane, pix);
    return PlaneBuf{};
}
// One element.  The magnitude m = (w fl(1/N)) / fl(photo + eps): `per_count` is the numerator (w / N as the adjoint holds it,
// or 1/N), `bt` the denominator in the loss kernels' units (photo_terms: fl(photo + eps) 2^-10 exactly), so m is ONE IEEE
// division and an exact power-of-two scale -- a pure function of w, N, eps and this photo value, each operation rounded
// once.  The sign is the sign of `lg` = log2(bt / b) = -delta / ln 2 as the loss and the map adjoint of the same launch
// hold it: lg == 0 (equal operands, a quotient that rounds to 1, a zero weight -- whatever the photo holds: m is then
// not selected) gives `zero`, which is w * 0: (+-)0, or NaN for the NaN of a weight outside [0, 1].  A NaN or infinite lg
// (non-finite maps, a photo that is NaN, infinite or <= -eps under w > 0) gives NaN through the FMA; a finite one adds
// (+-)0.  Stored once and never read again: a plain store.
template <bool WEIGHTED>
__device__ __forceinline__ void photo_grad_store(const PlaneBuf &gb, int k, float lg, float per_count, float bt, float zero)
{
    const float m = __builtin_amdgcn_ldexpf(per_count / bt, kLossScaleExp);
    const float sel = lg == 0.0f ? (WEIGHTED ? zero : 0.0f) : __builtin_copysignf(m, lg);
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, fma_(lg, 0.0f, sel)), gb.rsrc, gb.lane_bytes,
                                          k * gb.plane_bytes, 0);
}

// one (pixel, scene), tied roughness: loss_pixel_scene with the target shading replaced by the photo's three values.
// WEIGHTED: `w` is the render's checked weight and `inv_count` already carries it (w / N, folded once per render); a
// weight of exactly 0 selects every term to exactly 0 -- whatever the photo holds, NaN included: 0 * NaN is never
// formed -- and lg = 0 with M = 0 gives a gradient of exactly (+-)0.
// EXPO: q[k] = -sign(lg) w (1 - ec / b[k]) `unit` as well, by loss_grad_of_b's clamp (sign(0) = 0: a zero weight gives
// (+-)0), collected for render `s` in front of the adjoint: the three q are dead before its registers are needed.
// POSE: behind the adjoint, the bars pose_bwd needs from the same registers (shade_bwd's own expressions: the compiler
// forms them once).
// PGRAD: the three elements of grad_photos of this render, each stored as soon as its lg is known (photo_grad_store).
template <bool WITH_GRAD, int DEFER, bool WEIGHTED = false, bool EXPO = false, bool POSE = false, bool PGRAD = false>
__device__ __forceinline__ void photo_pixel_scene(const VConst &K, const Geom &g, const MapK &mi, const float ph[3],
                                                  float s10, float eps, float inv_count, float &lsum, Grad &acc,
                                                  [[maybe_unused]] float w = 1.0f,
                                                  [[maybe_unused]] const ExpoLoop *xl = nullptr, [[maybe_unused]] int s = 0,
                                                  [[maybe_unused]] const PoseRender *pr = nullptr,
                                                  [[maybe_unused]] const PlaneBuf *gb = nullptr)
{
    static_assert(!POSE || WITH_GRAD, "the scene-gradient kernels are forward + adjoint");
    const float ec = __builtin_amdgcn_ldexpf(eps, kLossScaleExp);
    [[maybe_unused]] float q[3];
    [[maybe_unused]] const float unit = !EXPO ? 0.0f : WEIGHTED ? xl->per_weight : expo_unit(*xl);
    float bt[3];
    photo_terms(ph, s10, ec, bt);
    const Dots di = dots(K, g, mi);
    Lobe li[1];
    float Fi[3], fi[3], b[3], g_rad[3];
    shade_loss<1, WITH_GRAD>(K, g, mi, di, li, Fi, fi, ec, b);
    // K3's economy of transcendentals (loss_pixel_scene): the three 1/b from ONE v_rcp of their product, one log of the
    // quotient per channel, equal operands select exactly 0 (sign(0) = 0)
    float ib[3];
    {
        const float P = b[0] * b[1];
        const float r = rcp_(P * b[2]);
        const float t = r * b[2];
        ib[0] = t * b[1]; ib[1] = t * b[0]; ib[2] = r * P;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const bool differ = WEIGHTED ? (b[k] != bt[k] && w != 0.0f) : (b[k] != bt[k]);
        const float lg = differ ? log2_(bt[k] * ib[k]) : 0.0f;
        add_term<WEIGHTED>(w, lg, lsum);
        if (PGRAD) photo_grad_store<WEIGHTED>(*gb, k, lg, inv_count, bt[k], w * 0.0f);
        g_rad[k] = loss_grad_of_b(K, lg, inv_count * ib[k]);
        if (EXPO) {
            const float share = fma_(-ec, ib[k], 1.0f);     // rad / (rad + eps)
            q[k] = loss_grad_of_b(K, lg, WEIGHTED ? (share * inv_count) * unit : share * unit);
        }
    }
    if (EXPO) expo_collect<3, 0>(*xl, s, q, lsum);
    if (WITH_GRAD) shade_bwd<1, (DEFER & 1) != 0, (DEFER & 2) != 0, (DEFER & 4) != 0>(K, g, mi, di, li, Fi, fi, g_rad, acc);
    if (POSE) {
        float Q[3], g_LNp = 0.0f, g_p = 0.0f, Wg = 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float gE = g_rad[k] * g.E[k];
            const float g_f = gE * di.LNp;
            Q[k] = g_f * fi[k];
            g_LNp = k == 0 ? gE * fi[k] : fma_(gE, fi[k], g_LNp);
            g_p = fma_(g_f * (li[0].GD - mi.dpi[k]), mi.oms[k], g_p);
            const float gGD = g_f * Fi[k];
            Wg = k == 0 ? gGD : Wg + gGD;
        }
        float g_VN = Wg * li[0].KV, g_LN = Wg * li[0].KL;
        float g_NH = ((Wg * li[0].KN) * 2.0f) * di.NH;
        if (!(di.nh_raw >= K.tiny)) g_NH = 0.0f;
        if (!(di.vn_raw >= K.tiny)) g_VN = 0.0f;
        if (!(di.ln_raw >= K.tiny)) g_LN = 0.0f;
        if (!(di.ln_raw >= 0.0f)) g_LNp = 0.0f;
        pose_bwd(K, *pr, g, mi, di, g_NH, g_VN, g_LN + g_LNp, g_p, Q);
    }
}

// independent roughness channels: loss_pixel_scene_by_channel with the photo as the target side (POSE: the bar of p and
// the three Q beside the channels' adjoint)
template <bool WITH_GRAD, int DEFER, bool WEIGHTED = false, bool EXPO = false, bool POSE = false, bool PGRAD = false>
__device__ __forceinline__ void photo_pixel_scene_by_channel(const VConst &K, const Geom &g, const MapK &mi, const float ph[3],
                                                             float s10, float eps, float inv_count, float &lsum, Grad &acc,
                                                             [[maybe_unused]] float w = 1.0f,
                                                             [[maybe_unused]] const ExpoLoop *xl = nullptr,
                                                             [[maybe_unused]] int s = 0,
                                                             [[maybe_unused]] const PoseRender *pr = nullptr,
                                                             [[maybe_unused]] const PlaneBuf *gb = nullptr)
{
    const Dots di = dots(K, g, mi);
    const float ec = __builtin_amdgcn_ldexpf(eps, kLossScaleExp);
    [[maybe_unused]] const float unit = !EXPO ? 0.0f : WEIGHTED ? xl->per_weight : expo_unit(*xl);
    const float omp = 1.0f - g.p;
    float g_LNp = 0.0f, g_VN = 0.0f, g_LN = 0.0f, sN = 0.0f;
    [[maybe_unused]] float Q[3], g_p = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float bt = fma_(ph[k], s10, ec);
        const Lobe li = lobe<WITH_GRAD, false>(K, mi.A[k], mi.oA[k], di);
        const float Fi = fma_(mi.oms[k], g.p, mi.s[k]);
        const float fi = fma_(Fi, li.GD - mi.dpi[k], mi.dpi[k]);
        const float b = fma_(fi, g.E[k] * di.LNp, ec);
        const float ib = rcp_(b);
        const bool differ = WEIGHTED ? (b != bt && w != 0.0f) : (b != bt);
        const float lg = differ ? log2_(bt * ib) : 0.0f;
        add_term<WEIGHTED>(w, lg, lsum);
        if (EXPO) {
            const float share = fma_(-ec, ib, 1.0f);
            const float qk[1] = {loss_grad_of_b(K, lg, WEIGHTED ? (share * inv_count) * unit : share * unit)};
            if (k == 0) expo_collect<1, 0>(*xl, s, qk, lsum);
            else if (k == 1) expo_collect<1, 1>(*xl, s, qk, lsum);
            else expo_collect<1, 2>(*xl, s, qk, lsum);
        }
        if (WITH_GRAD) {
            const float gE = loss_grad_of_b(K, lg, inv_count * ib) * g.E[k];
            const float g_f = gE * di.LNp;
            g_LNp = fma_(gE, fi, g_LNp);
            const float g_F = g_f * (li.GD - mi.dpi[k]);
            acc.s[k] = fma_(g_F, omp, acc.s[k]);
            acc.d[k] = (DEFER & 1) ? fma_(g_f, 1.0f - Fi, acc.d[k]) : fma_(g_f * (1.0f - Fi), K.inv_pi, acc.d[k]);
            const float gGD = g_f * Fi;
            acc.r[k] = (DEFER & 2) ? fma_(gGD, li.KA, acc.r[k]) : fma_(gGD * li.KA, mi.r4m[k], acc.r[k]);
            g_VN = fma_(gGD, li.KV, g_VN);
            g_LN = fma_(gGD, li.KL, g_LN);
            sN = fma_(gGD, li.KN, sN);
            if (POSE) {
                Q[k] = g_f * fi;
                g_p = fma_(g_F, mi.oms[k], g_p);
            }
        }
        if (PGRAD) {
            // behind the channel's adjoint, where its lobe is dead, and held there: the division's temporaries on top of the
            // lobe's cost the weighted maps kernel ten VGPRs spilled to scratch around this loop.  (The forward-only loop
            // has the registers, and the barriers cost it 18 of them: free placement there.)
            if (WITH_GRAD) __builtin_amdgcn_sched_barrier(0);
            photo_grad_store<WEIGHTED>(*gb, k, lg, inv_count, bt, w * 0.0f);
            if (WITH_GRAD) __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (WITH_GRAD) {
        float g_NH = (sN * 2.0f) * di.NH;
        if (!(di.nh_raw >= K.tiny)) g_NH = 0.0f;
        if (!(di.vn_raw >= K.tiny)) g_VN = 0.0f;
        if (!(di.ln_raw >= K.tiny)) g_LN = 0.0f;
        if (!(di.ln_raw >= 0.0f)) g_LNp = 0.0f;
        const float gl = g_LN + g_LNp;
        acc.n[0] = fma_(g_NH, g.hx, fma_(g_VN, g.wox, fma_(gl, g.wix, acc.n[0])));
        acc.n[1] = fma_(g_NH, g.hy, fma_(g_VN, g.woy, fma_(gl, g.wiy, acc.n[1])));
        acc.n[2] = fma_(g_NH, g.hz, fma_(g_VN, g.woz, fma_(gl, g.wiz, acc.n[2])));
        if (POSE) pose_bwd(K, *pr, g, mi, di, g_NH, g_VN, gl, g_p, Q);
    }
}

template <int NL, bool WITH_GRAD, int DEFER, bool WEIGHTED = false, bool EXPO = false, bool PGRAD = false>
__device__ __forceinline__ void photo_pixel_scene_any(const VConst &K, const Geom &g, const MapK &mi, const float ph[3],
                                                      float s10, float eps, float inv_count, float &lsum, Grad &acc,
                                                      [[maybe_unused]] float w_raw = 1.0f,
                                                      [[maybe_unused]] const ExpoLoop *xl = nullptr, [[maybe_unused]] int s = 0,
                                                      [[maybe_unused]] const PlaneBuf *gb = nullptr)
{
    if (PGRAD) {        // (a branch of its own: the calls below stand as they stood before the flag)
        static_assert(!PGRAD || !EXPO, "the photo-gradient kernels take no exposure");
        const float w = WEIGHTED ? checked_weight(w_raw) : 1.0f;
        const float icw = WEIGHTED ? inv_count * w : inv_count;
        if (NL == 3)
            photo_pixel_scene_by_channel<WITH_GRAD, DEFER & 3, WEIGHTED, false, false, PGRAD>(K, g, mi, ph, s10, eps, icw, lsum, acc,
                                                                                              w, nullptr, 0, nullptr, gb);
        else
            photo_pixel_scene<WITH_GRAD, DEFER, WEIGHTED, false, false, PGRAD>(K, g, mi, ph, s10, eps, icw, lsum, acc, w, nullptr,
                                                                               0, nullptr, gb);
    } else if (WEIGHTED) {
        if (EXPO) w_raw = xl->live ? w_raw : 0.0f;
        const float w = checked_weight(w_raw);
        const float icw = inv_count * w;        // the weight folded into 1/N once per render
        if (NL == 3)
            photo_pixel_scene_by_channel<WITH_GRAD, DEFER & 3, true, EXPO>(K, g, mi, ph, s10, eps, icw, lsum, acc, w, xl, s);
        else
            photo_pixel_scene<WITH_GRAD, DEFER, true, EXPO>(K, g, mi, ph, s10, eps, icw, lsum, acc, w, xl, s);
    } else if (NL == 3)
        photo_pixel_scene_by_channel<WITH_GRAD, DEFER & 3, false, EXPO>(K, g, mi, ph, s10, eps, inv_count, lsum, acc, 1.0f, xl, s);
    else
        photo_pixel_scene<WITH_GRAD, DEFER, false, EXPO>(K, g, mi, ph, s10, eps, inv_count, lsum, acc, 1.0f, xl, s);
}

// the three photo values of one (pixel, render): planes 3 s .. 3 s + 2 of the item's [S,3,H,W] photos.  One buffer resource
// per render (base and size are wave-uniform: scalar arithmetic), so any S fits the 32-bit byte offsets.
__device__ __forceinline__ void load_photo(const float *__restrict__ render_base, size_t plane, size_t pix, float ph[3])
{
    const PlaneBuf pb = plane_buf(render_base, 3, plane, pix);
#pragma unroll
    for (int k = 0; k < 3; ++k) ph[k] = plane_load(pb, k);
}

// WEIGHTED: the render's confidence weight as a fourth load of the same back-to-back group.  Its plane lives in another
// allocation, hence a second resource (scalar arithmetic, made in front of the group).
__device__ __forceinline__ void load_photo_weight(const float *__restrict__ render_base, const float *__restrict__ weight_base,
                                                  size_t plane, size_t pix, float ph[3], float &w)
{
    const PlaneBuf pb = plane_buf(render_base, 3, plane, pix);
    const PlaneBuf wb = plane_buf(weight_base, 1, plane, pix);
    __builtin_amdgcn_sched_barrier(0);      // both resources stand: nothing but the four loads from here to the caller's barrier
#pragma unroll
    for (int k = 0; k < 3; ++k) ph[k] = plane_load(pb, k);
    w = plane_load(wb, 0);
}

// Scene loop, software-pipelined like K3's (loss_scene_loop): the geometry of render s+1 is computed beside the shading /
// loss / adjoint of render s, and the three photo values of render s+1 -- the only loads inside the loop -- are issued at
// the top of the pass that shades render s: they have a whole pass (~200 VALU instructions) to arrive, and because they
// are issued behind the loads of render s the compiler's wait in front of the first use of render s's values is a counted
// vmcnt that leaves them in flight (tests/test_photo_loss_cpu.py checks that in the assembly).  The loop body holds two
// passes with the roles of the geometry and photo register sets swapped: nothing is copied from "next" to "current".
// Left alone, the compiler SINKS the prefetch out of the pass that issues it, across the loop's exit test, to just in front
// of its first use in the next pass (seen in the assembly: ~140 instructions ahead of the use instead of a whole pass).  An
// empty asm that reads the three registers at the end of the issuing pass keeps the loads in that pass -- in front of its
// scheduling barrier -- and puts their wait at its end (behind a second scheduling barrier: the empty asm may otherwise be
// moved up), a whole pass of arithmetic behind the issue.
// WEIGHTED: the weight of render s+1 travels with its photo values -- fourth load of the group, same prefetch distance,
// pinned by the same empty asm -- and its pointer advances by the wave-uniform `wstride`: one plane ([B,S,H,W] weights) or
// zero ([B,1,H,W]: the item's one plane, re-read from cache).
#define SVBRDF_PHOTO_PIN(P, WT)                                                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                                               \
    if (WEIGHTED) asm volatile("" ::"v"(P[0]), "v"(P[1]), "v"(P[2]), "v"(WT));                                       \
    else asm volatile("" ::"v"(P[0]), "v"(P[1]), "v"(P[2]));
#define SVBRDF_PHOTO_LOAD(P, WT)                                                                                     \
    if (WEIGHTED) load_photo_weight(pp, wp, plane, pix, P, WT);                                                      \
    else load_photo(pp, plane, pix, P);
// EXPO (forward + adjoint only): the colour of every render is scaled by its gains in front of its geometry
// (expo_scale), and the render's three q go to the workgroup's sums behind its shading (expo_collect).
// PGRAD: `gp` is the base of grad_photos of the render that is being SHADED -- `pp` already points at the next one -- so it
// advances at the end of a pass, one pass behind `pp`: wave-uniform scalar arithmetic, one buffer resource per render as
// load_photo makes.  In the forward-only loop the store belongs to the render whose values stand in `pa`.
template <int NL, bool WITH_GRAD, int DEFER, bool WEIGHTED = false, bool EXPO = false, bool PGRAD = false>
__device__ __forceinline__ float photo_scene_loop(const MapK &mi, float x, float y, const float *__restrict__ scp,
                                                  const float *sc_lds, const float *__restrict__ pp, size_t plane,
                                                  size_t pix, int S, float eps, float inv_count, Grad &acc,
                                                  [[maybe_unused]] const float *__restrict__ wp = nullptr,
                                                  [[maybe_unused]] size_t wstride = 0, [[maybe_unused]] float poison = 0.0f,
                                                  [[maybe_unused]] const ExpoLoop *xl = nullptr,
                                                  [[maybe_unused]] const float *__restrict__ gain = nullptr,
                                                  [[maybe_unused]] float *__restrict__ gp = nullptr)
{
    static_assert(!EXPO || WITH_GRAD, "the exposure kernels are forward + adjoint");
    constexpr int ST = 9;
    // WEIGHTED: the sum starts from the maps' non-finite guard (+0, or NaN which every FMA below keeps) instead of holding
    // it in a register of its own across the loop; 1/N stays a scalar operand of the one multiply per render that uses it
    float lsum = WEIGHTED ? poison : 0.0f;
    const VConst K = make_vconst();
    const float s10 = vreg(0.0009765625f);      // 2^-10 (kLossScaleExp) as a VGPR operand of photo_terms' FMA
    eps = vreg(eps);
    if (!WEIGHTED) inv_count = vreg(inv_count);
    const size_t render = 3 * plane;            // floats per photo
    float sc[9];
    float pa[3], pb[3];
    [[maybe_unused]] float wa = 1.0f, wb = 1.0f;
    SVBRDF_PHOTO_LOAD(pa, wa)                   // render 0
    if (WITH_GRAD) {
        [[maybe_unused]] float sg[3];
        load_scene(scp, sc);
        if (EXPO) {
            load_gain(gain, sg);
            expo_scale(sg, sc);
        }
        Geom ga = geometry<true>(K, sc, x, y), gb;
        load_scene(scp + (S > 1 ? ST : 0), sc);
        if (EXPO) load_gain(gain + (S > 1 ? 3 : 0), sg);
#define SVBRDF_PHOTO_PASS(G_CUR, G_NEXT, P_CUR, P_NEXT, W_CUR, W_NEXT, SI)                                                        \
        {                                                                                                          \
            asm volatile("" ::"s"(sc[0]), "s"(sc[8]));                                                             \
            float cur[9];                                                                                          \
            _Pragma("unroll") for (int i = 0; i < 9; ++i) cur[i] = sc[i];                                          \
            if (EXPO) {                                                                                            \
                expo_scale(sg, cur);                                                                               \
                load_gain(gain + ((SI) + 2 < S ? 6 : ((SI) + 1 < S ? 3 : 0)), sg);                                 \
                gain += ((SI) + 1 < S) ? 3 : 0;                                                                    \
            }                                                                                                      \
            load_scene(scp + ((SI) + 2 < S ? 2 * ST : ((SI) + 1 < S ? ST : 0)), sc);                               \
            scp += ((SI) + 1 < S) ? ST : 0;                                                                        \
            pp += ((SI) + 1 < S) ? render : 0;          /* photo of render s+1 (a harmless repeat on the last pass) */ \
            if (WEIGHTED) wp += ((SI) + 1 < S) ? wstride : 0;                                                      \
            SVBRDF_PHOTO_LOAD(P_NEXT, W_NEXT)                                                                      \
            __builtin_amdgcn_sched_barrier(0);                                                                     \
            G_NEXT = geometry<true>(K, cur, x, y);                                                                 \
            if (PGRAD) {                                                                                           \
                const PlaneBuf gbuf = photo_grad_buf<PGRAD>(gp, plane, pix);                                       \
                photo_pixel_scene_any<NL, WITH_GRAD, DEFER, WEIGHTED, EXPO, PGRAD>(K, G_CUR, mi, P_CUR, s10, eps,  \
                                                                                   inv_count, lsum, acc, W_CUR,    \
                                                                                   xl, (SI), &gbuf);               \
                gp += ((SI) + 1 < S) ? render : 0;                                                                 \
            } else                                                                                                 \
            photo_pixel_scene_any<NL, WITH_GRAD, DEFER, WEIGHTED, EXPO>(K, G_CUR, mi, P_CUR, s10, eps, inv_count,  \
                                                                        lsum, acc, W_CUR, xl, (SI));               \
            SVBRDF_PHOTO_PIN(P_NEXT, W_NEXT)                                                                       \
        }
        for (int s = 0;;) {
            SVBRDF_PHOTO_PASS(ga, gb, pa, pb, wa, wb, s)
            if (++s >= S) break;
            SVBRDF_PHOTO_PASS(gb, ga, pb, pa, wb, wa, s)
            if (++s >= S) break;
        }
#undef SVBRDF_PHOTO_PASS
    } else {
        // forward only: scene table of the item staged in LDS (K3's measured choice for its forward-only kernels)
        load_scene(sc_lds, sc);
        Geom g_next = geometry<true>(K, sc, x, y);
        for (int s = 0; s < S; ++s) {
            const Geom g = g_next;
            pp += (s + 1 < S) ? render : 0;
            if (WEIGHTED) wp += (s + 1 < S) ? wstride : 0;
            SVBRDF_PHOTO_LOAD(pb, wb)
            __builtin_amdgcn_sched_barrier(0);      // (the scheduler otherwise sinks the three loads to their first use)
            load_scene(sc_lds + (s + 1 < S ? s + 1 : s) * 9, sc);
            g_next = geometry<true>(K, sc, x, y);
            if (PGRAD) {
                const PlaneBuf gbuf = photo_grad_buf<PGRAD>(gp, plane, pix);
                photo_pixel_scene_any<NL, WITH_GRAD, DEFER, WEIGHTED, false, PGRAD>(K, g, mi, pa, s10, eps, inv_count, lsum, acc,
                                                                                    wa, nullptr, 0, &gbuf);
                gp += (s + 1 < S) ? render : 0;
            } else
            photo_pixel_scene_any<NL, WITH_GRAD, DEFER, WEIGHTED>(K, g, mi, pa, s10, eps, inv_count, lsum, acc, wa);
            SVBRDF_PHOTO_PIN(pb, wb)
#pragma unroll
            for (int k = 0; k < 3; ++k) pa[k] = pb[k];
            if (WEIGHTED) wa = wb;
        }
    }
#undef SVBRDF_PHOTO_PIN
#undef SVBRDF_PHOTO_LOAD
    lsum *= 0.693147180559945309417f;       // the loop sums |log2|
    if (WITH_GRAD && DEFER) {               // the per-pixel constants the adjoint left out (shade_bwd's DEFER_*)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (DEFER & 4) acc.d[k] *= mi.oms[k] * K.inv_pi;
            else if (DEFER & 1) acc.d[k] *= K.inv_pi;
            if (DEFER & 2) acc.r[k] *= EXPO ? expo_stash(k, 0.0f, true) : mi.r4m[k];
        }
    }
    return lsum;
}

// ---- The small pieces every photo body is made of, each written once. ----

// The guard against non-finite maps, the numerics contract of every photo kernel: a NaN or infinite normal / roughness
// value would vanish in the clamps (v_max returns the other operand), so t - t -- 0 for finite t and NaN otherwise -- is
// added to the pixel's x coordinate (rendering_loss_body).  Diffuse, specular and the photo values propagate through the
// arithmetic by themselves.  WEIGHTED: a zero weight deselects the shading's value, so the diffuse and specular planes are
// guarded too and `poison` (+0 for finite maps, NaN otherwise) starts the pixel's loss sum: a weight does not excuse the
// maps.
template <bool WEIGHTED>
__device__ __forceinline__ void maps_guard(const Maps &in, float &x, float &poison)
{
    const float chk = ((in.n[0] + in.n[1]) + (in.n[2] + in.r[0])) + (in.r[1] + in.r[2]);
    x += chk - chk;
    if (WEIGHTED) {
        const float ds = ((in.d[0] + in.d[1]) + (in.d[2] + in.s[0])) + (in.s[1] + in.s[2]);
        poison = (chk - chk) + (ds - ds);
    }
}
// HEAD: the same guard from the 9 encoded values, formed where they are loaded -> what head_guard_apply adds to x where
// maps_guard stands.  The values that feed the normal and the roughness each on their own: a sum of large finite values
// must not overflow into a NaN report.  WEIGHTED: the diffuse and specular planes too (their way through the arithmetic
// ends at a select).
template <bool WEIGHTED>
__device__ __forceinline__ float head_guard(const float e[9], float &poison)
{
    const float head_chk = ((e[0] - e[0]) + (e[1] - e[1])) + (e[5] - e[5]);
    if (WEIGHTED)
        poison = (((e[2] - e[2]) + (e[3] - e[3])) + ((e[4] - e[4]) + (e[6] - e[6]))) + ((e[7] - e[7]) + (e[8] - e[8]));
    return head_chk;
}
template <bool WEIGHTED>
__device__ __forceinline__ void head_guard_apply(float head_chk, float &x, float &poison)
{
    x += head_chk;
    if (WEIGHTED) poison += head_chk;
}

// The pixel's coordinates: a shift and a mask for a power-of-two width, pixel_coords' division otherwise.  `pow2`:
// (W & (W - 1)) == 0, formed by the caller -- photo_loss_body forms it in front of its plane loads, for its early
// coordinates, and formed here instead it moves the scalar code of six kernels of svbrdf_photo_loss.hip.
__device__ __forceinline__ void pixel_xy(const float *xrow, size_t pix, int W, bool pow2, float &x, float &y)
{
    if (pow2) {
        const unsigned p32 = (unsigned)pix, sh = (unsigned)__builtin_ctz((unsigned)W);
        x = xrow[p32 & (unsigned)(W - 1)];
        y = -xrow[p32 >> sh];
    } else {
        float xs[1];
        pixel_coords<1>(xrow, pix, W, xs, y);
        x = xs[0];
    }
}

// (NOT among them: the item's base pointers scp, pp, wp, wstride, four lines that every body writes out.  As one function
// that returns them, the same expressions in the same order, the compiler schedules the scalar address arithmetic otherwise:
// loops with transcendentals of seven kernels carried other registers and the joint kernels gained an instruction --
// profiles/r29_photo_shared_pieces.txt.  Nor the twelve-line loss tail of photo_loss_body, photo_grad_body and fit_body: as
// one function it moved two instruction lines in each of the 28 kernels, and against the parent's library the photo-gradient
// launch with both gradients then took 51.02 us where 50.68 + 0.06 were allowed, and PhotoFit(smooth=).step 84.52 us where
// 82.06 + 0.66 were: the same record.)

// The item's 3 S values p[stride s + first + k], a lane each: one that is NaN, infinite or <= 0 makes the loss sum NaN,
// whatever the weights.  The light colours of the scene-gradient kernels (stride 9, from column 6: the colour gradient
// divides by them) and the gains of the exposure kernels (stride 3, from 0: the compiler folds the index to i, and their
// kernels keep their machine code).
__device__ __forceinline__ void positive_check(const float *p, int stride, int first, int S, float &lsum)
{
    for (int i = threadIdx.x & 63; i < 3 * S; i += 64) {
        const float v = p[(i / 3) * stride + first + i % 3];
        if (!(v > 0.0f && v < __builtin_inff())) lsum = __builtin_nanf("");
    }
}

// One thread = one pixel, all S renders of it; workgroup = 256 pixels of one batch item (as K3).
// HEAD: `input` is the generator's [B,9,H,W] post-tanh output and `grad_input` its gradient: the network head
// (decode_head / head_bwd, K3's own: svbrdf_head_loss_fwd_bwd) is folded in, 9 planes in and 9 out instead of 12 and 12.
// Decoded roughness is one channel repeated, so only the tied scene loop is instantiated for it.
// WEIGHTED: `weights` holds `weight_planes` = S ([B,S,H,W]) or 1 ([B,1,H,W]) confidence planes per item.  A zero weight
// deselects the shading's value, so the non-finite guard of the maps is ALSO added to the pixel's loss sum: a weight does
// not excuse the maps.
template <bool WITH_GRAD, bool EARLY_COORDS, bool HEAD = false, bool WEIGHTED = false>
__device__ __forceinline__ void photo_loss_body(const float *__restrict__ input, const float *__restrict__ photos,
                                                const float *__restrict__ scenes, const float *__restrict__ xrow,
                                                float eps, float inv_count, double loss_scale, float fixed_scale,
                                                float *__restrict__ grad_input, unsigned long long *__restrict__ ws,
                                                float *__restrict__ loss_out, int S, int H, int W,
                                                [[maybe_unused]] const float *__restrict__ weights = nullptr,
                                                [[maybe_unused]] int weight_planes = 0)
{
    extern __shared__ __attribute__((aligned(16))) float sc_lds[];      // [S][9], forward-only kernels
    const size_t plane = (size_t)H * W;
    const size_t pix = (size_t)blockIdx.x * kLossThreads + threadIdx.x;
    const int b = blockIdx.y;
    const bool active = pix < plane;
    float lsum = 0.0f;
    if (!WITH_GRAD) {
        for (int i = threadIdx.x; i < S * 9; i += kLossThreads) sc_lds[i] = scenes[(size_t)b * S * 9 + i];
        __syncthreads();
    }
    if (active) {
        // (the ORDER of a pixel's set-up -- loads, decode, prepare, coordinates, guard -- stands a second time in
        // wave_pixel_setup below, which says why; the guard and the coordinates themselves are maps_guard's, head_guard's
        // and pixel_xy's, once)
        Maps in;
        Grad acc;
        [[maybe_unused]] Head head;
        [[maybe_unused]] float head_chk = 0.0f;
        [[maybe_unused]] float poison = 0.0f;       // WEIGHTED: maps_guard's, added to the loss sum
        // pixel coordinates issued in front of the plane loads (by-value-table kernels, power-of-two width): see
        // rendering_loss_body
        [[maybe_unused]] float x_early = 0.0f, y_early = 0.0f;
        const bool pow2 = (W & (W - 1)) == 0;
        const bool early_coords = EARLY_COORDS && WITH_GRAD && pow2;
        if (early_coords) {
            const unsigned p32 = (unsigned)pix, sh = (unsigned)__builtin_ctz((unsigned)W);
            x_early = xrow[p32 & (unsigned)(W - 1)];
            y_early = xrow[p32 >> sh];
            __builtin_amdgcn_sched_barrier(0);
        }
        if (HEAD) {
            float e[9];
            const PlaneBuf pb = plane_buf(input + (size_t)b * 9 * plane, 9, plane, pix);
#pragma unroll
            for (int k = 0; k < 9; ++k) e[k] = plane_load(pb, k);
            head = decode_head(e, in);
            head_chk = head_guard<WEIGHTED>(e, poison);
        } else {
            load_maps_k3(input + (size_t)b * 12 * plane, plane, pix, in);
        }
        zero_grad(acc);
        const bool tied = HEAD || tied_roughness(in);
        const MapK mi = prepare<WITH_GRAD>(in);
        float x, y;
        if (early_coords) {
            x = x_early;
            y = -y_early;
        } else {
            pixel_xy(xrow, pix, W, pow2, x, y);
        }
        if (HEAD) head_guard_apply<WEIGHTED>(head_chk, x, poison);
        else maps_guard<WEIGHTED>(in, x, poison);
        const float *__restrict__ scp = scenes + (size_t)b * S * 9;
        const float *__restrict__ pp = photos + (size_t)b * S * 3 * plane;
        const float *__restrict__ wp = WEIGHTED ? weights + (size_t)b * weight_planes * plane : nullptr;
        const size_t wstride = weight_planes == 1 ? 0 : plane;
        constexpr int kDefer = WITH_GRAD ? 7 : 0;
        if (HEAD || __all(tied))        // wave-uniform
            lsum = photo_scene_loop<1, WITH_GRAD, kDefer, WEIGHTED>(mi, x, y, scp, sc_lds, pp, plane, pix, S, eps, inv_count, acc,
                                                                    wp, wstride, poison);
        else
            lsum = photo_scene_loop<3, WITH_GRAD, kDefer & 3, WEIGHTED>(mi, x, y, scp, sc_lds, pp, plane, pix, S, eps, inv_count,
                                                                        acc, wp, wstride, poison);
        if (WITH_GRAD) {
            if (HEAD) store_pixel_grad<true>(head, acc, grad_input, b, plane, pix);
            else store_grads_k3(grad_input + (size_t)b * 12 * plane, plane, pix, acc);
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

// ---- What the kernels that also sum per-item values share (exposure_body of svbrdf_photo_exposure.hip: 3 S gains,
// pose_body of svbrdf_photo_pose.hip: 9 S scene values).  No kernel of svbrdf_photo_loss.hip uses any of it. ----

// Where a lane of such a kernel stands.  A wave that holds at least one pixel runs WHOLE -- the lanes past the item's last
// pixel shade that last pixel again, deselected from the loss, the sums and the stores -- so that the wave sums never read
// a disabled lane.  A wave without pixels zeroes its row of sums and skips the pixel: that one-line loop is each body's own
// (zeroing here, in front of an `if (wave_live)` of the body, cost k_exposure_maps_weighted a fifth spilled SGPR).
struct WaveIndex {
    size_t pix;         // the lane's pixel, or the item's last one
    bool live;          // the lane's pixel exists
    bool wave_live;     // the wave holds a pixel (wave-uniform)
    int row;            // the wave's row of the dynamic LDS, in words: spill words that the lanes which do not hold the
                        // wave's sums store theirs to, then its sums
};
[[maybe_unused]] __device__ __forceinline__ WaveIndex wave_index(size_t plane, int row_words)
{
    WaveIndex wi;
    const size_t first = (size_t)blockIdx.x * kLossThreads + (threadIdx.x & ~63u);
    wi.live = first + (threadIdx.x & 63) < plane;
    wi.pix = wi.live ? first + (threadIdx.x & 63) : plane - 1;
    wi.wave_live = __builtin_amdgcn_readfirstlane((int)(first < plane)) != 0;
    wi.row = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * row_words;
    return wi;
}

// The set-up of a pixel: photo_loss_body<true, false, HEAD, WEIGHTED>'s statements from the plane loads to the guards on x
// and `poison`, in its source order (the order the scheduler sees).  What is SHARED with that body: the guards (maps_guard,
// head_guard) and the coordinates (pixel_xy), each written once above.  What is NOT: the order of the statements around them
// stands twice.  photo_loss_body on a generalised wave_pixel_setup<HEAD, WEIGHTED, WITH_GRAD, EARLY> was tried (compiled
// only, profiles/r29_photo_shared_pieces.txt): all 16 kernels of svbrdf_photo_loss.hip moved, 7 with altered scene loops, and the by-value forward +
// adjoint kernels gained 11-12 instructions and 3 VALU; round 16's decision stands.  A change to the order of the loads
// is made here and there.
struct PixelSetup {
    MapK mi;
    Grad acc;       // zeroed
    Head head;      // HEAD only
    bool tied;
    float x, y, poison;
};
template <bool HEAD, bool WEIGHTED>
__device__ __forceinline__ PixelSetup wave_pixel_setup(const float *__restrict__ input, const float *__restrict__ xrow, int b,
                                                       size_t plane, size_t pix, int W)
{
    PixelSetup ps;
    Maps in;
    [[maybe_unused]] float head_chk = 0.0f;
    ps.poison = 0.0f;
    if (HEAD) {
        float e[9];
        const PlaneBuf pb = plane_buf(input + (size_t)b * 9 * plane, 9, plane, pix);
#pragma unroll
        for (int k = 0; k < 9; ++k) e[k] = plane_load(pb, k);
        ps.head = decode_head(e, in);
        head_chk = head_guard<WEIGHTED>(e, ps.poison);
    } else {
        load_maps_k3(input + (size_t)b * 12 * plane, plane, pix, in);
    }
    zero_grad(ps.acc);
    ps.tied = HEAD || tied_roughness(in);
    ps.mi = prepare<true>(in);
    pixel_xy(xrow, pix, W, (W & (W - 1)) == 0, ps.x, ps.y);
    if (HEAD) head_guard_apply<WEIGHTED>(head_chk, ps.x, ps.poison);
    else maps_guard<WEIGHTED>(in, ps.x, ps.poison);
    return ps;
}

// The end of such a launch.  `workgroup_sum(i, sane)`: sum i of this workgroup from its waves' rows of LDS, as a 64-bit
// fixed-point integer; CHECKED: it may clear `sane`, and the loss of the launch -- and with it every gradient -- is then NaN.
// `write(i, sum, nan)`: the finisher's result i of all B n_sums from the launch's sum.
//   * behind one barrier, n_sums lanes add the workgroup's sums to the accumulator words of the workspace (behind
//     loss_arrive's 65) with 64-bit agent-scope RETURNING atomics and wait for their return; then the barrier of the loss
//     reduction; then lane 0 arrives (loss_arrive).  Whoever finishes the launch therefore knows every accumulator
//     complete: each workgroup's adds returned before its arrival was counted.
//   * the finisher's wave 0 (told by readfirstlane of loss_arrive's answer: no LDS word, no third barrier, the other three
//     waves have left) fetches and zeroes every accumulator with 64-bit agent-scope atomic exchanges -- 8-byte agent
//     atomics on both sides of the hand-off, no fence; a plain load could be served by this compute unit's L1 or its
//     die's L2.
// Three dependent round trips (accumulator adds, slot + tail, exchanges) against two in the kernels of svbrdf_photo_loss.hip.
template <bool CHECKED, typename Sum, typename Write>
__device__ __forceinline__ void photo_sums_finish(float lsum, int b, int n_sums, float fixed_scale, double loss_scale,
                                                  unsigned long long *__restrict__ ws, float *__restrict__ loss_out,
                                                  Sum workgroup_sum, Write write)
{
    constexpr int kWaves = kLossThreads / 64;
    __shared__ float wave_part[kWaves];
    [[maybe_unused]] __shared__ int wild;       // CHECKED: a sum was not sane
    lsum = wave_sum(lsum);
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = lsum;
    if (CHECKED && threadIdx.x == 0) wild = 0;
    __syncthreads();        // the workgroup's sums stand in LDS
    unsigned long long *__restrict__ accum = ws + (kLossSlots + 1);
    for (int i = threadIdx.x; i < n_sums; i += kLossThreads) {
        bool sane = true;
        const long long sum = workgroup_sum(i, sane);
        if (CHECKED && !sane) wild = 1;
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
        for (int w = 0; w < kWaves; ++w) t += wave_part[w];
        if (CHECKED && wild) t = __builtin_nanf("");
        finished = loss_arrive(t, fixed_scale, loss_scale, ws, loss_out);
    }
    finished = __builtin_amdgcn_readfirstlane(finished);
    if (finished == 0) return;
    // the finisher: every workgroup's adds returned before it arrived, and its arrival before the finisher's own returned
    const int n_all = (int)gridDim.y * n_sums;
    for (int i = threadIdx.x; i < n_all; i += 64) {
        const unsigned long long sum = __hip_atomic_exchange(&accum[i], 0ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        write(i, (long long)sum, finished == 2);
    }
}

// Host side: workspace_bytes of an entry with `per_scene` sums per (item, scene), and the argument checks of its
// launcher (all before the launch, one order, one set of codes) with plan_loss's grid and fixed-point scale.  `required`
// holds grad_scenes; grad_exposure may be null and is `optional_out`.  -> p->lds_bytes: the [waves][spill + per_scene S]
// rows; *units = N 2^24, what one unit of the accumulators is the reciprocal of.
[[maybe_unused]] size_t sums_workspace_bytes(int per_scene, int B, int S, int H, int W)
{
    const size_t sums = (B > 0 && S > 0) ? (size_t)B * (size_t)S * per_scene : 0;
    return svbrdf_rendering_loss_workspace_bytes(B, S, H, W) + sums * sizeof(unsigned long long);
}
// The weights of every photo and fit entry, behind plan_loss: an optional pointer (4-byte aligned), `weight_planes` 1 or S
// with it and 0 without.  (`rule`: the eight oldest entries, whose weights are among plan_loss's required pointers, word it
// shorter.  kAlignRule is the sentence for the pointers plan_loss does not see -- plan_loss's own, in svbrdf_host.h, names
// the workspace too and is another text.)
constexpr const char *kAlignRule = "pointers must be 4-byte aligned";
constexpr const char *kWeightsRule = "weight_planes must be 1 (one plane per item) or S (one per photo) with weights, 0 without";
[[maybe_unused]] int weights_check(const char *who, const float *weights, int weight_planes, int S,
                                   const char *rule = kWeightsRule)
{
    if (!aligned(weights, 4)) return fail_as(who, SVBRDF_ERR_ALIGN, kAlignRule);
    if (weights ? (weight_planes != 1 && weight_planes != S) : weight_planes != 0) return fail_as(who, SVBRDF_ERR_DIMS, rule);
    return 0;
}
[[maybe_unused]] int plan_sums(const char *who, std::initializer_list<const void *> required, const float *weights,
                               int weight_planes, const float *optional_out, float eps, const float *grad_input,
                               void *workspace, size_t workspace_bytes, int per_scene, int spill, int B, int S, int H, int W,
                               LossPlan *p, double *units)
{
    constexpr size_t kRowBytes = kLossThreads / 64 * sizeof(float), kLdsMax = 60 * 1024;
    char lds_text[80];
    if (!grad_input) return fail(SVBRDF_ERR_NULL, who);      // forward + adjoint only
    if (int e = plan_loss(who, false, required, grad_input, workspace, workspace_bytes, "eps", eps, 0.0f, B, S, H, W, p)) return e;
    if (!aligned(optional_out, 4)) return fail_as(who, SVBRDF_ERR_ALIGN, kAlignRule);
    if (int e = weights_check(who, weights, weight_planes, S)) return e;
    if (workspace_bytes < sums_workspace_bytes(per_scene, B, S, H, W))
        return fail_as(who, SVBRDF_ERR_WORKSPACE, "workspace too small");
    p->lds_bytes = kRowBytes * (spill + (size_t)S * per_scene);
    std::snprintf(lds_text, sizeof(lds_text), "too many scenes per item for the LDS sums (max %d)",
                  (int)((kLdsMax / kRowBytes - spill) / per_scene));
    if (p->lds_bytes > kLdsMax) return fail_as(who, SVBRDF_ERR_DIMS, lds_text);
    *units = (double)B * S * 3.0 * (double)H * W * (double)kExpoFixedScale;
    return 0;
}

#ifndef SVBRDF_PHOTO_LOSS_MIN_WAVES
#define SVBRDF_PHOTO_LOSS_MIN_WAVES 4      // 128 VGPRs, as K3
#endif
#define SVBRDF_PHOTO_LOSS_ATTRS \
    __launch_bounds__(kLossThreads) __attribute__((amdgpu_waves_per_eu(SVBRDF_PHOTO_LOSS_MIN_WAVES, 8)))

}  // namespace

#endif  // SVBRDF_PHOTO_LOSS_DEVICE_H
