// svbrdf_photo_pose_device.h -- the scene loop with the gradient towards the scene table and the body around it, shared by
// svbrdf_photo_pose.hip (which describes them) and, through svbrdf_photo_fit_pose_device.h, the joint fit units.
#ifndef SVBRDF_PHOTO_POSE_DEVICE_H
#define SVBRDF_PHOTO_POSE_DEVICE_H
#include "svbrdf_photo_loss_device.h"

namespace {

constexpr int kPoseWaves = kLossThreads / 64;
constexpr int kPoseSpill = 9;       // words per LDS row that the 63 lanes which do not hold the wave's sums store to
constexpr float kPoseWaveLimit = 8796093022208.0f;          // 2^43 units of 2^-24 / N: a wave's sum of N |term| up to 2^19

__device__ __forceinline__ float *pose_lds()
{
    extern __shared__ __attribute__((aligned(16))) float pose_words[];      // [waves][kPoseSpill + 9 S]
    return pose_words;
}

// v + (v of the row DPP control CTRL names) in the rows of ROW_MASK, v + 0 elsewhere
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add_rows(float v)
{
    return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, false));
}

// The 9 values of render s summed over the wave -- inside each row of 16 lanes (dpp_row_sums), then rows 0 -> 1, 2 -> 3 and
// 1 -> 3: fixed lanes, fixed order, so the sum is the same bits in every launch -- and stored by the wave's last lane (the
// others store to the row's spill words: a select of the address, not a branch inside the scene loop).
__device__ __forceinline__ void pose_collect(int row, int s, const float v[9])
{
    float r[9];
    dpp_row_sums<9>(v, r);
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = dpp_add_rows<0x142, 0xa>(r[k]);      // row_bcast:15 into rows 1 and 3
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = dpp_add_rows<0x143, 0xc>(r[k]);      // row_bcast:31 into rows 2 and 3
    const int dst = (threadIdx.x & 63) == 63 ? row + kPoseSpill + 9 * s : row;
#pragma unroll
    for (int k = 0; k < 9; ++k) pose_lds()[dst + k] = r[k];
}

// The scene loop: what photo_scene_loop<NL, true, NL == 1 ? 7 : 3, WEIGHTED> computes for the loss and the map gradient,
// render by render in the same order and through the same per-render functions, plus the render's 9 pose sums.  `live`:
// the lane's pixel exists; a lane without one shades the item's last pixel with 1/N = 0 (and a weight of 0), so that its
// adjoint is (+-)0 everywhere.
template <int NL, bool WEIGHTED>
__device__ __forceinline__ float pose_scene_loop(const MapK &mi, float x, float y, const float *__restrict__ scp,
                                                 const float *__restrict__ pp, size_t plane, size_t pix, int S, float eps,
                                                 float inv_count, Grad &acc, const float *__restrict__ wp, size_t wstride,
                                                 float poison, int row, bool live)
{
    float lsum = WEIGHTED ? poison : 0.0f;
    const VConst K = make_vconst();
    const float s10 = vreg(0.0009765625f);
    eps = vreg(eps);
    inv_count = live ? inv_count : 0.0f;
    const size_t render = 3 * plane;
    float pa[3], wa = 1.0f;
    if (WEIGHTED) load_photo_weight(pp, wp, plane, pix, pa, wa);
    else load_photo(pp, plane, pix, pa);
    for (int s = 0; s < S; ++s) {
        float sc[9], pn[3], wn = 1.0f;
        load_scene(scp, sc);
        scp += 9;
        pp += (s + 1 < S) ? render : 0;         // photo of render s+1 (a harmless repeat on the last pass)
        if (WEIGHTED) {
            wp += (s + 1 < S) ? wstride : 0;
            load_photo_weight(pp, wp, plane, pix, pn, wn);
        } else {
            load_photo(pp, plane, pix, pn);
        }
        const Geom g = geometry<true>(K, sc, x, y);
        float out[9];
        const PoseRender pr{sc, x, y, out};
        float w = 1.0f, ic = inv_count;
        if (WEIGHTED) {
            w = checked_weight(live ? wa : 0.0f);
            ic = inv_count * w;         // the weight folded into 1/N once per render
        }
        if (NL == 3)
            photo_pixel_scene_by_channel<true, 3, WEIGHTED, false, true>(K, g, mi, pa, s10, eps, ic, lsum, acc, w, nullptr, 0, &pr);
        else
            photo_pixel_scene<true, 7, WEIGHTED, false, true>(K, g, mi, pa, s10, eps, ic, lsum, acc, w, nullptr, 0, &pr);
        pose_collect(row, s, out);
#pragma unroll
        for (int k = 0; k < 3; ++k) pa[k] = pn[k];
        wa = wn;
    }
    lsum *= 0.693147180559945309417f;       // the loop sums |log2|
#pragma unroll
    for (int k = 0; k < 3; ++k) {           // the per-pixel constants the adjoint left out (photo_scene_loop)
        if (NL == 1) acc.d[k] *= mi.oms[k] * K.inv_pi;
        else acc.d[k] *= K.inv_pi;
        acc.r[k] *= expo_stash(k, 0.0f, true);      // dA/dr_hat waits in LDS: no register holds it across the loop
    }
    return lsum;
}

template <bool HEAD, bool WEIGHTED>
__device__ __forceinline__ void pose_body(const float *__restrict__ input, const float *__restrict__ photos,
                                          const float *__restrict__ weights, int weight_planes,
                                          const float *__restrict__ scenes, const float *__restrict__ xrow, float eps,
                                          float inv_count, double loss_scale, float fixed_scale, double grad_scale,
                                          float per_count, float *__restrict__ grad_input,
                                          float *__restrict__ grad_scenes, unsigned long long *__restrict__ ws,
                                          float *__restrict__ loss_out, int S, int H, int W)
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
        PixelSetup ps = wave_pixel_setup<HEAD, WEIGHTED>(input, xrow, b, plane, wi.pix, W);
        const float *__restrict__ scp = scenes + (size_t)b * n_sums;
        const float *__restrict__ pp = photos + (size_t)b * S * 3 * plane;
        const float *__restrict__ wp = WEIGHTED ? weights + (size_t)b * weight_planes * plane : nullptr;
        const size_t wstride = weight_planes == 1 ? 0 : plane;
#pragma unroll
        for (int k = 0; k < 3; ++k) expo_stash(k, ps.mi.r4m[k], false);
        if (HEAD || __builtin_amdgcn_readfirstlane((int)__all(ps.tied)))      // wave-uniform, and known to be
            lsum = pose_scene_loop<1, WEIGHTED>(ps.mi, ps.x, ps.y, scp, pp, plane, wi.pix, S, eps, inv_count, ps.acc, wp,
                                                wstride, ps.poison, wi.row, wi.live);
        else
            lsum = pose_scene_loop<3, WEIGHTED>(ps.mi, ps.x, ps.y, scp, pp, plane, wi.pix, S, eps, inv_count, ps.acc, wp,
                                                wstride, ps.poison, wi.row, wi.live);
        positive_check(scp, 9, 6, S, lsum);         // the item's light colours
        if (wi.live) {
            if (HEAD) store_pixel_grad<true>(ps.head, ps.acc, grad_input, b, plane, wi.pix);
            else store_grads_k3(grad_input + (size_t)b * 12 * plane, plane, wi.pix, ps.acc);
        } else {
            lsum -= lsum;       // +0; a NaN stays
        }
    }
    photo_sums_finish<true>(
        lsum, b, n_sums, fixed_scale, loss_scale, ws, loss_out,
        [&](int i, bool &sane) {        // the waves' floats, each checked against kPoseWaveLimit, to fixed point
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

#endif  // SVBRDF_PHOTO_POSE_DEVICE_H
