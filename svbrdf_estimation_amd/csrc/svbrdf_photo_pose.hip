// svbrdf_photo_pose.hip -- translation unit of libsvbrdf_hip.so: the fused photo losses with the gradient towards the
// SCENE TABLE -- camera position, light position, light colour of every photo -- in the one launch (added to ABI version 8
// without a bump).
//
//   L = (1/N) sum w | log(render(scene[b,s], input[b]) + eps) - log(p' + eps) |
//   grad_scenes[b,s,0:3] = dL/d camera, [3:6] = dL/d light position, [6:9] = dL/d light colour
//
// A captured flash photograph comes with a camera position estimated from a homography and a flash "somewhere next to the
// lens"; with the table frozen a light that is a few centimetres off is absorbed into the normals and the roughness.  The
// loss and the map gradient are bit for bit those of the existing entries on the same table: the forward and the map
// adjoint below are the statements of svbrdf_photo_loss.hip's per-render functions (photo_pixel_scene,
// photo_pixel_scene_by_channel), float operation for float operation in the same order, and float arithmetic without
// contraction does not depend on how the compiler schedules it.
//
// Four kernels, {maps, head} x {unweighted, weighted}, forward + adjoint, scene table in device memory.  The shape is the
// exposure kernels' (svbrdf_photo_exposure.hip): a wave that holds at least one pixel runs WHOLE, per-wave rows of sums in
// LDS, 64-bit agent-scope returning adds to accumulator words behind loss_arrive's 65, drained by the finisher with
// exchanges.  What differs:
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
//     VGPRs (maps), and the pipelined form, which holds a second geometry, was not built and is unmeasured.
// pose_body repeats photo_loss_body's set-up of a pixel, as exposure_body does and for its reason, and the per-render
// functions repeat photo_pixel_scene[_by_channel]'s statements: DEBT -- a change to the guards, the forward or the map adjoint
// is made in every copy, and only the bitwise GPU tests (tests/test_gpu_pose_photo_loss.py) notice a copy that was missed.
#define SVBRDF_PHOTO_SHARED_ONLY
#include "svbrdf_photo_loss.hip"

namespace {

constexpr int kPoseWaves = kLossThreads / 64;
constexpr int kPoseSpill = 9;       // words per LDS row that the 63 lanes which do not hold the wave's sums store to
constexpr float kPoseFixedScale = 16777216.0f;              // 2^24: the accumulators count units of 2^-24 / N
constexpr float kPoseWaveLimit = 8796093022208.0f;          // 2^43 of those units: a wave's sum of N |term| up to 2^19

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

// The 9 values of render s summed over the wave -- four steps inside each row of 16 lanes, then rows 0 -> 1, 2 -> 3 and
// 1 -> 3: fixed lanes, fixed order, so the sum is the same bits in every launch -- and stored by the wave's last lane (the
// others store to the row's spill words: a select of the address, not a branch inside the scene loop).  Every lane of the
// wave must be here (DPP does not read a disabled lane).
__device__ __forceinline__ void pose_collect(int row, int s, const float v[9])
{
    float r[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = dpp_add<0xb1>(v[k]);         // quad_perm [1,0,3,2]
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = dpp_add<0x4e>(r[k]);         // quad_perm [2,3,0,1]
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = dpp_add<0x141>(r[k]);        // row_half_mirror
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = dpp_add<0x140>(r[k]);        // row_mirror: every lane holds its row's sum
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = dpp_add_rows<0x142, 0xa>(r[k]);      // row_bcast:15 into rows 1 and 3
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = dpp_add_rows<0x143, 0xc>(r[k]);      // row_bcast:31 into rows 2 and 3
    const int dst = (threadIdx.x & 63) == 63 ? row + kPoseSpill + 9 * s : row;
#pragma unroll
    for (int k = 0; k < 9; ++k) pose_lds()[dst + k] = r[k];
}

// The adjoint of one render from the bars of its dot products to its scene row, PyTorch's sub-gradient conventions.
//   g_NH, g_VN: d loss / d (n.h), d (n.wo), clamp masks applied;  gl: d loss / d (n.wi), both clamps of it;
//   g_p: d loss / d p, p = (1 - VH)^5;  Q[k] = d loss / d b[k] times (b[k] - ec): the radiance's share, which is
//   d loss / d log colour[k] and d loss / d log falloff.
// With s = wi + wo, h = s / |s| and VH = wo.h = |s| / 2 (unit wo, wi), the bar of s is g_NH (n - (n.h) h) / |s| + g_VH h / 2,
// it joins the bars of wo and wi, and each goes through its normalisation: (bar - (bar.w) w) / |r|.  The falloff 1 / |rl|^2
// adds -2 sum(Q) wi / |rl|.  -> out[0:3] d / d camera, out[3:6] d / d light, out[6:9] = Q (the finisher divides by the colour).
// The lengths are 1-ULP rsq of the sums geometry() forms: the gradient is well conditioned in them.
__device__ __forceinline__ void pose_bwd(const VConst &K, const float sc[9], float x, float y, const Geom &g,
                                         const MapK &mi, const Dots &di, float g_NH, float g_VN, float gl, float g_p,
                                         const float Q[3], float out[9])
{
    const float rcx = sc[0] - x, rcy = sc[1] - y, rcz = sc[2];
    const float rlx = sc[3] - x, rly = sc[4] - y, rlz = sc[5];
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

// one (pixel, scene), tied roughness: photo_pixel_scene<true, 7, WEIGHTED>'s statements, then the bars pose_bwd needs
// from the same registers (shade_bwd's own expressions: the compiler forms them once)
template <bool WEIGHTED>
__device__ __forceinline__ void pose_pixel_scene(const VConst &K, const float sc[9], float x, float y, const Geom &g,
                                                 const MapK &mi, const float ph[3], float s10, float eps, float inv_count,
                                                 float &lsum, Grad &acc, float w, float out[9])
{
    const float ec = __builtin_amdgcn_ldexpf(eps, kLossScaleExp);
    float bt[3];
    photo_terms(ph, s10, ec, bt);
    const Dots di = dots(K, g, mi);
    Lobe li[1];
    float Fi[3], fi[3], b[3], g_rad[3];
    shade_loss<1, true>(K, g, mi, di, li, Fi, fi, ec, b);
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
        g_rad[k] = loss_grad_of_b(K, lg, inv_count * ib[k]);
    }
    shade_bwd<1, true, true, true>(K, g, mi, di, li, Fi, fi, g_rad, acc);
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
    pose_bwd(K, sc, x, y, g, mi, di, g_NH, g_VN, g_LN + g_LNp, g_p, Q, out);
}

// independent roughness channels: photo_pixel_scene_by_channel<true, 3, WEIGHTED>'s statements with the bars of p and the
// three Q beside them
template <bool WEIGHTED>
__device__ __forceinline__ void pose_pixel_scene_by_channel(const VConst &K, const float sc[9], float x, float y,
                                                            const Geom &g, const MapK &mi, const float ph[3], float s10,
                                                            float eps, float inv_count, float &lsum, Grad &acc, float w,
                                                            float out[9])
{
    const Dots di = dots(K, g, mi);
    const float ec = __builtin_amdgcn_ldexpf(eps, kLossScaleExp);
    const float omp = 1.0f - g.p;
    float g_LNp = 0.0f, g_VN = 0.0f, g_LN = 0.0f, sN = 0.0f;
    float Q[3], g_p = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float bt = fma_(ph[k], s10, ec);
        const Lobe li = lobe<true, false>(K, mi.A[k], mi.oA[k], di);
        const float Fi = fma_(mi.oms[k], g.p, mi.s[k]);
        const float fi = fma_(Fi, li.GD - mi.dpi[k], mi.dpi[k]);
        const float b = fma_(fi, g.E[k] * di.LNp, ec);
        const float ib = rcp_(b);
        const bool differ = WEIGHTED ? (b != bt && w != 0.0f) : (b != bt);
        const float lg = differ ? log2_(bt * ib) : 0.0f;
        add_term<WEIGHTED>(w, lg, lsum);
        const float gE = loss_grad_of_b(K, lg, inv_count * ib) * g.E[k];
        const float g_f = gE * di.LNp;
        g_LNp = fma_(gE, fi, g_LNp);
        const float g_F = g_f * (li.GD - mi.dpi[k]);
        acc.s[k] = fma_(g_F, omp, acc.s[k]);
        acc.d[k] = fma_(g_f, 1.0f - Fi, acc.d[k]);
        const float gGD = g_f * Fi;
        acc.r[k] = fma_(gGD, li.KA, acc.r[k]);
        g_VN = fma_(gGD, li.KV, g_VN);
        g_LN = fma_(gGD, li.KL, g_LN);
        sN = fma_(gGD, li.KN, sN);
        Q[k] = g_f * fi;
        g_p = fma_(g_F, mi.oms[k], g_p);
    }
    float g_NH = (sN * 2.0f) * di.NH;
    if (!(di.nh_raw >= K.tiny)) g_NH = 0.0f;
    if (!(di.vn_raw >= K.tiny)) g_VN = 0.0f;
    if (!(di.ln_raw >= K.tiny)) g_LN = 0.0f;
    if (!(di.ln_raw >= 0.0f)) g_LNp = 0.0f;
    const float gl = g_LN + g_LNp;
    acc.n[0] = fma_(g_NH, g.hx, fma_(g_VN, g.wox, fma_(gl, g.wix, acc.n[0])));
    acc.n[1] = fma_(g_NH, g.hy, fma_(g_VN, g.woy, fma_(gl, g.wiy, acc.n[1])));
    acc.n[2] = fma_(g_NH, g.hz, fma_(g_VN, g.woz, fma_(gl, g.wiz, acc.n[2])));
    pose_bwd(K, sc, x, y, g, mi, di, g_NH, g_VN, gl, g_p, Q, out);
}

// The scene loop: what photo_scene_loop<NL, true, NL == 1 ? 7 : 3, WEIGHTED> computes for the loss and the map gradient,
// render by render in the same order, plus the render's 9 pose sums.  `live`: the lane's pixel exists; a lane without one
// shades the item's last pixel with 1/N = 0 (and a weight of 0), so that its adjoint is (+-)0 everywhere.
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
        float w = 1.0f, ic = inv_count;
        if (WEIGHTED) {
            w = checked_weight(live ? wa : 0.0f);
            ic = inv_count * w;         // the weight folded into 1/N once per render
        }
        if (NL == 3) pose_pixel_scene_by_channel<WEIGHTED>(K, sc, x, y, g, mi, pa, s10, eps, ic, lsum, acc, w, out);
        else pose_pixel_scene<WEIGHTED>(K, sc, x, y, g, mi, pa, s10, eps, ic, lsum, acc, w, out);
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
    const size_t first = (size_t)blockIdx.x * kLossThreads + (threadIdx.x & ~63u);
    const bool live = first + (threadIdx.x & 63) < plane;
    const size_t pix = live ? first + (threadIdx.x & 63) : plane - 1;
    const bool wave_live = __builtin_amdgcn_readfirstlane((int)(first < plane)) != 0;
    const int b = blockIdx.y;
    const int n_sums = 9 * S;
    const int row_words = kPoseSpill + n_sums;
    const int row = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * row_words;
    float lsum = 0.0f;
    if (!wave_live) {
        for (int i = threadIdx.x & 63; i < n_sums; i += 64) sums[row + kPoseSpill + i] = 0.0f;     // a wave without pixels
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
        const float *__restrict__ scp = scenes + (size_t)b * n_sums;
        const float *__restrict__ pp = photos + (size_t)b * S * 3 * plane;
        const float *__restrict__ wp = WEIGHTED ? weights + (size_t)b * weight_planes * plane : nullptr;
        const size_t wstride = weight_planes == 1 ? 0 : plane;
#pragma unroll
        for (int k = 0; k < 3; ++k) expo_stash(k, mi.r4m[k], false);
        if (HEAD || __builtin_amdgcn_readfirstlane((int)__all(tied)))      // wave-uniform, and known to be
            lsum = pose_scene_loop<1, WEIGHTED>(mi, x[0], y, scp, pp, plane, pix, S, eps, inv_count, acc, wp, wstride,
                                                poison, row, live);
        else
            lsum = pose_scene_loop<3, WEIGHTED>(mi, x[0], y, scp, pp, plane, pix, S, eps, inv_count, acc, wp, wstride,
                                                poison, row, live);
        // the item's light colours, a lane each: one that is NaN, infinite or <= 0 makes the loss sum NaN (the rule of the
        // exposure gains: the colour gradient divides by it)
        for (int i = threadIdx.x & 63; i < 3 * S; i += 64) {
            const float c = scp[(i / 3) * 9 + 6 + i % 3];
            if (!(c > 0.0f && c < __builtin_inff())) lsum = __builtin_nanf("");
        }
        if (live) {
            if (HEAD) store_pixel_grad<true>(head, acc, grad_input, b, plane, pix);
            else store_grads_k3(grad_input + (size_t)b * 12 * plane, plane, pix, acc);
        } else {
            lsum -= lsum;       // +0; a NaN stays
        }
    }
    __shared__ float wave_part[kPoseWaves];
    __shared__ int wild;        // a wave sum was NaN or beyond kPoseWaveLimit
    lsum = wave_sum(lsum);
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = lsum;
    if (threadIdx.x == 0) wild = 0;
    __syncthreads();        // the workgroup's sums stand in LDS
    unsigned long long *__restrict__ accum = ws + (kLossSlots + 1);
    for (int i = threadIdx.x; i < n_sums; i += kLossThreads) {
        long long sum = 0;
        bool sane = true;
#pragma unroll
        for (int w = 0; w < kPoseWaves; ++w) {
            const float v = sums[w * row_words + kPoseSpill + i] * per_count;
            const bool ok = fabsf(v) <= kPoseWaveLimit;         // false for NaN
            sane = sane && ok;
            sum += ok ? (long long)v : 0LL;
        }
        if (!sane) wild = 1;
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
        for (int w = 0; w < kPoseWaves; ++w) t += wave_part[w];
        if (wild) t = __builtin_nanf("");
        finished = loss_arrive(t, fixed_scale, loss_scale, ws, loss_out);
    }
    finished = __builtin_amdgcn_readfirstlane(finished);
    if (finished == 0) return;
    // the finisher: every workgroup's adds returned before it arrived, and its arrival before the finisher's own returned
    const int n_all = (int)gridDim.y * n_sums;
    for (int i = threadIdx.x; i < n_all; i += 64) {
        const unsigned long long sum = __hip_atomic_exchange(&accum[i], 0ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        float gr = (float)((double)(long long)sum * grad_scale);
        if (i % 9 >= 6) gr *= rcp_(scenes[i]);       // the colour columns hold sum(Q): d / d colour = Q / colour
        grad_scenes[i] = finished == 2 ? __builtin_nanf("") : gr;
    }
}

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

constexpr size_t kPoseLdsMax = 60 * 1024;

// Argument checks (all before the launch, in the exposure entries' order and with their codes), plan_loss's grid and
// fixed-point scale, the launch.
int pose_impl(const char *who, bool head, const float *input, const float *photos, const float *weights, int weight_planes,
              const float *scenes, const float *xrow, float eps, float *loss_out, float *grad_input, float *grad_scenes,
              void *workspace, size_t workspace_bytes, int B, int S, int H, int W, void *stream)
{
    char text[200];
    const auto bad = [&](int code, const char *what) {
        std::snprintf(text, sizeof(text), "%s: %s", who, what);
        return fail(code, text);
    };
    LossPlan p;
    if (!grad_input) return fail(SVBRDF_ERR_NULL, who);      // forward + adjoint only
    if (int e = plan_loss(who, false, {input, photos, grad_scenes, scenes, xrow, loss_out}, grad_input, workspace,
                          workspace_bytes, "eps", eps, 0.0f, B, S, H, W, &p)) return e;
    if (!aligned(weights, 4)) return bad(SVBRDF_ERR_ALIGN, "pointers must be 4-byte aligned");
    if (weights ? (weight_planes != 1 && weight_planes != S) : weight_planes != 0)
        return bad(SVBRDF_ERR_DIMS, "weight_planes must be 1 (one plane per item) or S (one per photo) with weights, 0 without");
    if (workspace_bytes < svbrdf_photo_scene_grad_workspace_bytes(B, S, H, W)) return bad(SVBRDF_ERR_WORKSPACE, "workspace too small");
    const size_t lds_bytes = (size_t)kPoseWaves * (kPoseSpill + (size_t)S * 9) * sizeof(float);
    if (lds_bytes > kPoseLdsMax) return bad(SVBRDF_ERR_DIMS, "too many scenes per item for the LDS sums (max 425)");
    const double count = (double)B * S * 3.0 * (double)H * W;
    const auto kernel = head ? (weights ? k_pose_head_weighted : k_pose_head) : (weights ? k_pose_maps_weighted : k_pose_maps);
    hipLaunchKernelGGL(kernel, p.grid, dim3(kLossThreads), lds_bytes, static_cast<hipStream_t>(stream), input, photos,
                       weights, weight_planes, scenes, xrow, eps, p.inv_count, p.loss_scale, p.fixed_scale,
                       1.0 / (count * (double)kPoseFixedScale), (float)(count * (double)kPoseFixedScale), grad_input,
                       grad_scenes, p.ws, loss_out, S, H, W);
    return launch_status(who);
}

}  // namespace

extern "C" {

size_t svbrdf_photo_scene_grad_workspace_bytes(int B, int S, int H, int W)
{
    const size_t sums = (B > 0 && S > 0) ? (size_t)B * (size_t)S * 9 : 0;
    return svbrdf_rendering_loss_workspace_bytes(B, S, H, W) + sums * sizeof(unsigned long long);
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
