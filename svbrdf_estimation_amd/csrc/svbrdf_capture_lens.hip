// svbrdf_capture_lens.hip -- translation unit of libsvbrdf_hip.so: captured photographs onto the patch grid through a
// homography AND a lens distortion model, ONE launch (ABI version 8).
//
// A homography is exact only for a pinhole camera; a hand-held phone bends straight lines by several pixels towards the
// frame's edge, and no 3x3 matrix absorbs that.  A gather needs the FORWARD model, ideal pixel -> distorted pixel, which is a
// closed-form polynomial (OpenCV's fx, fy, cx, cy, k1, k2, p1, p2, k3): it sits between k_rectify's quotient and its tap cell
// and needs no iteration.  k_lens_rectify is k_rectify with that map in between; with the null lens (1, 1, 0, 0, 0, 0, 0, 0,
// 0) every added statement is exact and the results are k_rectify's bit for bit.
//
// Definition (include/svbrdf_hip.h has it in full; tests/capture_lens_checks.py restates it in numpy float32, and the
// kernel equals that restatement bit for bit).  Per sub-sample, up to u = X / Z, v = Y / Z as svbrdf_capture.hip; then
//     xn = (u - cx) / fx,  yn = (v - cy) / fy,  xx = xn xn,  yy = yn yn,  xy = xn yn,  r2 = xx + yy
//     rad  = 1 + r2 (k1 + r2 (k2 + r2 k3)),   mono = 1 + r2 (3 k1 + r2 (5 k2 + r2 (7 k3)))
//     t = 2 xy,  tx = (p1 t) + (p2 (r2 + 2 xx)),  ty = (p1 (r2 + 2 yy)) + (p2 t)
//     xd = (xn rad) + tx,  yd = (yn rad) + ty,  ud = (xd fx) + cx,  vd = (yd fy) + cy
//     valid  <=>  Z > 0 and fx > 0 and fy > 0 and mono > 0 and 0 <= ud <= Ws-1 and 0 <= vd <= Hs-1     (false for NaN)
// and the cell, the taps, the tap rule, the bilinear value and the sub-sample sum are k_rectify's at (ud, vd).  mono is
// d(r rad)/dr: where it is not positive the radial map has folded back, and a destination pixel outside the camera's view
// would otherwise get a confident, wrong value.
//
// Arithmetic, addressing and the shape of a launch are svbrdf_capture.hip's: the Makefile's HIPFLAGS (-ffp-contract=off), no
// fused multiply-add written here, the four quotients the language's IEEE `/`; ud and vd clamped in float before the
// conversion to int; a 64 x 4 tile per workgroup, the photo in blockIdx.z, the 256-entry table in LDS for uint8 sources; the
// matrix and the lens row are wave-uniform loads.  No atomics, no scratch, no second pass.
#include "svbrdf_host.h"
#include "svbrdf_capture_device.h"
#include "svbrdf_capture_lens_device.h"

namespace {

// k_lens_rectify keeps the body it had before the capture units were put on shared device functions, with its own cell: on
// the shared ones its uint8 k = 1 launch was 0.32 us above the criterion of profiles/r27_capture_refactor.txt.  A change to
// rectify_point, rectify_lens_map or rectify_cell (the shared headers) has to be made here as well.
//
// One sub-sample at (xs, ys) through m0..m8 and the lens: the forward's statements from X to the quotients, the lens map, and
// the tap cell at (ud, vd); one rounded float32 operation each.  Z, u, v are the pinhole quantities as they are; xn .. vd the
// lens map's; the cell and the fractions come from the clamped copies of ud, vd, so every index lies in the source whatever
// the matrix and the lens hold.
struct RectifyLensCell {
    float Z, u, v;
    float xn, yn, xx, yy, r2, rad, t, xd, yd, ud, vd;
    float fx, fy;                   // the bilinear fractions
    int x0, y0, x1, y1;
    bool valid;
};

__device__ __forceinline__ RectifyLensCell rectify_lens_cell(const float m[9], const RectifyLens &L, float xs, float ys, int Hs,
                                                             int Ws)
{
    const float wmax = (float)(Ws - 1), hmax = (float)(Hs - 1);
    RectifyLensCell g;
    const float X = (m[0] * xs + m[1] * ys) + m[2];
    const float Y = (m[3] * xs + m[4] * ys) + m[5];
    g.Z = (m[6] * xs + m[7] * ys) + m[8];
    g.u = X / g.Z;
    g.v = Y / g.Z;
    g.xn = (g.u - L.cx) / L.fx;
    g.yn = (g.v - L.cy) / L.fy;
    g.xx = g.xn * g.xn;
    g.yy = g.yn * g.yn;
    const float xy = g.xn * g.yn;
    g.r2 = g.xx + g.yy;
    g.rad = 1.0f + g.r2 * (L.k1 + g.r2 * (L.k2 + g.r2 * L.k3));
    const float mono = 1.0f + g.r2 * (L.k1_3 + g.r2 * (L.k2_5 + g.r2 * L.k3_7));
    g.t = 2.0f * xy;
    const float tx = (L.p1 * g.t) + (L.p2 * (g.r2 + 2.0f * g.xx));
    const float ty = (L.p1 * (g.r2 + 2.0f * g.yy)) + (L.p2 * g.t);
    g.xd = (g.xn * g.rad) + tx;
    g.yd = (g.yn * g.rad) + ty;
    g.ud = (g.xd * L.fx) + L.cx;
    g.vd = (g.yd * L.fy) + L.cy;
    // (`&`, not `&&`: a wave-uniform operand of `&&` becomes a branch per sub-sample, and behind it the taps of all K^2
    // sub-samples are held in registers to the kernel's end)
    g.valid = L.focal & (g.Z > 0.0f) & (mono > 0.0f) & (g.ud >= 0.0f) & (g.ud <= wmax) & (g.vd >= 0.0f) & (g.vd <= hmax);
    float u = g.valid ? g.ud : 0.0f;
    float v = g.valid ? g.vd : 0.0f;
    u = fminf(fmaxf(u, 0.0f), wmax);        // in float, before the conversion: NaN and +-inf cannot reach it
    v = fminf(fmaxf(v, 0.0f), hmax);
    const float x0f = floorf(u), y0f = floorf(v);
    g.fx = u - x0f;
    g.fy = v - y0f;
    g.x0 = (int)x0f;
    g.y0 = (int)y0f;
    g.x1 = min(g.x0 + 1, Ws - 1);
    g.y1 = min(g.y0 + 1, Hs - 1);
    return g;
}

template <bool U8, int K>
__global__ __launch_bounds__(kRectifyTileW * kRectifyTileH) void k_lens_rectify(
    const void *__restrict__ src, const float *__restrict__ matrices, const float *__restrict__ lens,
    const float *__restrict__ lut, RectifyClip clip, float *__restrict__ out, float *__restrict__ weights_out, int Hs, int Ws,
    int Hd, int Wd)
{
    __shared__ float s_lut[U8 ? 256 : 1];
    if (U8) {
        s_lut[threadIdx.x] = lut[threadIdx.x];      // 256 threads, 256 entries
        __syncthreads();
    }
    const int p = blockIdx.z;
    const int x = blockIdx.x * kRectifyTileW + (threadIdx.x & (kRectifyTileW - 1));
    const int y = blockIdx.y * kRectifyTileH + (threadIdx.x / kRectifyTileW);
    if (x >= Wd || y >= Hd) return;                 // (behind the barrier)
    float m[9];
#pragma unroll
    for (int n = 0; n < 9; ++n) m[n] = matrices[(size_t)p * 9 + n];
    const RectifyLens L = rectify_lens_row(lens, p);
    const size_t plane = (size_t)Hs * Ws;
    const size_t base = (size_t)p * 3 * plane;      // first element of photo p in either layout
    float acc[3] = {0.0f, 0.0f, 0.0f};
    bool ok = true;
#pragma unroll
    for (int j = 0; j < K; ++j) {
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const float xs = (float)x + ((i + 0.5f) / K - 0.5f);        // the offset is a compile-time constant, exact
            const float ys = (float)y + ((j + 0.5f) / K - 0.5f);
            const RectifyLensCell c = rectify_lens_cell(m, L, xs, ys, Hs, Ws);
            ok = ok && c.valid;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float ta = rectify_tap<U8>(src, rectify_index<U8>(base, plane, Ws, c.y0, c.x0, ch), s_lut, clip, ok);
                const float tb = rectify_tap<U8>(src, rectify_index<U8>(base, plane, Ws, c.y0, c.x1, ch), s_lut, clip, ok);
                const float tc = rectify_tap<U8>(src, rectify_index<U8>(base, plane, Ws, c.y1, c.x0, ch), s_lut, clip, ok);
                const float td = rectify_tap<U8>(src, rectify_index<U8>(base, plane, Ws, c.y1, c.x1, ch), s_lut, clip, ok);
                const float top = ta + c.fx * (tb - ta);
                const float bot = tc + c.fx * (td - tc);
                const float val = top + c.fy * (bot - top);
                acc[ch] = (i == 0 && j == 0) ? val : acc[ch] + val;
            }
        }
    }
    const size_t dplane = (size_t)Hd * Wd;
    const size_t pix = (size_t)y * Wd + x;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
        out[((size_t)p * 3 + ch) * dplane + pix] = ok ? acc[ch] * (1.0f / (K * K)) : 0.0f;
    if (weights_out) weights_out[(size_t)p * dplane + pix] = ok ? 1.0f : 0.0f;
}

}  // namespace

extern "C" {

int svbrdf_rectify_photos_lens(const void *src, int src_format, int P, int Hs, int Ws, const float *matrices,
                               const float *lens, int Hd, int Wd, int k, const float *lut, float clip_lo, float clip_hi,
                               float *out, float *weights_out, void *stream)
{
    const char *who = "svbrdf_rectify_photos_lens";
    int rc = rectify_check(who, "out", src, src_format, P, Hs, Ws, matrices, Hd, Wd, k, lut, clip_lo, clip_hi, out, weights_out);
    if (rc) return rc;
    rc = rectify_lens_check(who, lens);
    if (rc) return rc;
    const RectifyClip clip = rectify_clip(clip_lo, clip_hi);
    const dim3 grid = rectify_grid(P, Hd, Wd);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    rectify_dispatch(src_format, k, [&](auto u8, auto kk) {
        k_lens_rectify<decltype(u8)::value, decltype(kk)::value><<<grid, kRectifyBlock, 0, st>>>(
            src, matrices, lens, lut, clip, out, weights_out, Hs, Ws, Hd, Wd);
    });
    return launch_status(who);
}

}  // extern "C"
