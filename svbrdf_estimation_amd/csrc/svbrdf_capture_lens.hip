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

template <bool U8>
void launch_rectify_lens(int k, dim3 grid, hipStream_t st, const void *src, const float *matrices, const float *lens,
                         const float *lut, RectifyClip clip, float *out, float *weights_out, int Hs, int Ws, int Hd, int Wd)
{
    const dim3 block(kRectifyTileW * kRectifyTileH);
    if (k == 1)
        k_lens_rectify<U8, 1><<<grid, block, 0, st>>>(src, matrices, lens, lut, clip, out, weights_out, Hs, Ws, Hd, Wd);
    else if (k == 2)
        k_lens_rectify<U8, 2><<<grid, block, 0, st>>>(src, matrices, lens, lut, clip, out, weights_out, Hs, Ws, Hd, Wd);
    else
        k_lens_rectify<U8, 4><<<grid, block, 0, st>>>(src, matrices, lens, lut, clip, out, weights_out, Hs, Ws, Hd, Wd);
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
    const bool u8 = src_format == SVBRDF_RECTIFY_U8_INTERLEAVED;
    const RectifyClip clip = rectify_clip(clip_lo, clip_hi);
    const dim3 grid = rectify_grid(P, Hd, Wd);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (u8) launch_rectify_lens<true>(k, grid, st, src, matrices, lens, lut, clip, out, weights_out, Hs, Ws, Hd, Wd);
    else launch_rectify_lens<false>(k, grid, st, src, matrices, lens, lut, clip, out, weights_out, Hs, Ws, Hd, Wd);
    return launch_status(who);
}

}  // extern "C"
