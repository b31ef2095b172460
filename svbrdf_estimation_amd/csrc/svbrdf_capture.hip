// svbrdf_capture.hip -- translation unit of libsvbrdf_hip.so: captured photographs onto the patch grid (ABI version 8).
//
// The photo losses and the photo fit take their photographs as [B,S,3,H,W] float32, linear, on the patch's orthographic
// pixel grid, with a {0,1} confidence plane beside them.  A captured photograph is a perspective image, usually 8-bit and
// gamma encoded, much larger than the grid, with clipped highlights and pixels that fall outside the patch.  One launch of
// k_rectify resamples P source photographs through a 3x3 homography each onto a destination grid with bilinear taps,
// decodes 8-bit codes through a 256-entry table, and writes the three value planes and the confidence plane.  Run with the
// inverse matrix the same kernel is the reference's rendering-to-perspective mapping (OrthoToPerspectiveMapping.apply,
// renderers.py:171-173: cv2.warpPerspective with a constant zero border).
//
// Definition (include/svbrdf_hip.h has it in full; tests/capture_checks.py restates it in numpy float32, and the kernel
// equals that restatement bit for bit).  M = m0..m8, row-major float32, sends a DESTINATION pixel index (x, y, 1) to
// SOURCE pixel-index coordinates; integer coordinates are pixel centres.  Per sub-sample (i, j) of K x K:
//     xs = x + ((i + 0.5)/K - 0.5)            ys likewise                     (the offsets are exact)
//     X = (m0 xs + m1 ys) + m2,  Y = (m3 xs + m4 ys) + m5,  Z = (m6 xs + m7 ys) + m8
//     u = X / Z,  v = Y / Z
//     valid  <=>  Z > 0  and  0 <= u <= Ws-1  and  0 <= v <= Hs-1             (false for NaN)
//     x0 = floor(u), fx = u - x0, x1 = min(x0 + 1, Ws-1); taps a = (y0,x0), b = (y0,x1), c = (y1,x0), d = (y1,x1)
//     top = a + fx (b - a),  bot = c + fx (d - c),  val = top + fy (bot - top)
// A pixel's value is the sum of its sub-samples in (j, i) row-major order times 1/K^2; one invalid sub-sample -- by
// geometry or by a tap that is not finite or beyond the clip thresholds -- makes the pixel's three values and its weight 0.
//
// Arithmetic.  Every operation above is ONE individually rounded float32 operation: the unit is built with the Makefile's
// HIPFLAGS (-ffp-contract=off: no FMA is formed; -fno-fast-math), and no fmaf() is written here.  The two quotients are the
// language's plain `/`: hipcc's default for float division is the correctly rounded IEEE sequence (v_div_scale /
// v_div_fmas / v_div_fixup, denormals kept), which the flags above leave in place -- div_rn of svbrdf_device.h is NOT
// used: it is exact only for operands of moderate magnitude, and M is the caller's.  tests/test_capture_cpu.py holds the
// compiled kernels to that (two v_div_fixup_f32 per sub-sample, no v_fma / v_mad / v_rcp-only quotient).
//
// Addressing.  u and v are clamped IN FLOAT to [0, Ws-1] x [0, Hs-1] (fmaxf / fminf return the other operand for a NaN
// and saturate +-inf) BEFORE the conversion to int, and an invalid sub-sample addresses texel (0, 0): every load address
// lies inside the source whatever M holds.  Threads beyond the destination store nothing.
//
// Shape of a launch.  One workgroup of 256 threads covers a 64 x 4 tile of one photo's destination: a wave is 64
// consecutive pixels of ONE row, so each of its four stores (three value planes, the weight plane) is one contiguous
// 256-byte row segment.  The photo index is blockIdx.z; its nine matrix entries are wave-uniform loads from the [P,9]
// table (scalar loads; nothing is stored through the scalar unit).  The uint8 kernels stage the 256-entry table in LDS once
// per workgroup (1 KiB).  Neighbouring destination pixels hit neighbouring source texels, so the gather leans on L2: the
// source is not tiled through LDS.  No atomics, no scratch, no second pass.  It includes svbrdf_host.h for the
// host-side helpers (fail, aligned, launch_status).
//
// Where each statement lives.  svbrdf_capture_device.h holds every statement above once, as functions that k_rectify and
// k_lens_grad call: xs, ys (rectify_sub); X .. v (rectify_point); valid (rectify_pinhole_cell); the clamp, x0 .. y1 and the
// fractions (rectify_cell); the taps and the tap rule (rectify_taps, rectify_tap, rectify_index); top, bot, val and the sum
// (rectify_accumulate); the 1/K^2 and the four stores (rectify_store); the tile set-up, the launch shape, the dispatch and
// the argument checks.  k_rectify below is the sub-sample loop around them.
#include "svbrdf_host.h"
#include "svbrdf_capture_device.h"

namespace {

template <bool U8, int K>
__global__ __launch_bounds__(kRectifyBlock) void k_rectify(
    const void *__restrict__ src, const float *__restrict__ matrices, const float *__restrict__ lut, RectifyClip clip,
    float *__restrict__ out, float *__restrict__ weights_out, int Hs, int Ws, int Hd, int Wd)
{
    __shared__ float s_lut[U8 ? 256 : 1];
    const RectifyTile t = rectify_tile<U8>(lut, s_lut, Hd, Wd);
    if (!t.live) return;                            // (behind the barrier)
    float m[9];
    rectify_matrix_row(matrices, t.p, m);
    const RectifySource s = rectify_source(src, s_lut, clip, t.p, Hs, Ws);
    float acc[3] = {0.0f, 0.0f, 0.0f};
    bool ok = true;
#pragma unroll
    for (int j = 0; j < K; ++j) {
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const RectifyPoint q = rectify_point(m, rectify_sub<K>(t.x, i), rectify_sub<K>(t.y, j));
            rectify_accumulate<U8>(s, rectify_pinhole_cell(q, Hs, Ws), i == 0 && j == 0, ok, acc);
        }
    }
    rectify_store<K>(t, ok, acc, out, weights_out, Hd, Wd);
}

}  // namespace

extern "C" {

int svbrdf_rectify_photos(const void *src, int src_format, int P, int Hs, int Ws, const float *matrices, int Hd, int Wd,
                          int k, const float *lut, float clip_lo, float clip_hi, float *out, float *weights_out,
                          void *stream)
{
    const char *who = "svbrdf_rectify_photos";
    const int rc = rectify_check(who, "out", src, src_format, P, Hs, Ws, matrices, Hd, Wd, k, lut, clip_lo, clip_hi, out,
                                 weights_out);
    if (rc) return rc;
    const RectifyClip clip = rectify_clip(clip_lo, clip_hi);
    const dim3 grid = rectify_grid(P, Hd, Wd);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    rectify_dispatch(src_format, k, [&](auto u8, auto kk) {
        k_rectify<decltype(u8)::value, decltype(kk)::value><<<grid, kRectifyBlock, 0, st>>>(src, matrices, lut, clip, out,
                                                                                            weights_out, Hs, Ws, Hd, Wd);
    });
    return launch_status(who);
}

}  // extern "C"
