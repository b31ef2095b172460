// svbrdf_capture_lens_grad.hip -- translation unit of libsvbrdf_hip.so: the gradient of svbrdf_rectify_photos_lens' values
// towards the 3x3 matrices, THROUGH the lens's Jacobian, and towards the nine lens entries, ONE launch (ABI version 8).
//
// Refining a registration photometrically under a lens needs d loss / d M through the distortion, and a lens coefficient can
// be refined the same way (one coefficient per stage: k1 and k2 trade off against each other on a patch that covers the
// middle of the frame).  k_lens_grad repeats the forward's gather (the same geometry, lens map, clamped
// addressing and tap rule) and reduces eighteen terms per sub-sample to eighteen floats
// per photo.
//
// Definition (include/svbrdf_hip.h has it in full; tests/capture_lens_checks.py restates it in numpy float32).  Everything
// up to the taps and the pixel's `ok` is the forward's.  The gradient is that of the forward's expression with the cell,
// `valid` (mono's sign included) and `ok` held constant.  With g_ch = grad_values[p, ch, y, x], per sub-sample, every line
// ONE individually rounded float32 operation (HIPFLAGS: -ffp-contract=off; no fused multiply-add written; IEEE `/`):
//     gud, gvd: svbrdf_capture_grad.hip's gu, gv, formed at the cell of (ud, vd)
//     a = gud fx;  b = gvd fy;  q = k1 + (r2 ((2 k2) + ((3 k3) r2)))
//     jxx = ((rad + ((2 xx) q)) + ((2 p1) yn)) + ((6 p2) xn)
//     jxy = ((t q) + ((2 p1) xn)) + ((2 p2) yn)
//     jyy = ((rad + ((2 yy) q)) + ((6 p1) yn)) + ((2 p2) xn)
//     gxn = (a jxx) + (b jxy);  gyn = (a jxy) + (b jyy);  gu = gxn / fx;  gv = gyn / fy
//     rz = 1 / Z;  pu = gu rz;  pv = gv rz;  pz = -((pu u) + (pv v))
//     matrix terms:  pu xs, pu ys, pu,  pv xs, pv ys, pv,  pz xs, pz ys, pz
//     s = (a xn) + (b yn);  s1 = s r2;  s2 = s1 r2;  s3 = s2 r2
//     lens terms:    (gud xd) - (gu xn),  (gvd yd) - (gv yn),  gud - gu,  gvd - gv,  s1,  s2,
//                    (a t) + (b (r2 + (2 yy))),  (a (r2 + (2 xx))) + (b t),  s3            (fx fy cx cy k1 k2 p1 p2 k3)
//
// The reduction is k_homography_grad's with eighteen words per workgroup instead of nine: K^2 - 1 thread additions, the
// 64-lane butterfly, (w0 + w1) + (w2 + w3) through LDS, write-through stores of the workgroup's words, a drain, the
// per-photo integer ticket; the last workgroup acquires, adds the partials in float64 in index order, rounds once and
// leaves the workspace zeroed.  No float atomic, no release fence; SVBRDF_RECTIFY_GRAD_DEPTH bounds this sum as the other.
// Here it is rectify_grad_reduce<18> of svbrdf_capture_grad_device.h, which also forms gud, gvd (rectify_grad_taps); the gather
// is svbrdf_capture_device.h's, the lens map svbrdf_capture_lens_device.h's.  The Jacobian and the eighteen terms are
// k_lens_grad's own.
#include "svbrdf_host.h"
#include "svbrdf_capture_device.h"
#include "svbrdf_capture_grad_device.h"
#include "svbrdf_capture_lens_device.h"

namespace {

constexpr int kLensGradWords = 18;                  // nine matrix terms, nine lens terms

template <bool U8, int K>
__global__ __launch_bounds__(kRectifyBlock) void k_lens_grad(
    const void *__restrict__ src, const float *__restrict__ matrices, const float *__restrict__ lens,
    const float *__restrict__ lut, RectifyClip clip, const float *__restrict__ grad_values, float *__restrict__ grad_matrices,
    float *__restrict__ grad_lens, unsigned *tickets, float *partials, int Hs, int Ws, int Hd, int Wd)
{
    constexpr int N = kLensGradWords;
    constexpr int kLut = U8 ? 256 : 0;
    __shared__ float s_words[kLut + kRectifyTileH * N];     // the table, then the four waves' eighteen sums
    const RectifyTile t = rectify_tile<U8>(lut, s_words, Hd, Wd);
    float m[9], g[3];
    rectify_matrix_row(matrices, t.p, m);
    const RectifyLens L = rectify_lens_row(lens, t.p);
    const float k2_2 = 2.0f * L.k2, k3_3 = 3.0f * L.k3;
    const float p1_2 = 2.0f * L.p1, p1_6 = 6.0f * L.p1, p2_2 = 2.0f * L.p2, p2_6 = 6.0f * L.p2;
    const RectifySource photo = rectify_source(src, s_words, clip, t.p, Hs, Ws);
    rectify_grad_values(t, grad_values, Hd, Wd, g);
    float acc[N];
    bool ok = t.live;                               // a thread beyond the destination adds exact zeros
#pragma unroll
    for (int j = 0; j < K; ++j) {
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const float xs = rectify_sub<K>(t.x, i), ys = rectify_sub<K>(t.y, j);
            const RectifyPoint pt = rectify_point(m, xs, ys);
            const RectifyLensPoint c = rectify_lens_map(pt, L, Hs, Ws);
            float gud, gvd;
            rectify_grad_taps<U8, K>(photo, rectify_cell(c.ud, c.vd, c.valid, Hs, Ws), g, ok, gud, gvd);
            const float a = gud * L.fx;
            const float b = gvd * L.fy;
            const float q = L.k1 + (c.r2 * (k2_2 + (k3_3 * c.r2)));
            const float xx2 = 2.0f * c.xx, yy2 = 2.0f * c.yy;
            const float jxx = ((c.rad + (xx2 * q)) + (p1_2 * c.yn)) + (p2_6 * c.xn);
            const float jxy = ((c.t * q) + (p1_2 * c.xn)) + (p2_2 * c.yn);
            const float jyy = ((c.rad + (yy2 * q)) + (p1_6 * c.yn)) + (p2_2 * c.xn);
            const float gxn = (a * jxx) + (b * jxy);
            const float gyn = (a * jxy) + (b * jyy);
            const float gu = gxn / L.fx;
            const float gv = gyn / L.fy;
            const float rz = 1.0f / pt.Z;
            const float pu = gu * rz;
            const float pv = gv * rz;
            const float pz = -((pu * pt.u) + (pv * pt.v));
            const float s = (a * c.xn) + (b * c.yn);
            const float s1 = s * c.r2;
            const float s2 = s1 * c.r2;
            const float s3 = s2 * c.r2;
            const float term[N] = {pu * xs, pu * ys, pu, pv * xs, pv * ys, pv, pz * xs, pz * ys, pz,
                                   (gud * c.xd) - (gu * c.xn), (gvd * c.yd) - (gv * c.yn), gud - gu, gvd - gv, s1, s2,
                                   (a * c.t) + (b * (c.r2 + yy2)), (a * (c.r2 + xx2)) + (b * c.t), s3};
#pragma unroll
            for (int n = 0; n < N; ++n) acc[n] = (i == 0 && j == 0) ? term[n] : acc[n] + term[n];
        }
    }
    float *const rows[2] = {grad_matrices, grad_lens};
    rectify_grad_reduce<N>(t, ok, acc, s_words + kLut, rows, tickets, partials);
}

}  // namespace

extern "C" {

size_t svbrdf_rectify_lens_grad_workspace_bytes(int P, int Hd, int Wd)
{
    return rectify_grad_workspace_bytes(P, Hd, Wd, kLensGradWords);
}

int svbrdf_rectify_photos_lens_grad(const void *src, int src_format, int P, int Hs, int Ws, const float *matrices,
                                    const float *lens, int Hd, int Wd, int k, const float *lut, float clip_lo, float clip_hi,
                                    const float *grad_values, float *grad_matrices, float *grad_lens, void *workspace,
                                    size_t workspace_bytes, void *stream)
{
    const char *who = "svbrdf_rectify_photos_lens_grad";
    int rc = rectify_check(who, "grad_matrices", src, src_format, P, Hs, Ws, matrices, Hd, Wd, k, lut, clip_lo, clip_hi,
                           grad_matrices, grad_values);
    if (rc) return rc;
    rc = rectify_lens_check(who, lens);
    if (rc) return rc;
    rc = rectify_grad_check(who, "svbrdf_rectify_lens_grad_workspace_bytes", true, P, Hd, Wd, kLensGradWords, grad_values,
                            grad_lens, workspace, workspace_bytes);
    if (rc) return rc;
    const RectifyClip clip = rectify_clip(clip_lo, clip_hi);
    const dim3 grid = rectify_grid(P, Hd, Wd);
    unsigned *tickets = rectify_grad_tickets(workspace);
    float *partials = rectify_grad_partials(workspace, P);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    rectify_dispatch(src_format, k, [&](auto u8, auto kk) {
        k_lens_grad<decltype(u8)::value, decltype(kk)::value><<<grid, kRectifyBlock, 0, st>>>(
            src, matrices, lens, lut, clip, grad_values, grad_matrices, grad_lens, tickets, partials, Hs, Ws, Hd, Wd);
    });
    return launch_status(who);
}

}  // extern "C"
