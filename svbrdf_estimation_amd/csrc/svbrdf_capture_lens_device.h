// svbrdf_capture_lens_device.h -- what the two lens units share: svbrdf_capture_lens.hip (k_lens_rectify) and
// svbrdf_capture_lens_grad.hip (k_lens_grad).  The forward distortion model (ideal pixel -> distorted pixel, OpenCV's
// fx, fy, cx, cy, k1, k2, p1, p2, k3: a closed-form polynomial, nothing to iterate) between the homography's quotients and
// the tap cell: the lens row, the polynomial with mono, and the lens pointer's checks.  include/svbrdf_hip.h has the
// definition in full.  Everything else of the gather -- the quotients, the cell, the taps, the launch shape and the argument
// checks -- is svbrdf_capture_device.h's, which the including unit has in front together with svbrdf_host.h.  No kernel and
// no entry point.
#ifndef SVBRDF_CAPTURE_LENS_DEVICE_H
#define SVBRDF_CAPTURE_LENS_DEVICE_H

namespace {

// One photo's lens row and what depends on it alone (wave-uniform): each product is one rounded float32 operation.
struct RectifyLens {
    float fx, fy, cx, cy, k1, k2, p1, p2, k3;
    float k1_3, k2_5, k3_7;         // 3 k1, 5 k2, 7 k3: the coefficients of d(r rad)/dr
    bool focal;                     // fx > 0 and fy > 0
};

__device__ __forceinline__ RectifyLens rectify_lens_row(const float *__restrict__ lens, int p)
{
    const float *l = lens + (size_t)p * 9;
    RectifyLens L;
    L.fx = l[0];
    L.fy = l[1];
    L.cx = l[2];
    L.cy = l[3];
    L.k1 = l[4];
    L.k2 = l[5];
    L.p1 = l[6];
    L.p2 = l[7];
    L.k3 = l[8];
    L.k1_3 = 3.0f * L.k1;
    L.k2_5 = 5.0f * L.k2;
    L.k3_7 = 7.0f * L.k3;
    L.focal = (L.fx > 0.0f) & (L.fy > 0.0f);
    return L;
}

// The lens map of one sub-sample, between the quotients (svbrdf_capture_device.h: rectify_point) and the tap cell, one rounded
// float32 operation each: xn .. vd, and `valid` with mono's sign in it.  The cell is rectify_cell's at (ud, vd), so every
// index lies in the source whatever the matrix and the lens hold.
struct RectifyLensPoint {
    float xn, yn, xx, yy, r2, rad, t, xd, yd, ud, vd;
    bool valid;
};

__device__ __forceinline__ RectifyLensPoint rectify_lens_map(const RectifyPoint &q, const RectifyLens &L, int Hs, int Ws)
{
    const float wmax = (float)(Ws - 1), hmax = (float)(Hs - 1);
    RectifyLensPoint g;
    g.xn = (q.u - L.cx) / L.fx;
    g.yn = (q.v - L.cy) / L.fy;
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
    g.valid = L.focal & (q.Z > 0.0f) & (mono > 0.0f) & (g.ud >= 0.0f) & (g.ud <= wmax) & (g.vd >= 0.0f) & (g.vd <= hmax);
    return g;
}

// the lens pointer's checks, behind rectify_check's: 0, or the error code with its text set
inline int rectify_lens_check(const char *who, const float *lens)
{
    char text[200];
    if (!lens) {
        std::snprintf(text, sizeof(text), "%s: lens is required (the null lens is 1, 1, 0, 0, 0, 0, 0, 0, 0)", who);
        return fail(SVBRDF_ERR_NULL, text);
    }
    if (!aligned(lens, 4)) {
        std::snprintf(text, sizeof(text), "%s: lens must be 4-byte aligned", who);
        return fail(SVBRDF_ERR_ALIGN, text);
    }
    return 0;
}

}  // namespace

#endif  // SVBRDF_CAPTURE_LENS_DEVICE_H
