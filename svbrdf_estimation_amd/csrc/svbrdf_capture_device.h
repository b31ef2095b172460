// svbrdf_capture_device.h -- what the two capture units share: svbrdf_capture.hip (k_rectify, which describes the
// definition) and svbrdf_capture_grad.hip (k_homography_grad, its gradient towards the matrices).  The launch shape, the tap
// rule, the entries' argument checks, and -- as functions that k_homography_grad calls -- a sub-sample's geometry with the
// clamped-in-float addressing and a tap's index.  k_rectify keeps its own statements of those two: its six kernels' machine
// code moves when they go behind a function (profiles/r23_capture_grad_codehash.txt), and it is the text that describes
// the definition.  No kernel and no entry point.  The including unit has svbrdf_host.h in front (fail, aligned).
#ifndef SVBRDF_CAPTURE_DEVICE_H
#define SVBRDF_CAPTURE_DEVICE_H

namespace {

constexpr int kRectifyTileW = 64;       // one wave = one row segment
constexpr int kRectifyTileH = 4;        // four waves per workgroup
constexpr int kRectifyMaxDim = 32768;   // Hs, Ws, Hd, Wd: (float)(Ws - 1) is exact and every index fits an int

struct RectifyClip {
    float lo_f, hi_f;       // float sources: a tap is invalid at or below lo_f, at or above hi_f, or if not finite
    int lo_i, hi_i;         // uint8 sources: the same thresholds as integers (floor(lo), ceil(hi), within [-1, 256])
};

// one tap of one channel -> its value, and `ok` cleared if the tap rule refuses it
template <bool U8>
__device__ __forceinline__ float rectify_tap(const void *src, size_t index, const float *s_lut, const RectifyClip &clip,
                                             bool &ok)
{
    if (U8) {
        const int code = static_cast<const unsigned char *>(src)[index];
        ok = ok && code > clip.lo_i && code < clip.hi_i;
        return s_lut[code];
    }
    const float t = static_cast<const float *>(src)[index];
    // (t > -inf and t < +inf already refuse NaN and the infinities; the finiteness test is written out for thresholds
    // that are themselves finite on one side only)
    ok = ok && t > clip.lo_f && t < clip.hi_f && fabsf(t) < __builtin_inff();
    return t;
}

// index of channel ch of texel (yy, xx); `base`: first element of the photo in either layout, `plane` = Hs * Ws
template <bool U8>
__device__ __forceinline__ size_t rectify_index(size_t base, size_t plane, int Ws, int yy, int xx, int ch)
{
    if (U8) return base + ((size_t)yy * Ws + xx) * 3 + ch;      // [P,Hs,Ws,3]
    return (base + ch * plane) + (size_t)yy * Ws + xx;          // [P,3,Hs,Ws]
}

// One sub-sample at (xs, ys) through m0..m8: the statements of k_rectify from X to the tap cell, one rounded float32
// operation each, in k_rectify's order.  u and v
// are the quotients as they are; the cell and the fractions come from their clamped copies, so every index lies in
// the source whatever the matrix holds.
struct RectifyCell {
    float Z, u, v, fx, fy;
    int x0, y0, x1, y1;
    bool valid;
};

__device__ __forceinline__ RectifyCell rectify_cell(const float m[9], float xs, float ys, int Hs, int Ws)
{
    const float wmax = (float)(Ws - 1), hmax = (float)(Hs - 1);
    RectifyCell g;
    const float X = (m[0] * xs + m[1] * ys) + m[2];
    const float Y = (m[3] * xs + m[4] * ys) + m[5];
    g.Z = (m[6] * xs + m[7] * ys) + m[8];
    g.u = X / g.Z;
    g.v = Y / g.Z;
    g.valid = g.Z > 0.0f && g.u >= 0.0f && g.u <= wmax && g.v >= 0.0f && g.v <= hmax;
    float u = g.valid ? g.u : 0.0f;
    float v = g.valid ? g.v : 0.0f;
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

// The argument checks of svbrdf_rectify_photos and svbrdf_rectify_photos_grad_matrices, before any launch: `out` is the
// entry's required output, `aux` its optional or second float pointer (NULL passes).  0, or the error code with its text set.
inline int rectify_check(const char *who, const char *out_name, const void *src, int src_format, int P, int Hs, int Ws,
                         const float *matrices, int Hd, int Wd, int k, const float *lut, float clip_lo, float clip_hi,
                         const void *out, const void *aux)
{
    char text[200];
    const auto bad = [&](int code, const char *what) {
        std::snprintf(text, sizeof(text), "%s: %s", who, what);
        return fail(code, text);
    };
    if (src_format != SVBRDF_RECTIFY_F32_PLANAR && src_format != SVBRDF_RECTIFY_U8_INTERLEAVED)
        return bad(SVBRDF_ERR_DIMS, "src_format must be SVBRDF_RECTIFY_F32_PLANAR (0) or SVBRDF_RECTIFY_U8_INTERLEAVED (1)");
    const bool u8 = src_format == SVBRDF_RECTIFY_U8_INTERLEAVED;
    if (!src || !matrices || !out) {
        char what[96];
        std::snprintf(what, sizeof(what), "src, matrices and %s are required", out_name);
        return bad(SVBRDF_ERR_NULL, what);
    }
    if (u8 && !lut) return bad(SVBRDF_ERR_NULL, "uint8 sources need the 256-entry lut");
    if (k != 1 && k != 2 && k != 4) return bad(SVBRDF_ERR_DIMS, "k must be 1, 2 or 4 (k x k sub-samples per pixel)");
    if (P < 1 || Hs < 1 || Ws < 1 || Hd < 1 || Wd < 1) return bad(SVBRDF_ERR_DIMS, "P, Hs, Ws, Hd, Wd must be at least 1");
    if (P > 65535) return bad(SVBRDF_ERR_DIMS, "P exceeds 65535 (grid.z)");
    if (Hs > kRectifyMaxDim || Ws > kRectifyMaxDim || Hd > kRectifyMaxDim || Wd > kRectifyMaxDim)
        return bad(SVBRDF_ERR_DIMS, "Hs, Ws, Hd, Wd must not exceed 32768");
    if (clip_lo != clip_lo || clip_hi != clip_hi) return bad(SVBRDF_ERR_DIMS, "clip_lo and clip_hi must not be NaN");
    if (!aligned(matrices, 4) || !aligned(out, 4) || !aligned(aux, 4) || !aligned(lut, 4) || (!u8 && !aligned(src, 4)))
        return bad(SVBRDF_ERR_ALIGN, "float pointers must be 4-byte aligned");
    return 0;
}

inline RectifyClip rectify_clip(float clip_lo, float clip_hi)
{
    RectifyClip clip;
    clip.lo_f = clip_lo;
    clip.hi_f = clip_hi;
    // code <= clip_lo <=> code <= floor(clip_lo), code >= clip_hi <=> code >= ceil(clip_hi), for integer codes: exact
    clip.lo_i = (int)std::floor(std::fmin(std::fmax((double)clip_lo, -1.0), 256.0));
    clip.hi_i = (int)std::ceil(std::fmin(std::fmax((double)clip_hi, -1.0), 256.0));
    return clip;
}

inline dim3 rectify_grid(int P, int Hd, int Wd)
{
    return dim3((unsigned)((Wd + kRectifyTileW - 1) / kRectifyTileW), (unsigned)((Hd + kRectifyTileH - 1) / kRectifyTileH),
                (unsigned)P);
}

}  // namespace

#endif  // SVBRDF_CAPTURE_DEVICE_H
