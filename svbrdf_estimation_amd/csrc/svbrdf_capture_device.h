// svbrdf_capture_device.h -- what the four capture units share: svbrdf_capture.hip (k_rectify, whose header describes the
// definition), svbrdf_capture_grad.hip (k_homography_grad), svbrdf_capture_lens.hip (k_lens_rectify) and
// svbrdf_capture_lens_grad.hip (k_lens_grad).  Every statement of the gather is written once, here (k_homography_grad and
// k_lens_rectify call the tap rule and the tap index only and keep the rest in their old bodies: their units say why): the tile set-up
// (rectify_tile, rectify_matrix_row, rectify_source), a sub-sample's position and geometry (rectify_sub, rectify_point), the
// clamped-in-float tap cell (rectify_cell), the tap rule and a tap's index (rectify_tap, rectify_index), the forward's tap
// block and epilogue (rectify_accumulate, rectify_store), and on the host the launch shape, the U8 x K dispatch and the
// entries' argument checks.  The lens map is svbrdf_capture_lens_device.h's, the gradient's tap block and its reduction
// svbrdf_capture_grad_device.h's.  No kernel and no entry point.  The including unit has svbrdf_host.h in front (fail, aligned).
#ifndef SVBRDF_CAPTURE_DEVICE_H
#define SVBRDF_CAPTURE_DEVICE_H

#include <type_traits>

namespace {

constexpr int kRectifyTileW = 64;       // one wave = one row segment
constexpr int kRectifyTileH = 4;        // four waves per workgroup
constexpr int kRectifyBlock = kRectifyTileW * kRectifyTileH;
constexpr int kRectifyMaxDim = 32768;   // Hs, Ws, Hd, Wd: (float)(Ws - 1) is exact and every index fits an int

struct RectifyClip {
    float lo_f, hi_f;       // float sources: a tap is invalid at or below lo_f, at or above hi_f, or if not finite
    int lo_i, hi_i;         // uint8 sources: the same thresholds as integers (floor(lo), ceil(hi), within [-1, 256])
};

// A thread's place in the launch: photo p, destination pixel (x, y); `live` is false beyond the destination.
struct RectifyTile {
    int p, x, y, lane, wave;
    bool live;
};

// The tile set-up of every capture kernel: the uint8 kernels stage the 256-entry table in `s_lut` (256 threads, 256
// entries, one barrier -- before any thread leaves), then the thread's place.
template <bool U8>
__device__ __forceinline__ RectifyTile rectify_tile(const float *__restrict__ lut, float *s_lut, int Hd, int Wd)
{
    if (U8) {
        s_lut[threadIdx.x] = lut[threadIdx.x];
        __syncthreads();
    }
    RectifyTile t;
    t.p = blockIdx.z;
    t.lane = threadIdx.x & (kRectifyTileW - 1);
    t.wave = threadIdx.x / kRectifyTileW;
    t.x = blockIdx.x * kRectifyTileW + t.lane;
    t.y = blockIdx.y * kRectifyTileH + t.wave;
    t.live = t.x < Wd && t.y < Hd;
    return t;
}

// photo p's nine matrix entries: wave-uniform loads
__device__ __forceinline__ void rectify_matrix_row(const float *__restrict__ matrices, int p, float (&m)[9])
{
#pragma unroll
    for (int n = 0; n < 9; ++n) m[n] = matrices[(size_t)p * 9 + n];
}

// What a tap needs of photo p: `base` is its first element in either layout, `plane` = Hs * Ws.
struct RectifySource {
    const void *src;
    const float *s_lut;
    RectifyClip clip;
    size_t plane, base;
    int Hs, Ws;
};

__device__ __forceinline__ RectifySource rectify_source(const void *src, const float *s_lut, const RectifyClip &clip, int p,
                                                        int Hs, int Ws)
{
    RectifySource s;
    s.src = src;
    s.s_lut = s_lut;
    s.clip = clip;
    s.plane = (size_t)Hs * Ws;
    s.base = (size_t)p * 3 * s.plane;
    s.Hs = Hs;
    s.Ws = Ws;
    return s;
}

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

// sub-sample i of K along an axis, at pixel index x: the offset is a compile-time constant once unrolled, exact
template <int K>
__device__ __forceinline__ float rectify_sub(int x, int i)
{
    return (float)x + ((i + 0.5f) / K - 0.5f);
}

// One sub-sample at (xs, ys) through m0..m8: X, Y, Z and the two quotients, one rounded float32 operation each.
struct RectifyPoint {
    float Z, u, v;
};

__device__ __forceinline__ RectifyPoint rectify_point(const float (&m)[9], float xs, float ys)
{
    RectifyPoint q;
    const float X = (m[0] * xs + m[1] * ys) + m[2];
    const float Y = (m[3] * xs + m[4] * ys) + m[5];
    q.Z = (m[6] * xs + m[7] * ys) + m[8];
    q.u = X / q.Z;
    q.v = Y / q.Z;
    return q;
}

// The tap cell at (u, v): the cell and the fractions come from the clamped copies of u and v, and an invalid sub-sample
// addresses texel (0, 0), so every index lies in the source whatever the matrix (and the lens) hold.
struct RectifyCell {
    float fx, fy;
    int x0, y0, x1, y1;
    bool valid;
};

// in float, before the conversion to int: fmaxf / fminf return the other operand for a NaN and saturate +-inf
__device__ __forceinline__ float rectify_clamp(float u, float umax) { return fminf(fmaxf(u, 0.0f), umax); }

__device__ __forceinline__ RectifyCell rectify_cell(float u, float v, bool valid, int Hs, int Ws)
{
    RectifyCell g;
    g.valid = valid;
    u = rectify_clamp(valid ? u : 0.0f, (float)(Ws - 1));
    v = rectify_clamp(valid ? v : 0.0f, (float)(Hs - 1));
    const float x0f = floorf(u), y0f = floorf(v);
    g.fx = u - x0f;
    g.fy = v - y0f;
    g.x0 = (int)x0f;
    g.y0 = (int)y0f;
    g.x1 = min(g.x0 + 1, Ws - 1);
    g.y1 = min(g.y0 + 1, Hs - 1);
    return g;
}

// the pinhole's cell: valid  <=>  Z > 0 and (u, v) inside the source (false for NaN).  (`&`, not `&&`, here and in the lens
// map: an operand of `&&` can become a branch per sub-sample, and behind it the taps of all K^2 sub-samples are held in
// registers to the kernel's end.  For the same reason the arrays below are passed as references to arrays.)
__device__ __forceinline__ RectifyCell rectify_pinhole_cell(const RectifyPoint &q, int Hs, int Ws)
{
    const float wmax = (float)(Ws - 1), hmax = (float)(Hs - 1);
    const bool valid = (q.Z > 0.0f) & (q.u >= 0.0f) & (q.u <= wmax) & (q.v >= 0.0f) & (q.v <= hmax);
    return rectify_cell(q.u, q.v, valid, Hs, Ws);
}

// channel ch's four taps of a cell: a = (y0, x0), b = (y0, x1), c = (y1, x0), d = (y1, x1)
template <bool U8>
__device__ __forceinline__ void rectify_taps(const RectifySource &s, const RectifyCell &c, int ch, bool &ok, float &ta,
                                             float &tb, float &tc, float &td)
{
    ta = rectify_tap<U8>(s.src, rectify_index<U8>(s.base, s.plane, s.Ws, c.y0, c.x0, ch), s.s_lut, s.clip, ok);
    tb = rectify_tap<U8>(s.src, rectify_index<U8>(s.base, s.plane, s.Ws, c.y0, c.x1, ch), s.s_lut, s.clip, ok);
    tc = rectify_tap<U8>(s.src, rectify_index<U8>(s.base, s.plane, s.Ws, c.y1, c.x0, ch), s.s_lut, s.clip, ok);
    td = rectify_tap<U8>(s.src, rectify_index<U8>(s.base, s.plane, s.Ws, c.y1, c.x1, ch), s.s_lut, s.clip, ok);
}

// The forward's tap block: a sub-sample's bilinear value per channel, added to `acc` (`first`: it starts the sum).
template <bool U8>
__device__ __forceinline__ void rectify_accumulate(const RectifySource &s, const RectifyCell &c, bool first, bool &ok,
                                                   float (&acc)[3])
{
    ok = ok && c.valid;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float ta, tb, tc, td;
        rectify_taps<U8>(s, c, ch, ok, ta, tb, tc, td);
        const float top = ta + c.fx * (tb - ta);
        const float bot = tc + c.fx * (td - tc);
        const float val = top + c.fy * (bot - top);
        acc[ch] = first ? val : acc[ch] + val;
    }
}

// The forward's epilogue: the pixel's three values (the sum times 1/K^2) and its weight, zeros unless `ok`.
template <int K>
__device__ __forceinline__ void rectify_store(const RectifyTile &t, bool ok, const float (&acc)[3], float *__restrict__ out,
                                              float *__restrict__ weights_out, int Hd, int Wd)
{
    const size_t dplane = (size_t)Hd * Wd;
    const size_t pix = (size_t)t.y * Wd + t.x;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
        out[((size_t)t.p * 3 + ch) * dplane + pix] = ok ? acc[ch] * (1.0f / (K * K)) : 0.0f;
    if (weights_out) weights_out[(size_t)t.p * dplane + pix] = ok ? 1.0f : 0.0f;
}

// The argument checks of the four entries, before any launch: `out` is the entry's required output, `aux` its optional or
// second float pointer (NULL passes).  0, or the error code with its text set.
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

// The one U8 x K dispatch of the four entries: launch(U8, K) gets the source format and the checked k in {1, 2, 4} as
// std::integral_constants, to name its kernel's template arguments with.
template <class Launch>
void rectify_dispatch(int src_format, int k, Launch launch)
{
    const auto with_k = [&](auto u8) {
        if (k == 1) launch(u8, std::integral_constant<int, 1>());
        else if (k == 2) launch(u8, std::integral_constant<int, 2>());
        else launch(u8, std::integral_constant<int, 4>());
    };
    if (src_format == SVBRDF_RECTIFY_U8_INTERLEAVED) with_k(std::true_type());
    else with_k(std::false_type());
}

}  // namespace

#endif  // SVBRDF_CAPTURE_DEVICE_H
