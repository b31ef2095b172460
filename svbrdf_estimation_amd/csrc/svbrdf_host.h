// svbrdf_host.h -- the host side every unit with entry points shares: error reporting, the argument checks, the launch
// shapes and the plan of a fused-loss launch.  One copy per including unit (unnamed namespace).  No kernel, no entry point.
#ifndef SVBRDF_HOST_H
#define SVBRDF_HOST_H
#include "svbrdf_device.h"

// the thread-local error text of svbrdf_last_error() lives in the main unit (svbrdf_main.hip); every other unit
// reports through the same two functions
extern "C" __attribute__((visibility("hidden"))) int svbrdf_internal_fail(int code, const char *what);
extern "C" __attribute__((visibility("hidden"))) int svbrdf_internal_launch_status(const char *what);

namespace {

inline int fail(int code, const char *what) { return svbrdf_internal_fail(code, what); }

// the error reported as "<who>: <what>", who being the entry
inline int fail_as(const char *who, int code, const char *what)
{
    char text[200];
    std::snprintf(text, sizeof(text), "%s: %s", who, what);
    return fail(code, text);
}

inline int check_dims(int B, int S, int H, int W)
{
    if (B <= 0 || S <= 0 || H <= 0 || W <= 0) return fail(SVBRDF_ERR_DIMS, "B, S, H, W must be positive");
    if (H != W) return fail(SVBRDF_ERR_DIMS, "H must equal W (renderers.py:75 transposes the x grid)");
    if (B > 65535) return fail(SVBRDF_ERR_DIMS, "B exceeds 65535 (grid.y)");
    if ((long long)H * W > (1LL << 30)) return fail(SVBRDF_ERR_DIMS, "H*W too large");
    return 0;
}

inline bool aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// widest vector width (<= want) every pointer and the row length allow
inline int pick_vec(int want, int W, std::initializer_list<const void *> ptrs)
{
    int vec = want;
    while (vec > 1) {
        bool ok = (W % vec) == 0;
        for (const void *p : ptrs) ok = ok && (p == nullptr || aligned(p, sizeof(float) * vec));
        if (ok) break;
        vec >>= 1;
    }
    return vec;
}

inline int env_vec(const char *name, int dflt)
{
    const char *e = std::getenv(name);
    if (!e) return dflt;
    const int v = std::atoi(e);
    return (v == 1 || v == 2 || v == 4) ? v : dflt;
}

inline int launch_status(const char *what) { return svbrdf_internal_launch_status(what); }

inline dim3 grid_for(int B, int H, int W, int vec)
{
    const long long plane = (long long)H * W;
    const long long per_block = (long long)kThreads * vec;
    return dim3((unsigned)((plane + per_block - 1) / per_block), (unsigned)B, 1);
}

// What every fused loss (K3 and the photo kernels of svbrdf_photo_loss.hip) needs to launch: one workgroup per 256 pixels
// of one item, the fixed-point scale of the per-workgroup partial sums and the scratch words they are summed in.
struct LossPlan {
    dim3 grid;
    float inv_count;          // 1 / (B S 3 H W)
    double loss_scale;        // fixed-point sum -> mean
    float fixed_scale;        // 2^k
    size_t lds_bytes;         // forward-only kernels stage the scenes in LDS
    unsigned long long *ws;
};

// The argument checks of every fused-loss entry point, in one order, and the plan.  `required`: the 4-byte-aligned
// pointers that must not be null; `grad` may be null (forward only); `eps_name`: what the entry's header calls `eps`
// (for the message).  `l1_weight` widens the worst case of a slot by the
// L1 term's share (0: none).
inline int plan_loss(const char *who, bool scenes_on_host, std::initializer_list<const void *> required,
                     const float *grad, void *workspace, size_t workspace_bytes, const char *eps_name,
                     float eps, float l1_weight, int B, int S, int H, int W, LossPlan *out)
{
    char text[200];
    const auto bad = [&](int code, const char *what) {
        std::snprintf(text, sizeof(text), "%s: %s", who, what);
        return fail(code, text);
    };
    bool null = !workspace, misaligned = !aligned(workspace, 8) || !aligned(grad, 4);
    for (const void *p : required) { null = null || !p; misaligned = misaligned || !aligned(p, 4); }
    if (null) return fail(SVBRDF_ERR_NULL, who);
    if (int e = check_dims(B, S, H, W)) return e;
    if (!(eps >= 1e-9f) || !(eps <= 1e9f)) {
        std::snprintf(text, sizeof(text), "%s: %s must lie in [1e-9, 1e9] (the reference uses 0.1)", who, eps_name);
        return fail(SVBRDF_ERR_DIMS, text);
    }
    if (scenes_on_host && (long long)B * S > SVBRDF_HOST_SCENES_MAX_ROWS)
        return bad(SVBRDF_ERR_DIMS, "B*S exceeds SVBRDF_HOST_SCENES_MAX_ROWS (upload the table and use the device-pointer entry)");
    if (misaligned) return bad(SVBRDF_ERR_ALIGN, "pointers must be 4-byte aligned (workspace 8-byte)");
    if (workspace_bytes < svbrdf_rendering_loss_workspace_bytes(B, S, H, W))
        return bad(SVBRDF_ERR_WORKSPACE, "workspace too small");
    const long long plane = (long long)H * W;
    if (plane > (1LL << 25))
        return bad(SVBRDF_ERR_DIMS, "H*W exceeds 2^25 (one item's 12 planes are addressed with 32-bit byte offsets)");
    out->grid = dim3((unsigned)((plane + kLossThreads - 1) / kLossThreads), (unsigned)B, 1);    // 256 pixels per workgroup
    const double count = (double)B * S * 3.0 * (double)plane;
    out->inv_count = (float)(1.0 / count);
    out->ws = static_cast<unsigned long long *>(workspace);
    // Fixed-point scale 2^k of the per-workgroup partial sums: as fine as 2^-24, coarser only if
    // a slot could otherwise outgrow its 48 bits (|dlog| <= 32 per term is far beyond any
    // radiance this renderer can produce: log(1e13/0.1)).
    int k = 24;
    const double l1_share = 1.0 + 4.0 * std::fabs((double)l1_weight);
    const double worst_per_slot = (count * 32.0 / (double)kLossSlots + 32.0 * kLossThreads * 3 * S) * l1_share;
    while (k > 0 && worst_per_slot * std::ldexp(1.0, k) >= std::ldexp(1.0, kLossCountShift - 1)) --k;
    out->fixed_scale = (float)std::ldexp(1.0, k);
    out->loss_scale = std::ldexp(1.0, -k) / count;
    if ((unsigned long long)out->grid.x * out->grid.y >= (1ULL << 16) * kLossSlots)
        return bad(SVBRDF_ERR_DIMS, "too many workgroups for the arrival counters");
    out->lds_bytes = grad ? 0 : (size_t)S * 9 * sizeof(float);
    if (out->lds_bytes > 60 * 1024) return bad(SVBRDF_ERR_DIMS, "too many scenes per item for the LDS stage (max 1706)");
    return 0;
}

}  // namespace

#endif  // SVBRDF_HOST_H
