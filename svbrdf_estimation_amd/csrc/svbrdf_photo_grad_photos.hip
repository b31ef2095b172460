// svbrdf_photo_grad_photos.hip -- translation unit of libsvbrdf_hip.so: the fused photo losses with the GRADIENT TOWARDS THE
// PHOTOGRAPHS in the one launch (added to ABI version 8 without a bump).
//
//   L = (1/N) sum w | log(render(scene[b,s], input[b]) + eps) - log(p' + eps) |,   delta = log(render + eps) - log(p' + eps)
//   dL/dphoto[b,s,c,i,j] = -(w/N) sign(delta) / (photo + eps)
//
// What capture.rectify's gradient entries take as their upstream gradient: with it the homographies and the lens of a
// capture sit in one autograd graph with the maps, and the registration stage optimises the loss the maps are fitted with.
// The sign is the `lg` the loss and the map adjoint of the same launch hold; the magnitude is one IEEE division per channel
// (photo_grad_store of svbrdf_photo_loss_device.h); the layout is the photos' own, so the store reuses the photo load's
// offsets on another base, which follows the photos' base one pass behind (photo_scene_loop).  Loss and map gradient are
// bit for bit those of the kernels of svbrdf_photo_loss.hip: the same device functions with PGRAD set, nothing reordered.
//
// Eight kernels, {maps, head} x {unweighted, weighted} x {forward + adjoint, forward only}, scene table in device memory.
// The forward-only form -- loss + grad_photos, table staged in LDS -- is what a registration stage launches: the maps are
// constants there.  A unit of its own so that no earlier unit's machine code moves with it.
#include "svbrdf_photo_loss_device.h"

namespace {

// One thread = one pixel, all S renders of it; workgroup = 256 pixels of one item: photo_loss_body<WITH_GRAD, false, HEAD,
// WEIGHTED>'s flow -- the set-up of a pixel (wave_pixel_setup: that body's statements; what prepare<true> forms beyond
// prepare<false> is dead in the forward-only kernels), the scene loops with PGRAD set and the base of the item's gradient
// planes, the map gradient's stores, the loss reduction -- so the loss and the map gradient are that body's bit for bit.
// A lane without a pixel stores nothing: it does not enter the loop.
template <bool WITH_GRAD, bool HEAD, bool WEIGHTED>
__device__ __forceinline__ void photo_grad_body(const float *__restrict__ input, const float *__restrict__ photos,
                                                const float *__restrict__ weights, int weight_planes,
                                                const float *__restrict__ scenes, const float *__restrict__ xrow, float eps,
                                                float inv_count, double loss_scale, float fixed_scale,
                                                float *__restrict__ grad_input, float *__restrict__ grad_photos,
                                                unsigned long long *__restrict__ ws, float *__restrict__ loss_out, int S,
                                                int H, int W)
{
    extern __shared__ __attribute__((aligned(16))) float sc_lds[];      // [S][9], forward-only kernels
    const size_t plane = (size_t)H * W;
    const size_t pix = (size_t)blockIdx.x * kLossThreads + threadIdx.x;
    const int b = blockIdx.y;
    float lsum = 0.0f;
    if (!WITH_GRAD) {
        for (int i = threadIdx.x; i < S * 9; i += kLossThreads) sc_lds[i] = scenes[(size_t)b * S * 9 + i];
        __syncthreads();
    }
    if (pix < plane) {
        PixelSetup ps = wave_pixel_setup<HEAD, WEIGHTED>(input, xrow, b, plane, pix, W);
        const float *__restrict__ scp = scenes + (size_t)b * S * 9;
        const float *__restrict__ pp = photos + (size_t)b * S * 3 * plane;
        float *__restrict__ gp = grad_photos + (size_t)b * S * 3 * plane;
        const float *__restrict__ wp = WEIGHTED ? weights + (size_t)b * weight_planes * plane : nullptr;
        const size_t wstride = weight_planes == 1 ? 0 : plane;
        constexpr int kDefer = WITH_GRAD ? 7 : 0;
        if (HEAD || __all(ps.tied))     // wave-uniform
            lsum = photo_scene_loop<1, WITH_GRAD, kDefer, WEIGHTED, false, true>(ps.mi, ps.x, ps.y, scp, sc_lds, pp, plane, pix, S,
                                                                                 eps, inv_count, ps.acc, wp, wstride, ps.poison,
                                                                                 nullptr, nullptr, gp);
        else
            lsum = photo_scene_loop<3, WITH_GRAD, kDefer & 3, WEIGHTED, false, true>(ps.mi, ps.x, ps.y, scp, sc_lds, pp, plane, pix,
                                                                                     S, eps, inv_count, ps.acc, wp, wstride,
                                                                                     ps.poison, nullptr, nullptr, gp);
        if (WITH_GRAD) {
            if (HEAD) store_pixel_grad<true>(ps.head, ps.acc, grad_input, b, plane, pix);
            else store_grads_k3(grad_input + (size_t)b * 12 * plane, plane, pix, ps.acc);
        }
    }
    {
        __shared__ float wave_part[kLossThreads / 64];
        lsum = wave_sum(lsum);
        if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = lsum;
        __syncthreads();
        if (threadIdx.x == 0) {
            float t = 0.0f;
#pragma unroll
            for (int w = 0; w < kLossThreads / 64; ++w) t += wave_part[w];
            loss_arrive(t, fixed_scale, loss_scale, ws, loss_out);
        }
    }
}

// (names that hold none of "k_photo_loss", "k_head_photo", "wphoto", "k_exposure": the other photo kernels are counted by those)
#define SVBRDF_PGRAD_KERNEL(NAME, HEAD, WEIGHTED)                                                                     \
    template <bool WITH_GRAD>                                                                                         \
    __global__ SVBRDF_PHOTO_LOSS_ATTRS void NAME(const float *__restrict__ input, const float *__restrict__ photos,   \
                                                 const float *__restrict__ weights, int weight_planes,                \
                                                 const float *__restrict__ scenes, const float *__restrict__ xrow,    \
                                                 float eps, float inv_count, double loss_scale, float fixed_scale,    \
                                                 float *__restrict__ grad_input, float *__restrict__ grad_photos,     \
                                                 unsigned long long *__restrict__ ws, float *__restrict__ loss_out,   \
                                                 int S, int H, int W)                                                 \
    {                                                                                                                 \
        photo_grad_body<WITH_GRAD, HEAD, WEIGHTED>(input, photos, weights, weight_planes, scenes, xrow, eps,          \
                                                   inv_count, loss_scale, fixed_scale, grad_input, grad_photos, ws,   \
                                                   loss_out, S, H, W);                                                \
    }
SVBRDF_PGRAD_KERNEL(k_pgrad_maps, false, false)
SVBRDF_PGRAD_KERNEL(k_pgrad_maps_weighted, false, true)
SVBRDF_PGRAD_KERNEL(k_pgrad_head, true, false)
SVBRDF_PGRAD_KERNEL(k_pgrad_head_weighted, true, true)
#undef SVBRDF_PGRAD_KERNEL

// The argument checks (plan_loss, with grad_photos among the required pointers; the weights' rules as the exposure and
// scene-gradient entries have them), the grid and the scales, the launch.  All checks come before the launch.
int photo_grad_impl(const char *who, bool head, const float *input, const float *photos, const float *weights,
                    int weight_planes, const float *scenes, const float *xrow, float eps, float *loss_out,
                    float *grad_input, float *grad_photos, void *workspace, size_t workspace_bytes, int B, int S, int H,
                    int W, void *stream)
{
    LossPlan p;
    if (int e = plan_loss(who, false, {input, photos, scenes, xrow, loss_out, grad_photos}, grad_input, workspace,
                          workspace_bytes, "eps", eps, 0.0f, B, S, H, W, &p)) return e;
    if (int e = weights_check(who, weights, weight_planes, S)) return e;
    const auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, p.grid, dim3(kLossThreads), p.lds_bytes, static_cast<hipStream_t>(stream), input, photos,
                           weights, weight_planes, scenes, xrow, eps, p.inv_count, p.loss_scale, p.fixed_scale, grad_input,
                           grad_photos, p.ws, loss_out, S, H, W);
    };
    if (grad_input) {
        if (head) weights ? launch(k_pgrad_head_weighted<true>) : launch(k_pgrad_head<true>);
        else weights ? launch(k_pgrad_maps_weighted<true>) : launch(k_pgrad_maps<true>);
    } else {
        if (head) weights ? launch(k_pgrad_head_weighted<false>) : launch(k_pgrad_head<false>);
        else weights ? launch(k_pgrad_maps_weighted<false>) : launch(k_pgrad_maps<false>);
    }
    return launch_status(who);
}

}  // namespace

extern "C" {

int svbrdf_photo_loss_photo_grad_fwd_bwd(const float *input, const float *photos, const float *weights, int weight_planes,
                                         const float *scenes, const float *xrow, float eps, float *loss_out,
                                         float *grad_input, float *grad_photos, void *workspace, size_t workspace_bytes,
                                         int B, int S, int H, int W, void *stream)
{
    return photo_grad_impl("photo_loss_photo_grad", false, input, photos, weights, weight_planes, scenes, xrow, eps, loss_out,
                           grad_input, grad_photos, workspace, workspace_bytes, B, S, H, W, stream);
}

int svbrdf_head_photo_loss_photo_grad_fwd_bwd(const float *encoded9, const float *photos, const float *weights,
                                              int weight_planes, const float *scenes, const float *xrow, float eps,
                                              float *loss_out, float *grad_encoded9, float *grad_photos, void *workspace,
                                              size_t workspace_bytes, int B, int S, int H, int W, void *stream)
{
    return photo_grad_impl("head_photo_loss_photo_grad", true, encoded9, photos, weights, weight_planes, scenes, xrow, eps,
                           loss_out, grad_encoded9, grad_photos, workspace, workspace_bytes, B, S, H, W, stream);
}

}  // extern "C"
