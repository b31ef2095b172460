/*
 * svbrdf_hip.h -- C ABI of libsvbrdf_hip.so, the MI355X (gfx950) rendering-loss engine.
 *
 * Drop-in boundary for ONE hot path of mworchel/svbrdf-estimation:
 *     LocalRenderer.render            development/multiImage_pytorch/renderers.py:67-104
 *     RenderingLoss.forward (+autograd backward)
 *                                     development/multiImage_pytorch/losses.py:29-52
 * The reference has no FFI (it is pure PyTorch); the "binding" a maintainer adds is
 * the ctypes stub shown in INTEGRATION.md, which replaces the bodies of those two
 * methods.  Signatures use plain pointers and sizes only -- no torch types.
 *
 * Conventions
 *   - every pointer except `workspace`/`xrow_host` is DEVICE memory owned by the
 *     caller, C-contiguous fp32, 4-byte aligned (16-byte alignment enables the
 *     vectorised path; anything else takes the scalar path -- same results).
 *   - layouts:  maps/input/target/grad  [B,12,H,W]  channel order
 *               normals(0:3) diffuse(3:6) roughness(6:9) specular(9:12)
 *               (utils.py:36-58 pack_svbrdf/unpack_svbrdf)
 *               scenes  [B,S,9] = camera xyz | light xyz | light rgb   per render
 *               (environment.py:4-16 Camera/Light/Scene)
 *               xrow    [W]     = torch.linspace(-1, 1, W)  (renderers.py:73); pixel
 *               (i,j) sits at (xrow[j], -xrow[i], 0) (renderers.py:74-76), so H == W.
 *               renderings / grad_out [B,S,3,H,W]
 *   - the library never allocates, frees or retains device memory and never
 *     synchronises; kernels are enqueued on `stream` (a hipStream_t; NULL = the
 *     default stream) and the call returns immediately.
 *   - return value: 0 success; <0 argument error (-1 null pointer, -2 bad dims or
 *     H != W, -3 misaligned pointer, -4 workspace too small); >0 hipError_t of the
 *     launch.  svbrdf_last_error() gives a thread-local message.
 *   - stateless and re-entrant; results are bitwise run-to-run reproducible (fixed
 *     shape two-stage loss reduction, no float atomics).
 */
#ifndef SVBRDF_HIP_H
#define SVBRDF_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVBRDF_ABI_VERSION 8

#if defined(__GNUC__)
#define SVBRDF_API __attribute__((visibility("default")))
#else
#define SVBRDF_API
#endif

#define SVBRDF_OK 0
#define SVBRDF_ERR_NULL (-1)
#define SVBRDF_ERR_DIMS (-2)
#define SVBRDF_ERR_ALIGN (-3)
#define SVBRDF_ERR_WORKSPACE (-4)

SVBRDF_API int svbrdf_abi_version(void);

/* thread-local, static storage; valid until the next failing call on this thread */
SVBRDF_API const char *svbrdf_last_error(void);

/* Host helper: fills xrow_host[W] (HOST memory) with the bit pattern of
 * torch.linspace(-1, 1, W) as the reference's CPU path produces it
 * (renderers.py:73).  Upload it once per W. */
SVBRDF_API int svbrdf_make_xrow(float *xrow_host, int W);

/* K1 -- replaces LocalRenderer.render (renderers.py:67-104), S scenes per map in
 * one launch: out[b,s] = render(scene[b,s], maps[b]). */
SVBRDF_API int svbrdf_render_fwd(const float *maps, const float *scenes, const float *xrow,
                      float *out, int B, int S, int H, int W, void *stream);

/* K2 -- replaces the autograd graph of render(): grad_maps[b] = sum_s J(b,s)^T
 * grad_out[b,s]; grad_maps is overwritten. */
SVBRDF_API int svbrdf_render_bwd(const float *maps, const float *scenes, const float *xrow,
                      const float *grad_out, float *grad_maps,
                      int B, int S, int H, int W, void *stream);

/* K1 / K2 with the scene rows in HOST memory -- what a reference-shaped `render(scene, svbrdf)` call has: the scene is a
 * Python object (environment.py:4-16) and the reference uploads its three vectors with three synchronous H2D copies per
 * call (renderers.py:79,91,98).  Here the rows travel BY VALUE in the launch's kernel-argument block: one dispatch per
 * call, no copy command, nothing retained past return.  `scenes_host` (HOST pointer) holds
 *     scenes_shared != 0 :  S rows, the SAME scenes for every map   (render's "one scene, B maps", renderers.py:98)
 *     scenes_shared == 0 :  B*S rows, as svbrdf_render_fwd
 * at most svbrdf_host_scenes_max_rows() of them (SVBRDF_ERR_DIMS beyond: upload the table and use the device entry).
 * Same kernel bodies, bitwise the same results as svbrdf_render_fwd / svbrdf_render_bwd on an uploaded table. */
SVBRDF_API int svbrdf_render_fwd_host_scenes(const float *maps, const float *scenes_host, int scenes_shared,
                                             const float *xrow, float *out, int B, int S, int H, int W, void *stream);
SVBRDF_API int svbrdf_render_bwd_host_scenes(const float *maps, const float *scenes_host, int scenes_shared,
                                             const float *xrow, const float *grad_out, float *grad_maps,
                                             int B, int S, int H, int W, void *stream);

/* Ragged forms of K1 / K2 (SURVEY section 8b "arbitrary (map, scene) pairs in one launch"): R renders in all, grouped
 * by map -- the renders of map b are rows offsets[b] .. offsets[b+1]-1 of `scenes` [R,9] and of `out` / `grad_out`
 * [R,3,H,W]; `offsets` is a DEVICE array of B+1 int32 with offsets[0] = 0 and offsets[B] = R (CSR row pointers; a map
 * may have zero renders).  One launch, each map read once, no atomics: bitwise reproducible like the regular forms, of
 * which these are the generalisation (offsets[b] = b*S).  The proposal's per-render `map_index` is this layout's
 * inverse; grouping by map is what lets the backward accumulate in registers instead of with float atomics.
 * svbrdf_render_bwd_ragged overwrites ALL of grad_maps (zeros for a map without renders). */
SVBRDF_API int svbrdf_render_fwd_ragged(const float *maps, const float *scenes, const int *offsets, const float *xrow,
                                        float *out, int B, int R, int H, int W, void *stream);
SVBRDF_API int svbrdf_render_bwd_ragged(const float *maps, const float *scenes, const int *offsets, const float *xrow,
                                        const float *grad_out, float *grad_maps, int B, int R, int H, int W,
                                        void *stream);

/* Bytes of device scratch svbrdf_rendering_loss_fwd_bwd needs for these dims (65 64-bit
 * words: sharded fixed-point loss accumulators with arrival counts, and a tail word that
 * sums the completed ones).  The scratch must be
 * 8-byte aligned and ZERO-INITIALISED ONCE by the caller (hipMemset) before its first use;
 * every completed call leaves it zeroed again, so it can be reused call after call on
 * the same stream.  Do not share one scratch buffer between concurrently running calls. */
SVBRDF_API size_t svbrdf_rendering_loss_workspace_bytes(int B, int S, int H, int W);

/* K3 -- replaces RenderingLoss.forward AND its backward (losses.py:29-52):
 *   loss_out[0] = mean_{b,s,c,i,j} | log(render(input)+eps) - log(render(target)+eps) |
 *   grad_input  = d loss / d input  (for upstream gradient 1.0), or NULL for
 *                 forward-only.
 * A NaN or infinite value anywhere in `input` / `target` (or a radiance beyond any the
 * renderer can produce) gives loss_out[0] = NaN, like the reference's clamp/log chain, and
 * the scratch is still left zeroed for the next call.
 * `scenes` are the light/view samples the caller drew (losses.py:35).  `eps` (losses.py:45:
 * 0.1) must lie in [1e-9, 1e9] (SVBRDF_ERR_DIMS otherwise): the kernel derives the three
 * 1/(render+eps) of a pixel from one reciprocal of their product. */
SVBRDF_API int svbrdf_rendering_loss_fwd_bwd(const float *input, const float *target,
                                  const float *scenes, const float *xrow, float eps,
                                  float *loss_out, float *grad_input,
                                  void *workspace, size_t workspace_bytes,
                                  int B, int S, int H, int W, void *stream);

/* K3 with SVBRDFL1Loss folded in -- replaces MixedLoss.forward AND its backward
 * (losses.py:54-63 = l1_weight * SVBRDFL1Loss (losses.py:7-19) + RenderingLoss):
 *   loss_out[0] = l1_weight * [ mean|n_i-n_t| + mean|log(d_i+eps_l1)-log(d_t+eps_l1)|
 *                               + mean|r_i-r_t| + mean|log(s_i+eps_l1)-log(s_t+eps_l1)| ]
 *                 + rendering loss (as above)
 * on the 24 planes the kernel reads anyway: zero extra HBM traffic.  Same scratch and
 * conventions as svbrdf_rendering_loss_fwd_bwd.  Reference values: l1_weight 0.1,
 * eps_l1 0.01, eps_render 0.1. */
SVBRDF_API int svbrdf_mixed_loss_fwd_bwd(const float *input, const float *target, const float *scenes,
                                         const float *xrow, float eps_render, float l1_weight, float eps_l1,
                                         float *loss_out, float *grad_input, void *workspace,
                                         size_t workspace_bytes, int B, int S, int H, int W, void *stream);

/* K3 with the network head folded in (the north star's "normal-map
 * decode"): `encoded9` is the generator's [B,9,H,W] output AFTER tanh, channels
 * normals_xy(0:2) | diffuse(2:5) | roughness(5) | specular(6:9) (utils.py:49-53).  The kernel
 * decodes it exactly like models.py:338-346 (utils.decode_svbrdf, then (x+1)/2 for
 * diffuse/roughness/specular), evaluates the mixed loss against the 12-channel `target`
 * (l1_weight = 0: rendering loss only) and returns d loss / d encoded9 in `grad_encoded9`
 * ([B,9,H,W], or NULL).  Replaces ~15 elementwise launches of the model head and their
 * backward; HBM traffic 120 instead of 144 bytes per pixel. */
SVBRDF_API int svbrdf_head_loss_fwd_bwd(const float *encoded9, const float *target, const float *scenes,
                                        const float *xrow, float eps_render, float l1_weight, float eps_l1,
                                        float *loss_out, float *grad_encoded9, void *workspace,
                                        size_t workspace_bytes, int B, int S, int H, int W, void *stream);

/* Scene table handed over in HOST memory.  The reference draws the table on the CPU for every
 * call (losses.py:35 -> environment.py:18-55), so the caller of this path always holds it in
 * host memory first.  These two entry points take it there: the B*S rows are copied into the
 * kernel-argument block of the launch (consumed before the call returns: `scenes_host` may be
 * reused or freed immediately), so the call enqueues ONE kernel dispatch and nothing else -- no
 * device buffer for the table, no H2D copy command, no pinned staging.  Limit:
 * B*S <= SVBRDF_HOST_SCENES_MAX_ROWS (288 rows = a 10 KB argument block: configs[3]'s 16 x 9 and config 5's
 * 8 x 32 rows fit; the HIP runtime on gfx950 takes argument blocks of at least 32 KB, measured); larger tables return
 * SVBRDF_ERR_DIMS and go through the device-pointer entry points above.  Everything else
 * (results, scratch, stream semantics) is identical to svbrdf_mixed_loss_fwd_bwd /
 * svbrdf_head_loss_fwd_bwd; l1_weight = 0 gives the plain RenderingLoss. */
#define SVBRDF_HOST_SCENES_MAX_ROWS 288
SVBRDF_API int svbrdf_host_scenes_max_rows(void);
SVBRDF_API int svbrdf_mixed_loss_fwd_bwd_host_scenes(const float *input, const float *target,
                                                     const float *scenes_host, const float *xrow,
                                                     float eps_render, float l1_weight, float eps_l1,
                                                     float *loss_out, float *grad_input, void *workspace,
                                                     size_t workspace_bytes, int B, int S, int H, int W,
                                                     void *stream);
SVBRDF_API int svbrdf_head_loss_fwd_bwd_host_scenes(const float *encoded9, const float *target,
                                                    const float *scenes_host, const float *xrow,
                                                    float eps_render, float l1_weight, float eps_l1,
                                                    float *loss_out, float *grad_encoded9, void *workspace,
                                                    size_t workspace_bytes, int B, int S, int H, int W,
                                                    void *stream);

/* Fused PHOTO loss (ABI version 8) -- the rendering loss against given photographs instead of against the renderings of
 * target maps, and its backward, in ONE launch:
 *   loss_out[0] = mean_{b,s,c,i,j} | log(render(scene[b,s], input[b]) + eps) - log(photos[b,s] + eps) |
 *   grad_input  = d loss / d input  (for upstream gradient 1.0), or NULL for forward-only (same loss, bit for bit).
 * What fitting maps to captured or synthesised photos, or self-supervised training on the input photos, needs when no
 * ground-truth maps exist: `photos` [B,S,3,H,W] are the photographs and `scenes` [B,S,9] the light / view each was taken
 * under (e.g. svbrdf_render_inputs' output and table).  The kernel reads the 12 input planes and the 3 S photo planes of a
 * pixel once and writes the 12 gradient planes once -- (12 + 3 S + 12) * 4 bytes per pixel -- and shades each pixel-render
 * once, where K3 shades twice.  Conventions as svbrdf_rendering_loss_fwd_bwd: PyTorch's sub-gradients (sign(0) = 0,
 * inclusive clamp masks; a term whose two sides are equal is exactly 0 with gradient 0); a NaN or infinite value anywhere
 * in `input` or `photos`, or a photo value at or below -eps (where torch.log gives NaN or -inf), gives loss_out[0] = NaN
 * with the scratch still left zeroed; bitwise run-to-run reproducible; error codes, 4-byte alignment rule (every aligned
 * pointer takes the same one-pixel-per-lane path: same results), eps in [1e-9, 1e9], and the scratch of
 * svbrdf_rendering_loss_workspace_bytes() with its zero-once / left-zeroed contract.  No gradient w.r.t. photos or scenes
 * (photos: svbrdf_[head_]photo_loss_photo_grad_fwd_bwd below; scenes: the scene-gradient entries).
 * `_host_scenes`: the B*S rows in HOST memory travel by value in the launch's argument block
 * (B*S <= SVBRDF_HOST_SCENES_MAX_ROWS, SVBRDF_ERR_DIMS beyond); bitwise the results of the device-table entry.
 * Limits of S, for every photo entry below as well: forward-only (grad NULL) S <= 1706 -- the item's table is staged in LDS --,
 * SVBRDF_ERR_DIMS beyond; with the gradient any S.
 * ACCURACY OF THE LOSS AT LARGE S (every photo entry; measured on an MI355X at 17 x 17, tests/test_gpu_many_photos.py,
 * profiles/r24_many_photos.txt): a thread adds the 3 S terms of its pixel one after the other in float32, so loss_out can be
 * off by up to (3 S + 16) 2^-24 of the mean |term| -- 7.7e-5 relative at S = 425, 3.1e-4 at S = 1706.  Measured: within 1e-6
 * of a float64 evaluation at every S <= 383 and for 12-map inputs at every S (1e-7 typical); 1.0e-6 to 2.0e-6 for the head
 * entries in five of the cases tried at S = 425, 1278, 1706 and 1707 (the float32 oracle itself: 2e-8).  The gradients do not
 * go through that sum and keep their bounds. */
SVBRDF_API int svbrdf_photo_loss_fwd_bwd(const float *input, const float *photos, const float *scenes,
                                         const float *xrow, float eps, float *loss_out, float *grad_input,
                                         void *workspace, size_t workspace_bytes, int B, int S, int H, int W,
                                         void *stream);
SVBRDF_API int svbrdf_photo_loss_fwd_bwd_host_scenes(const float *input, const float *photos, const float *scenes_host,
                                                     const float *xrow, float eps, float *loss_out, float *grad_input,
                                                     void *workspace, size_t workspace_bytes, int B, int S, int H,
                                                     int W, void *stream);

/* The fused photo loss with the network head folded in: svbrdf_photo_loss_fwd_bwd(decode(encoded9), ...) in ONE launch,
 *   loss_out[0]   = mean_{b,s,c,i,j} | log(render(scene[b,s], decode(encoded9[b])) + eps) - log(photos[b,s] + eps) |
 *   grad_encoded9 = d loss / d encoded9 ([B,9,H,W], upstream gradient 1.0), or NULL for forward-only (same loss bitwise).
 * `encoded9` [B,9,H,W] is the generator's output after tanh, channel layout and decode exactly those of
 * svbrdf_head_loss_fwd_bwd (models.py:338-346); defined for any finite value, no clamp of its own.  What training or
 * fine-tuning the network against photographs needs: (9 + 3 S + 9) * 4 bytes per pixel, no 12-channel map tensor, no
 * elementwise launches of the head.  Decoded roughness is one channel repeated: the tied scene loop only.  Everything else
 * is svbrdf_photo_loss_fwd_bwd's: a NaN or infinity in any of the 9 channels or in `photos`, or a photo value at or below
 * -eps, gives NaN with the scratch left zeroed; equal operands give term 0 and gradient 0; bitwise reproducible; the
 * same error codes before any launch, alignment rule, eps range, workspace and `_host_scenes` limit.
 * ADDED TO ABI VERSION 8 WITHOUT A BUMP (a backward-compatible addition: nothing existing changed).  A caller that may meet
 * an older build of version 8 detects the two entry points by symbol presence (dlsym / hasattr). */
SVBRDF_API int svbrdf_head_photo_loss_fwd_bwd(const float *encoded9, const float *photos, const float *scenes,
                                              const float *xrow, float eps, float *loss_out, float *grad_encoded9,
                                              void *workspace, size_t workspace_bytes, int B, int S, int H, int W,
                                              void *stream);
SVBRDF_API int svbrdf_head_photo_loss_fwd_bwd_host_scenes(const float *encoded9, const float *photos,
                                                          const float *scenes_host, const float *xrow, float eps,
                                                          float *loss_out, float *grad_encoded9, void *workspace,
                                                          size_t workspace_bytes, int B, int S, int H, int W,
                                                          void *stream);

/* The two photo losses with a CONFIDENCE WEIGHT per photo pixel, still ONE launch: what captured photographs need, whose
 * clipped highlights, pixels outside the rectified patch, noise-floor shadows and invalid (NaN) pixels of an HDR merge
 * must not vote.  With w in [0, 1], N = B S 3 H W and p' = (w > 0 ? photo : 0):
 *   loss_out[0] = (1/N) sum_{b,s,c,i,j} w[b,s,i,j] | log(render(scene[b,s], input[b])[c,i,j] + eps) - log(p'[b,s,c,i,j] + eps) |
 *   grad_input  = d loss / d input (upstream gradient 1.0), or NULL for forward-only (same loss bitwise).
 * `weights` holds `weight_planes` planes per item: weight_planes = S is [B,S,H,W], one plane per photo; weight_planes = 1
 * is [B,1,H,W], one plane per item shared by its photos (the patch outline).  Any other count: SVBRDF_ERR_DIMS.  One
 * weight serves the three colour channels of its pixel (per-channel confidence: pass the minimum over the channels).
 *  - A weight of exactly 0 EXCUSES THE PHOTO VALUE UNDER IT: the term is exactly 0 and its gradient exactly 0 whatever
 *    the photo holds there -- NaN, +-inf, a value at or below -eps.  The photo is replaced, not multiplied: 0 * NaN is
 *    never formed.  A pixel whose weights are 0 for every photo gets an all-zero (+-0) gradient.
 *  - A weight does NOT excuse the maps: a NaN or infinity anywhere in `input` / `encoded9` gives loss_out[0] = NaN, also at
 *    a pixel whose weights are all 0.
 *  - WEIGHTS MUST LIE IN [0, 1].  A weight that is NaN, negative or above 1 gives loss_out[0] = NaN (the sticky flag) with
 *    the scratch left zeroed.  The range is what keeps a term within the bound the fixed-point scale of the partial sums
 *    is planned for (|dlog| <= 32 per term): scale larger confidences down to 1 and the loss by the same factor.
 *  - A photo value that is NaN, infinite or at or below -eps where w > 0 gives NaN, as in the unweighted entries.
 *  - Weights of all ones give the loss and the gradient of the unweighted entry point BIT FOR BIT.
 * The weight of a (pixel, photo) is one more load beside the photo's three values: HBM traffic
 * (12 + 3 S + P + 12) * 4 bytes per pixel for the maps entries and (9 + 3 S + P + 9) * 4 for the head entries,
 * P = weight_planes (a shared plane is read from HBM once and from cache for the other photos).  Everything else is the
 * unweighted entries': PyTorch's sub-gradient conventions, bitwise run-to-run reproducibility, the scratch contract, the
 * error codes before any launch (`weights` is required: SVBRDF_ERR_NULL; 4-byte aligned: SVBRDF_ERR_ALIGN; every aligned
 * pointer gives the same results), the eps range and the `_host_scenes` limit.  No gradient w.r.t. weights, photos or
 * scenes (photos: svbrdf_[head_]photo_loss_photo_grad_fwd_bwd below).  ADDED TO ABI VERSION 8 WITHOUT A BUMP, like the head entries above: detect the four by symbol presence. */
SVBRDF_API int svbrdf_photo_loss_weighted_fwd_bwd(const float *input, const float *photos, const float *weights,
                                                  int weight_planes, const float *scenes, const float *xrow, float eps,
                                                  float *loss_out, float *grad_input, void *workspace,
                                                  size_t workspace_bytes, int B, int S, int H, int W, void *stream);
SVBRDF_API int svbrdf_photo_loss_weighted_fwd_bwd_host_scenes(const float *input, const float *photos,
                                                              const float *weights, int weight_planes,
                                                              const float *scenes_host, const float *xrow, float eps,
                                                              float *loss_out, float *grad_input, void *workspace,
                                                              size_t workspace_bytes, int B, int S, int H, int W,
                                                              void *stream);
SVBRDF_API int svbrdf_head_photo_loss_weighted_fwd_bwd(const float *encoded9, const float *photos, const float *weights,
                                                       int weight_planes, const float *scenes, const float *xrow,
                                                       float eps, float *loss_out, float *grad_encoded9, void *workspace,
                                                       size_t workspace_bytes, int B, int S, int H, int W, void *stream);
SVBRDF_API int svbrdf_head_photo_loss_weighted_fwd_bwd_host_scenes(const float *encoded9, const float *photos,
                                                                   const float *weights, int weight_planes,
                                                                   const float *scenes_host, const float *xrow, float eps,
                                                                   float *loss_out, float *grad_encoded9,
                                                                   void *workspace, size_t workspace_bytes, int B, int S,
                                                                   int H, int W, void *stream);

/* The photo losses with a PER-PHOTO EXPOSURE and its gradient, still ONE launch: every captured photograph has an unknown
 * radiometric scale (flash power, shutter, ISO, white balance).  `exposure` [B,S,3] holds a positive gain per photo and
 * colour channel that multiplies the light colour of its scene row; with w, p' and N as in the weighted entries (w = 1,
 * p' = photo when `weights` is NULL, and then weight_planes must be 0):
 *   loss_out[0]   = (1/N) sum w | log(render(scene[b,s] with colour fl32(colour_c e[b,s,c]), input[b]) + eps) - log(p' + eps) |
 *   grad_input    = d loss / d input (REQUIRED: these entries are forward + adjoint only)
 *   grad_exposure = d loss / d exposure [B,S,3] = sum_{i,j} w sign(delta) rad_c / (N (rad_c + eps) e_c), or NULL: the
 *                   loss and grad_input are bit for bit the same without it.
 *  - EXPOSURE MUST BE FINITE AND > 0.  A component that is NaN, infinite, 0 or negative gives loss_out[0] = NaN and an
 *    all-NaN grad_exposure, as does anything else that makes the loss NaN (NaN maps, a bad weight); scratch left zeroed.
 *  - The gain enters as ONE float32 multiply of the colour column in front of the falloff: loss and grad_input EQUAL BIT FOR
 *    BIT those of svbrdf_[head_]photo_loss[_weighted]_fwd_bwd on a scene table whose columns 6:9 were multiplied by
 *    `exposure` in float32; an all-ones exposure gives those entries' results on the table as it is.
 *  - grad_exposure is summed in integers (fixed point 2^-24 per wave of 64 pixels): bitwise reproducible run to run.  A
 *    zero-weight plane gives exactly (+-)0 in its photo's three entries.
 *  - NO GRADIENT WITH RESPECT TO LIGHT OR CAMERA POSITIONS here (the scene-gradient entries below have it), nor to weights or photos
 *    (photos: svbrdf_[head_]photo_loss_photo_grad_fwd_bwd below, without an exposure).
 * The scene table is in device memory (no by-value form).  `workspace`: svbrdf_photo_exposure_workspace_bytes(B, S, H, W)
 * bytes = the 65 words of svbrdf_rendering_loss_workspace_bytes plus B S 3 accumulator words, under the same contract:
 * zeroed once by the caller, left zeroed by every completed call (a NaN report included), so one buffer zeroed at that
 * size serves every fused loss.  Error codes before any launch as the weighted entries'; S <= 1278 (the per-workgroup
 * sums live in LDS; the loss at such S: "ACCURACY OF THE LOSS AT LARGE S" at svbrdf_photo_loss_fwd_bwd).  ADDED TO ABI VERSION 8 WITHOUT A BUMP: detect the three by symbol presence. */
SVBRDF_API size_t svbrdf_photo_exposure_workspace_bytes(int B, int S, int H, int W);
SVBRDF_API int svbrdf_photo_loss_exposure_fwd_bwd(const float *input, const float *photos, const float *weights,
                                                  int weight_planes, const float *exposure, const float *scenes,
                                                  const float *xrow, float eps, float *loss_out, float *grad_input,
                                                  float *grad_exposure, void *workspace, size_t workspace_bytes, int B,
                                                  int S, int H, int W, void *stream);
SVBRDF_API int svbrdf_head_photo_loss_exposure_fwd_bwd(const float *encoded9, const float *photos, const float *weights,
                                                       int weight_planes, const float *exposure, const float *scenes,
                                                       const float *xrow, float eps, float *loss_out,
                                                       float *grad_encoded9, float *grad_exposure, void *workspace,
                                                       size_t workspace_bytes, int B, int S, int H, int W, void *stream);

/* The photo losses with the gradient towards the SCENE TABLE, still ONE launch: the camera position, the light position
 * and the light colour of every photo are the last unknowns of a capture.  With w, p' and N as in the weighted entries
 * (w = 1, p' = photo when `weights` is NULL, and then weight_planes must be 0):
 *   loss_out[0] = (1/N) sum w | log(render(scene[b,s], input[b]) + eps) - log(p' + eps) |
 *   grad_input  = d loss / d input (REQUIRED: these entries are forward + adjoint only)
 *   grad_scenes = d loss / d scenes [B,S,9] (REQUIRED): columns 0:3 camera xyz, 3:6 light xyz, 6:9 light rgb.
 *  - loss and grad_input EQUAL BIT FOR BIT those of svbrdf_[head_]photo_loss[_weighted]_fwd_bwd on the same table.
 *  - Positions: the derivative of the composed definition (renderers.py:67-104, then the log-L1 mean) with PyTorch's
 *    sub-gradient conventions -- clamp(min=m) passes the gradient iff x >= m, sign(0) = 0 -- through (1 - VH)^5, both
 *    Smith terms, D, 1/(4 VN LN), LN+ and the falloff, and back through the normalisations of wo, wi and h.
 *  - Colour: sum_{i,j} w sign(delta) rad_c / (N (rad_c + eps) colour_c).  A COLOUR MUST BE FINITE AND > 0: one that is NaN,
 *    infinite, 0 or negative gives loss_out[0] = NaN.  A gain is applied to the table in front of the call; the chain rule
 *    takes grad_scenes[..., 6:9] back to it.
 *  - Whatever makes the loss NaN (NaN maps, a bad weight, a bad colour, a wave of 64 pixels whose sum of N |term| is NaN
 *    or exceeds 2^19) gives an all-NaN grad_scenes; scratch left zeroed.
 *  - grad_scenes is summed in float inside a wave of 64 pixels (fixed lanes, fixed order) and in 64-bit integers from there
 *    on (fixed point, unit 2^-24 / N): bitwise reproducible run to run.
 * The scene table is in device memory (no by-value form).  `workspace`: svbrdf_photo_scene_grad_workspace_bytes(B, S, H, W)
 * bytes = the 65 words of svbrdf_rendering_loss_workspace_bytes plus B S 9 accumulator words, under the same contract:
 * zeroed once by the caller, left zeroed by every completed call (a NaN report included).  Error codes before any launch
 * as the exposure entries'; S <= 425 (the per-workgroup sums live in LDS; the loss at such S: "ACCURACY OF THE LOSS AT LARGE
 * S" at svbrdf_photo_loss_fwd_bwd).  ADDED TO ABI VERSION 8 WITHOUT A BUMP: detect
 * the three by symbol presence. */
SVBRDF_API size_t svbrdf_photo_scene_grad_workspace_bytes(int B, int S, int H, int W);
SVBRDF_API int svbrdf_photo_loss_scene_grad_fwd_bwd(const float *input, const float *photos, const float *weights,
                                                    int weight_planes, const float *scenes, const float *xrow, float eps,
                                                    float *loss_out, float *grad_input, float *grad_scenes,
                                                    void *workspace, size_t workspace_bytes, int B, int S, int H, int W,
                                                    void *stream);
SVBRDF_API int svbrdf_head_photo_loss_scene_grad_fwd_bwd(const float *encoded9, const float *photos, const float *weights,
                                                         int weight_planes, const float *scenes, const float *xrow,
                                                         float eps, float *loss_out, float *grad_encoded9,
                                                         float *grad_scenes, void *workspace, size_t workspace_bytes,
                                                         int B, int S, int H, int W, void *stream);

/* The photo losses with the gradient towards the PHOTOGRAPHS, still ONE launch: what the gradient entries of
 * svbrdf_rectify_photos take as `grad_values`, so that the homographies and the lens of a capture are fitted against the
 * loss the maps are fitted with.  With w, p' and N as in the weighted entries (w = 1, p' = photo when `weights` is NULL,
 * and then weight_planes must be 0) and delta = log(render + eps) - log(p' + eps):
 *   loss_out[0] = (1/N) sum w | delta |
 *   grad_input  = d loss / d input, or NULL: the forward-only scene loop (loss + grad_photos; what a registration stage
 *                 launches, the maps being constants there)
 *   grad_photos = d loss / d photos [B,S,3,H,W] (REQUIRED) = -(w/N) sign(delta) / (photo + eps), upstream gradient 1.0
 *  - loss_out and grad_input / grad_encoded9 EQUAL BIT FOR BIT those of svbrdf_[head_]photo_loss[_weighted]_fwd_bwd on the
 *    same arguments; with grad_input NULL the loss equals the forward-only twin's bit for bit.
 *  - Every element of grad_photos is +m, -m or 0.  The magnitude m = (w fl(1/N)) / fl(photo + eps) is a pure function of w,
 *    N, eps and that one photo value: fl(1/N) is the double quotient rounded to float32, then one float32 multiply, one
 *    float32 add and one IEEE float32 division, each individually rounded (4 roundings; no fused multiply-add).  The
 *    kernel divides by fl(photo + eps) 2^-10 and scales by 2^-10: a power of two commutes with the rounding.
 *  - The sign is -sign(delta) as the kernel's own log of the quotient decides it -- the sign the map adjoint of the same
 *    launch uses -- with torch's sign(0) = 0: equal operands, or a quotient that rounds to exactly 1, give exactly 0.
 *  - A weight of exactly 0 gives exactly (+-)0 whatever the photo holds there (NaN, +-inf, a value at or below -eps): a
 *    select, 0 * NaN is never formed.
 *  - Elements are independent: another photo value changes its own element and the loss, and no other bit of grad_photos.
 *  - A term whose delta is NaN gives a NaN element: non-finite maps at that pixel, a photo value that is NaN or at or
 *    below -eps under w > 0, a weight outside [0, 1] or NaN (its pixel's three elements).  Every other element keeps its
 *    value even when loss_out[0] is NaN.  Under a +inf photo with w > 0 the element is 0 or NaN, nothing more is specified.
 *  - NO GRADIENT WITH RESPECT TO WEIGHTS, and none towards scenes or an exposure in these entries.
 * The scene table is in device memory (no by-value form).  `workspace`: svbrdf_rendering_loss_workspace_bytes with its
 * zero-once / left-zeroed contract, left zeroed in every case above.  Error codes before any launch as the weighted
 * entries': grad_photos NULL gives SVBRDF_ERR_NULL, every pointer 4-byte aligned (every aligned pointer gives the same
 * results).  Limits of S are the twin loops': S <= 1706 with grad_input NULL, any S with it.  HBM traffic
 * (12 + 3 S + P + 12 + 3 S) * 4 bytes per pixel for the maps entry ((9 + 3 S + P + 9 + 3 S) * 4 for the head entry; without
 * grad_input its planes less), plain stores.  ADDED TO ABI VERSION 8 WITHOUT A BUMP: detect the two by symbol presence. */
SVBRDF_API int svbrdf_photo_loss_photo_grad_fwd_bwd(const float *input, const float *photos, const float *weights,
                                                    int weight_planes, const float *scenes, const float *xrow, float eps,
                                                    float *loss_out, float *grad_input, float *grad_photos,
                                                    void *workspace, size_t workspace_bytes, int B, int S, int H, int W,
                                                    void *stream);
SVBRDF_API int svbrdf_head_photo_loss_photo_grad_fwd_bwd(const float *encoded9, const float *photos, const float *weights,
                                                         int weight_planes, const float *scenes, const float *xrow,
                                                         float eps, float *loss_out, float *grad_encoded9,
                                                         float *grad_photos, void *workspace, size_t workspace_bytes,
                                                         int B, int S, int H, int W, void *stream);

/* One STEP of a fit of the maps to photographs, ONE launch: the (weighted) photo loss at the maps as they are, its gradient
 * and the Adam update of the maps with it -- what PhotoLoss, backward(), torch.optim.Adam.step() and clamp_ do in several
 * passes over the same tensors.  `maps`, `exp_avg`, `exp_avg_sq` [B,12,H,W] are updated IN PLACE; with w, p' and N as in
 * the weighted entries (w = 1, p' = photo when `weights` is NULL, and then weight_planes must be 0) and g = d loss / d maps,
 * per element, every operation an individually rounded float32 one (no fused multiply-add, IEEE division and square root):
 *   m' = (beta1 m) + (c1 g)
 *   v' = (beta2 v) + ((c2 g) g)
 *   x' = clamp(x - step_size (m' / ((sqrt(v') rsb2) + adam_eps)), lo[ch], hi[ch])
 * with c1 = 1 - beta1, c2 = 1 - beta2, step_size = lr / (1 - beta1^step), rsb2 = 1 / sqrt(1 - beta2^step), computed on the
 * host in double from the float arguments and rounded once to float: svbrdf_photo_fit_adam_scalars writes the four, in that
 * order, to out4 (host only, nothing launched) -- torch.optim.Adam's update without AMSGrad and weight decay.
 *   loss_out[0] = the loss at the maps BEFORE the update; grad_out = g [B,12,H,W], or NULL: the gradient is never written.
 *  - loss_out and grad_out EQUAL BIT FOR BIT those of svbrdf_photo_loss[_weighted]_fwd_bwd on the same inputs.
 *  - `bounds_host`: NULL, or 12 x (lo, hi) floats ON THE HOST, one pair per channel (they ride in the launch's argument block);
 *    -inf / +inf = no bound on that side, and all-infinite bounds are NULL's results bit for bit.  A NaN x' stays NaN.
 *  - Non-finite maps behave as the composition does: the loss is NaN, the pixel's 36 values become NaN, every other pixel
 *    is updated normally, scratch left zeroed.
 *  - `step` is Adam's t, 1 for the first update.  SVBRDF_ERR_DIMS for step < 1, lr or adam_eps negative or not finite, a
 *    beta outside [0, 1), a NaN bound or lo > hi; the other codes as the weighted entries'; all before any launch.
 * The scene table is in device memory (no by-value form).  `workspace`: svbrdf_rendering_loss_workspace_bytes, same
 * contract.  ADDED TO ABI VERSION 8 WITHOUT A BUMP: detect the two by symbol presence. */
SVBRDF_API int svbrdf_photo_fit_adam_scalars(float lr, float beta1, float beta2, int step, float *out4);
SVBRDF_API int svbrdf_photo_fit_adam_step(float *maps, float *exp_avg, float *exp_avg_sq, const float *photos,
                                          const float *weights, int weight_planes, const float *scenes, const float *xrow,
                                          float eps, const float *bounds_host, float lr, float beta1, float beta2,
                                          float adam_eps, int step, float *loss_out, float *grad_out, void *workspace,
                                          size_t workspace_bytes, int B, int S, int H, int W, void *stream);

/* SEVERAL steps of the same fit in ONE launch.  The call leaves `maps`, `exp_avg`, `exp_avg_sq` and losses_out[k]
 * EQUAL BIT FOR BIT to n_steps successive calls of svbrdf_photo_fit_adam_step with step = first_step + k and the same
 * other arguments, in one kernel launch.  losses_out[k], k < n_steps, is the loss BEFORE update k (a NaN compares as
 * "both NaN").
 * The fit is pixel-local, so the thread that owns a pixel runs the steps on it with maps and state kept on chip: they are
 * read from memory once and written once, and no workgroup waits for another.
 *  - 1 <= n_steps <= SVBRDF_PHOTO_FIT_MAX_STEPS and first_step >= 1, else SVBRDF_ERR_DIMS; the other checks are the single
 *    step's, in its order; all before any launch.
 *  - `workspace`: svbrdf_photo_fit_steps_workspace_bytes(n_steps, B, S, H, W) bytes = n_steps times
 *    svbrdf_rendering_loss_workspace_bytes (every step sums its loss in 65 words of its own), same contract: zeroed once by
 *    the caller, left zeroed by every completed call.  Too small for n_steps: SVBRDF_ERR_WORKSPACE.
 *  - Non-finite maps behave as n single steps do: every losses_out[k] is NaN, the pixel's 36 values become NaN, every other
 *    pixel is updated normally.
 * No gradient output (of which step?) and no learning-rate schedule inside a launch.  ADDED TO ABI VERSION 8 WITHOUT A BUMP:
 * detect the two by symbol presence. */
#define SVBRDF_PHOTO_FIT_MAX_STEPS 64
SVBRDF_API size_t svbrdf_photo_fit_steps_workspace_bytes(int n_steps, int B, int S, int H, int W);
SVBRDF_API int svbrdf_photo_fit_adam_steps(float *maps, float *exp_avg, float *exp_avg_sq, const float *photos,
                                           const float *weights, int weight_planes, const float *scenes, const float *xrow,
                                           float eps, const float *bounds_host, float lr, float beta1, float beta2,
                                           float adam_eps, int first_step, int n_steps, float *losses_out, void *workspace,
                                           size_t workspace_bytes, int B, int S, int H, int W, void *stream);

/* One step of the fit WITH the gradient towards the scene table, still ONE launch: svbrdf_photo_fit_adam_step's argument
 * list with `grad_scenes` [B,S,9] added (REQUIRED) -- the light position, the camera position and the gain of a captured
 * photograph are refined together with the maps, and everything that is H W-sized stays inside the launch.
 *  - loss_out, grad_out (if given) and grad_scenes EQUAL BIT FOR BIT svbrdf_photo_loss_scene_grad_fwd_bwd's loss_out,
 *    grad_input and grad_scenes on the same inputs, its NaN rules included: a colour that is NaN, infinite or <= 0, a bad
 *    weight, or a wave sum beyond the limit gives a NaN loss and an all-NaN grad_scenes.
 *  - maps', exp_avg', exp_avg_sq' EQUAL BIT FOR BIT svbrdf_photo_fit_adam_step's on that gradient: the three lines above
 *    with the scalars of svbrdf_photo_fit_adam_scalars.  The gradients are those at the maps BEFORE the update.
 *  - The map update is applied whatever the loss turns out to be (the thread that owns a pixel cannot know the launch's
 *    loss), as svbrdf_photo_fit_adam_step applies it beside a NaN pixel.
 *  - `workspace`: svbrdf_photo_scene_grad_workspace_bytes(B, S, H, W) bytes, same contract: left zeroed.
 *  - Error codes, all before any launch and with no device buffer touched: the scene-gradient entry's checks in its order
 *    (its LDS limit on S included, and here S <= 383: six more words per thread wait in LDS across the scene loop), then
 *    the fit entry's of step, lr, the betas, adam_eps and the bounds.
 * Not offered: several steps in one launch (grad_scenes sums over all pixels of an item: applying it between two steps
 * needs a grid barrier), a head variant, and the Adam update of the table itself (a few hundred floats whose
 * parameterisation is the caller's).  ADDED TO ABI VERSION 8 WITHOUT A BUMP: detect it by symbol presence. */
SVBRDF_API int svbrdf_photo_fit_adam_step_scene_grad(float *maps, float *exp_avg, float *exp_avg_sq, const float *photos,
                                                     const float *weights, int weight_planes, const float *scenes,
                                                     const float *xrow, float eps, const float *bounds_host, float lr,
                                                     float beta1, float beta2, float adam_eps, int step, float *loss_out,
                                                     float *grad_out, float *grad_scenes, void *workspace,
                                                     size_t workspace_bytes, int B, int S, int H, int W, void *stream);

/* One step of the fit WITH A SMOOTHNESS PRIOR ACROSS PIXELS, still ONE launch.  Every entry above is pixel-local: a pixel
 * that no photograph sees (weight 0 in all of them) has an all-zero gradient and never moves.  The objective here is
 *   photo loss + R(x),  R(x) = sum_ch lambda[ch] / (B H W) sum_b ( sum_{i, j < W-1} |x[b,ch,i,j+1] - x[b,ch,i,j]|
 *                                                                  + sum_{i < H-1, j} |x[b,ch,i+1,j] - x[b,ch,i,j]| )
 * an anisotropic total variation per plane, no wrap-around, no coupling between items.  The gradient the step uses, per
 * element, with g the photo gradient exactly as svbrdf_photo_fit_adam_step[_scene_grad] forms it:
 *   s(a, b) = +1 if a > b, -1 if a < b, 0 if a == b, NaN if unordered     (compares of the stored values, no subtraction)
 *   k       = s(x, left) + s(x, right) + s(x, up) + s(x, down)            (a neighbour outside the patch contributes 0)
 *   g'      = g + (c[ch] (float)k)                                        (two individually rounded float32 operations)
 *   c[ch]   = (float)((double)lambda[ch] / ((double)B H W))               (on the host, rounded once)
 * and g' goes through the three lines of svbrdf_photo_fit_adam_step unchanged.
 *  - `smooth_host`: lambda, 12 finite floats >= 0 ON THE HOST, one per plane (REQUIRED; they ride in the launch's argument
 *    block).  A channel with lambda == 0 skips the term: no neighbour is read and g' = g bit for bit, so all-zero lambda
 *    leaves maps_out, exp_avg and exp_avg_sq EQUAL BIT FOR BIT to the twin entry's in-place results.
 *  - OUT OF PLACE for the maps: the neighbours are read as they were before the update, and other workgroups own them.
 *    `maps_in` is only read and is left intact; `maps_out` [B,12,H,W] receives x' and MUST NOT OVERLAP maps_in
 *    (SVBRDF_ERR_DIMS).  exp_avg and exp_avg_sq are element-wise and stay in place.
 *  - loss_out[0] is the PHOTO TERM alone, bit for bit the twin entry's: R is never reduced on the device.  grad_out, if
 *    given, is g'.  grad_scenes (the _scene_grad form) is the twin's bit for bit: R does not depend on the table.
 *  - A NaN neighbour makes the term NaN, as torch.sign(nan) does: that channel of the four neighbouring pixels becomes NaN
 *    in this step and the NaN spreads by one pixel per step; channels with lambda == 0 are untouched.  The NaN pixel itself:
 *    its 36 values become NaN, as in the twins.  Two EQUAL INFINITE neighbours give 0 where torch.sign(inf - inf) gives NaN.
 *  - Error codes, all before any launch and with no device buffer touched: smooth_host NULL or a lambda that is NaN,
 *    negative or infinite, then an overlap of maps_in and maps_out: SVBRDF_ERR_DIMS; then the twin entry's checks in its
 *    order (maps_out is required and 4-byte aligned like maps_in).
 * `workspace`: the twin's (svbrdf_rendering_loss_workspace_bytes; svbrdf_photo_scene_grad_workspace_bytes), same contract.
 * Not offered: several steps in one launch (a second step needs the neighbours' UPDATED values: a grid barrier), a head
 * form, isotropic or Huber variants, R reduced on the device.  ADDED TO ABI VERSION 8 WITHOUT A BUMP: detect the two by
 * symbol presence. */
SVBRDF_API int svbrdf_photo_fit_smooth_adam_step(const float *maps_in, float *maps_out, float *exp_avg, float *exp_avg_sq,
                                                 const float *photos, const float *weights, int weight_planes,
                                                 const float *scenes, const float *xrow, float eps,
                                                 const float *smooth_host, const float *bounds_host, float lr,
                                                 float beta1, float beta2, float adam_eps, int step, float *loss_out,
                                                 float *grad_out, void *workspace, size_t workspace_bytes, int B, int S,
                                                 int H, int W, void *stream);
SVBRDF_API int svbrdf_photo_fit_smooth_adam_step_scene_grad(const float *maps_in, float *maps_out, float *exp_avg,
                                                            float *exp_avg_sq, const float *photos, const float *weights,
                                                            int weight_planes, const float *scenes, const float *xrow,
                                                            float eps, const float *smooth_host, const float *bounds_host,
                                                            float lr, float beta1, float beta2, float adam_eps, int step,
                                                            float *loss_out, float *grad_out, float *grad_scenes,
                                                            void *workspace, size_t workspace_bytes, int B, int S, int H,
                                                            int W, void *stream);

/* CAPTURED PHOTOGRAPHS ONTO THE PATCH GRID, ONE launch: what stands between a camera image -- a perspective view, usually
 * 8-bit and gamma encoded, far larger than the grid, with clipped highlights and pixels outside the patch -- and the
 * `photos` / `weights` of the entries above.  P source photographs are resampled through a 3x3 homography each onto an
 * [Hd,Wd] grid with bilinear taps; 8-bit codes are decoded through a 256-entry table; the {0,1} confidence plane is written
 * beside the values.  With the inverse matrix the same call is the reference's rendering-to-perspective mapping
 * (OrthoToPerspectiveMapping.apply, renderers.py:171-173: zeros outside, like cv2's constant border).
 *   src          SVBRDF_RECTIFY_F32_PLANAR:     float32 [P,3,Hs,Ws], used as it is
 *                SVBRDF_RECTIFY_U8_INTERLEAVED: uint8 [P,Hs,Ws,3] (what an image decoder returns; any byte alignment);
 *                a tap's value is lut[code], `lut` a DEVICE float32 [256] table of the caller's (gamma 2.2, sRGB, a camera
 *                response; NULL for float sources).  No pow runs on the device.
 *   matrices     DEVICE float32 [P,9], row-major m0..m8 per photo: a DESTINATION pixel index (x, y, 1) -> SOURCE pixel-index
 *                coordinates.  Integer coordinates are pixel centres (cv2's convention, and the patch grid's: pixel 0's
 *                centre lies on the patch edge, xrow = linspace(-1, 1, W)).
 *   k            k x k sub-samples per destination pixel, k in {1, 2, 4}
 *   out          [P,3,Hd,Wd];  weights_out [P,Hd,Wd], or NULL: not wanted
 * Every line is one individually rounded float32 operation (no fused multiply-add, IEEE division):
 *   xs = x + ((i + 0.5)/k - 0.5),  ys = y + ((j + 0.5)/k - 0.5)               sub-sample (i, j); the offsets are exact
 *   X = (m0 xs + m1 ys) + m2,  Y = (m3 xs + m4 ys) + m5,  Z = (m6 xs + m7 ys) + m8,  u = X / Z,  v = Y / Z
 *   geometrically valid  <=>  Z > 0 and 0 <= u <= Ws-1 and 0 <= v <= Hs-1     (false for NaN; else u = v = 0 for addressing)
 *   x0 = floor(u), fx = u - x0, x1 = min(x0 + 1, Ws-1), likewise y;  a = (y0,x0), b = (y0,x1), c = (y1,x0), d = (y1,x1)
 *   top = a + fx (b - a),  bot = c + fx (d - c),  val = top + fy (bot - top)
 *   value = (sum of val over the sub-samples, (j, i) row-major) * (1/k^2)
 * A tap is invalid if any of its three channels is not finite, <= clip_lo or >= clip_hi (float sources: -inf / +inf switch
 * the thresholds off), or has a code <= clip_lo or >= clip_hi (uint8 sources: the floats are converted exactly, floor and
 * ceil; -1 / 256 or beyond switch them off).  All four taps are checked, also where fx or fy is 0.  If ANY sub-sample of a
 * pixel is invalid, by geometry or by a tap, its three values are 0.0 and its weight 0.0; otherwise its weight is 1.0.
 * u and v are clamped in float before the conversion to int: every load address lies inside the source WHATEVER `matrices`
 * holds (NaN, infinities, 1e30, m8 = 0: such pixels are invalid, nothing else happens).  Results are a pure function of the
 * arguments: bit for bit the numpy float32 restatement of tests/capture_checks.py.
 * Error codes before any launch: SVBRDF_ERR_DIMS for another src_format, k not in {1, 2, 4}, a size < 1, P > 65535, a size
 * > 32768 or a NaN threshold; SVBRDF_ERR_NULL for src, matrices, out, or lut with uint8 sources; SVBRDF_ERR_ALIGN for a
 * float pointer that is not 4-byte aligned.  No workspace.  The gradient towards the matrices
 * is svbrdf_rectify_photos_grad_matrices below; there is none towards the images.
 * ADDED TO ABI VERSION 8 WITHOUT A BUMP: detect it by symbol presence. */
#define SVBRDF_RECTIFY_F32_PLANAR 0
#define SVBRDF_RECTIFY_U8_INTERLEAVED 1
SVBRDF_API int svbrdf_rectify_photos(const void *src, int src_format, int P, int Hs, int Ws, const float *matrices, int Hd,
                                     int Wd, int k, const float *lut, float clip_lo, float clip_hi, float *out,
                                     float *weights_out, void *stream);

/* THE GRADIENT OF svbrdf_rectify_photos' VALUES TOWARDS THE MATRICES, ONE launch: grad_matrices[p, n] = d (sum over `out`
 * of grad_values * out) / d m_n of photo p, for photometric refinement of a registration (move a photograph's corners until
 * its rectification agrees with a rendering).  src, src_format, P, Hs, Ws, matrices, Hd, Wd, k, lut, clip_lo, clip_hi: the
 * forward's arguments, unchanged.  grad_values: DEVICE float32 [P,3,Hd,Wd], the gradient towards `out`.  grad_matrices:
 * DEVICE float32 [P,9], written whole.
 * Definition.  Per sub-sample (i, j) of pixel (x, y) of photo p, everything up to `val` is the forward's as it stands: xs,
 * ys, X, Y, Z, u, v, valid; the clamp; x0, y0, fx, fy, x1, y1; the taps a, b, c, d per channel; and the pixel's `ok`, which
 * is true where the forward's weight is 1 (every sub-sample valid and every tap of every sub-sample passing the tap rule).
 * The gradient is that of the forward's expression with the cell (x0, y0), `valid` and `ok` held constant: at an integer u
 * the right-hand derivative, and 0 at u = Ws-1, where the clamped x1 = x0 (likewise v).  With g_ch = grad_values[p,ch,y,x],
 * every line one individually rounded float32 operation (no fused multiply-add, IEEE division):
 *   per channel:  ba = b - a;  dc = d - c;  du = ba + fy (dc - ba);  dv = bot - top      (top, bot: the forward's)
 *   gu = ((g0 du0 + g1 du1) + g2 du2) * (1/k^2);   gv = ((g0 dv0 + g1 dv1) + g2 dv2) * (1/k^2)
 *   rz = 1 / Z;   pu = gu rz;   pv = gv rz;   pz = -((pu u) + (pv v))
 *   the nine terms:  pu xs, pu ys, pu,   pv xs, pv ys, pv,   pz xs, pz ys, pz
 * grad_matrices[p, n] is the sum of term n over all sub-samples of all pixels of photo p whose `ok` holds.  A pixel whose
 * `ok` is false contributes nothing -- a select, not a multiplication: a NaN in grad_values under it changes no bit.  A
 * non-finite g under an ok pixel makes the sums it enters non-finite.  A matrix under which no sub-sample is valid (NaN,
 * +-inf, 1e30, m8 = 0) gives an all-zero row.  Every load address lies inside the source whatever `matrices` holds, as in
 * the forward.  No gradient towards `src`; none of the weights, which are piecewise constant.
 * The sum: one launch, no float atomics, bitwise the same in every launch and whatever else runs.  A workgroup covers the
 * forward's 64 x 4 tile.  A thread adds its k^2 sub-samples in (j, i) order into nine float32 accumulators (k^2 - 1
 * additions; +0 for a pixel that is not ok or lies beyond the grid); a butterfly over the wave's 64 lanes (lane ^ 32, 16, 8,
 * 4, 2, 1: 6 additions) and (w0 + w1) + (w2 + w3) over the four waves (2 additions) give the workgroup's nine words, which
 * go to the workspace with plain stores; behind an agent-scope release a per-photo integer ticket names the photo's last
 * workgroup, which adds the photo's partials in FLOAT64 -- lane l the workgroups l, l + 64, ... in index order
 * (x fastest, then y), then the same butterfly over the 64 lane sums -- and rounds ONCE to float32.
 * SVBRDF_RECTIFY_GRAD_DEPTH bounds the float32 additions any single term passes through: 15 + 6 + 2 = 23 <= 24.  So
 * with A_n the sum of |term n| over the photo,  |grad_matrices[p, n] - exact sum of the float32 terms| <=
 * (SVBRDF_RECTIFY_GRAD_DEPTH + 1) * 2^-24 * A_n  (the additions and the one final rounding).
 * `workspace`: svbrdf_rectify_grad_workspace_bytes(P, Hd, Wd) bytes (0 for sizes outside the limits), 8-byte aligned,
 * zeroed once by the caller and left zeroed by every completed call: a second call needs no memset.
 * Error codes before any launch: the forward's, with grad_matrices in the place of `out` and grad_values among the
 * 4-byte-aligned float pointers; SVBRDF_ERR_NULL for grad_values or workspace; SVBRDF_ERR_ALIGN for a workspace off 8
 * bytes; SVBRDF_ERR_WORKSPACE for one that is too small.
 * ADDED TO ABI VERSION 8 WITHOUT A BUMP: detect the two by symbol presence. */
#define SVBRDF_RECTIFY_GRAD_DEPTH 24
SVBRDF_API size_t svbrdf_rectify_grad_workspace_bytes(int P, int Hd, int Wd);
SVBRDF_API int svbrdf_rectify_photos_grad_matrices(const void *src, int src_format, int P, int Hs, int Ws,
                                                   const float *matrices, int Hd, int Wd, int k, const float *lut,
                                                   float clip_lo, float clip_hi, const float *grad_values,
                                                   float *grad_matrices, void *workspace, size_t workspace_bytes,
                                                   void *stream);

/* svbrdf_rectify_photos BEHIND A LENS, ONE launch: a homography is exact only for a pinhole camera, and a phone's lens bends
 * straight lines by several pixels towards the frame's edge.  The gather needs the FORWARD distortion model, ideal pixel ->
 * distorted pixel, a closed-form polynomial: it stands between the forward's quotient and its tap cell, nothing iterates.
 *   lens         DEVICE float32 [P,9] per photo: fx, fy, cx, cy, k1, k2, p1, p2, k3 -- OpenCV's camera matrix entries and its
 *                distortion vector in OpenCV's order, so a calibration can be pasted in.  `matrices` then map a destination
 *                pixel to IDEAL (undistorted) source pixel coordinates.
 * Every other argument is svbrdf_rectify_photos'.  Per sub-sample, everything up to u = X / Z, v = Y / Z is the forward's as
 * it stands.  Then, every line ONE individually rounded float32 operation, no fused multiply-add, IEEE `/`:
 *   xn = (u - cx) / fx          yn = (v - cy) / fy
 *   xx = xn xn   yy = yn yn   xy = xn yn   r2 = xx + yy
 *   rad  = 1 + r2 (k1 + r2 (k2 + r2 k3))
 *   mono = 1 + r2 (3 k1 + r2 (5 k2 + r2 (7 k3)))          d(r rad)/dr: the radial map has not folded back
 *   t  = 2 xy
 *   tx = (p1 t) + (p2 (r2 + 2 xx))      ty = (p1 (r2 + 2 yy)) + (p2 t)
 *   xd = (xn rad) + tx                   yd = (yn rad) + ty
 *   ud = (xd fx) + cx                    vd = (yd fy) + cy
 *   valid  <=>  Z > 0  and  fx > 0  and  fy > 0  and  mono > 0  and  0 <= ud <= Ws-1  and  0 <= vd <= Hs-1   (false for NaN)
 * (3 k1, 5 k2, 7 k3, 2 xx, 2 yy are rounded products of their own; a focal length of 0 or below makes every sub-sample
 * invalid: with a negative one the polynomial alone would map back into the frame.)  From here on it is the forward's text
 * with (ud, vd) in the place of (u, v): the select to 0 if not valid, the clamp in float before the conversion to int, cell,
 * taps, tap rule, bilinear value, the sub-sample sum in (j, i) order times 1/k^2, values and weight 0 for a pixel with any
 * invalid sub-sample.  Every load address lies inside the source WHATEVER `matrices` and `lens` hold (NaN, +-inf, 1e30, a
 * focal length of 0 or below: such sub-samples are invalid, nothing else happens).
 * Why mono: under strong barrel distortion the polynomial maps far-off ideal points back into the frame; without the guard
 * a destination pixel outside the camera's view would get a confident, wrong value.
 * With the null lens (1, 1, 0, 0, 0, 0, 0, 0, 0) every added statement is exact: values and weights are svbrdf_rectify_photos'
 * bit for bit.  Results are a pure function of the arguments: bit for bit the numpy float32 restatement of
 * tests/capture_lens_checks.py.  Six kernels <uint8, k>, the forward's launch shape, no atomics, no scratch, no workspace.
 * Error codes before any launch: svbrdf_rectify_photos', then SVBRDF_ERR_NULL for a NULL lens, SVBRDF_ERR_ALIGN for one off
 * 4 bytes.
 * ADDED TO ABI VERSION 8 WITHOUT A BUMP: detect it by symbol presence. */
SVBRDF_API int svbrdf_rectify_photos_lens(const void *src, int src_format, int P, int Hs, int Ws, const float *matrices,
                                          const float *lens, int Hd, int Wd, int k, const float *lut, float clip_lo,
                                          float clip_hi, float *out, float *weights_out, void *stream);

/* THE GRADIENT OF svbrdf_rectify_photos_lens' VALUES TOWARDS THE MATRICES AND THE LENS, ONE launch:
 * grad_matrices[p, n] = d (sum over `out` of grad_values * out) / d m_n of photo p THROUGH the lens's Jacobian, and
 * grad_lens[p, n] the same towards lens entry n (fx, fy, cx, cy, k1, k2, p1, p2, k3), both DEVICE float32 [P,9], written
 * whole.  The forward's arguments unchanged; grad_values DEVICE float32 [P,3,Hd,Wd].
 * Definition.  Per sub-sample everything up to the taps and the pixel's `ok` is the forward's.  The gradient is that of the
 * forward's expression with the cell, `valid` (mono's sign included) and `ok` held constant.  Every line one individually
 * rounded float32 operation (no fused multiply-add, IEEE division; 2 k2, 3 k3, 2 p1, 6 p1, 2 p2, 6 p2, 2 xx, 2 yy are rounded
 * products of their own):
 *   gud, gvd = svbrdf_rectify_photos_grad_matrices' gu, gv, formed at the cell and fractions of (ud, vd)
 *   a = gud fx;   b = gvd fy;   q = k1 + (r2 ((2 k2) + ((3 k3) r2)))
 *   jxx = ((rad + ((2 xx) q)) + ((2 p1) yn)) + ((6 p2) xn)                              d xd / d xn
 *   jxy = ((t q) + ((2 p1) xn)) + ((2 p2) yn)                                           d xd / d yn = d yd / d xn
 *   jyy = ((rad + ((2 yy) q)) + ((6 p1) yn)) + ((2 p2) xn)                              d yd / d yn
 *   gxn = (a jxx) + (b jxy);   gyn = (a jxy) + (b jyy);   gu = gxn / fx;   gv = gyn / fy
 *   rz = 1 / Z;   pu = gu rz;   pv = gv rz;   pz = -((pu u) + (pv v))                   (u, v: the pinhole quotients)
 *   the nine matrix terms:  pu xs, pu ys, pu,   pv xs, pv ys, pv,   pz xs, pz ys, pz
 *   s = (a xn) + (b yn);   s1 = s r2;   s2 = s1 r2;   s3 = s2 r2
 *   the nine lens terms:  fx: (gud xd) - (gu xn)     fy: (gvd yd) - (gv yn)     cx: gud - gu     cy: gvd - gv
 *                         k1: s1     k2: s2     p1: (a t) + (b (r2 + (2 yy)))     p2: (a (r2 + (2 xx))) + (b t)     k3: s3
 * A pixel whose `ok` is false contributes nothing -- a select: a NaN in grad_values under it changes no bit.  A matrix or a
 * lens row under which no sub-sample is valid gives all-zero rows in both outputs.  With the null lens the nine matrix
 * sums are svbrdf_rectify_photos_grad_matrices' bit for bit.  Every load address lies inside the source, as in the forward.
 * The sum is svbrdf_rectify_photos_grad_matrices' with eighteen words per workgroup instead of nine: k^2 - 1 thread
 * additions, the 64-lane butterfly, (w0 + w1) + (w2 + w3), write-through vector stores, a drain, the per-photo integer
 * ticket; the last workgroup adds the partials in float64 in index order and rounds ONCE.  No float atomic, bitwise the same
 * in every launch.  SVBRDF_RECTIFY_GRAD_DEPTH bounds it as it bounds the other:  |sum_n - exact sum of the float32 terms|
 * <= (SVBRDF_RECTIFY_GRAD_DEPTH + 1) * 2^-24 * A_n.
 * `workspace`: svbrdf_rectify_lens_grad_workspace_bytes(P, Hd, Wd) bytes (the tickets and eighteen words per tile; 0 for
 * sizes outside the limits), 8-byte aligned, zeroed once by the caller and left zeroed by every completed call.
 * Error codes before any launch: svbrdf_rectify_photos_grad_matrices', then the forward's for `lens`; SVBRDF_ERR_NULL for
 * grad_lens, SVBRDF_ERR_ALIGN for one off 4 bytes.
 * ADDED TO ABI VERSION 8 WITHOUT A BUMP: detect the two by symbol presence. */
SVBRDF_API size_t svbrdf_rectify_lens_grad_workspace_bytes(int P, int Hd, int Wd);
SVBRDF_API int svbrdf_rectify_photos_lens_grad(const void *src, int src_format, int P, int Hs, int Ws, const float *matrices,
                                               const float *lens, int Hd, int Wd, int k, const float *lut, float clip_lo,
                                               float clip_hi, const float *grad_values, float *grad_matrices,
                                               float *grad_lens, void *workspace, size_t workspace_bytes, void *stream);

/* data[i] *= scale_dev[0] for i < n, on the device and without a host sync; when the
 * scalar is exactly 1.0 the kernel exits without touching `data`.  Used by the autograd
 * wrapper to apply the upstream gradient of the loss (the chain rule through
 * RenderingLoss.forward's scalar output) to grad_input. */
SVBRDF_API int svbrdf_scale_inplace(float *data, const float *scale_dev, size_t n, void *stream);

/* Test aid: evaluates the kernels' Newton square root and shared-reciprocal division
 * (the primitives that stand in for the reference's torch.sqrt / torch.div, i.e.
 * normalize() of renderers.py:11-12, on the ill-conditioned coords -> NH path) on n
 * pseudo-random operands -- squared lengths x log-uniform in [lo, hi], numerators a
 * uniform in [-hi, hi] -- and ADDS the number of results that differ from the
 * IEEE-correct a / sqrtf(x) to counts_dev[0] and from sqrtf(x) to counts_dev[1].  counts_dev: two zero-initialised device uint64. */
SVBRDF_API int svbrdf_debug_check_arith(unsigned long long n, unsigned seed, float lo, float hi,
                                        unsigned long long *counts_dev, void *stream);

/* K4 -- replaces SvbrdfDataset.mix (dataset.py:142-160), the material-mixing augmentation, for a whole batch:
 *   out[b] = mix(svbrdf0[b], svbrdf1[b], alpha[b])   all [B,12,H,W] device, alpha [B] device (the reference draws
 *   it per sample from U(0.1, 0.9), dataset.py:144).  Normals are projected to z = 1 (n / max(0.01, n.z)), blended
 *   with weights alpha and fp32(1 - alpha) and renormalised; diffuse, roughness and specular are blended.  Same
 *   operation order and roundings as the reference.  H and W are independent here.  `out` may not alias the inputs. */
SVBRDF_API int svbrdf_mix_materials(const float *svbrdf0, const float *svbrdf1, const float *alpha, float *out,
                                    int B, int H, int W, void *stream);

/* K1 with the sensor-noise epilogue (ABI version 7) -- replaces the loop body of SvbrdfDataset.render_inputs
 * (dataset.py:206-219: render, + N(0, std_image) from the CPU generator, torch.clamp(0, 1)) for a whole batch of samples
 * and all their photos in ONE launch that writes each photo once:
 *   out[b,s] = clamp(render(scene[b,s], maps[b]) + noise_std[b,s] * n(seed, offset, element), 0, 1)     [B,S,3,H,W]
 * `noise_std` holds one level per render ([B*S], the reference draws it per image, dataset.py:215); NULL = no noise,
 * clamp only: bitwise clamp(svbrdf_render_fwd(...)).  The standard-normal field n is counter-based and a pure function of
 * (seed, offset, linear index e of the element in `out`): Philox4x32-10 with key = (seed lo, seed hi) and counter =
 * (g lo, g hi, offset lo, offset hi), g = e / 4, gives four 32-bit words x0..x3; u_i = ((x_i >> 8) + 0.5) / 2^24;
 * n(4g) = r(u0) cos(2 pi u1), n(4g+1) = r(u0) sin(2 pi u1), n(4g+2) = r(u2) cos(2 pi u3), n(4g+3) = r(u2) sin(2 pi u3),
 * r(u) = sqrt(-2 ln u).  The field does not depend on the vector width of the launch; a caller advances `offset` (or the
 * seed) between calls, like a device generator.  Different numbers than the reference's CPU field, the same distribution.
 * `svbrdf_render_inputs`: scenes and levels are DEVICE tables.  `_host_scenes`: both are HOST arrays of B*S rows
 * (<= SVBRDF_HOST_SCENES_MAX_ROWS) that travel by value in the launch's argument block, as in
 * svbrdf_render_fwd_host_scenes (one scene table row per render; not shared between maps: every sample draws its own
 * views, dataset.py:172-204). */
SVBRDF_API int svbrdf_render_inputs(const float *maps, const float *scenes, const float *noise_std, unsigned long long seed,
                                    unsigned long long offset, const float *xrow, float *out, int B, int S, int H, int W,
                                    void *stream);
SVBRDF_API int svbrdf_render_inputs_host_scenes(const float *maps, const float *scenes_host, const float *noise_std_host,
                                                unsigned long long seed, unsigned long long offset, const float *xrow,
                                                float *out, int B, int S, int H, int W, void *stream);

/* Measurement aid (ABI version 7): dst[i] = src[i] for i < n floats (n a multiple of 4, both pointers 16-byte aligned,
 * no overlap) as a plain streaming copy, 16 bytes per lane and access, non-temporal loads and stores.  bench.py and the
 * speed guard time it on buffers beyond the Infinity Cache: 2 * 4 * n bytes / duration is the copy bandwidth of THIS
 * box, the "measured-copy peak" the HBM-bound kernels are priced against beside the nominal 8 TB/s. */
SVBRDF_API int svbrdf_debug_copy(float *dst, const float *src, size_t n, void *stream);

/* Test aid (ABI version 7): how many kernels this library has enqueued in this process (every entry point enqueues
 * exactly one; failed calls are not counted).  tests/test_gpu_perf_guard.py asserts ONE launch per training step. */
SVBRDF_API unsigned long long svbrdf_debug_launch_count(void);

/* Measurement aid: one wave spins for `ticks_100mhz` ticks of the chip's constant 100 MHz counter on `stream`
 * and writes out_dev[0] = shader-clock cycles elapsed, out_dev[1] = 100 MHz ticks elapsed (two device uint64).
 * cycles / ticks * 0.1 = the shader clock in GHz while whatever else is running runs (bench.py launches it on a
 * stream of its own beside the fused loss: the clock the chip holds under that kernel). */
SVBRDF_API int svbrdf_debug_clock_probe(unsigned long long *out_dev, unsigned long long ticks_100mhz, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * AUXILIARY entry points -- NOT part of the north-star path (BASELINE.json: fp32 maps, first-order training).
 * The three svbrdf_*_f64 symbols below serve callers who hand the renderer double maps or differentiate through its
 * backward (gradient checks, notebook-style direct map optimisation); the reference itself never does either.  They are
 * compiled from a translation unit of their own (csrc/svbrdf_aux_f64.hip), take none of the tuned kernels' paths, are
 * frozen since ABI version 6, and a replacement library that serves training only may return SVBRDF_ERR_DIMS from them.
 * --------------------------------------------------------------------------------------------------------------- */

/* float64 maps (ABI version 5).  LocalRenderer.render is dtype-agnostic in the reference (renderers.py:67-104); with double
 * maps it computes in MIXED precision: pixel grid (torch.linspace, :73), camera / light positions and light colour
 * (torch.Tensor(...), :79,:91,:98) are float32, so wo, wi, h, (1-VH)^5 and colour*falloff are the float32 values of the
 * float32 path, and everything that touches the maps is promoted to double.  These two entry points do exactly that:
 *   maps / grad_maps [B,12,H,W] double, scenes [B,S,9] float32 DEVICE, xrow [W] float32, out / grad_out [B,S,3,H,W] double.
 * Shading op by op in the reference's order (the slow path of gradient checks and notebooks, not of training); the losses
 * for double maps are composed from these through autograd on the host side.  Same error convention as above. */
SVBRDF_API int svbrdf_render_fwd_f64(const double *maps, const float *scenes, const float *xrow, double *out,
                                     int B, int S, int H, int W, void *stream);
SVBRDF_API int svbrdf_render_bwd_f64(const double *maps, const float *scenes, const float *xrow, const double *grad_out,
                                     double *grad_maps, int B, int S, int H, int W, void *stream);

/* Second order (ABI version 6): what autograd needs to differentiate THROUGH the backward of render() -- the reference's
 * render is built from differentiable torch ops (renderers.py:8-104), so `backward(create_graph=True)` /
 * `torch.autograd.grad(..., create_graph=True)` work there (gradient penalties, Hessian-vector products in the notebooks'
 * style of direct map optimisation).  For a direction `tangent` [B,12,H,W] of the maps, one forward-mode (dual number)
 * evaluation of the float64 shading and its adjoint gives
 *   out_tangent       [B,S,3,H,W] = J(maps) tangent                      (derivative of <J^T grad_out, tangent> w.r.t. grad_out)
 *   grad_maps_tangent [B,12,H,W]  = d/dmaps <J(maps)^T grad_out, tangent>  (the Hessian of <grad_out, render(maps)> times tangent)
 * with clamps and sub-gradient selections treated as torch's double-backward formulas treat them (masks compare values,
 * zero derivative).  Buffers and error convention as svbrdf_render_bwd_f64; float32 callers are served by the host side
 * through these in double. */
SVBRDF_API int svbrdf_render_bwd_jvp_f64(const double *maps, const double *tangent, const float *scenes, const float *xrow,
                                         const double *grad_out, double *grad_maps_tangent, double *out_tangent,
                                         int B, int S, int H, int W, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SVBRDF_HIP_H */
