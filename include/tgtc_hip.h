/*
 * tgtc_hip.h -- C ABI of the MI355X (gfx950) render hot path of TGTC-Style.
 *
 * One shared library (libtgtc_hip.so) of hand-written HIP kernels.  Every entry point is
 * `extern "C"`, takes plain device pointers + sizes + a hipStream_t (passed as void*), writes only
 * into caller-allocated outputs, never synchronises the device and never allocates inside a launch
 * function (network handles own their packed weights; they are created / destroyed explicitly).
 *
 * Return value: 0 = ok, <0 = error class (below); tgtc_last_error() gives the thread-local text.
 *
 * The reference (PaiDii/TGTC-Style) is pure Python on PyTorch; there is no FFI in it.  Each entry
 * point replaces the reference *Python callable* cited beside it (file:line under /root/reference).
 * INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Layouts (all row-major, dense):
 *   rays_o, rays_d   double [R,3]        (the reference keeps rays in float64: dataset.py:420-429)
 *   ts               float  [R,N]        sample depths
 *   pts              double [R,N,3]
 *   rgb              float  [R,N,3]      sigma float [R,N]
 *   per-ray outputs  float  [R,3] / [R]
 */
#ifndef TGTC_HIP_H
#define TGTC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TGTC_OK 0
#define TGTC_ERR_ARG (-1)         /* null pointer, negative size, bad enum */
#define TGTC_ERR_UNSUPPORTED (-2) /* a shape / configuration the kernels are not built for */
#define TGTC_ERR_HIP (-3)         /* a HIP runtime call failed */

/* Arithmetic mode of the fused MLP kernels (MFMA operands; accumulation is always fp32). */
#define TGTC_PREC_FP16X3 0 /* split fp16 (hi+lo) x 3 MFMA products: fp32-equivalent, the parity mode */
#define TGTC_PREC_FP16 1   /* single fp16 MFMA product: fastest, ~2e-3 abs error on composited RGB */
#define TGTC_PREC_FP16_FP6 2 /* fp16 product + two block-scaled fp6 (e2m3) correction products: ~1e-4, NeRF nets only */

typedef struct tgtc_net tgtc_net; /* opaque: packed weights of one network, resident in HBM */

/* One nn.Linear in the reference layout: weight [out_features, in_features] row-major, bias [out]. HOST pointers. */
typedef struct {
    const float* weight;
    const float* bias;
    int32_t out_features;
    int32_t in_features;
} tgtc_linear;

int tgtc_version(void);
const char* tgtc_last_error(void);

/* ------------------------------------------------------------------ a1+a2: ray generation
 * dataset.py:33-42 (get_rays_np) + dataset.py:44-61 (ndc_rays_np, near given by caller; the datasets pass 1.0).
 * Generates rays for pixels [first_pixel, first_pixel+n) of an H x W frame in row-major pixel order
 * (so ranks can generate their own shard).  c2w: 12 HOST floats (3x4 row-major).  ndc=0 skips the warp. */
int tgtc_gen_rays(int H, int W, double fx, double fy, double cx, double cy, const float* c2w,
                  int pixel_alignment, int ndc, double ndc_near, int64_t first_pixel, int64_t n,
                  double* rays_o, double* rays_d, void* stream);

/* ------------------------------------------------------------------ a3: coarse sampling
 * utils.py:509-531 sampling_pts_uniform (harmony=False).  jitter: float [R,N] uniform(0,1) or NULL (perturb=False).
 * pts may be NULL (the fused path never materialises it). */
int tgtc_sample_coarse(const double* rays_o, const double* rays_d, int64_t R, int N, float near_, float far_,
                       const float* jitter, double* pts, float* ts, void* stream);

/* ------------------------------------------------------------------ a4: positional encoding
 * models.py:46-60 Embedder.forward with log-sampled bands 2^0..2^(L-1), include_input.  x: [M,3] double
 * (x_is_f64=1) or float; out: float [M, 3+6L] (the float32 cast of models.py:219-220 is applied). */
int tgtc_posenc(const void* x, int x_is_f64, int64_t M, int L, float* out, void* stream);

/* ------------------------------------------------------------------ a5: NeRF MLP
 * models.py:63-117 MLP_style / :182-223 StyleNerf with D=8, W=256, skips=[4], use_viewdir, ReLU, PE 10/4.
 * layers: the 12 linears in the order of MLP_style.layers (models.py:93):
 *   base_layers[0..7], sigma_layer, base_remap_layer, rgb_layers[0], rgb_layers[1]. */
int tgtc_nerf_create(const tgtc_linear* layers, int n_layers, int precision, tgtc_net** out);
int tgtc_net_destroy(tgtc_net* net);
int tgtc_net_precision(const tgtc_net* net);

/* StyleNerf.forward (models.py:216-223): raw points / view dirs [M,3] double -> outputs.  Any output may be NULL.
 * base_remap float [M,256]; pts_enc float [M,63]; dirs_enc float [M,27].
 * Coordinate range (every entry point that encodes positions itself: this one, tgtc_nerf_forward_rays / _list, the render
 * and restyle calls): the in-kernel encoder reduces 2^band x / (2 pi) in float64 and takes the quadrant from a 32-bit integer,
 * so its accuracy does not depend on |x| up to |x| < 2^31 x 2 pi / (4 x 2^9) ~ 6.5e6 for positions (band 9) and
 * 2^31 x 2 pi / (4 x 2^3) ~ 4.2e8 for directions (band 3); beyond that the quadrant saturates and sin / cos are wrong.  A sample with non-finite coordinates
 * changes no other sample's outputs. */
int tgtc_nerf_forward(const tgtc_net* net, const double* pts, const double* dirs, int64_t M,
                      float* rgb, float* sigma, float* base_remap, float* pts_enc, float* dirs_enc, void* stream);

/* MLP_style.forward (models.py:95-117) on already-encoded float inputs [M,63] / [M,27]. */
int tgtc_nerf_mlp_forward(const tgtc_net* net, const float* pts_enc, const float* dirs_enc, int64_t M,
                          float* rgb, float* sigma, float* base_remap, void* stream);

/* Hot path: points are never materialised; sample (r,i) is rays_o[r] + ts[r,i]*rays_d[r], dirs = rays_d[r]
 * (rendering.py:27-31).  need_rgb=0 skips the colour head (the coarse pass of a render only consumes weights
 * when its RGB is discarded; the reference still computes it). */
int tgtc_nerf_forward_rays(const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts,
                           int64_t R, int N, float* rgb, float* sigma, void* stream);

/* The same per-sample arithmetic over a device-side LIST of samples (the colour phase of the two-phase fine pass below):
 * live uint32 [*n_live] ascending sample indices s = r x N + i, each < R x N; n_live a DEVICE pointer to one uint32 (the host
 * never learns the count: the grid is one workgroup per CU and every workgroup reads it).  rgb[s] is written for the listed
 * samples only -- the bits tgtc_nerf_forward_rays gives that sample -- and nothing else of rgb is touched; no density is
 * written.  *n_live == 0 reads nothing of `live` (which must still be a valid pointer).
 * Built for TGTC_PREC_FP16_FP6 handles only (one more instance of the two-tile persistent kernel, csrc/mlp_nerf_mx2.hip):
 * any other precision, or R x N >= 2^31 -> TGTC_ERR_UNSUPPORTED.  Null pointers, R < 0, N < 1 -> TGTC_ERR_ARG; R == 0 -> TGTC_OK. */
int tgtc_nerf_forward_list(const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts,
                           int64_t R, int N, const uint32_t* live, const uint32_t* n_live, float* rgb, void* stream);

/* ------------------------------------------------------------------ a6: alpha compositing
 * utils.py:354-386 alpha_composition with sigma_noise_std=0, white_bkgd=False.  weights may be NULL. */
int tgtc_composite(const float* rgb, const float* sigma, const float* ts, int64_t R, int N,
                   float* rgb_exp, float* t_exp, float* weights, void* stream);

/* Training-side forms of a6 (train_tgtcs.py:218-309 differentiates through alpha_composition):
 * composite_train: sigma + noise in front of the ReLUs (noise float [R,N] = randn * sigma_noise_std drawn by the caller,
 *   utils.py:371-376, or NULL) and the optional white background (utils.py:381-384).
 * composite_backward: dL/d rgb [R,N,3] and dL/d sigma [R,N] from dL/d rgb_exp [R,3], dL/d t_exp [R], dL/d weights [R,N]
 *   (any of the three may be NULL = zero); either output may be NULL. */
int tgtc_composite_train(const float* rgb, const float* sigma, const float* ts, const float* noise, int white_bkgd,
                         int64_t R, int N, float* rgb_exp, float* t_exp, float* weights, void* stream);
int tgtc_composite_backward(const float* rgb, const float* sigma, const float* ts, const float* noise, int white_bkgd,
                            int64_t R, int N, const float* grad_rgb_exp, const float* grad_t_exp,
                            const float* grad_weights, float* grad_rgb, float* grad_sigma, void* stream);

/* ------------------------------------------------------------------ a7: fine sampling
 * utils.py:573-580 sampling_pts_fine_torch -> utils.py:583-609 sample_pdf(det=True), then the sorted merge.
 * ts [R,N], weights [R,N] -> ts_out [R,N+n_fine] ascending; pts_out [R,N+n_fine,3] double or NULL. */
int tgtc_sample_fine(const double* rays_o, const double* rays_d, const float* ts, const float* weights,
                     int64_t R, int N, int n_fine, double* pts_out, float* ts_out, void* stream);

/* a6 (weights only) + a7 (depths only) of a ray in ONE kernel: what the chain renders run between their passes when no
 * coarse image is asked.  sigma [R,N], ts [R,N] -> ts_out [R,N+n_fine], the bits of tgtc_composite(weights) followed by
 * tgtc_sample_fine on the same planes; weights_out [R,N] (the bits of tgtc_composite's weights) or NULL, in which case the
 * weights never reach memory.  The sorted merge is two binary searches per element where a ray's coarse depths and its new
 * samples are each non-decreasing (checked per ray on the device), the stable counting sort of tgtc_sample_fine otherwise.
 * 3 <= N <= 256, n_fine >= 1, N + n_fine <= 512, else TGTC_ERR_UNSUPPORTED; null sigma / ts / ts_out -> TGTC_ERR_ARG;
 * R == 0 -> TGTC_OK.  TGTC_PER_RAY_PAIR=1 in the environment makes the render entry points keep the two-kernel pair.
 * _traced: the same launch; took_sort uint32 [R] receives 1 for a ray that took the counting sort, 0 for a merged ray. */
int tgtc_coarse_to_fine(const float* sigma, const float* ts, int64_t R, int N, int n_fine, float* ts_out,
                        float* weights_out, void* stream);
int tgtc_coarse_to_fine_traced(const float* sigma, const float* ts, int64_t R, int N, int n_fine, float* ts_out,
                               float* weights_out, uint32_t* took_sort, void* stream);

/* tgtc_composite that reads rgb[r,i] only where sigma[r,i] > 0 and leaves every other sample out of the colour sums: over
 * ANY bits at those entries (NaN patterns included) the outputs are the bits of tgtc_composite over a plane that holds +0
 * there.  What the two-phase fine pass composites with, instead of zero-filling its colour plane.  weights may be NULL. */
int tgtc_composite_live_colours(const float* rgb, const float* sigma, const float* ts, int64_t R, int N,
                                float* rgb_exp, float* t_exp, float* weights, void* stream);

/* ------------------------------------------------------------------ render paths
 * Which kernels render a frame is the caller's explicit choice, resolved by ONE rule (tgtc_render_path), so that a ray's
 * result never depends on the size of a buffer or on R:
 *   TGTC_PATH_RAY_KERNEL  one launch of the persistent ray kernel (a wavefront owns a ray; per-sample tensors never exist;
 *                         HBM sees 48 B of ray in and 16 B of pixel out); the workspace is not touched and may be NULL.
 *                         Built when n_coarse and n_coarse+n_fine are multiples of 16 (32 in TGTC_PREC_FP16), n_coarse <= 192,
 *                         n_coarse+n_fine <= 256, no coarse image is requested, and the precisions (coarse + fine) are
 *                         fp16x3+fp16x3, fp16x3+fp16_fp6 or fp16+fp16 (plain), fp16x3 in all three handles (stylised).
 *   TGTC_PATH_CHAIN       the same arithmetic as a sequence of per-sample kernels through `workspace` (device scratch of at
 *                         least tgtc_render_workspace_bytes(R, n_coarse, n_fine) bytes); every shape and precision.
 *                         For fp16x3 (coarse) + fp16_fp6 (fine) this is the split path: its fine pass runs ~10 % faster on
 *                         the two-tile per-sample kernel (csrc/mlp_nerf_mx2.hip) than inside the ray kernel, and the
 *                         per-sample tensors cost 0.3 % of the frame in HBM traffic.
 *   TGTC_PATH_AUTO        the fastest: CHAIN for fp16x3 + fp16_fp6, otherwise RAY_KERNEL where it is built, otherwise CHAIN.
 * tgtc_render_path is pure host code (no GPU needed): it returns the path `request` resolves to for these precisions
 * (prec_style = -1 for the plain render), sample counts and want_coarse (nonzero: the coarse image is requested),
 * TGTC_ERR_UNSUPPORTED when RAY_KERNEL is requested where it is not built, and TGTC_ERR_ARG for a bad enum or
 * n_coarse < 3 or n_fine < 1. */
#define TGTC_PATH_AUTO 0
#define TGTC_PATH_RAY_KERNEL 1
#define TGTC_PATH_CHAIN 2
int tgtc_render_path(int request, int prec_coarse, int prec_fine, int prec_style, int n_coarse, int n_fine, int want_coarse);

/* The first half of a ray kernel on its own -- coarse depths -> coarse sigma -> weights -> inverse-CDF fine sampling + merge --
 * as the depths-only instance of the plain ray kernel computes it (the one the stylised chain, the multi-latent, culled and
 * restyle renders take their depths from): ts_out float [R, n_coarse + n_fine], ascending, the depths a ray kernel built
 * for this coarse handle evaluates its fine pass at.  jitter: float [R,n_coarse] or NULL.  One launch, no workspace.
 * TGTC_ERR_UNSUPPORTED where no plain ray kernel is built for (coarse precision, n_coarse, n_fine) -- the shape rule of
 * TGTC_PATH_RAY_KERNEL above -- or the coarse handle is TGTC_PREC_FP16_FP6 (no depths-only instance exists for it);
 * null pointers or a handle that is not a NeRF handle -> TGTC_ERR_ARG;  R == 0 -> TGTC_OK without a launch. */
int tgtc_render_depths(const tgtc_net* coarse, const double* rays_o, const double* rays_d, int64_t R, int n_coarse,
                       int n_fine, float near_, float far_, const float* jitter, float* ts_out, void* stream);

/* ------------------------------------------------------------------ fused plain render (cal_geometry chain)
 * rendering.py:27-51: coarse sample -> NeRF(coarse) -> composite -> fine sample -> NeRF(fine) -> composite.
 * jitter: float [R,n_coarse] or NULL.  Outputs: rgb float [R,3], depth float [R]; optional coarse outputs.
 * path: a TGTC_PATH_* request, resolved by tgtc_render_path (errors are returned as it returns them).  A render that
 * resolves to TGTC_PATH_CHAIN with a NULL or too small workspace returns TGTC_ERR_ARG; no path is ever switched for it. */
size_t tgtc_render_workspace_bytes(int64_t R, int n_coarse, int n_fine);
int tgtc_render_rays_plain(const tgtc_net* coarse, const tgtc_net* fine, const double* rays_o, const double* rays_d,
                           int64_t R, int n_coarse, int n_fine, float near_, float far_, const float* jitter, int path,
                           void* workspace, size_t workspace_bytes,
                           float* rgb_fine, float* t_fine, float* rgb_coarse, float* t_coarse, void* stream);

/* ------------------------------------------------------------------ two-phase fine pass of the plain chain
 * A fine sample with sigma <= 0 has alpha = 1 - exp(-relu(sigma) x delta) = 0 exactly, weight +0, and leaves the pixel sum
 * unchanged (acc + 0 x c), so its colour head is work the image does not need.  Inside TGTC_PATH_CHAIN, for a fine handle
 * in TGTC_PREC_FP16_FP6, the fine pass can therefore run as: the density-only launch of the fine network over all
 * R x (n_coarse + n_fine) samples; the compaction of the samples with sigma > 0 into an ascending device-side list; a
 * zero-fill of the colour plane; tgtc_nerf_forward_list over that list; the dense compositing kernel, unchanged.  The list
 * and the compaction scratch live in workspace planes that are dead by then: tgtc_render_workspace_bytes is what it was.
 * tgtc_render_path and the TGTC_PATH_* values have no part in it.
 * Images: the same BITS as the dense fine pass for finite network outputs.  The one accepted difference: a sample with
 *   sigma <= 0 whose colour is not finite contributed 0 x NaN = NaN to the dense sum and contributes +0 now.
 * Cost: with live share L, f the full fine launch and s the density-only one, s + L x f + ~0.5 ms instead of f: a gain
 *   below L* = 1 - s / f and a loss above, hence a policy, held by the FINE HANDLE:
 *   TGTC_CULL_AUTO (default)  cull iff the live share of the last chain render with this fine handle THAT HAS LANDED is
 *                             below the library's threshold (L* less a margin); unknown share: dense.
 *   TGTC_CULL_OFF             always dense (and no statistic is taken).
 *   TGTC_CULL_ON              always two-phase.
 *   Every mode takes the dense pass where the list does not fit the dead planes (6 x R x n_coarse floats <
 *   R x (n_coarse + n_fine) x 4 + 8192 bytes), where R x (n_coarse + n_fine) >= 2^31, or for a fine handle in
 *   TGTC_PREC_FP16.
 * A fine handle in TGTC_PREC_FP16X3 takes the two-phase pass under TGTC_CULL_ON ONLY (no break-even has chosen a threshold for
 *   it: under AUTO and OFF its pass is dense, with the launches and counters it always had, and no statistic is taken).  Its
 *   colour phase is tgtc_nerf_forward_list_x3 (below), its density launch tgtc_nerf_forward_rays(rgb = NULL); the compositor,
 *   the bits and the accepted difference are those above.  No stash exists for it.
 * Statistic: the handle owns one pinned 8-byte host word.  Every chain render with it as the fine handle (AUTO and ON; in
 *   dense mode at the price of one run of the compaction's count kernel over sigma_f) ends with an asynchronous copy of
 *   (live count, R x (n_coarse + n_fine)) into it (none where the dead planes are smaller than the 8192-byte scratch).  AUTO reads the word without waiting for the device: a pipeline that
 *   never synchronises stays dense until a value lands.  Only the time depends on it, never a pixel.
 * tgtc_net_set_cull: TGTC_ERR_ARG for a bad mode or a handle that is not a NeRF handle.
 * tgtc_net_live_fraction: the share that has landed, or -1 while none has (and for NULL / style handles).
 * tgtc_net_culled_renders: how many chain renders with this fine handle took the two-phase pass (-1 for NULL / style handles).
 * Renders that share one fine handle from several host threads must not race on these calls. */
#define TGTC_CULL_AUTO 0
#define TGTC_CULL_OFF 1
#define TGTC_CULL_ON 2
int tgtc_net_set_cull(tgtc_net* net, int mode);
float tgtc_net_live_fraction(const tgtc_net* net);
long long tgtc_net_culled_renders(const tgtc_net* net);

/* tgtc_nerf_forward_list for TGTC_PREC_FP16X3 handles: the full network (trunk, density head, base_remap, colour head) over a
 * device-side list, the arithmetic of tgtc_nerf_forward_rays sample for sample (csrc/mlp_nerf_x3_list.hip: a persistent
 * kernel, one workgroup per CU at most, 128 list slots per pass).  rgb[s] of the listed samples -- the bits
 * tgtc_nerf_forward_rays(rgb, sigma) gives them -- and, where sigma is not NULL, sigma[s], the bits of
 * tgtc_nerf_forward_rays(rgb = NULL); nothing else is touched.  List rules as tgtc_nerf_forward_list: n_live is a DEVICE
 * pointer, *n_live == 0 writes nothing, a listed index >= R x N is not written.
 * Any other precision, or R x N >= 2^31 -> TGTC_ERR_UNSUPPORTED.  Null pointers (sigma excepted), R < 0, N < 1 or a handle
 * that is not a NeRF handle -> TGTC_ERR_ARG; R == 0 -> TGTC_OK without a launch. */
int tgtc_nerf_forward_list_x3(const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts, int64_t R,
                              int N, const uint32_t* live, const uint32_t* n_live, float* rgb, float* sigma, void* stream);

/* The stash: the two-phase fine pass without the second trunk.  The list launch above runs layers 0-7 and the sigma head
 * again on samples the density launch has just finished; only base_remap and the colour head are new work.  With a STASH
 * attached to the fine handle the two-phase pass is instead: a density launch that also parks layer 7's output (58 dwords per
 * lane, 928 bytes per sample, + 4 for the sample index) of every sample with sigma > 0 in the stash; the zero-fill; a
 * heads-only launch (base_remap, colour head) over the parked samples; tgtc_nerf_forward_list over the samples that found
 * no room (an empty list runs its prologue alone); the dense compositing kernel.  Same bits as without a stash.
 * The stash is a caller-owned device buffer of 1024 regions, one per wave of the two launches; a wave parks its live
 * samples in its own region and what does not fit goes to the overflow list, so ANY size is correct and a size for the
 * scene's live share is fast.  tgtc_net_stash_bytes(R, nt, share): the size at which a wave's region holds `share` of the
 * samples it sees in a render of R rays x nt samples (0 for R <= 0, nt <= 0 or a negative share).  RayRenderer sizes it for
 * the share above which AUTO stops culling (0.14): about 4 GB for 400 x 400 rays at 128 + 64.
 * tgtc_net_set_stash(net, ptr, bytes): attach (ptr aligned to 256 bytes; the buffer stays the caller's and must outlive
 * every render that uses it) or, with (NULL, 0), detach.  TGTC_ERR_UNSUPPORTED for a handle that is not TGTC_PREC_FP16_FP6;
 * TGTC_ERR_ARG for a misaligned pointer or fewer bytes than one slot per region (tgtc_net_stash_bytes(1, 1, 0)).
 * Without a stash, with TGTC_CULL_OFF, or where AUTO decides for the dense pass, nothing changes.  Renders that share a
 * handle share its stash: like a shared workspace, they must be ordered on one stream.
 * The two launches as entries of their own (tests, tools): tgtc_nerf_stash_fill writes sigma [R,N] as
 * tgtc_nerf_forward_rays(rgb = NULL) does, zeroes `scratch` (8192 bytes: word 0 becomes the overflow list's length, words
 * 64.. the live count of each wave) and fills the stash and `overflow` (uint32 [R x N]); tgtc_nerf_stash_heads writes
 * sigmoid(rgb) of the parked samples into rgb [R,N,3] and nothing else.  Both need a stash attached (TGTC_ERR_ARG). */
size_t tgtc_net_stash_bytes(int64_t R, int nt, float share);
int tgtc_net_set_stash(tgtc_net* net, void* ptr, size_t bytes);
int tgtc_nerf_stash_fill(const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts, int64_t R, int N,
                         float* sigma, uint32_t* scratch, uint32_t* overflow, void* stream);
int tgtc_nerf_stash_heads(const tgtc_net* net, const double* rays_o, const double* rays_d, int64_t R, int N,
                          uint32_t* scratch, float* rgb, void* stream);

/* ------------------------------------------------------------------ density screen of the plain chain
 * All a frame takes from a density is relu(sigma): a sample with sigma <= 0 has alpha 0 and weight +0 exactly, in the coarse
 * weights that feed the inverse CDF and in the fine composite.  A NeRF handle in TGTC_PREC_FP16X3 or TGTC_PREC_FP16_FP6 can
 * carry its weights a second time, in the form tgtc_nerf_create packs for TGTC_PREC_FP16 (an allocation of its own), and a
 * margin m.  A SCREENED pass of tgtc_render_rays_plain on TGTC_PATH_CHAIN is then: the fp16 sigma-only launch over all
 * samples; the compaction of the candidates (screen density not <= -m; NaN and +inf are candidates) into an ascending
 * device-side list; the pass's exact kernel over that list alone.  While |sigma_screen - sigma_exact| < m every sample the
 * list leaves out has sigma_exact < 0, and the frame has the BITS of the dense pass.
 * THE DOMAIN RULE.  The screen decides only inside its declared box |x|, |y|, |z| <= 2 (sample position o + t d in float64; a
 *   coordinate exactly +-2 is inside).  A sample with a coordinate outside it, or not finite, gets NaN from the screen launch
 *   and so is ALWAYS a candidate: the exact kernel computes it, as in a dense pass -- the bits hold there by construction,
 *   whatever near / far and whatever the scene's scale.  Inside the box they rest on the margin, which is measured, not
 *   proven: m is calibrated on rays that fill this box, and tests/test_screen_domain_gpu.py holds the error to m / 2 on it for
 *   the synthetic nets in four weight families (largest seen: 0.13 m).  NDC frames (|x|, |y| <= 1.3, |z| <= 1) never meet the
 *   rule; a scene that lives outside the box renders correctly with every sample a candidate, and AUTO then leaves its
 *   passes dense.
 *   coarse pass: when no coarse image is asked and the coarse handle (fp16x3) has a screen; the exact densities of the
 *                candidates from tgtc_nerf_sigma_list.  List + scratch live in the fine colour plane (dense where
 *                R x (n_coarse + n_fine) x 12 bytes < R x n_coarse x 4 + 8192).
 *   fine pass:   a fine handle in fp16mx with a screen; density AND colour of the candidates from
 *                tgtc_nerf_forward_list_sigma, the compositor of the two-phase pass.  List + scratch live where the
 *                two-phase pass keeps its list; no stash is used.  Counts in tgtc_net_culled_renders; TGTC_CULL_OFF on the
 *                handle switches it off as well.  A fine handle in fp16x3 with a screen is screened the same way under
 *                TGTC_CULL_ON only (the candidates from tgtc_nerf_forward_list_x3 with sigma; AUTO is pass 3 of
 *                tgtc_screen_auto_decision); under TGTC_CULL_AUTO / OFF its screen has no part in a plain render.
 * tgtc_render_workspace_bytes is what it was; there is no host synchronisation in a render.
 * tgtc_net_enable_screen(net, stream): packs the fp16 form and calibrates the margin -- screen and exact sigma-only launches
 *   on 256 fixed host-generated rays (each between two points uniform in the box) x 128 depths equally spaced on [0, 1]: the
 *   positions fill the box; m = 8 x max |sigma_screen - sigma_exact|.  ONE host synchronisation, a host
 *   call like packing.  Idempotent.  A zero or non-finite calibration error leaves the screen disabled (TGTC_OK; the handle
 *   renders as before).  Style handles and TGTC_PREC_FP16 handles -> TGTC_ERR_UNSUPPORTED; NULL -> TGTC_ERR_ARG.
 * tgtc_net_screen_margin: m, or -1 when no screen is enabled (and for NULL).
 * tgtc_net_set_screen: the policy of the passes this handle is screened in.
 *   TGTC_SCREEN_AUTO (default)  screen iff the candidate share of the last such pass THAT HAS LANDED in the handle's pinned
 *                               word is below the pass's threshold; unknown: not screened.  Read without waiting.
 *   TGTC_SCREEN_OFF             never (and no statistic is taken).
 *   TGTC_SCREEN_ON              wherever the list fits.
 *   "Not screened" is the pass as it was: in the fine pass whatever TGTC_CULL_* and the stash decide.
 *   TGTC_ERR_ARG for a bad mode or a handle that is not a NeRF handle, TGTC_ERR_UNSUPPORTED for a TGTC_PREC_FP16 handle.
 * tgtc_net_screen_fraction: the candidate share that has landed (from the compaction's count in a screened pass, from one run
 *   of the count kernel at -m over the exact densities otherwise), or -1 while none has.
 * tgtc_net_screened_renders: how many chain renders screened their pass with this handle (-1 for NULL / no screen state).
 * tgtc_screen_list_fits / tgtc_screen_auto_decision: the two rules as pure host functions -- does a list of up to M indices
 *   and the 8192-byte scratch fit `bytes`; does AUTO screen pass 0 (coarse) / 1 (fine) / 2 (the sigma-only fine pass of the
 *   chain geometry, below) / 3 (the two-phase fine pass of a fine handle in fp16x3) on a landed (candidates, total).
 * The launches as entries of their own (tests, tools):
 *   tgtc_nerf_screen_rays: sigma [R,N] from the screen form (TGTC_ERR_UNSUPPORTED without a screen): NaN for exactly the
 *     samples outside the box or not finite, and for the others the bits of the sigma-only launch of a TGTC_PREC_FP16 handle
 *     of the same layers.
 *   tgtc_nerf_sigma_list: sigma[s] of the listed samples, the bits of tgtc_nerf_forward_rays(rgb = NULL), nothing else
 *     touched; TGTC_PREC_FP16X3 handles only (csrc/mlp_nerf_x3s.hip, the IN_LIST instance).  List rules as tgtc_nerf_forward_list.
 *   tgtc_nerf_forward_list_sigma: tgtc_nerf_forward_list that also writes sigma[s] of the listed samples. */
#define TGTC_SCREEN_AUTO 0
#define TGTC_SCREEN_OFF 1
#define TGTC_SCREEN_ON 2
int tgtc_net_enable_screen(tgtc_net* net, void* stream);
float tgtc_net_screen_margin(const tgtc_net* net);
int tgtc_net_set_screen(tgtc_net* net, int mode);
float tgtc_net_screen_fraction(const tgtc_net* net);
long long tgtc_net_screened_renders(const tgtc_net* net);
int tgtc_screen_list_fits(size_t bytes, int64_t M);
int tgtc_screen_auto_decision(int pass, uint32_t candidates, uint32_t total);
int tgtc_nerf_screen_rays(const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts, int64_t R, int N,
                          float* sigma, void* stream);
int tgtc_nerf_sigma_list(const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts, int64_t R, int N,
                         const uint32_t* live, const uint32_t* n_live, float* sigma, void* stream);
int tgtc_nerf_forward_list_sigma(const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts, int64_t R,
                                 int N, const uint32_t* live, const uint32_t* n_live, float* rgb, float* sigma, void* stream);

/* ------------------------------------------------------------------ a8: latent table
 * models.py:490-506 StyleLatents_variational.forward.  latents float [S,F,D] device, mu float [S,D] device,
 * style_ids / frame_ids int64 [R] device.  tile7: the llff `repeat((7,1))` wrap (models.py:496).
 * The ids live on the device and are NOT checked here: every style id must lie in [0, S), every frame id must be >= 0 and
 * style * F + frame must be < S * F (< 7 * S * F with tile7).  The kernels index mu[style] and the flattened table with them,
 * so anything else reads -- and tgtc_latents_backward's atomics write -- out of bounds.  They are the caller's
 * responsibility (the Python binding raises IndexError on the host before it launches: models.check_latent_ids). */
int tgtc_latents_forward(const float* latents, const float* mu, int S, int F, int D, const int64_t* style_ids,
                         const int64_t* frame_ids, int64_t R, float sigma_scale, int tile7, float* out, void* stream);
/* Its gradient for the training side (Style_train optimises the table, train_tgtcs.py:312-571): grad_out [R,D] ->
 * d_latents [S,F,D] += sigma_scale * g at the gathered rows, d_mu [S,D] += (1 - sigma_scale) * g; both buffers zeroed by the
 * caller, either may be NULL.  The same rule for the ids: unchecked here, the caller's responsibility. */
int tgtc_latents_backward(const float* grad_out, int S, int F, int D, const int64_t* style_ids, const int64_t* frame_ids,
                          int64_t R, float sigma_scale, int tile7, float* d_latents, float* d_mu, void* stream);

/* ------------------------------------------------------------------ a13 (image epilogue)
 * rendering.py:66-71 (cal_geometry), :202-206 (render_style), :358-361 (render_train_style): what the drivers do to
 * every finished frame before imageio.imwrite -- per-frame sv_t = (t - min t) / (max t - min t + eps), then
 * np.array(x * 255, np.int32) and to8b = np.uint8 cast (utils.py:463; wraps modulo 256, e.g. 1.0039 -> 0).
 * rgb float [frames*pixels,3], t float [frames*pixels] -> rgb8 uint8 [frames*pixels,3], depth8 uint8 [frames*pixels]
 * (either output may be NULL).  eps = 1e-7 for cal_geometry / render_style, 0 for render_train_style (whose depth
 * image is the same plane written three times, host side).  Only 4 bytes per ray cross PCIe afterwards. */
int tgtc_image_epilogue(const float* rgb, const float* t, int64_t frames, int64_t pixels, float eps, unsigned char* rgb8,
                        unsigned char* depth8, void* stream);

/* ------------------------------------------------------------------ a10+a11: the two style MLPs
 * models.py:120-147 StyleMLP_before_concat (5 linears: 95,288,288,288,351 -> 256) and
 * models.py:149-180 StyleMLP_Wild_multilayers (8 linears: 607,288,288,288,351,288,288 -> 256, 288 -> 3). */
int tgtc_style_create(const tgtc_linear* concat_layers, int n_concat, const tgtc_linear* style_layers, int n_style,
                      int precision, tgtc_net** out);
/* x float [M,63], latent float [M,32] -> concat_features float [M,256] */
int tgtc_concat_mlp_forward(const tgtc_net* style, const float* x, const float* latent, int64_t M,
                            float* concat_features, void* stream);
/* x float [M,63], concated float [M,512], latent float [M,32] -> rgb float [M,3] */
int tgtc_style_mlp_forward(const tgtc_net* style, const float* x, const float* concated, const float* latent,
                           int64_t M, float* rgb, void* stream);
/* One stylised pass over rays (rendering.py:122-142): NeRF trunk (sigma, base_remap), concat MLP on the per-ray
 * latent z [R,32], style MLP on mean(z) broadcast.  Outputs rgb [R,N,3], sigma [R,N]. */
int tgtc_styled_forward_rays(const tgtc_net* nerf, const tgtc_net* style, const double* rays_o, const double* rays_d,
                             const float* ts, const float* z, int64_t R, int N, float* rgb, float* sigma, void* stream);
/* The stylised render of rays (rendering.py:109-182 render_style): like tgtc_render_rays_plain with the stylised colour
 * (per-ray latent z float [R,32]) and the same `path` argument.  TGTC_PATH_RAY_KERNEL is ONE launch of the stylised ray
 * kernel (coarse passes, fine sampling, concat MLP + NeRF trunk + style MLP per fine tile and compositing back to back);
 * TGTC_PATH_CHAIN the same arithmetic as a sequence of per-sample kernels through `workspace` (its coarse passes and fine
 * sampling are one launch of the plain ray kernel's first half where that is built and no coarse image is requested). */
int tgtc_render_rays_styled(const tgtc_net* coarse, const tgtc_net* fine, const tgtc_net* style,
                            const double* rays_o, const double* rays_d, const float* z, int64_t R, int n_coarse,
                            int n_fine, float near_, float far_, const float* jitter, int path, void* workspace,
                            size_t workspace_bytes, float* rgb_fine, float* t_fine, float* rgb_coarse,
                            float* t_coarse, void* stream);

/* ------------------------------------------------------------------ K latent sets per ray, shared geometry
 * The same rays under K latents (the styles of one frame, a --sigma_scale sweep, a style transition).  In the stylised
 * chain the latent enters only the concat MLP and the style MLP; the coarse pass, the fine depths, the fine NeRF trunk
 * (sigma, base_remap), hence the compositing weights and the depth, are functions of the ray alone and are computed ONCE:
 * per ray at 128 + 64 samples 169.8 M multiply-accumulates are shared and 182.4 M are per latent, K latents cost
 * 169.8 + K x 182.4 instead of K x 352.2.  All K images have the same sample positions and bit-identical depth.
 *
 * Layouts:  z float [K,R,32];  rgb float [K,R,N,3];  sigma float [R,N] (one plane, may be NULL);
 *           rgb_fine float [K,R,3];  t_fine float [R].
 * Identity: per latent the kernel performs the MFMA sequence of tgtc_styled_forward_rays on the same operands, so
 *   rgb[k] and sigma of tgtc_styled_forward_rays_multi are the bits of tgtc_styled_forward_rays(..., z[k], ...), and
 *   rgb_fine[k], t_fine of tgtc_render_rays_styled_multi are the bits of tgtc_render_rays_styled(..., z[k], ...,
 *   TGTC_PATH_CHAIN, ...) without coarse outputs; K = 1 is a valid call.
 * The render is always the chain of per-sample kernels (there is no `path`, tgtc_render_path has no say): the geometry
 * half of the stylised TGTC_PATH_CHAIN, ONE launch of the multi-latent kernel (csrc/mlp_style_multi.hip), K compositing
 * launches over the shared sigma / depths.  There are no coarse-image outputs.
 * Errors: K < 1, R < 0, wrong handle kinds, null pointers, n_coarse < 3, n_fine < 1, NeRF (fine) and style handles of
 *   different precisions, a workspace below tgtc_render_styled_multi_workspace_bytes -> TGTC_ERR_ARG;
 *   K x R x N >= 2^31 (N = n_coarse + n_fine for the render) -> TGTC_ERR_UNSUPPORTED: chunk the rays.  R == 0 -> TGTC_OK.
 * Workspace (device scratch, 0 is returned for negative arguments or K < 1): six planes, each rounded up to 256 bytes, in
 *   this order:  ts_c, sigma_c, w_c float [R,n_coarse];  ts_f, sigma_f float [R,n_coarse+n_fine];
 *   rgb_f float [K,R,n_coarse+n_fine,3].  The per-sample colour dominates: a 400 x 400 frame at 128 + 64 and K = 4 takes
 *   about 1.5 GB (369 MB per latent); chunk the rays where that is too much.
 * Scratch slab: the kernel keeps base_remap of the tile in a second per-workgroup region (128 KiB per CU, 32 MiB on 256
 *   CUs) that tgtc_style_create allocates beside the first.  Like the first it belongs to the STYLE HANDLE: two launches
 *   that use one style handle (these entry points, tgtc_styled_forward_rays, tgtc_render_rays_styled) must not overlap
 *   on different streams. */
int tgtc_styled_forward_rays_multi(const tgtc_net* nerf, const tgtc_net* style, const double* rays_o,
                                   const double* rays_d, const float* ts, const float* z, int K, int64_t R, int N,
                                   float* rgb, float* sigma, void* stream);
size_t tgtc_render_styled_multi_workspace_bytes(int64_t R, int n_coarse, int n_fine, int K);
int tgtc_render_rays_styled_multi(const tgtc_net* coarse, const tgtc_net* fine, const tgtc_net* style,
                                  const double* rays_o, const double* rays_d, const float* z, int K, int64_t R,
                                  int n_coarse, int n_fine, float near_, float far_, const float* jitter,
                                  void* workspace, size_t workspace_bytes, float* rgb_fine, float* t_fine, void* stream);

/* ------------------------------------------------------------------ K latent sets per ray, style networks on live samples only
 * tgtc_render_rays_styled_multi with the per-latent work culled.  In the stylised chain sigma depends on the ray alone, so
 * the compositing weight w_i = alpha_i x T_i of every fine sample is known before a style network has run; a sample with
 * w_i == 0 (relu(sigma_i) = 0) enters rgb = sum w_i x c_i as exactly +0 whatever finite colour the style MLP would give.
 * Order of work on the stream: the geometry half of the multi render; a sigma-only pass of the fine NeRF over all R x N
 * samples (N = n_coarse + n_fine); tgtc_composite's kernel for t_fine and the weights plane w_f; a compaction that writes
 * the ASCENDING list live[] of the sample indices s = r x N + i with w_f[s] > min_weight and its length, both on the
 * device; hipMemsetAsync of the K colour planes; ONE launch of the indexed multi-latent kernel (csrc/mlp_style_sparse.hip:
 * NeRF trunk + concat MLP + style MLP over the list, the number of tiles read from the device count, rgb scattered to the
 * dense planes); K compositing launches over the shared sigma / depths.  The host never learns the count.
 * min_weight = 0: rgb_fine[k], t_fine are the BITS of tgtc_render_rays_styled_multi (a live sample's result does not depend
 *   on which samples share its tile; a dead sample contributes +0 either way).
 * min_weight > 0: t_fine is unchanged (depth never sees the colours); colours lie in [0,1], so each ray and channel moves
 *   by at most the sum of the ray's dropped weights (those with 0 < w <= min_weight), up to float32 summation rounding.
 * Cost per fine sample with live fraction f: 491 264 + f x (556 800 + K x 950 112) multiply-accumulates against
 *   556 800 + K x 950 112 of the multi render; break-even at K = 1 is f ~ 0.67, and with everything live the call costs
 *   1.33 x the multi render.  It is a mode the caller asks for; no `path` rule ever selects it.
 * Layouts, conventions and errors are those of tgtc_render_rays_styled_multi; additionally min_weight < 0 or NaN ->
 *   TGTC_ERR_ARG.  Every argument check returns before a device is touched.
 * live_count: device pointer to ONE uint32 that receives the length of the list, or NULL.
 * Workspace (0 is returned for negative arguments or K < 1), each plane rounded up to 256 bytes, in this order:
 *   the six planes of tgtc_render_styled_multi_workspace_bytes(R, n_coarse, n_fine, K);
 *   w_f   float  [R,N]   the fine compositing weights (the bits of tgtc_composite's weights output on sigma_f, ts_f);
 *   live  uint32 [R x N] the list (the first `count` entries are written);
 *   8192 bytes of scratch for the compaction: word 0 is the count, the rest partial counts.
 * Scratch slab: as for the multi render, both slab regions of the STYLE HANDLE are used; launches on one style handle
 *   must not overlap. */
size_t tgtc_render_styled_sparse_workspace_bytes(int64_t R, int n_coarse, int n_fine, int K);
int tgtc_render_rays_styled_sparse(const tgtc_net* coarse, const tgtc_net* fine, const tgtc_net* style,
                                   const double* rays_o, const double* rays_d, const float* z, int K, int64_t R,
                                   int n_coarse, int n_fine, float near_, float far_, const float* jitter,
                                   float min_weight, void* workspace, size_t workspace_bytes, float* rgb_fine,
                                   float* t_fine, uint32_t* live_count, void* stream);

/* ------------------------------------------------------------------ restyle rays from a cached geometry
 * Steps 1-4 of tgtc_render_rays_styled_sparse (geometry half, sigma pass, depth + weights, compaction) depend on the ray
 * alone.  tgtc_geometry_build runs them once, tgtc_geometry_pack keeps what a later render needs as a compact device
 * buffer, and tgtc_restyle_rays renders the same rays under new latents from that buffer: ONE launch of the compact form
 * of the indexed multi-latent kernel over the cached list, ONE compositing launch over (latent, ray), one device copy of
 * the depth image.  No coarse handle, no hipMemset, no dense per-sample plane.
 * Identity: rgb_fine, t_fine of tgtc_restyle_rays are the BITS of tgtc_render_rays_styled_sparse with the build's
 *   min_weight: a live sample is the same column of the same MFMA sequence on the same operands, and a sample that is not in
 *   the list enters the dense compositing sum as acc + w x 0 or acc + 0 x c, which leaves acc unchanged.
 * It is a mode the caller asks for; TGTC_PATH_AUTO never selects it.
 *
 * tgtc_geometry_build: `workspace` is the sparse workspace at K = 1, tgtc_render_styled_sparse_workspace_bytes(R, n_coarse,
 *   n_fine, 1), in that layout; the depth image is also left in the first R floats of its colour plane, where the pack
 *   reads it.  t_fine float [R] or NULL.  live_count: device pointer to ONE uint32, required: the caller reads it once (the
 *   one synchronisation per build) to allocate the cache.  No style handle is involved.
 * tgtc_geometry_pack: workspace of the build, count = the value read from live_count -> cache (device, at least
 *   tgtc_geometry_cache_bytes(R, count) bytes).  Deterministic, no atomics.  Cache layout, every plane rounded up to 256 bytes:
 *     header    256 bytes: uint32 words  0 magic 0x43475447 ("TGGC"), 1 layout version (1), 2-3 R (low, high), 4 N =
 *               n_coarse + n_fine, 5 count, 6 the bits of min_weight, the rest 0
 *     t_fine    float  [R]
 *     ray_start uint32 [R+1]    list entries [ray_start[r], ray_start[r+1]) are the live samples of ray r
 *     live      uint32 [count]  dense sample indices s = r x N + i, ascending
 *     ts_live   float  [count]  ts_f[live]
 *     w_live    float  [count]  w_f[live]
 *   About 12 bytes per live sample + 8 per ray.  The buffer is position independent: it may be copied, saved and reloaded.
 * tgtc_restyle_rays: z float [K,R,32], rgb_fine float [K,R,3], t_fine float [R] or NULL.  rays_o / rays_d, n_coarse, n_fine
 *   and the fine handle must be those of the build (the cache stores depths, not positions).  workspace: at least
 *   tgtc_restyle_workspace_bytes(count, K) bytes = rgb_live float [K,count,3] rounded up to 256 (may be NULL when count == 0).
 *   count == 0: no style kernel is launched; rgb_fine is +0 and t_fine is copied.  The call reads the cache only.
 * Both size functions return 0 for negative arguments (K < 1).
 * Errors (every argument check returns before a device is touched): null pointers, K < 1, R < 0, count < 0, wrong handle
 *   kinds, fine and style handles of different precisions, min_weight < 0 or NaN, n_coarse < 3, n_fine < 1, a cache or
 *   workspace below its size function, count > R x N -> TGTC_ERR_ARG;  R x N >= 2^31 or K x count >= 2^31 ->
 *   TGTC_ERR_UNSUPPORTED;  R == 0 -> TGTC_OK.
 * Scratch slab: tgtc_restyle_rays uses both slab regions of the STYLE HANDLE; launches on one style handle must not overlap. */
int tgtc_geometry_build(const tgtc_net* coarse, const tgtc_net* fine, const double* rays_o, const double* rays_d, int64_t R,
                        int n_coarse, int n_fine, float near_, float far_, const float* jitter, float min_weight,
                        void* workspace, size_t workspace_bytes, float* t_fine, uint32_t* live_count, void* stream);
size_t tgtc_geometry_cache_bytes(int64_t R, int64_t count);
int tgtc_geometry_pack(const void* workspace, int64_t R, int n_coarse, int n_fine, float min_weight, int64_t count,
                       void* cache, size_t cache_bytes, void* stream);
size_t tgtc_restyle_workspace_bytes(int64_t count, int K);
int tgtc_restyle_rays(const tgtc_net* fine, const tgtc_net* style, const double* rays_o, const double* rays_d, const float* z,
                      int K, int64_t R, int n_coarse, int n_fine, const void* cache, size_t cache_bytes, int64_t count,
                      void* workspace, size_t workspace_bytes, float* rgb_fine, float* t_fine, void* stream);

/* ------------------------------------------------------------------ frame-constant latents folded into per-latent biases
 * In a stylised frame the latent depends on (style, frame), not on the ray: the callers above receive K vectors copied R
 * times.  For a latent that is constant over a call, its k-step in each of the 13 layers of the two style networks computes
 * the same 256-vector for every sample -- a bias.  The entry points below take z float [K,32]:
 *   tgtc_style_fold_latents writes K bias tables, each in the layout of the handle's own pair bias table (16 KiB: 16 floats
 *     per row tile, concat layers 0..4 then style layers 0..7):
 *       b'[l][o] = b[l][o] + sum_j Wz[l][o][j] x u_j,   u = z[k] for the concat layers, u_j = mean(z[k]) for the style layers,
 *     from the handle's power-of-two equalised rows and biases (those its streams were packed from), accumulated in float64
 *     over j = 0..31 and rounded once.  z[k] = 0 reproduces the handle's table bit for bit.
 *   the folded kernels (csrc/mlp_style_sparse.hip) walk a second pair of streams the handle packs without the latent k-steps:
 *     576 + 1096 fragments per latent instead of 656 + 1209 (10.3 % fewer MFMAs per latent), no latent operand, no z plane.
 *     A folded layer is the unfolded layer's MFMA sequence with the latent k-step left out: with z = 0 the results are the
 *     bits of the unfolded siblings with zs = 0.  With z != 0 they differ from the unfolded ones within the precision's error
 *     (the fold is exact to float32 rounding; the unfolded kernels round the latent operand to fp16 or fp16 hi + lo).
 * They are modes the caller asks for; nothing selects them.  The geometry cache holds no latents: the same cache serves
 * tgtc_restyle_rays and tgtc_restyle_rays_folded.
 *
 * tgtc_style_folded_bytes(K): K x 16384; 0 for K < 1.
 * tgtc_style_fold_latents: z float [K,32] (device) -> folded (device, at least tgtc_style_folded_bytes(K) bytes).
 * tgtc_styled_forward_list_folded: the scattered kernel alone (the seam the parity tests use).  ts float [R,N]; folded: the K
 *   tables; live uint32 [*n_live] ascending sample indices s = r x N + i, n_live a DEVICE pointer to one uint32; rgb float
 *   [K,R,N,3], zero-filled by the caller: rgb[k,s] is written for the listed samples only.
 * tgtc_render_rays_styled_sparse_folded: tgtc_render_rays_styled_sparse with z float [K,32].  Workspace: the sparse workspace
 *   followed by one more plane, tgtc_style_folded_bytes(K) rounded up to 256 (the tables).
 * tgtc_restyle_rays_folded: tgtc_restyle_rays with z float [K,32].  Workspace: tgtc_restyle_workspace_bytes(count, K) followed
 *   by the same plane; count == 0 launches neither the fold nor a style kernel.
 * Errors and conventions are those of the unfolded siblings (every argument check returns before a device is touched):
 *   K < 1, null pointers, wrong handle kinds, differing precisions, min_weight < 0 or NaN, buffers below their size functions
 *   -> TGTC_ERR_ARG;  K x R x N >= 2^31 or K x count >= 2^31 -> TGTC_ERR_UNSUPPORTED;  R == 0 -> TGTC_OK.  The size and range
 *   checks come before the handles are looked at.  Both slab regions of the STYLE HANDLE are used; launches on one style handle
 *   must not overlap. */
size_t tgtc_style_folded_bytes(int K);
int tgtc_style_fold_latents(const tgtc_net* style, const float* z, int K, void* folded, size_t folded_bytes, void* stream);
int tgtc_styled_forward_list_folded(const tgtc_net* nerf, const tgtc_net* style, const double* rays_o, const double* rays_d,
                                    const float* ts, const void* folded, int K, int64_t R, int N, const uint32_t* live,
                                    const uint32_t* n_live, float* rgb, void* stream);
size_t tgtc_render_styled_sparse_folded_workspace_bytes(int64_t R, int n_coarse, int n_fine, int K);
int tgtc_render_rays_styled_sparse_folded(const tgtc_net* coarse, const tgtc_net* fine, const tgtc_net* style,
                                          const double* rays_o, const double* rays_d, const float* z, int K, int64_t R,
                                          int n_coarse, int n_fine, float near_, float far_, const float* jitter,
                                          float min_weight, void* workspace, size_t workspace_bytes, float* rgb_fine,
                                          float* t_fine, uint32_t* live_count, void* stream);
size_t tgtc_restyle_folded_workspace_bytes(int64_t count, int K);
int tgtc_restyle_rays_folded(const tgtc_net* fine, const tgtc_net* style, const double* rays_o, const double* rays_d,
                             const float* z, int K, int64_t R, int n_coarse, int n_fine, const void* cache, size_t cache_bytes,
                             int64_t count, void* workspace, size_t workspace_bytes, float* rgb_fine, float* t_fine, void* stream);

/* ------------------------------------------------------------------ restyle from cached trunk features, without the NeRF network
 * One ray-only piece is still recomputed by every tgtc_restyle_rays: the fine NeRF trunk (layers 0-7, the sigma layer's
 * fragments, base_remap_layer), 556 800 multiply-accumulates per live sample against 950 112 per latent -- 1 096 fragments
 * against 656 + 1 209 (576 + 1 096 folded).  tgtc_geometry_trunk runs it once over the cached list and keeps base_remap in a
 * caller-owned TRUNK PLANE beside the cache; tgtc_restyle_rays_trunk[_folded] restyle from cache + plane with the style
 * handle alone: the concat MLP, style layer 0 on [plane | concat features | encoding | mean z] and the style tail.  NO NeRF
 * HANDLE, coarse or fine, is involved in a restyle from the plane.
 * The price is memory: one 128 KiB tile per workgroup tile of the list, i.e. 1 KiB per live sample in TGTC_PREC_FP16X3 and
 *   512 B in TGTC_PREC_FP16 (a 400 x 400 frame with 3.04 M live samples: 3.1 GB / 1.6 GB, against 38 MB for the cache).  It is
 *   a mode the caller asks for; nothing selects it.
 * Plane layout: the library's operand-fragment layout, the bytes the style kernels park in the handle's slab.  With S = 128
 *   (FP16X3) or 256 (FP16) samples per tile, NCT = S / 128 column tiles per wave and P = 2 (FP16X3: hi, then lo) or 1 parts,
 *   thread tid (0..511) of tile t owns the 16 bytes (its 8 halves of the MFMA B fragment of k-step ks, whose column tid % 16 is
 *   list entry t S + (tid / 64) 16 NCT + 16 c + tid % 16) at
 *       t x 131072 + ((ks x NCT + c) x P + p) x 8192 + tid x 16,      ks = 0..7, c = 0..NCT-1, p = 0..P-1.
 *   Every byte of every tile is written: columns past the list's end hold the last live sample's fragments.  No zero-fill is
 *   needed and two builds are byte-equal.  The plane is position independent (it may be copied, saved and reloaded) and valid
 *   ONLY for the precision and the cached list it was built for.  A plane built in the other precision that happens to be large
 *   enough CANNOT be detected here: the caller keeps the precision beside the plane (the Python layer does and checks it).
 *
 * tgtc_geometry_trunk_bytes(precision, count): ceil(count / S) x 131072; 0 for count <= 0 or any other precision.
 * tgtc_geometry_trunk: reads live and ts_live of a packed cache (tgtc_geometry_pack) and writes the plane with ONE launch of the
 *   trunk form of the compact indexed kernel (csrc/mlp_style_sparse.hip) on `fine`, which must be the fine handle of the build.
 *   No coarse pass, no sigma pass, no synchronisation, no style handle; the slab of no handle is touched.  count == 0: nothing
 *   is launched and trunk may be NULL.
 * tgtc_restyle_rays_trunk / tgtc_restyle_rays_trunk_folded: the arguments, workspaces (tgtc_restyle_workspace_bytes /
 *   tgtc_restyle_folded_workspace_bytes) and results of tgtc_restyle_rays / tgtc_restyle_rays_folded without the fine handle and
 *   with the plane; z float [K,R,32] / [K,32].  They finish with the same compositing launch and the same depth copy.  The
 *   plane is only read.  count == 0: no kernel but the compositing is launched, trunk may be NULL, rgb_fine is +0, t_fine is copied.
 * Identity: rgb_fine, t_fine are the BITS of tgtc_restyle_rays / tgtc_restyle_rays_folded on the same cache when the plane was
 *   built by tgtc_geometry_trunk with the fine handle those calls would be given, packed in the style handle's precision: a
 *   live sample is the same column of the same MFMA sequence on the same operands, and base_remap's half8 values make a
 *   round trip through memory either way (the slab there, the plane here).
 * Errors (every check returns before a device is touched): null pointers, K < 1, R < 0, count < 0, count > R x N, n_coarse < 3,
 *   n_fine < 1, a wrong handle kind, a cache, plane or workspace below its size function (the plane's by the handle's
 *   precision) -> TGTC_ERR_ARG;  R x N >= 2^31, K x count >= 2^31, a fine handle in TGTC_PREC_FP16_FP6 given to
 *   tgtc_geometry_trunk -> TGTC_ERR_UNSUPPORTED;  R == 0 -> TGTC_OK.  The size and range checks come before the handle is looked at.
 * Scratch slab: the restyles use slab region A of the STYLE HANDLE; launches on one style handle must not overlap. */
size_t tgtc_geometry_trunk_bytes(int precision, int64_t count);
int tgtc_geometry_trunk(const tgtc_net* fine, const double* rays_o, const double* rays_d, int64_t R, int n_coarse, int n_fine,
                        const void* cache, size_t cache_bytes, int64_t count, void* trunk, size_t trunk_bytes, void* stream);
int tgtc_restyle_rays_trunk(const tgtc_net* style, const double* rays_o, const double* rays_d, const float* z, int K, int64_t R,
                            int n_coarse, int n_fine, const void* cache, size_t cache_bytes, int64_t count,
                            const void* trunk, size_t trunk_bytes, void* workspace, size_t workspace_bytes,
                            float* rgb_fine, float* t_fine, void* stream);
int tgtc_restyle_rays_trunk_folded(const tgtc_net* style, const double* rays_o, const double* rays_d, const float* z, int K,
                                   int64_t R, int n_coarse, int n_fine, const void* cache, size_t cache_bytes, int64_t count,
                                   const void* trunk, size_t trunk_bytes, void* workspace, size_t workspace_bytes,
                                   float* rgb_fine, float* t_fine, void* stream);

/* ------------------------------------------------------------------ restyle from the trunk plane, style networks in fp16mx
 * tgtc_style_create refuses TGTC_PREC_FP16_FP6: the dense stylised kernels have no room for its third activation set.  The
 * folded restyle from a trunk plane has -- no NeRF stream, no latent k-step -- so the fp16mx arithmetic of the NeRF nets
 * (one fp16 product plus two block-scaled e2m3 correction products per 128-deep block, csrc/mlp_mx.h) arrives there as a
 * SECOND PAIR OF STREAMS on a TGTC_PREC_FP16X3 style handle, behind entry points of its own.  It is a mode the caller asks
 * for; nothing selects it, and nothing else on the handle changes.
 *
 * tgtc_style_enable_mx: packs the handle's 13 equalised layers without their latent k-steps as fp16mx group streams (K groups
 *   of 7 KiB: Wh x 4, Wl6, Wh6; the encoding k-steps in fp16 hi + lo) and one pair of e2m3 row exponents per output row, chosen
 *   as tgtc_nerf_create chooses them, into an allocation of its own (about 3 MB) that tgtc_net_destroy frees.  The tables of
 *   tgtc_style_fold_latents apply unchanged.  `stream` orders the upload; the call returns when it is done.  A second call is a
 *   no-op (TGTC_OK).  A handle in TGTC_PREC_FP16 -> TGTC_ERR_UNSUPPORTED: its plane has no lo halves to correct from.
 * tgtc_style_has_mx: 1 once enabled, else 0 (also for NULL and for NeRF handles).
 * tgtc_style_mx_read (the seam the packing test uses; HOST buffers, synchronous): the packed group streams (both, in stream
 *   order), the row-exponent table (8192 bytes) and the 13 equalised weight matrices they were packed from ([out,in] row-major,
 *   concat layers 0..4 then style layers 0..7; 1 020 384 floats).  The three sizes must be exact -> TGTC_ERR_ARG otherwise, with
 *   the sizes in the message; no mx streams -> TGTC_ERR_UNSUPPORTED.
 * tgtc_restyle_rays_trunk_folded_mx: the arguments (z float [K,32]), workspace (tgtc_restyle_folded_workspace_bytes), compositing
 *   launch, depth copy, count == 0 rule and errors of tgtc_restyle_rays_trunk_folded, with the concat MLP and the style MLP run by
 *   the fp16mx plane consumer (csrc/mlp_style_mx.hip).  The plane is the TGTC_PREC_FP16X3 plane of tgtc_geometry_trunk: its hi
 *   and lo fragments are the fp16 operand and the source of the e2m3 blocks.  A handle without mx streams ->
 *   TGTC_ERR_UNSUPPORTED, checked where the handle's kind is.
 *   Results differ from tgtc_restyle_rays_trunk_folded within the precision's error (1e-3 against float64 per sample, the
 *   TGTC_PREC_FP16_FP6 bar); t_fine is the same copy.  Deterministic: K latents in one call are the bits of K calls.
 * Scratch slab: slab region A of the STYLE HANDLE; launches on one style handle must not overlap. */
int tgtc_style_enable_mx(tgtc_net* style, void* stream);
int tgtc_style_has_mx(const tgtc_net* style);
int tgtc_style_mx_read(const tgtc_net* style, void* groups, size_t groups_bytes, void* row_exp, size_t row_exp_bytes, float* weights,
                       size_t weight_floats);
int tgtc_restyle_rays_trunk_folded_mx(const tgtc_net* style, const double* rays_o, const double* rays_d, const float* z, int K,
                                      int64_t R, int n_coarse, int n_fine, const void* cache, size_t cache_bytes, int64_t count,
                                      const void* trunk, size_t trunk_bytes, void* workspace, size_t workspace_bytes,
                                      float* rgb_fine, float* t_fine, void* stream);

/* ------------------------------------------------------------------ the trunk plane from an fp16mx fine network
 * tgtc_geometry_trunk refuses a fine handle in TGTC_PREC_FP16_FP6, and stays that way: a plane is read by the style kernels
 * and exists in their two layouts only.  tgtc_geometry_trunk_mx is the producer for such a handle: it runs the NeRF trunk in
 * fp16mx (csrc/mlp_trunk_mx.hip: the fp16mx per-sample kernel's layers 0-7, sigma groups and base_remap_layer on the handle's
 * own group stream and row exponents, one workgroup per 128-entry tile) and writes a TGTC_PREC_FP16X3 PLANE -- base_remap,
 * ReLU-ed, split into fp16 hi and lo = fp16(v - hi), in the layout above -- which tgtc_restyle_rays_trunk[_folded] and
 * tgtc_restyle_rays_trunk_folded_mx read with a TGTC_PREC_FP16X3 style handle.  Densities (the cache) and base_remap (the
 * plane) then come from the same packed network.  It is a mode the caller asks for; nothing selects it.
 *
 * tgtc_geometry_trunk_mx: the arguments, checks, check order and count == 0 / R == 0 rules of tgtc_geometry_trunk.  `fine`
 *   must be a NeRF handle in TGTC_PREC_FP16_FP6 (any other precision -> TGTC_ERR_UNSUPPORTED: tgtc_geometry_trunk takes those);
 *   trunk_bytes >= tgtc_geometry_trunk_bytes(TGTC_PREC_FP16X3, count).  One launch, no synchronisation, every byte of every tile
 *   written (columns past the list's end hold the last live sample's fragments): two builds are byte-equal.
 * Identity: hi and lo of list entry i are the split of relu(base_remap) as tgtc_nerf_forward on the same handle returns it for the
 *   point o + t d of that entry, bit for bit: the same dense_mx sequence on the same operands.
 * tgtc_geometry_trunk_read (the seam the tests look into a plane through; DEVICE buffers, one launch, no synchronisation): a
 *   plane of `precision` (TGTC_PREC_FP16X3 or TGTC_PREC_FP16) of `count` list entries as floats, hi [count,256] and lo
 *   [count,256]: base_remap of list entry i, feature f.  lo may be NULL and is not written for TGTC_PREC_FP16.  count == 0 ->
 *   TGTC_OK, nothing launched.
 * Errors (before a device is touched): as tgtc_geometry_trunk;  tgtc_geometry_trunk_read: count < 0, another precision, a null
 *   plane or hi with count > 0, a plane below tgtc_geometry_trunk_bytes(precision, count) -> TGTC_ERR_ARG;  count >= 2^31 ->
 *   TGTC_ERR_UNSUPPORTED. */
int tgtc_geometry_trunk_mx(const tgtc_net* fine, const double* rays_o, const double* rays_d, int64_t R, int n_coarse, int n_fine,
                           const void* cache, size_t cache_bytes, int64_t count, void* trunk, size_t trunk_bytes, void* stream);
int tgtc_geometry_trunk_read(int precision, const void* trunk, size_t trunk_bytes, int64_t count, float* hi, float* lo,
                             void* stream);

/* ------------------------------------------------------------------ the fp16x3+fp16mx pair in one call, without a plane
 * Every stylised entry point above that takes a fine handle refuses a fine handle and a style handle of different precisions, and
 * stays that way.  The three entry points here are the folded list entry points for the pair a TGTC_PREC_FP16_FP6 fine network
 * forms with a TGTC_PREC_FP16X3 style handle that carries mx streams (tgtc_style_enable_mx): ONE persistent kernel
 * (csrc/mlp_list_mx.hip) runs, per 128-entry tile of the list, the trunk of tgtc_geometry_trunk_mx and then the K latents of
 * tgtc_restyle_rays_trunk_folded_mx, with base_remap parked in the workgroup's tile of slab region B of the style handle
 * instead of a plane: nothing of 1 KiB per live sample is allocated, written to HBM for later or kept.  It is a mode the caller
 * asks for; nothing selects it.
 *
 * tgtc_styled_forward_list_folded_mx: the arguments and rules of tgtc_styled_forward_list_folded -- rgb float [K,R,N,3] is
 *   written at the samples live[0 .. *n_live) only (the caller zero-fills it), the list's length is read on the device, a
 *   length of 0 writes nothing.  The kernel alone: the seam the tests use.
 * tgtc_render_rays_styled_sparse_folded_mx: the arguments, workspace (tgtc_render_styled_sparse_folded_workspace_bytes), order
 *   of work and live_count of tgtc_render_rays_styled_sparse_folded: fold, the geometry half, the zero-fill, the kernel above,
 *   K compositing launches.  No synchronisation; the host never learns the list's length.
 * tgtc_restyle_rays_folded_mx: the arguments and workspace (tgtc_restyle_folded_workspace_bytes) of tgtc_restyle_rays_folded:
 *   fold, the compact form of the kernel over the cached list, the compositing launch, the depth copy.  count == 0: neither the
 *   fold nor the kernel is launched, rgb_fine is +0, t_fine is copied.
 * Handles: `fine` / `nerf` must be a NeRF handle in TGTC_PREC_FP16_FP6, `style` a style handle in TGTC_PREC_FP16X3 with mx
 *   streams (tgtc_style_has_mx) -> TGTC_ERR_UNSUPPORTED otherwise (an fp16 pair has no lo halves), checked where the siblings
 *   compare the two precisions.  Every other error and the check order are the sibling's: K < 1, null pointers, wrong handle
 *   kinds, min_weight < 0 or NaN, count > R x N, buffers below their size functions -> TGTC_ERR_ARG;  K x R x N >= 2^31 or
 *   K x count >= 2^31 -> TGTC_ERR_UNSUPPORTED;  R == 0 -> TGTC_OK.  The size and range checks come before the handles are looked
 *   at, and nothing touches a device before the checks pass.
 * Identity: a live sample is the same column of the same dense_mx sequences on the same operands, and base_remap's half8
 *   values make a round trip through memory either way (the slab here, the plane there).  So rgb_fine and t_fine of
 *   tgtc_restyle_rays_folded_mx are the BITS of tgtc_geometry_trunk_mx + tgtc_restyle_rays_trunk_folded_mx on the same cache, and
 *   those of tgtc_render_rays_styled_sparse_folded_mx the bits of tgtc_geometry_build + tgtc_geometry_pack + that pair.
 *   Deterministic: K latents in one call are the bits of K calls.
 * Scratch slab: BOTH slab regions of the STYLE HANDLE are used; launches on one style handle must not overlap. */
int tgtc_styled_forward_list_folded_mx(const tgtc_net* nerf, const tgtc_net* style, const double* rays_o, const double* rays_d,
                                       const float* ts, const void* folded, int K, int64_t R, int N, const uint32_t* live,
                                       const uint32_t* n_live, float* rgb, void* stream);
int tgtc_render_rays_styled_sparse_folded_mx(const tgtc_net* coarse, const tgtc_net* fine, const tgtc_net* style,
                                             const double* rays_o, const double* rays_d, const float* z, int K, int64_t R,
                                             int n_coarse, int n_fine, float near_, float far_, const float* jitter,
                                             float min_weight, void* workspace, size_t workspace_bytes, float* rgb_fine,
                                             float* t_fine, uint32_t* live_count, void* stream);
int tgtc_restyle_rays_folded_mx(const tgtc_net* fine, const tgtc_net* style, const double* rays_o, const double* rays_d,
                                const float* z, int K, int64_t R, int n_coarse, int n_fine, const void* cache, size_t cache_bytes,
                                int64_t count, void* workspace, size_t workspace_bytes, float* rgb_fine, float* t_fine,
                                void* stream);

/* ------------------------------------------------------------------ the chain geometry: screened density passes for the
 * culled stylised render and the geometry cache
 * tgtc_render_rays_styled_sparse* and tgtc_geometry_build take their fine depths from the first half of the plain ray kernel
 * and run a dense sigma-only fine pass.  The CHAIN GEOMETRY is a second ray-only half for the same calls: the passes of
 * tgtc_render_rays_plain on TGTC_PATH_CHAIN without a coarse image -- tgtc_sample_coarse, the coarse sigma pass, the per-ray
 * stage, a sigma-only fine pass -- each SCREENED where its handle's policy (tgtc_net_set_screen) says so:
 *   coarse pass: as in the plain chain (an fp16x3 handle with a screen); list + scratch live in the first colour plane of the
 *                workspace, which nothing uses before the zero-fill (dense where R x N x 12 bytes < R x n_coarse x 4 + 8192).
 *   fine pass:   sigma only.  A fine handle in fp16x3 or fp16mx with a screen: the screen launch, the candidates' list, their
 *                exact densities from tgtc_nerf_sigma_list (fp16x3) / tgtc_nerf_sigma_list_mx (fp16mx).  List + scratch are the
 *                workspace's live[] and scratch, which the compaction at min_weight overwrites afterwards.  There is no colour
 *                phase, so TGTC_CULL_* has no say.  AUTO is pass 2 of tgtc_screen_auto_decision, with a threshold of its own.
 *   Screened or dense, each pass lands its candidate share in its handle's pinned word and counts in
 *   tgtc_net_screened_renders; a handle without a screen (fp16, a coarse fp16mx) runs its pass dense.  No synchronisation.
 * Identity: a screened call gives the BITS of the unscreened one (the argument of the density screen above), and t_fine is the
 *   BITS of tgtc_render_rays_plain's on TGTC_PATH_CHAIN for the same handles, rays and jitter.  The fine depths agree with
 *   those of the siblings without _chain only to rounding (two coarse kernels), so the chain geometry never replaces them
 *   silently: it is a mode the caller asks for, and nothing selects it.
 * tgtc_geometry_build_chain: the arguments, workspace, checks and errors of tgtc_geometry_build; the workspace feeds
 *   tgtc_geometry_pack as before, and a cache does not know which geometry built it.
 * tgtc_render_rays_styled_sparse_chain: `form`, then the arguments of tgtc_render_rays_styled_sparse.  form 0: z [K,R,32], the
 *   workspace, handle rules and list launch of tgtc_render_rays_styled_sparse; 1: those of ..._folded (z [K,32]); 2: those of
 *   ..._folded_mx.  Any other form -> TGTC_ERR_ARG.  The workspace size functions are the siblings', unchanged.
 * tgtc_nerf_sigma_list_mx: tgtc_nerf_sigma_list for TGTC_PREC_FP16_FP6 handles (csrc/mlp_nerf_mx2.hip, the <IN_LIST, false>
 *   instance): sigma[s] of the listed samples, the bits of tgtc_nerf_forward_rays(rgb = NULL) and of the full kernels' sigma,
 *   nothing else touched.  Any other precision -> TGTC_ERR_UNSUPPORTED (tgtc_nerf_sigma_list keeps refusing fp16mx). */
int tgtc_nerf_sigma_list_mx(const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts, int64_t R, int N,
                            const uint32_t* live, const uint32_t* n_live, float* sigma, void* stream);
int tgtc_geometry_build_chain(const tgtc_net* coarse, const tgtc_net* fine, const double* rays_o, const double* rays_d, int64_t R,
                              int n_coarse, int n_fine, float near_, float far_, const float* jitter, float min_weight,
                              void* workspace, size_t workspace_bytes, float* t_fine, uint32_t* live_count, void* stream);
int tgtc_render_rays_styled_sparse_chain(int form, const tgtc_net* coarse, const tgtc_net* fine, const tgtc_net* style,
                                         const double* rays_o, const double* rays_d, const float* z, int K, int64_t R,
                                         int n_coarse, int n_fine, float near_, float far_, const float* jitter,
                                         float min_weight, void* workspace, size_t workspace_bytes, float* rgb_fine,
                                         float* t_fine, uint32_t* live_count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TGTC_HIP_H */
