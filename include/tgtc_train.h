/* libtgtc_hip.so -- fused training path of the NeRF MLP.
 *
 * The reference trains through PyTorch autograd: `Origin_train` (train_tgtcs.py:218-309) runs MLP_style.forward
 * (models.py:95-117 inside StyleNerf.forward :216-223) on every sample of a batch and `loss.backward()` walks the recorded
 * graph.  These entry points are what a binding would call in place of that forward / backward pair for one StyleNerf:
 * same inputs (sample points and view directions), same outputs (rgb, sigma), and on the way back the gradients of the
 * twelve nn.Linear weight / bias tensors given dL/d rgb and dL/d sigma.  Same conventions as tgtc_hip.h: int return codes,
 * tgtc_last_error(), device pointers, caller-allocated outputs and workspace, a hipStream_t, no implicit synchronisation.
 *
 * `params` / `grads`: HOST arrays of 24 DEVICE pointers in the order of MLP_style.layers (models.py:93) --
 * base_layers[0..7], sigma_layer, base_remap_layer, rgb_layers[0], rgb_layers[1] -- weight then bias for each
 * (weight [out, in] row-major fp32 as nn.Linear stores it).  The weights are read on the device at every call: an
 * optimiser may update them in place between calls.  Network shape: D = 8, W = 256, skip at 4, view directions, ReLU. */
#ifndef TGTC_TRAIN_H
#define TGTC_TRAIN_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct tgtc_trainer tgtc_trainer; /* opaque: pack maps and the packed streams of ONE network */

int tgtc_trainer_create(tgtc_trainer** out);
int tgtc_trainer_destroy(tgtc_trainer* trainer);
/* bytes of workspace for M samples: activations of every layer (fp16 hi/lo), their ReLU gates, pre-activation gradients */
size_t tgtc_trainer_workspace_bytes(int64_t M);
/* forward of StyleNerf on pts / dirs double [M,3]: rgb float [M,3], sigma float [M]; leaves in `workspace` what backward needs */
int tgtc_trainer_forward(tgtc_trainer* trainer, const float* const* params, const double* pts, const double* dirs, int64_t M,
                         void* workspace, size_t workspace_bytes, float* rgb, float* sigma, void* stream);
/* backward of the same call (same M, same workspace, untouched in between): rgb = the forward's output, d_rgb [M,3] and
 * d_sigma [M] = dL/d outputs; grads[i] (shapes of params[i]) are OVERWRITTEN with dL/d params[i].
 * grads[17], d sigma_layer.bias, is ONE number -- the sum of d_sigma -- and is taken in float64 in a fixed order and rounded
 * once (one small launch after the weight gradients, dense and sparse mode alike): the same bits at every call, also where
 * the summands cancel.  Every other gradient is accumulated in float32 by atomics, in whatever order they land. */
int tgtc_trainer_backward(tgtc_trainer* trainer, const float* const* params, const float* rgb, const float* d_rgb,
                          const float* d_sigma, int64_t M, void* workspace, size_t workspace_bytes, float* const* grads,
                          void* stream);
/* synchronises `stream`; non-zero (with tgtc_last_error) if the last backward overflowed its fp16 operand range */
int tgtc_trainer_status(tgtc_trainer* trainer, void* stream);
/* Overflow guard: a backward whose scaled gradients left the fp16 range (growth above ~2^7 across one transposed layer), or
 * that produced any non-finite gradient for whatever reason (a forward that overflowed fp16, non-finite dL/d outputs),
 * ZERO-FILLS grads[0..23] on the device before it returns control to the stream -- an optimiser step on them cannot write
 * inf / NaN into the weights -- and counts the event.  *count = such backwards since trainer_create (synchronises `stream`;
 * read it at the reference's i_print cadence, train_tgtcs.py:257-266, not per iteration). */
int tgtc_trainer_overflows(tgtc_trainer* trainer, void* stream, unsigned* count);

/* Sparse backward: most samples of a NeRF training batch carry an upstream gradient that is exactly zero (a sample with
 * sigma + noise <= 0 has alpha = 0: its compositing weight, and with it d_rgb and d_sigma, are +-0), and such a sample adds
 * exactly nothing to any gradient.  In TGTC_TRAIN_SPARSE mode tgtc_trainer_backward first builds, on the device, the
 * ascending list of the LIVE samples -- sample m is live iff not all of d_sigma[m], d_rgb[m, 0..2] compare == 0.0f: -0.0 is
 * dead, NaN and inf are live, so the overflow guard still sees them -- and runs the input-gradient chain and the weight
 * gradients over that list alone.  The gradients are those of the dense backward up to fp32 / fp16x3 rounding, not the
 * same bits (the 16-sample tiles are composed of other samples, and the chain's per-tile scales follow the tile maximum).
 * No host synchronisation: the host never learns the count, the grids are those of M samples.  The forward is untouched.
 * The mode is the caller's and is never chosen or changed by the library: TGTC_TRAIN_DENSE is the default, and a sparse
 * backward whose workspace is below tgtc_trainer_workspace_bytes_sparse(M) returns TGTC_ERR_ARG with nothing launched -- it
 * does not run dense instead.  The forward and the dense backward take a workspace of either size.
 *   tgtc_trainer_set_sparse                TGTC_ERR_ARG for a NULL trainer or any other mode
 *   tgtc_trainer_workspace_bytes_sparse    the dense size + the list (uint32 [M_pad]), its count and the compaction's partial
 *                                          counts; 0 for M <= 0
 *   tgtc_trainer_live_counts               *live / *total = live samples / all samples, summed over the SPARSE backwards since
 *                                          trainer_create (dense backwards add nothing); synchronises `stream` like
 *                                          tgtc_trainer_overflows: read it at the i_print cadence */
#define TGTC_TRAIN_DENSE 0
#define TGTC_TRAIN_SPARSE 1
int tgtc_trainer_set_sparse(tgtc_trainer* trainer, int mode);
size_t tgtc_trainer_workspace_bytes_sparse(int64_t M);
int tgtc_trainer_live_counts(tgtc_trainer* trainer, void* stream, unsigned long long* live, unsigned long long* total);

/* Workspace: about 20 KB per sample -- two fp16 planes of 2 528 activations, 2 448 fp32 pre-activation gradients, one
 * 64-bit gate word per gated layer, 16-sample tile and lane -- e.g. 2.6 GB at M = 131 072 (1 024 rays x 128 samples of the
 * fine network).  It belongs to ONE forward / backward pair: a second forward before the backward of the first needs its
 * own workspace (the reference's batchify, utils.py:435-456, makes two forwards before one backward). */

/* One training batch of `Origin_train` from shuffled pixel indices (csrc/train_batch.hip), in place of the reference's
 * float64 ray tables of every pixel of every training frame and the DataLoader's gather of their rows
 * (dataset.py:63-144).  index[r] = frame * H * W + row * W + col.  Row r of rays_o / rays_d double [R,3] carries the bits
 * that tgtc_gen_rays writes for that pixel of the camera c2w_table[frame] (float64 get_rays_np + ndc_rays_np, same
 * intrinsics and flags for every frame); rgb_gt float [R,3] is images[frame, row, col], copied.
 *   c2w_table  DEVICE float [F,12], 3x4 row-major per frame      images  DEVICE float [F,H,W,3], or NULL with rgb_gt NULL
 *   index      DEVICE int64 [R]
 * A row whose index lies outside [0, F*H*W) is not dereferenced: it gets NaN rays and zero colour.  R == 0 is TGTC_OK;
 * a null index / rays_o / rays_d / c2w_table, rgb_gt without images, or F, H, W <= 0 is TGTC_ERR_ARG. */
int tgtc_train_batch(int H, int W, double fx, double fy, double cx, double cy, const float* c2w_table, int F,
                     const float* images, const int64_t* index, int64_t R, int pixel_alignment, int ndc, double ndc_near,
                     double* rays_o, double* rays_d, float* rgb_gt, void* stream);

/* Both batches of one `Style_train` iteration in one launch (csrc/style_train_batch.hip), in place of the reference's
 * StyleRaySampler_gen / LightDataLoader, which build them row by row on the host (dataset.py:498-539, :658-779).  Every
 * output has R + n_coh rows.
 *   rows 0 .. R-1      decode index[r] = style * F*H*W + frame * H*W + row * W + col (dataset.py:498-502)
 *   rows R .. R+n_coh-1  the frame-ordered batch of loss_coh_get_batch: pixel (coh_start + i) mod (H*W) of frame coh_frame
 *                      of style coh_style; no index is read for them
 * rays_o / rays_d double [.,3]: the bits tgtc_gen_rays writes for that pixel of camera c2w_table[frame]; rgb_gt float [.,3]
 * = float(stylized[style, frame, row, col]) / 255, a float32 division; rgb_origin float [.,3] = images[frame, row, col],
 * copied; style_id / frame_id int64 [.].  rgb_gt, rgb_origin, style_id, frame_id may each be NULL.
 *   c2w_table  DEVICE float [F,12]          images    DEVICE float [F,H,W,3], or NULL with rgb_origin NULL
 *   index      DEVICE int64 [R], or NULL with R == 0      stylized  DEVICE uint8 [S,F,H,W,3], or NULL with rgb_gt NULL
 * A row whose index lies outside [0, S*F*H*W) is not dereferenced: NaN rays, zero colours, ids -1.  R == 0 && n_coh == 0
 * is TGTC_OK with nothing written.  TGTC_ERR_ARG, nothing launched: H, W, F or S <= 0; a null c2w_table, rays_o or rays_d;
 * a null index with R > 0; a colour output without its table; with n_coh > 0, coh_style outside [0,S), coh_frame outside
 * [0,F) or coh_start < 0. */
int tgtc_style_train_batch(int H, int W, double fx, double fy, double cx, double cy, const float* c2w_table, int F, int S,
                           const float* images, const uint8_t* stylized, const int64_t* index, int64_t R, int64_t n_coh,
                           int coh_style, int coh_frame, int64_t coh_start, int pixel_alignment, int ndc, double ndc_near,
                           double* rays_o, double* rays_d, float* rgb_gt, float* rgb_origin, int64_t* style_id,
                           int64_t* frame_id, void* stream);

/* Style trainer (csrc/style2d.hip): forward and backward of BOTH style MLPs of `Style_train` -- StyleMLP_before_concat
 * (models.py:120-147, 5 linears) feeding StyleMLP_Wild_multilayers (models.py:149-180, 7 hidden linears and the 3-wide
 * sigmoid head) -- in two calls, in place of one GEMM call per layer and pass from a binding (tgtc_s2d_linear_pre /
 * tgtc_s2d_linear_backward).  It is the same per-layer arithmetic on the same GEMM kernel, chained inside the library; no
 * layer input is ever concatenated: the GEMM's row loader reads the segments in place.
 *   x           DEVICE float [M,63]   the encoded sample points (ret['pts']), M = R * n, sample m belongs to ray m / n
 *   base_remap  DEVICE float [M,256]  the NeRF trunk's remap features
 *   lat_c       DEVICE float [R,32]   one latent row per ray, read by every layer of the concat MLP
 *   lat_s       DEVICE float [R,32]   the style MLP's latent row (the reference hands it mean(z) in all 32 columns)
 *   rgb         DEVICE float [M,3]
 * Layer inputs, in the column order of the weights: concat 0 [x | lat_c], 1-3 [h | lat_c], 4 [h | lat_c | x]; style 0
 * [base_remap | concat output | x | lat_s], 1-3, 5, 6 and the head [h | lat_s], 4 [h | lat_s | x].
 * `params` / `grads`: HOST arrays of 26 DEVICE pointers -- the concat MLP's layers[0..4], then the style MLP's layers[0..7],
 * weight ([out, in] row-major fp32) then bias for each.  The weights are read on the device at every call.  Every layer's
 * output equals, bit for bit, tgtc_s2d_linear_pre on the concatenated input (halves from tgtc_s2d_split where in % 4 == 0).
 * `precision`: TGTC_PREC_FP16X3 or TGTC_PREC_FP16, of the forward and of the backward that follows it.
 *
 * Backward (same R, n and workspace as the forward, workspace untouched in between; x, base_remap, lat_c and lat_s of the
 * forward are read again and must still hold the same values): d_rgb [M,3] = dL/d rgb; grads[i] (shape of params[i]) is
 * OVERWRITTEN with dL/d params[i]; d_lat_c / d_lat_s float [R,32], each may be NULL, are overwritten with dL/d lat_c /
 * dL/d lat_s -- per layer the gated gradient rows of a ray are summed first and multiplied by the latent columns of the
 * weight once per ray.  x and base_remap receive no gradient.  Gradient scaling is that of tgtc_s2d_linear_backward.  A
 * backward consumes the forward's record: a second backward on one forward is TGTC_ERR_ARG.
 *
 * Workspace: about 19 KB per sample -- 12 fp32 activation planes of 256 (12 KB) and rgb, kept from forward to backward, and
 * the backward's per-layer scratch, reused layer after layer: two gradient planes of 256, the row-scaled gradient, the
 * transposed fp16 hi/lo gradient (256 columns) and input (607 columns) -- plus at most 12 MB that do not grow with M.  It
 * belongs to ONE forward / backward pair, like tgtc_trainer's: Style_train's coarse and fine passes hold two.
 * R == 0 is TGTC_OK (backward then zero-fills grads).  TGTC_ERR_ARG with nothing launched: a NULL trainer, params, grads (or
 * entry of them), x, base_remap, lat_c, lat_s, rgb, d_rgb or workspace; R < 0, n <= 0, R * n > 2 097 120 (65 535 x 32: the
 * sample dimension of the weight-gradient transposes is a grid dimension; larger batches go in chunks, their gradients
 * added); a workspace below tgtc_style_trainer_workspace_bytes(R, n) (0 for a shape that is refused); any other precision;
 * a backward without its forward.
 * The record of a forward (a few words on the host, keyed by the workspace's address) is dropped by its backward, replaced
 * by the next forward into the same workspace, and freed with the trainer -- by nothing else.  A forward whose backward
 * never runs leaves it behind; if its workspace is then freed and another allocation lands on the same address, a
 * backward of the same (R, n) into that memory WITHOUT a forward is not refused, and reads whatever the memory holds.
 * Callers that drop forwards (evaluation, an exception between the two calls) keep their workspaces, as a pool does, or
 * destroy the trainer. */
typedef struct tgtc_style_trainer tgtc_style_trainer; /* opaque: which forward each workspace holds */
int tgtc_style_trainer_create(tgtc_style_trainer** out);
int tgtc_style_trainer_destroy(tgtc_style_trainer* trainer);
size_t tgtc_style_trainer_workspace_bytes(int64_t R, int n);
int tgtc_style_trainer_forward(tgtc_style_trainer* trainer, const float* const* params, const float* x, const float* base_remap,
                               const float* lat_c, const float* lat_s, int64_t R, int n, int precision, void* workspace,
                               size_t workspace_bytes, float* rgb, void* stream);
int tgtc_style_trainer_backward(tgtc_style_trainer* trainer, const float* const* params, const float* d_rgb, int64_t R, int n,
                                void* workspace, size_t workspace_bytes, float* const* grads, float* d_lat_c, float* d_lat_s,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif
