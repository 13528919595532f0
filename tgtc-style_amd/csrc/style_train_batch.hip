// Both batches of one `Style_train` iteration in one launch (reference StyleRaySampler_gen.get_item_train_style,
// dataset.py:498-518, and LightDataLoader.loss_coh_get_batch, dataset.py:752-779, which build them row by row on the host
// from float64 ray tables of every pixel).  Rows 0 .. R-1 decode the shuffled index style * F*H*W + frame * H*W + pixel;
// rows R .. R+n_coh-1 are the frame-ordered batch: pixel (coh_start + i) mod H*W of ONE frame of ONE style, no index read.
// A row's ray is pixel_ray (raygen.h, the bits of gen_rays_kernel) from its frame's camera, rgb_gt the stylised byte
// divided by 255 in float32 (a true division: np.float32(u8) / 255 is what the reference feeds), rgb_origin the frame's
// un-stylised colour, and the two ids what the latent gather takes.
//
// Latency- and HBM-bound like train_batch_kernel: one thread per row.  Per row in: 8 B index (shuffled rows only,
// coalesced) + 48 B camera + 3 B stylised bytes + 12 B colour, the last three gathers by nature for a shuffled row and
// consecutive addresses across the lanes of an ordered row; out: 48 B rays + 24 B colours + 16 B ids, consecutive per lane.
#include <cmath>

#include "common.h"
#include "raygen.h"
#include "../../include/tgtc_train.h"

namespace tgtc {

struct StyleBatchRows {
    long long F, S, R, n_coh;
    long long coh_style, coh_frame, coh_start;      // coh_start already reduced mod H*W by the host
};

__global__ void __launch_bounds__(256) style_train_batch_kernel(RayIntrinsics cam, StyleBatchRows rows,
                                                                const float* __restrict__ c2w_table,
                                                                const float* __restrict__ images,
                                                                const unsigned char* __restrict__ stylized,
                                                                const long long* __restrict__ index,
                                                                double* __restrict__ rays_o, double* __restrict__ rays_d,
                                                                float* __restrict__ rgb_gt, float* __restrict__ rgb_origin,
                                                                long long* __restrict__ style_id, long long* __restrict__ frame_id) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows.R + rows.n_coh) return;
    const long long hw = (long long)cam.H * cam.W;
    long long s = -1, f = -1, pix = 0;
    if (r < rows.R) {
        const long long at = index[r];
        if (at >= 0 && at < rows.S * rows.F * hw) {     // a row outside the tables is not dereferenced
            s = at / (rows.F * hw);
            const long long rem = at - s * rows.F * hw;
            f = rem / hw;
            pix = rem - f * hw;
        }
    } else {
        s = rows.coh_style, f = rows.coh_frame;
        pix = (rows.coh_start + (r - rows.R)) % hw;
    }
    double o[3], d[3];
    float gt[3] = {0.0f, 0.0f, 0.0f}, org[3] = {0.0f, 0.0f, 0.0f};
    if (s >= 0) {
        pixel_ray(cam, c2w_table + f * 12, pix, o, d);
        if (rgb_gt) {
            const unsigned char* px = stylized + ((s * rows.F + f) * hw + pix) * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) gt[k] = (float)px[k] / 255.0f;
        }
        if (rgb_origin) {
            const float* px = images + (f * hw + pix) * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) org[k] = px[k];
        }
    } else {
        const double nan = __builtin_nan("");
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = d[k] = nan;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        rays_o[r * 3 + k] = o[k];
        rays_d[r * 3 + k] = d[k];
    }
    if (rgb_gt) {
#pragma unroll
        for (int k = 0; k < 3; ++k) rgb_gt[r * 3 + k] = gt[k];
    }
    if (rgb_origin) {
#pragma unroll
        for (int k = 0; k < 3; ++k) rgb_origin[r * 3 + k] = org[k];
    }
    if (style_id) style_id[r] = s;
    if (frame_id) frame_id[r] = f;
}

}  // namespace tgtc

using namespace tgtc;

extern "C" int tgtc_style_train_batch(int H, int W, double fx, double fy, double cx, double cy, const float* c2w_table, int F,
                                      int S, const float* images, const uint8_t* stylized, const int64_t* index, int64_t R,
                                      int64_t n_coh, int coh_style, int coh_frame, int64_t coh_start, int pixel_alignment,
                                      int ndc, double ndc_near, double* rays_o, double* rays_d, float* rgb_gt,
                                      float* rgb_origin, int64_t* style_id, int64_t* frame_id, void* stream) {
    TGTC_REQUIRE(H > 0 && W > 0 && F > 0 && S > 0 && c2w_table, "style_train_batch: bad argument");
    TGTC_REQUIRE(R >= 0 && n_coh >= 0, "style_train_batch: negative batch size");
    if (R == 0 && n_coh == 0) return TGTC_OK;       // no rows to point at
    TGTC_REQUIRE(rays_o && rays_d && (index || R == 0), "style_train_batch: null pointer");
    TGTC_REQUIRE(!rgb_gt || stylized, "style_train_batch: rgb_gt asked for without a stylised table");
    TGTC_REQUIRE(!rgb_origin || images, "style_train_batch: rgb_origin asked for without an image table");
    TGTC_REQUIRE(n_coh == 0 || (coh_style >= 0 && coh_style < S && coh_frame >= 0 && coh_frame < F && coh_start >= 0),
                 "style_train_batch: ordered batch outside the tables");
    RayIntrinsics cam;
    cam.H = H, cam.W = W, cam.fx = fx, cam.fy = fy, cam.cx = cx, cam.cy = cy;
    cam.pixel_alignment = pixel_alignment, cam.ndc = ndc, cam.ndc_near = ndc_near;
    StyleBatchRows rows;
    rows.F = F, rows.S = S, rows.R = R, rows.n_coh = n_coh;
    rows.coh_style = coh_style, rows.coh_frame = coh_frame;
    rows.coh_start = n_coh > 0 ? coh_start % ((int64_t)H * W) : 0;
    const unsigned blocks = (unsigned)((R + n_coh + 255) / 256);
    style_train_batch_kernel<<<blocks, 256, 0, as_stream(stream)>>>(
        cam, rows, c2w_table, images, stylized, reinterpret_cast<const long long*>(index), rays_o, rays_d, rgb_gt, rgb_origin,
        reinterpret_cast<long long*>(style_id), reinterpret_cast<long long*>(frame_id));
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}
