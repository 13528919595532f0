// One training batch of the reference's RaySampler / DataLoader(shuffle=True) (dataset.py:63-144) in one launch: row r
// takes the shuffled index frame * H * W + row * W + col, computes that pixel's ray from the frame's camera (raygen.h: the
// body of gen_rays_kernel, same bits) and copies the pixel's colour.  The reference keeps float64 ray tables of every pixel
// of every frame on the host (0.6 GB for fern at factor 4) and gathers rows of them per batch.
//
// Latency- and HBM-bound: one thread per ray, 8 B index + 48 B camera + 12 B colour in, 60 B out.  The index is coalesced,
// the camera row and the colour are gathers by nature (a shuffled batch touches a different pixel per lane); the outputs
// are 3 consecutive words per lane, so a wave's stores cover contiguous 1 536-byte (rays) / 768-byte (colour) spans.
#include <cmath>

#include "common.h"
#include "raygen.h"
#include "../../include/tgtc_train.h"

namespace tgtc {

__global__ void __launch_bounds__(256) train_batch_kernel(RayIntrinsics cam, const float* __restrict__ c2w_table, long long F,
                                                          const float* __restrict__ images, const long long* __restrict__ index,
                                                          long long R, double* __restrict__ rays_o, double* __restrict__ rays_d,
                                                          float* __restrict__ rgb_gt) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const long long hw = (long long)cam.H * cam.W;
    const long long at = index[r];
    double o[3], d[3];
    float c[3] = {0.0f, 0.0f, 0.0f};
    if (at >= 0 && at < F * hw) {       // a row outside the tables is not dereferenced: NaN rays, zero colour
        const long long frame = at / hw;
        pixel_ray(cam, c2w_table + frame * 12, at - frame * hw, o, d);
        if (images) {
#pragma unroll
            for (int k = 0; k < 3; ++k) c[k] = images[at * 3 + k];
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
        for (int k = 0; k < 3; ++k) rgb_gt[r * 3 + k] = c[k];
    }
}

}  // namespace tgtc

using namespace tgtc;

extern "C" int tgtc_train_batch(int H, int W, double fx, double fy, double cx, double cy, const float* c2w_table, int F,
                                const float* images, const int64_t* index, int64_t R, int pixel_alignment, int ndc,
                                double ndc_near, double* rays_o, double* rays_d, float* rgb_gt, void* stream) {
    TGTC_REQUIRE(H > 0 && W > 0 && F > 0 && c2w_table, "train_batch: bad argument");
    TGTC_REQUIRE(R >= 0, "train_batch: negative batch size");
    if (R == 0) return TGTC_OK;         // an empty batch has no rows to point at
    TGTC_REQUIRE(index && rays_o && rays_d, "train_batch: null pointer");
    TGTC_REQUIRE(!rgb_gt || images, "train_batch: rgb_gt asked for without an image table");
    RayIntrinsics cam;
    cam.H = H, cam.W = W, cam.fx = fx, cam.fy = fy, cam.cx = cx, cam.cy = cy;
    cam.pixel_alignment = pixel_alignment, cam.ndc = ndc, cam.ndc_near = ndc_near;
    const unsigned blocks = (unsigned)((R + 255) / 256);
    train_batch_kernel<<<blocks, 256, 0, as_stream(stream)>>>(cam, c2w_table, (long long)F, images,
                                                              reinterpret_cast<const long long*>(index), R, rays_o, rays_d, rgb_gt);
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}
