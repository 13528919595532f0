// One pixel's ray: reference dataset.py:33-42 (get_rays_np) + dataset.py:44-61 (ndc_rays_np), float64, in the reference's
// evaluation order.  Shared by gen_rays_kernel (raypath.hip: the pixels of ONE camera, in order) and train_batch_kernel
// (train_batch.hip: shuffled pixels of a table of cameras) so that both write the same bits for a pixel.
#pragma once

namespace tgtc {

struct RayIntrinsics {
    int H, W;
    double fx, fy, cx, cy;
    int pixel_alignment, ndc;
    double ndc_near;
};

// pix = row * W + col of an H x W frame; c2w = 12 floats, 3x4 row-major (any address space the caller can read)
__device__ __forceinline__ void pixel_ray(const RayIntrinsics& a, const float* c2w, long long pix, double o[3], double d[3]) {
    // the reference evaluates these formulas with separate multiplies and adds (numpy): keep the same roundings
#pragma clang fp contract(off)
    float col = (float)(pix % a.W), row = (float)(pix / a.W);
    if (a.pixel_alignment) {
        col = col + 0.5f;
        row = row + 0.5f;
    }
    // dataset.py:37: float32 grid minus float64 intrinsics -> float64
    const double cam[3] = {((double)col - a.cx) / a.fx, (-((double)row - a.cy)) / a.fy, -1.0};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        // dataset.py:39: sum over the last axis of dirs[...,None,:] * c2w[:3,:3]
        const double p0 = cam[0] * (double)c2w[4 * k + 0];
        const double p1 = cam[1] * (double)c2w[4 * k + 1];
        const double p2 = cam[2] * (double)c2w[4 * k + 2];
        d[k] = (p0 + p1) + p2;
        o[k] = (double)c2w[4 * k + 3];
    }
    if (a.ndc) {
        // dataset.py:46-47
        const double t = (-(a.ndc_near + o[2])) / d[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = o[k] + t * d[k];
        // dataset.py:50-56
        const double sx = -1.0 / ((double)a.W / (2.0 * a.fx));
        const double sy = -1.0 / ((double)a.H / (2.0 * a.fx));
        const double o0 = sx * o[0] / o[2];
        const double o1 = sy * o[1] / o[2];
        const double o2 = 1.0 + 2.0 * a.ndc_near / o[2];
        const double d0 = sx * (d[0] / d[2] - o[0] / o[2]);
        const double d1 = sy * (d[1] / d[2] - o[1] / o[2]);
        const double d2 = -2.0 * a.ndc_near / o[2];
        o[0] = o0, o[1] = o1, o[2] = o2;
        d[0] = d0, d[1] = d1, d[2] = d2;
    }
}

}  // namespace tgtc
