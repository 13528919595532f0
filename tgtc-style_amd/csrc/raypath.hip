// Per-ray kernels of the render hot path: ray generation (+NDC warp), coarse sampling, positional
// encoding, alpha compositing, inverse-CDF fine sampling, latent gather.
//
// These are HBM-bound elementwise / per-ray-scan kernels (a few bytes and a few dozen flops per
// element); the design rules that matter are coalesced access, one wavefront per ray for the scans,
// and LDS staging of the per-ray sample buffers.  The arithmetic follows the reference's evaluation
// order (no FMA contraction where the reference has separate roundings) so float64 outputs agree to
// the last bits and float32 outputs to ~1 ulp.
#include <algorithm>

#include "common.h"
#include "raygen.h"
#include "raymarch_wave.h"

// The reference evaluates these formulas with separate multiplies and adds (numpy / ATen CPU);
// keep the same roundings.
#pragma clang fp contract(off)

namespace tgtc {

// ------------------------------------------------------------------------------------------- rays
// reference dataset.py:33-42 + dataset.py:44-61
struct RayGenArgs {
    RayIntrinsics cam;      // raygen.h: the per-pixel body, shared with train_batch.hip
    float c2w[12];
    long long first, n;
};

__global__ void __launch_bounds__(256) gen_rays_kernel(RayGenArgs a, double* __restrict__ rays_o,
                                                       double* __restrict__ rays_d) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.n) return;
    double d[3], o[3];
    pixel_ray(a.cam, a.c2w, a.first + idx, o, d);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        rays_o[idx * 3 + k] = o[k];
        rays_d[idx * 3 + k] = d[k];
    }
}

// ------------------------------------------------------------------------------- coarse sampling
// reference utils.py:509-531
__global__ void __launch_bounds__(256) sample_coarse_kernel(const double* __restrict__ rays_o,
                                                            const double* __restrict__ rays_d, long long R, int N,
                                                            float near_, float far_, const float* __restrict__ jitter,
                                                            double* __restrict__ pts, float* __restrict__ ts) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= R * N) return;
    const long long r = idx / N;
    const int i = (int)(idx % N);
    const float t = jitter ? coarse_t_jittered(i, N, near_, far_, jitter[idx]) : coarse_t(i, N, near_, far_);
    ts[idx] = t;
    if (pts) {
#pragma unroll
        for (int k = 0; k < 3; ++k) pts[idx * 3 + k] = rays_o[r * 3 + k] + (double)t * rays_d[r * 3 + k];  // :529
    }
}

// ------------------------------------------------------------------------------------------ posenc
// reference models.py:46-60; output cast to float32 (models.py:219-220)
template <typename T>
__global__ void __launch_bounds__(256) posenc_kernel(const T* __restrict__ x, long long M, int L,
                                                     float* __restrict__ out) {
    const int width = 3 + 6 * L;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= M * width) return;
    const long long m = idx / width;
    const int c = (int)(idx % width);
    if (c < 3) {
        out[idx] = (float)x[m * 3 + c];
        return;
    }
    const int band = (c - 3) / 6, rem = (c - 3) % 6;
    const T arg = x[m * 3 + rem % 3] * (T)(double)(1 << band);
    out[idx] = (float)(rem < 3 ? sin(arg) : cos(arg));
}

// -------------------------------------------------------------------------------------- composite
// reference utils.py:354-386.  One wavefront per ray; lane l owns the contiguous run of samples
// [l*C, l*C+C), C = ceil(N/64).  The transmittance is the reference's SEQUENTIAL product, sample after sample in
// float64 and rounded to float32 per element (torch.cumprod on the CPU accumulates in acc_type<float> = double):
// every lane walks the whole chain with the `keep` factors broadcast lane by lane, so the weights do not depend
// on the tiling (raymarch_wave.h composite_tile computes the same chain 16 samples at a time).  Then four weighted
// wave reductions.
// acc + w * c of one colour channel: ONE expression for composite_wave and composite_live_kernel, so that the compiler
// contracts (or does not contract) it the same way in both.
__device__ __forceinline__ float composite_accumulate(float acc, float w, float c) { return acc + w * c; }

// The same transmittance chain with the factors that are exactly 1 left out.  A sample with alpha == 0 has
// keep = 1.0f - 0 + 1e-10f = 1.0f, and run * 1.0 is run, bit for bit (whatever run is): only the samples with alpha != 0 (a
// NaN included) take a step of the sequential float64 product, in sample order -- one ballot per owned slot, then a walk
// over the set bits with the factor read by v_readlane.  trans[k] = the product in front of sample lane * C + k, rounded to
// float32: every sample behind the one that just multiplied takes the new value, so a sample (live or not) ends with
// the product over the live samples in front of it -- the value the full chain gives it.
template <int C>
__device__ __forceinline__ void transmittance_of_live(const float (&alpha)[C], const float (&keep)[C], int lane, float (&trans)[C]) {
    unsigned long long live[C], any = 0;
#pragma unroll
    for (int k = 0; k < C; ++k) {
        live[k] = __ballot(alpha[k] != 0.0f);
        any |= live[k];
        trans[k] = 1.0f;
    }
    double run = 1.0;
    while (any) {   // wave-uniform
        const int l = __builtin_ctzll(any);
        any &= any - 1;
#pragma unroll
        for (int k = 0; k < C; ++k) {
            if ((live[k] >> l) & 1ull) {   // wave-uniform
                run = run * (double)__builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, keep[k]), l));
                const float t = (float)run;
                const int cur = l * C + k;
#pragma unroll
                for (int kk = 0; kk < C; ++kk)
                    if (lane * C + kk > cur) trans[kk] = t;
            }
        }
    }
}

// LIVE_COLOURS: the transmittance chain runs over the samples with alpha != 0 alone (transmittance_of_live), and
// a sample whose raw sigma is not > 0 neither loads its colour nor enters the colour sums.  Its alpha is
// 1 - exp(-0 * delta) = 0 and its weight alpha * T = +0, so over a plane that holds +0 there it would enter as
// acc + 0 * 0, which leaves acc (never -0: it starts at +0) unchanged: the flagged instance over ANY bits at the dead
// entries equals the plain one over a zero-filled plane.  The depth sum and the weights are the plain instance's.
template <int C, bool LIVE_COLOURS = false>
__device__ __forceinline__ void composite_wave(const float* __restrict__ rgb, const float* __restrict__ sigma,
                                               const float* __restrict__ ts, int N, float* rgb_exp, float* t_exp,
                                               float* weights, const float* __restrict__ noise = nullptr,
                                               int white_bkgd = 0) {
    const int lane = threadIdx.x & 63;
    float alpha[C], tv[C], keep[C];
    bool live[C];
#pragma unroll
    for (int k = 0; k < C; ++k) {
        const int i = lane * C + k;
        alpha[k] = 0.0f, tv[k] = 0.0f, keep[k] = 1.0f, live[k] = false;
        if (i < N) {
            const float t0 = ts[i];
            const float delta = (i + 1 < N) ? ts[i + 1] - t0 : 1e10f;       // utils.py:367-369
            const float raw = noise ? sigma[i] + noise[i] : sigma[i];      // training-time regulariser, :371-376
            const float dens = fmaxf(fmaxf(raw, 0.0f), 0.0f);               // relu(relu(.)) :365,:376
            live[k] = raw > 0.0f;
            alpha[k] = 1.0f - expf(-dens * delta);
            tv[k] = t0;
            keep[k] = 1.0f - alpha[k] + 1e-10f;                             // :378
        }
    }
    float trans[C];
    if constexpr (LIVE_COLOURS) {
        transmittance_of_live<C>(alpha, keep, lane, trans);
    } else {
        double run = 1.0;
        for (int l = 0; l < 64; ++l) {   // wave-uniform trip count; samples behind N carry keep = 1
#pragma unroll
            for (int k = 0; k < C; ++k) {
                if (lane == l) trans[k] = (float)run;
                run = run * (double)__shfl(keep[k], l);
            }
        }
    }
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    float wsum = 0.0f;
#pragma unroll
    for (int k = 0; k < C; ++k) {
        const int i = lane * C + k;
        if (i < N) {
            const float w = alpha[k] * trans[k];
            wsum = wsum + w;
            if (weights) weights[i] = w;
            if (rgb && (!LIVE_COLOURS || live[k])) {  // rgb wave-uniform: the sigma-only coarse pass of a fused render has no colours
                acc[0] = composite_accumulate(acc[0], w, rgb[i * 3 + 0]);
                acc[1] = composite_accumulate(acc[1], w, rgb[i * 3 + 1]);
                acc[2] = composite_accumulate(acc[2], w, rgb[i * 3 + 2]);
            }
            acc[3] = acc[3] + w * tv[k];
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = acc[j] + __shfl_xor(acc[j], off);
    }
    if (white_bkgd) {                                                       // rgb + (1 - acc_map), :381-384
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) wsum = wsum + __shfl_xor(wsum, off);
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[j] = acc[j] + (1.0f - wsum);
    }
    if (lane == 0) {
        if (rgb_exp) rgb_exp[0] = acc[0], rgb_exp[1] = acc[1], rgb_exp[2] = acc[2];
        if (t_exp) t_exp[0] = acc[3];
    }
}

// Backward of alpha_composition (the training loops of the reference differentiate through it, train_tgtcs.py:218-309):
// given dL/d rgb_exp [3], dL/d t_exp, dL/d weights [N] of one ray, produce dL/d rgb [N,3] and dL/d sigma [N].
//   w_i = a_i T_i,  T_i = prod_{j<i} k_j,  k_j = 1 - a_j + 1e-10,  a_i = 1 - exp(-s_i d_i),  s_i = relu(relu(sigma_i + noise_i))
//   G_i = g_rgb . c_i + g_t t_i + g_w_i                      (dL/dw_i)
//   dL/da_i = G_i T_i - (sum_{m>i} G_m w_m) / k_i            (every later T_m carries the factor k_i)
//   dL/dsigma_i = dL/da_i * d_i (1 - a_i) * [sigma_i + noise_i > 0]
// One wavefront per ray, lane l owns samples [l*C, l*C+C); the suffix sum is a reverse wave scan.
template <int C>
__device__ __forceinline__ void composite_backward_wave(const float* __restrict__ rgb, const float* __restrict__ sigma,
                                                        const float* __restrict__ ts, const float* __restrict__ noise,
                                                        int N, int white_bkgd, const float* __restrict__ g_rgb,
                                                        const float* __restrict__ g_t, const float* __restrict__ g_w,
                                                        float* __restrict__ d_rgb, float* __restrict__ d_sigma) {
    const int lane = threadIdx.x & 63;
    float alpha[C], tv[C], keep[C], delta[C], live[C];
#pragma unroll
    for (int k = 0; k < C; ++k) {
        const int i = lane * C + k;
        alpha[k] = 0.0f, tv[k] = 0.0f, keep[k] = 1.0f, delta[k] = 0.0f, live[k] = 0.0f;
        if (i < N) {
            const float t0 = ts[i];
            delta[k] = (i + 1 < N) ? ts[i + 1] - t0 : 1e10f;
            const float raw = noise ? sigma[i] + noise[i] : sigma[i];
            live[k] = raw > 0.0f ? 1.0f : 0.0f;
            alpha[k] = 1.0f - expf(-fmaxf(raw, 0.0f) * delta[k]);
            tv[k] = t0;
            keep[k] = 1.0f - alpha[k] + 1e-10f;
        }
    }
    double run = 1.0;
    float trans[C];
    for (int l = 0; l < 64; ++l) {
#pragma unroll
        for (int k = 0; k < C; ++k) {
            if (lane == l) trans[k] = (float)run;
            run = run * (double)__shfl(keep[k], l);
        }
    }
    const float gr = g_rgb ? g_rgb[0] : 0.0f, gg = g_rgb ? g_rgb[1] : 0.0f, gb = g_rgb ? g_rgb[2] : 0.0f;
    const float gt = g_t ? g_t[0] : 0.0f;
    // with a white background rgb_exp also carries -(sum w) in every channel: dL/dw_i gets -(gr + gg + gb)
    const float gwhite = white_bkgd ? -(gr + gg + gb) : 0.0f;
    float G[C], Gw[C], part = 0.0f;
#pragma unroll
    for (int k = 0; k < C; ++k) {
        const int i = lane * C + k;
        G[k] = Gw[k] = 0.0f;
        if (i < N) {
            const float w = alpha[k] * trans[k];
            G[k] = gr * rgb[i * 3 + 0] + gg * rgb[i * 3 + 1] + gb * rgb[i * 3 + 2] + gt * tv[k] + (g_w ? g_w[i] : 0.0f) + gwhite;
            Gw[k] = G[k] * w;
            part += Gw[k];
            if (d_rgb) d_rgb[i * 3 + 0] = w * gr, d_rgb[i * 3 + 1] = w * gg, d_rgb[i * 3 + 2] = w * gb;
        }
    }
    // suffix sums: total of the lanes behind this one, then inside the run
    float incl = part;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float dn = __shfl_down(incl, off);
        if (lane + off < 64) incl = incl + dn;
    }
    float suffix = incl - part;   // sum over lanes > this lane
#pragma unroll
    for (int k = C - 1; k >= 0; --k) {
        const int i = lane * C + k;
        if (i < N && d_sigma) {
            const float d_alpha = G[k] * trans[k] - suffix / keep[k];
            d_sigma[i] = d_alpha * delta[k] * (1.0f - alpha[k]) * live[k];
        }
        suffix += Gw[k];
    }
}

template <int C>
__global__ void __launch_bounds__(256) composite_backward_kernel(const float* __restrict__ rgb, const float* __restrict__ sigma,
                                                                 const float* __restrict__ ts, const float* __restrict__ noise,
                                                                 long long R, int N, int white_bkgd,
                                                                 const float* __restrict__ g_rgb, const float* __restrict__ g_t,
                                                                 const float* __restrict__ g_w, float* __restrict__ d_rgb,
                                                                 float* __restrict__ d_sigma) {
    const long long r = (long long)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    if (r >= R) return;  // wave-uniform
    composite_backward_wave<C>(rgb + r * N * 3, sigma + r * N, ts + r * N, noise ? noise + r * N : nullptr, N, white_bkgd,
                               g_rgb ? g_rgb + r * 3 : nullptr, g_t ? g_t + r : nullptr, g_w ? g_w + r * N : nullptr,
                               d_rgb ? d_rgb + r * N * 3 : nullptr, d_sigma ? d_sigma + r * N : nullptr);
}

template <int C, bool LIVE_COLOURS = false>
__global__ void __launch_bounds__(256) composite_kernel(const float* __restrict__ rgb, const float* __restrict__ sigma,
                                                        const float* __restrict__ ts, long long R, int N,
                                                        float* __restrict__ rgb_exp, float* __restrict__ t_exp,
                                                        float* __restrict__ weights, const float* __restrict__ noise,
                                                        int white_bkgd) {
    const long long r = (long long)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    if (r >= R) return;  // wave-uniform
    composite_wave<C, LIVE_COLOURS>(rgb ? rgb + r * N * 3 : nullptr, sigma + r * N, ts + r * N, N,
                      rgb_exp ? rgb_exp + r * 3 : nullptr, t_exp ? t_exp + r : nullptr,
                      weights ? weights + r * N : nullptr, noise ? noise + r * N : nullptr, white_bkgd);
}

// ------------------------------------------------------------------------------------ geometry cache
// composite_wave's colour sums from a compact list (tgtc_restyle_rays, render.hip).  One wavefront per (latent k, ray r).
// The ray's live samples are the list entries [ray_start[r], ray_start[r+1]) (ascending dense indices s = r * N + i); lane l
// takes those with i in [l*C, l*C+C) -- the run it owns in composite_wave -- in ascending order into accumulators that start
// at 0, then the same xor butterfly.  A sample that is not in the list enters composite_wave's run as acc + w * 0 (its
// colour plane entry is +0) or acc + 0 * c (its weight is 0), which leaves acc unchanged with or without contraction:
// skipping it changes no bit.  w_live[j] = the weight composite_wave computes for the sample, colours rgb_live [K,count,3].
template <int C>
__global__ void __launch_bounds__(256) composite_live_kernel(const unsigned* __restrict__ ray_start,
                                                             const unsigned* __restrict__ live,
                                                             const float* __restrict__ w_live,
                                                             const float* __restrict__ rgb_live, long long R, int N, int K,
                                                             long long count, float* __restrict__ rgb_exp) {
    const long long id = (long long)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    if (id >= (long long)K * R) return;  // wave-uniform
    const long long k = id / R, r = id - k * R;
    const int lane = threadIdx.x & 63;
    const unsigned j1 = ray_start[r + 1];
    const unsigned base = (unsigned)(r * N);              // R * N < 2^31
    const unsigned first = base + (unsigned)(lane * C);   // this lane's run [first, last); lane * C <= 504
    const unsigned last = min(first + (unsigned)C, base + (unsigned)N);
    unsigned lo = ray_start[r], hi = j1;                  // first list entry of the ray that is >= first
    while (lo < hi) {
        const unsigned mid = (lo + hi) >> 1;
        if (live[mid] < first) lo = mid + 1; else hi = mid;
    }
    const float* __restrict__ c = rgb_live + k * count * 3;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int q = 0; q < C; ++q) {
        const unsigned j = lo + (unsigned)q;
        if (j >= j1 || live[j] >= last) break;
        const float w = w_live[j];
        acc[0] = composite_accumulate(acc[0], w, c[(size_t)j * 3 + 0]);
        acc[1] = composite_accumulate(acc[1], w, c[(size_t)j * 3 + 1]);
        acc[2] = composite_accumulate(acc[2], w, c[(size_t)j * 3 + 2]);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[j] = acc[j] + __shfl_xor(acc[j], off);
    }
    if (lane == 0) rgb_exp[id * 3 + 0] = acc[0], rgb_exp[id * 3 + 1] = acc[1], rgb_exp[id * 3 + 2] = acc[2];
}

// tgtc_geometry_pack: the planes of a geometry cache out of the culled render's workspace, one thread per entry of the
// longest plane.  ray_start[r] = the number of list entries below r * N (a binary search; r = R gives count).  A list entry
// outside the sample range (a `count` above the list's real length reads words no build wrote) is stored as sample 0.
struct GeometryPackArgs {
    const unsigned* live;   // the workspace's list
    const float* ts_f;      // [R,N]
    const float* w_f;       // [R,N]
    const float* t_fine;    // [R]
    long long R;
    int N;
    unsigned count;
    unsigned min_weight_bits;
    unsigned* header;       // kGeometryHeaderWords
    float* t_out;
    unsigned* ray_start;
    unsigned* live_out;
    float* ts_live;
    float* w_live;
};
constexpr unsigned kGeometryMagic = 0x43475447u;   // "TGGC"
constexpr unsigned kGeometryVersion = 1;
constexpr int kGeometryHeaderWords = 64;

__global__ void __launch_bounds__(256) geometry_pack_kernel(GeometryPackArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < kGeometryHeaderWords) {
        const unsigned long long R = (unsigned long long)a.R;
        const unsigned words[8] = {kGeometryMagic, kGeometryVersion, (unsigned)R, (unsigned)(R >> 32), (unsigned)a.N, a.count,
                                   a.min_weight_bits, 0u};
        a.header[i] = i < 8 ? words[i] : 0u;
    }
    if (i < a.R) a.t_out[i] = a.t_fine[i];
    if (i <= a.R) {
        const unsigned key = (unsigned)(i * a.N);   // <= R * N < 2^31
        unsigned lo = 0, hi = a.count;
        while (lo < hi) {
            const unsigned mid = (lo + hi) >> 1;
            if (a.live[mid] < key) lo = mid + 1; else hi = mid;
        }
        a.ray_start[i] = lo;
    }
    if (i < a.count) {
        unsigned s = a.live[i];
        if (s >= (unsigned)(a.R * a.N)) s = 0;
        a.live_out[i] = s, a.ts_live[i] = a.ts_f[s], a.w_live[i] = a.w_f[s];
    }
}

// ------------------------------------------------------------------------------------ fine sampling
// reference utils.py:573-609.  One wavefront per ray, per-ray buffers staged in LDS:
//   bins (N-1 midpoints), cdf (N-1), merged depths (N+n_fine).
// The cdf is a float64 running sum rounded to float32 per element, as ATen's CPU cumsum does
// (acc_type<float> = double).  The final torch.sort is realised as a stable rank (counting) sort,
// exact for any input order.
constexpr int kFineMaxN = 256;     // coarse samples per ray supported
constexpr int kFineMaxTotal = 512; // coarse + fine

__global__ void __launch_bounds__(64) sample_fine_kernel(const double* __restrict__ rays_o,
                                                         const double* __restrict__ rays_d,
                                                         const float* __restrict__ ts_in,
                                                         const float* __restrict__ w_in, long long R, int N,
                                                         int NF, double* __restrict__ pts_out,
                                                         float* __restrict__ ts_out) {
    __shared__ float s_bins[kFineMaxN];
    __shared__ float s_cdf[kFineMaxN];
    __shared__ float s_all[kFineMaxTotal];
    const long long r = blockIdx.x;
    const int lane = threadIdx.x;
    const float* ts = ts_in + r * N;
    const float* w = w_in + r * N;
    const int B = N - 1;  // bins / cdf entries
    const int P = N - 2;  // pdf entries

    for (int i = lane; i < N; i += 64) s_all[i] = ts[i];
    for (int i = lane; i < B; i += 64) s_bins[i] = 0.5f * (ts[i + 1] + ts[i]);  // utils.py:574

    // sum of (w + 1e-5) over the interior weights (utils.py:575,584-585)
    double part = 0.0;
    for (int i = lane; i < P; i += 64) part += (double)(w[i + 1] + 1e-5f);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) part += __shfl_xor(part, off);
    const float total = (float)part;

    // cdf[0] = 0, cdf[i+1] = float(sum_{j<=i} pdf[j]) with a float64 running sum (utils.py:586-587).
    // Blocked scan: lane owns pdf entries [lane*C, lane*C+C).
    const int C = (P + 63) / 64;
    double run = 0.0;
    for (int k = 0; k < C; ++k) {
        const int i = lane * C + k;
        if (i < P) run += (double)((w[i + 1] + 1e-5f) / total);
    }
    double incl = run;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double up = __shfl_up(incl, off);
        if (lane >= off) incl += up;
    }
    double prefix = incl - run;
    if (lane == 0) s_cdf[0] = 0.0f;
    for (int k = 0; k < C; ++k) {
        const int i = lane * C + k;
        if (i < P) {
            prefix += (double)((w[i + 1] + 1e-5f) / total);
            s_cdf[i + 1] = (float)prefix;
        }
    }
    __syncthreads();

    // inverse CDF at u = linspace(0,1,NF) (utils.py:589-607)
    for (int j = lane; j < NF; j += 64) {
        const float u = linspace01(j, NF);
        int lo = 0, hi = B;  // searchsorted(right=True): first index with cdf > u
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_cdf[mid] <= u) lo = mid + 1; else hi = mid;
        }
        const int below = max(lo - 1, 0), above = min(lo, B - 1);
        const float c0 = s_cdf[below], c1 = s_cdf[above];
        const float b0 = s_bins[below], b1 = s_bins[above];
        float den = c1 - c0;
        if (den < 1e-5f) den = 1.0f;
        const float t = (u - c0) / den;
        s_all[N + j] = b0 + t * (b1 - b0);
    }
    __syncthreads();

    // stable rank sort of the N+NF depths (utils.py:577)
    const int T = N + NF;
    const double o0 = rays_o[r * 3 + 0], o1 = rays_o[r * 3 + 1], o2 = rays_o[r * 3 + 2];
    const double d0 = rays_d[r * 3 + 0], d1 = rays_d[r * 3 + 1], d2 = rays_d[r * 3 + 2];
    for (int e = lane; e < T; e += 64) {
        const float v = s_all[e];
        int rank = 0;
        for (int q = 0; q < T; ++q) {
            const float x = s_all[q];
            rank += (x < v) || (x == v && q < e);
        }
        ts_out[r * T + rank] = v;
        if (pts_out) {
            double* p = pts_out + (r * T + rank) * 3;
            p[0] = o0 + d0 * (double)v;  // utils.py:578
            p[1] = o1 + d1 * (double)v;
            p[2] = o2 + d2 * (double)v;
        }
    }
}

// ------------------------------------------------------------------------------- coarse -> fine, one kernel
// composite_kernel<C> (weights only) followed by sample_fine_kernel, for a render that wants no coarse image: one wavefront
// per ray, kCtfWaves rays per workgroup, each wave on an LDS strip of its own and no workgroup barrier (wave_sync hands
// over).  The weights never leave the strip unless `weights_out` is given.
//   weights   composite_wave's: alpha, keep, the sequential float64 product rounded to float32 per sample, alpha * trans,
//             the product stepping over the factors that are exactly 1 (transmittance_of_live).
//   cdf       sample_fine_kernel's: the same strided float64 sum, the same blocked float64 scan with
//             ceil((N-2)/64) entries per lane, the same binary search, clamps and `den < 1e-5f` rule.
//   merge     the ray's coarse depths and its inverse-CDF samples are two runs.  Where both are non-decreasing (neighbour
//             compares, one ballot; a NaN fails them), the stable order of cat(coarse, fine) -- what the counting sort
//             gives -- puts coarse element i at i + #(fine < ts[i]) and fine element j at j + #(coarse <= v_j): two
//             binary searches in the other run instead of N + NF compares per element.  Otherwise (unsorted depths from
//             a caller, a one-ulp inversion between two bins) the ray takes the counting sort.  Both compare with the
//             float `<` / `==`, under which -0 and +0 tie.
constexpr int kCtfWaves = 4;

struct CtfStrip {
    float all[kFineMaxTotal];   // coarse depths, then the new samples
    float w[kFineMaxN];         // coarse weights, then the cdf
};

template <int C>
__global__ void __launch_bounds__(64 * kCtfWaves) coarse_to_fine_kernel(const float* __restrict__ sigma_in,
                                                                        const float* __restrict__ ts_in, long long R, int N,
                                                                        int NF, float* __restrict__ ts_out,
                                                                        float* __restrict__ weights_out,
                                                                        unsigned* __restrict__ took_sort) {
    __shared__ CtfStrip strips[kCtfWaves];
    const long long r = (long long)blockIdx.x * kCtfWaves + (threadIdx.x >> 6);
    if (r >= R) return;  // wave-uniform, and no workgroup barrier below
    const int lane = threadIdx.x & 63;
    float* const s_all = strips[threadIdx.x >> 6].all;
    float* const s_w = strips[threadIdx.x >> 6].w;
    const float* ts = ts_in + r * N;
    const float* sigma = sigma_in + r * N;
    const int B = N - 1;  // bins / cdf entries
    const int P = N - 2;  // pdf entries
    const int T = N + NF;

    for (int i = lane; i < N; i += 64) s_all[i] = ts[i];
    wave_sync();

    // ---- weights (composite_wave<C>): lane l owns samples [l*C, l*C+C)
    float alpha[C], keep[C];
#pragma unroll
    for (int k = 0; k < C; ++k) {
        const int i = lane * C + k;
        alpha[k] = 0.0f, keep[k] = 1.0f;
        if (i < N) {
            const float t0 = s_all[i];
            const float delta = (i + 1 < N) ? s_all[i + 1] - t0 : 1e10f;    // utils.py:367-369
            const float dens = fmaxf(fmaxf(sigma[i], 0.0f), 0.0f);          // relu(relu(.)) :365,:376
            alpha[k] = 1.0f - expf(-dens * delta);
            keep[k] = 1.0f - alpha[k] + 1e-10f;                             // :378
        }
    }
    float trans[C];
    transmittance_of_live<C>(alpha, keep, lane, trans);
#pragma unroll
    for (int k = 0; k < C; ++k) {
        const int i = lane * C + k;
        if (i < N) {
            const float w = alpha[k] * trans[k];
            s_w[i] = w;
            if (weights_out) weights_out[r * N + i] = w;
        }
    }
    wave_sync();

    // ---- cdf (sample_fine_kernel): sum of (w + 1e-5) over the interior weights (utils.py:575,584-585)
    double part = 0.0;
    for (int i = lane; i < P; i += 64) part += (double)(s_w[i + 1] + 1e-5f);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) part += __shfl_xor(part, off);
    const float total = (float)part;

    // cdf[0] = 0, cdf[i+1] = float(sum_{j<=i} pdf[j]) with a float64 running sum (utils.py:586-587).  Blocked scan: lane
    // owns pdf entries [lane*CP, lane*CP+CP), read into registers before any lane overwrites the weights with the cdf.
    const int CP = (P + 63) / 64;   // <= 4
    float pdf[4];
    double lane_sum = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = lane * CP + k;
        pdf[k] = 0.0f;
        if (k < CP && i < P) {
            pdf[k] = (s_w[i + 1] + 1e-5f) / total;
            lane_sum += (double)pdf[k];
        }
    }
    double incl = lane_sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double up = __shfl_up(incl, off);
        if (lane >= off) incl += up;
    }
    double prefix = incl - lane_sum;
    wave_sync();
    if (lane == 0) s_w[0] = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = lane * CP + k;
        if (k < CP && i < P) {
            prefix += (double)pdf[k];
            s_w[i + 1] = (float)prefix;
        }
    }
    wave_sync();

    // ---- inverse CDF at u = linspace(0,1,NF) (utils.py:589-607); bins = midpoints of the coarse depths (utils.py:574)
    for (int j = lane; j < NF; j += 64) {
        const float u = linspace01(j, NF);
        int lo = 0, hi = B;  // searchsorted(right=True): first index with cdf > u
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_w[mid] <= u) lo = mid + 1; else hi = mid;
        }
        const int below = max(lo - 1, 0), above = min(lo, B - 1);
        const float c0 = s_w[below], c1 = s_w[above];
        const float b0 = 0.5f * (s_all[below + 1] + s_all[below]), b1 = 0.5f * (s_all[above + 1] + s_all[above]);
        float den = c1 - c0;
        if (den < 1e-5f) den = 1.0f;
        const float t = (u - c0) / den;
        s_all[N + j] = b0 + t * (b1 - b0);
    }
    wave_sync();

    // ---- are both runs non-decreasing?  Element e is compared with its successor inside its own run.
    bool bad = false;
    for (int e = lane; e < T - 1; e += 64)
        if (e != N - 1) bad = bad || !(s_all[e] <= s_all[e + 1]);
    const bool merge = __ballot(bad) == 0ull;   // wave-uniform
    if (took_sort && lane == 0) took_sort[r] = merge ? 0u : 1u;

    float* out = ts_out + r * T;
    if (merge) {
        for (int e = lane; e < T; e += 64) {
            const float v = s_all[e];
            int lo, hi;
            if (e < N) {   // #(fine < v): first fine index whose value is not below v
                lo = N, hi = T;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (s_all[mid] < v) lo = mid + 1; else hi = mid;
                }
                out[e + (lo - N)] = v;
            } else {       // #(coarse <= v): first coarse index whose value is above v
                lo = 0, hi = N;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (s_all[mid] <= v) lo = mid + 1; else hi = mid;
                }
                out[(e - N) + lo] = v;
            }
        }
    } else {
        // stable rank sort of the N+NF depths (utils.py:577), exact for any input order
        for (int e = lane; e < T; e += 64) {
            const float v = s_all[e];
            int rank = 0;
            for (int q = 0; q < T; ++q) {
                const float x = s_all[q];
                rank += (x < v) || (x == v && q < e);
            }
            out[rank] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------ latents
// reference models.py:490-506
__global__ void __launch_bounds__(256) latents_kernel(const float* __restrict__ latents, const float* __restrict__ mu,
                                                      int S, int F, int D, const long long* __restrict__ style_ids,
                                                      const long long* __restrict__ frame_ids, long long R,
                                                      float sigma_scale, int tile7, float* __restrict__ out) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= R * D) return;
    const long long r = idx / D;
    const int c = (int)(idx % D);
    const long long sid = style_ids[r];
    long long flat = sid * F + frame_ids[r];   // :492
    const long long rows = (long long)S * F;
    if (tile7) flat = flat % rows;             // table.repeat(7,1)[flat] for flat < 7*rows (:496)
    const float z = latents[flat * D + c];
    const float m = mu[sid * D + c];
    out[idx] = m + sigma_scale * (z - m);      // :504-505
}

// gradient of the same: d_latents[flat] += sigma_scale * g, d_mu[sid] += (1 - sigma_scale) * g (both pre-zeroed, atomics:
// many rays share a row)
__global__ void __launch_bounds__(256) latents_backward_kernel(const float* __restrict__ g, int S, int F, int D,
                                                               const long long* __restrict__ style_ids,
                                                               const long long* __restrict__ frame_ids, long long R,
                                                               float sigma_scale, int tile7, float* __restrict__ d_latents,
                                                               float* __restrict__ d_mu) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= R * D) return;
    const long long r = idx / D;
    const int c = (int)(idx % D);
    const long long sid = style_ids[r];
    long long flat = sid * F + frame_ids[r];
    if (tile7) flat = flat % ((long long)S * F);
    const float v = g[idx];
    if (d_latents) atomicAdd(d_latents + flat * D + c, sigma_scale * v);
    if (d_mu) atomicAdd(d_mu + sid * D + c, (1.0f - sigma_scale) * v);
}

}  // namespace tgtc

using namespace tgtc;

static inline unsigned blocks_for(long long n, int per) { return (unsigned)((n + per - 1) / per); }

extern "C" int tgtc_gen_rays(int H, int W, double fx, double fy, double cx, double cy, const float* c2w,
                             int pixel_alignment, int ndc, double ndc_near, int64_t first_pixel, int64_t n,
                             double* rays_o, double* rays_d, void* stream) {
    TGTC_REQUIRE(H > 0 && W > 0 && c2w, "gen_rays: bad argument");
    TGTC_REQUIRE(first_pixel >= 0 && n >= 0 && first_pixel + n <= (int64_t)H * W, "gen_rays: pixel range outside the frame");
    if (n == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d, "gen_rays: null output");
    RayGenArgs a;
    a.cam.H = H, a.cam.W = W, a.cam.fx = fx, a.cam.fy = fy, a.cam.cx = cx, a.cam.cy = cy;
    for (int i = 0; i < 12; ++i) a.c2w[i] = c2w[i];
    a.cam.pixel_alignment = pixel_alignment, a.cam.ndc = ndc, a.cam.ndc_near = ndc_near, a.first = first_pixel, a.n = n;
    gen_rays_kernel<<<blocks_for(n, 256), 256, 0, as_stream(stream)>>>(a, rays_o, rays_d);
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

extern "C" int tgtc_sample_coarse(const double* rays_o, const double* rays_d, int64_t R, int N, float near_,
                                  float far_, const float* jitter, double* pts, float* ts, void* stream) {
    TGTC_REQUIRE(R >= 0 && N >= 2, "sample_coarse: bad argument");
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(ts && (!pts || (rays_o && rays_d)), "sample_coarse: null pointer");
    sample_coarse_kernel<<<blocks_for(R * N, 256), 256, 0, as_stream(stream)>>>(rays_o, rays_d, R, N, near_, far_,
                                                                               jitter, pts, ts);
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

extern "C" int tgtc_posenc(const void* x, int x_is_f64, int64_t M, int L, float* out, void* stream) {
    TGTC_REQUIRE(M >= 0 && L >= 0 && L <= 30, "posenc: bad argument");
    if (M == 0) return TGTC_OK;
    TGTC_REQUIRE(x && out, "posenc: null pointer");
    const unsigned nb = blocks_for(M * (3 + 6 * L), 256);
    if (x_is_f64)
        posenc_kernel<double><<<nb, 256, 0, as_stream(stream)>>>((const double*)x, M, L, out);
    else
        posenc_kernel<float><<<nb, 256, 0, as_stream(stream)>>>((const float*)x, M, L, out);
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

namespace tgtc {
int launch_composite_ex(const float* rgb, const float* sigma, const float* ts, int64_t R, int N, float* rgb_exp,
                        float* t_exp, float* weights, hipStream_t st, const float* noise, int white_bkgd) {
    const unsigned nb = blocks_for(R, 4);
    const int C = (N + 63) / 64;
#define TGTC_COMPOSITE(CC) composite_kernel<CC><<<nb, 256, 0, st>>>(rgb, sigma, ts, R, N, rgb_exp, t_exp, weights, noise, white_bkgd)
    switch (C) {
        case 1: TGTC_COMPOSITE(1); break;
        case 2: TGTC_COMPOSITE(2); break;
        case 3: TGTC_COMPOSITE(3); break;
        case 4: TGTC_COMPOSITE(4); break;
        case 5: case 6: case 7: case 8: TGTC_COMPOSITE(8); break;
        default: return fail(TGTC_ERR_UNSUPPORTED, "composite: N=%d samples per ray exceeds 512", N);
    }
#undef TGTC_COMPOSITE
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

int launch_composite(const float* rgb, const float* sigma, const float* ts, int64_t R, int N, float* rgb_exp,
                     float* t_exp, float* weights, hipStream_t st) {
    return launch_composite_ex(rgb, sigma, ts, R, N, rgb_exp, t_exp, weights, st, nullptr, 0);
}

// rgb_exp [K,R,3] from a geometry cache's list planes and the compact colours; the lane runs are launch_composite_ex's.
int launch_composite_live(const uint32_t* ray_start, const uint32_t* live, const float* w_live, const float* rgb_live, int64_t R,
                          int N, int K, int64_t count, float* rgb_exp, hipStream_t st) {
    const unsigned nb = blocks_for((long long)K * R, 4);
    const int C = (N + 63) / 64;
#define TGTC_COMPOSITE_LIVE(CC) composite_live_kernel<CC><<<nb, 256, 0, st>>>(ray_start, live, w_live, rgb_live, R, N, K, count, rgb_exp)
    switch (C) {
        case 1: TGTC_COMPOSITE_LIVE(1); break;
        case 2: TGTC_COMPOSITE_LIVE(2); break;
        case 3: TGTC_COMPOSITE_LIVE(3); break;
        case 4: TGTC_COMPOSITE_LIVE(4); break;
        case 5: case 6: case 7: case 8: TGTC_COMPOSITE_LIVE(8); break;
        default: return fail(TGTC_ERR_UNSUPPORTED, "composite_live: N=%d samples per ray exceeds 512", N);
    }
#undef TGTC_COMPOSITE_LIVE
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

int launch_geometry_pack(const uint32_t* live, const float* ts_f, const float* w_f, const float* t_fine, int64_t R, int N,
                         int64_t count, float min_weight, uint32_t* header, float* t_out, uint32_t* ray_start, uint32_t* live_out,
                         float* ts_live, float* w_live, hipStream_t st) {
    GeometryPackArgs a{live, ts_f, w_f, t_fine, R, N, (unsigned)count, __builtin_bit_cast(unsigned, min_weight),
                       header, t_out, ray_start, live_out, ts_live, w_live};
    const long long longest = std::max<long long>({count, R + 1, kGeometryHeaderWords});
    geometry_pack_kernel<<<blocks_for(longest, 256), 256, 0, st>>>(a);
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

int launch_composite_backward(const float* rgb, const float* sigma, const float* ts, const float* noise, int64_t R, int N,
                              int white_bkgd, const float* g_rgb, const float* g_t, const float* g_w, float* d_rgb,
                              float* d_sigma, hipStream_t st) {
    const unsigned nb = blocks_for(R, 4);
    const int C = (N + 63) / 64;
#define TGTC_COMPOSITE_BWD(CC) \
    composite_backward_kernel<CC><<<nb, 256, 0, st>>>(rgb, sigma, ts, noise, R, N, white_bkgd, g_rgb, g_t, g_w, d_rgb, d_sigma)
    switch (C) {
        case 1: TGTC_COMPOSITE_BWD(1); break;
        case 2: TGTC_COMPOSITE_BWD(2); break;
        case 3: TGTC_COMPOSITE_BWD(3); break;
        case 4: TGTC_COMPOSITE_BWD(4); break;
        case 5: case 6: case 7: case 8: TGTC_COMPOSITE_BWD(8); break;
        default: return fail(TGTC_ERR_UNSUPPORTED, "composite_backward: N=%d samples per ray exceeds 512", N);
    }
#undef TGTC_COMPOSITE_BWD
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

int launch_sample_fine(const double* rays_o, const double* rays_d, const float* ts, const float* weights, int64_t R,
                       int N, int n_fine, double* pts_out, float* ts_out, hipStream_t st) {
    if (N < 3 || N > kFineMaxN || n_fine < 1 || N + n_fine > kFineMaxTotal)
        return fail(TGTC_ERR_UNSUPPORTED, "sample_fine: N=%d n_fine=%d outside [3,%d] / total<=%d", N, n_fine,
                    kFineMaxN, kFineMaxTotal);
    sample_fine_kernel<<<(unsigned)R, 64, 0, st>>>(rays_o, rays_d, ts, weights, R, N, n_fine, pts_out, ts_out);
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

// launch_composite (weights only) + launch_sample_fine (depths only) in one kernel; took_sort [R] or null: 1 where the ray
// took the counting sort.
int launch_coarse_to_fine(const float* sigma, const float* ts, int64_t R, int N, int n_fine, float* ts_out, float* weights_out,
                          uint32_t* took_sort, hipStream_t st) {
    if (N < 3 || N > kFineMaxN || n_fine < 1 || N + n_fine > kFineMaxTotal)
        return fail(TGTC_ERR_UNSUPPORTED, "coarse_to_fine: N=%d n_fine=%d outside [3,%d] / total<=%d", N, n_fine, kFineMaxN,
                    kFineMaxTotal);
    const unsigned nb = blocks_for(R, kCtfWaves);
#define TGTC_CTF(CC) coarse_to_fine_kernel<CC><<<nb, 64 * kCtfWaves, 0, st>>>(sigma, ts, R, N, n_fine, ts_out, weights_out, took_sort)
    switch ((N + 63) / 64) {   // composite_kernel's C; N <= 256
        case 1: TGTC_CTF(1); break;
        case 2: TGTC_CTF(2); break;
        case 3: TGTC_CTF(3); break;
        default: TGTC_CTF(4); break;
    }
#undef TGTC_CTF
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

// launch_composite with colours read at live samples only (composite_wave's LIVE_COLOURS)
int launch_composite_live_colours(const float* rgb, const float* sigma, const float* ts, int64_t R, int N, float* rgb_exp,
                                  float* t_exp, float* weights, hipStream_t st) {
    const unsigned nb = blocks_for(R, 4);
    const int C = (N + 63) / 64;
#define TGTC_COMPOSITE_LC(CC) composite_kernel<CC, true><<<nb, 256, 0, st>>>(rgb, sigma, ts, R, N, rgb_exp, t_exp, weights, nullptr, 0)
    switch (C) {
        case 1: TGTC_COMPOSITE_LC(1); break;
        case 2: TGTC_COMPOSITE_LC(2); break;
        case 3: TGTC_COMPOSITE_LC(3); break;
        case 4: TGTC_COMPOSITE_LC(4); break;
        case 5: case 6: case 7: case 8: TGTC_COMPOSITE_LC(8); break;
        default: return fail(TGTC_ERR_UNSUPPORTED, "composite: N=%d samples per ray exceeds 512", N);
    }
#undef TGTC_COMPOSITE_LC
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}
}  // namespace tgtc

extern "C" int tgtc_coarse_to_fine(const float* sigma, const float* ts, int64_t R, int N, int n_fine, float* ts_out,
                                   float* weights_out, void* stream) {
    TGTC_REQUIRE(R >= 0, "coarse_to_fine: bad argument");
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(sigma && ts && ts_out, "coarse_to_fine: null pointer");
    return launch_coarse_to_fine(sigma, ts, R, N, n_fine, ts_out, weights_out, nullptr, as_stream(stream));
}

extern "C" int tgtc_coarse_to_fine_traced(const float* sigma, const float* ts, int64_t R, int N, int n_fine, float* ts_out,
                                          float* weights_out, uint32_t* took_sort, void* stream) {
    TGTC_REQUIRE(R >= 0, "coarse_to_fine_traced: bad argument");
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(sigma && ts && ts_out && took_sort, "coarse_to_fine_traced: null pointer");
    return launch_coarse_to_fine(sigma, ts, R, N, n_fine, ts_out, weights_out, took_sort, as_stream(stream));
}

extern "C" int tgtc_composite_live_colours(const float* rgb, const float* sigma, const float* ts, int64_t R, int N,
                                           float* rgb_exp, float* t_exp, float* weights, void* stream) {
    TGTC_REQUIRE(R >= 0 && N >= 1, "composite_live_colours: bad argument");
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rgb && sigma && ts && rgb_exp && t_exp, "composite_live_colours: null pointer");
    return launch_composite_live_colours(rgb, sigma, ts, R, N, rgb_exp, t_exp, weights, as_stream(stream));
}

extern "C" int tgtc_composite(const float* rgb, const float* sigma, const float* ts, int64_t R, int N,
                              float* rgb_exp, float* t_exp, float* weights, void* stream) {
    TGTC_REQUIRE(R >= 0 && N >= 1, "composite: bad argument");
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rgb && sigma && ts && rgb_exp && t_exp, "composite: null pointer");
    return launch_composite(rgb, sigma, ts, R, N, rgb_exp, t_exp, weights, as_stream(stream));
}

extern "C" int tgtc_composite_train(const float* rgb, const float* sigma, const float* ts, const float* noise,
                                    int white_bkgd, int64_t R, int N, float* rgb_exp, float* t_exp, float* weights,
                                    void* stream) {
    TGTC_REQUIRE(R >= 0 && N >= 1, "composite_train: bad argument");
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rgb && sigma && ts && rgb_exp && t_exp, "composite_train: null pointer");
    return launch_composite_ex(rgb, sigma, ts, R, N, rgb_exp, t_exp, weights, as_stream(stream), noise, white_bkgd);
}

extern "C" int tgtc_composite_backward(const float* rgb, const float* sigma, const float* ts, const float* noise,
                                       int white_bkgd, int64_t R, int N, const float* grad_rgb_exp,
                                       const float* grad_t_exp, const float* grad_weights, float* grad_rgb,
                                       float* grad_sigma, void* stream) {
    TGTC_REQUIRE(R >= 0 && N >= 1, "composite_backward: bad argument");
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rgb && sigma && ts && (grad_rgb || grad_sigma), "composite_backward: null pointer");
    return launch_composite_backward(rgb, sigma, ts, noise, R, N, white_bkgd, grad_rgb_exp, grad_t_exp, grad_weights, grad_rgb,
                                     grad_sigma, as_stream(stream));
}

extern "C" int tgtc_sample_fine(const double* rays_o, const double* rays_d, const float* ts, const float* weights,
                                int64_t R, int N, int n_fine, double* pts_out, float* ts_out, void* stream) {
    TGTC_REQUIRE(R >= 0, "sample_fine: bad argument");
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d && ts && weights && ts_out, "sample_fine: null pointer");
    return launch_sample_fine(rays_o, rays_d, ts, weights, R, N, n_fine, pts_out, ts_out, as_stream(stream));
}

// ------------------------------------------------------------------------------------------------ image epilogue
// One workgroup per frame finds min / max of the depth (exact: min/max are order independent), then the same
// workgroup converts its frame.  numpy semantics: float32 arithmetic throughout (x*255, the division), float ->
// int32 truncates toward zero, int32 -> uint8 keeps the low byte.
__global__ void __launch_bounds__(1024) image_epilogue_kernel(const float* __restrict__ rgb, const float* __restrict__ t,
                                                             long long pixels, float eps, unsigned char* __restrict__ rgb8,
                                                             unsigned char* __restrict__ depth8) {
    __shared__ float s_min[16], s_max[16];
    const long long base = (long long)blockIdx.x * pixels;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (depth8) {
        float lo = __builtin_inff(), hi = -__builtin_inff();
        for (long long i = tid; i < pixels; i += 1024) {
            const float v = t[base + i];
            lo = fminf(lo, v), hi = fmaxf(hi, v);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) lo = fminf(lo, __shfl_xor(lo, o)), hi = fmaxf(hi, __shfl_xor(hi, o));
        if (lane == 0) s_min[wave] = lo, s_max[wave] = hi;
        __syncthreads();
        lo = s_min[0], hi = s_max[0];
#pragma unroll
        for (int w = 1; w < 16; ++w) lo = fminf(lo, s_min[w]), hi = fmaxf(hi, s_max[w]);
        const float den = __fadd_rn(__fsub_rn(hi, lo), eps);
        for (long long i = tid; i < pixels; i += 1024) {
            const float v = __fdiv_rn(__fsub_rn(t[base + i], lo), den);   // IEEE division, as numpy
            depth8[base + i] = (unsigned char)(int)__fmul_rn(v, 255.0f);
        }
    }
    if (rgb8) {
        for (long long i = tid; i < pixels * 3; i += 1024) rgb8[base * 3 + i] = (unsigned char)(int)__fmul_rn(rgb[base * 3 + i], 255.0f);
    }
}

extern "C" int tgtc_image_epilogue(const float* rgb, const float* t, int64_t frames, int64_t pixels, float eps,
                                   unsigned char* rgb8, unsigned char* depth8, void* stream) {
    TGTC_REQUIRE(frames >= 0 && pixels >= 0 && frames < (1LL << 31), "image_epilogue: bad argument");
    if (frames == 0 || pixels == 0) return TGTC_OK;
    TGTC_REQUIRE((!rgb8 || rgb) && (!depth8 || t) && (rgb8 || depth8), "image_epilogue: null pointer");
    image_epilogue_kernel<<<(unsigned)frames, 1024, 0, as_stream(stream)>>>(rgb, t, pixels, eps, rgb8, depth8);
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

extern "C" int tgtc_latents_backward(const float* grad_out, int S, int F, int D, const int64_t* style_ids,
                                     const int64_t* frame_ids, int64_t R, float sigma_scale, int tile7, float* d_latents,
                                     float* d_mu, void* stream) {
    TGTC_REQUIRE(S > 0 && F > 0 && D > 0 && R >= 0, "latents_backward: bad argument");
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(grad_out && style_ids && frame_ids, "latents_backward: null pointer");
    latents_backward_kernel<<<blocks_for(R * D, 256), 256, 0, as_stream(stream)>>>(
        grad_out, S, F, D, (const long long*)style_ids, (const long long*)frame_ids, R, sigma_scale, tile7, d_latents, d_mu);
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

extern "C" int tgtc_latents_forward(const float* latents, const float* mu, int S, int F, int D,
                                    const int64_t* style_ids, const int64_t* frame_ids, int64_t R, float sigma_scale,
                                    int tile7, float* out, void* stream) {
    TGTC_REQUIRE(S > 0 && F > 0 && D > 0 && R >= 0, "latents_forward: bad argument");
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(latents && mu && style_ids && frame_ids && out, "latents_forward: null pointer");
    latents_kernel<<<blocks_for(R * D, 256), 256, 0, as_stream(stream)>>>(
        latents, mu, S, F, D, (const long long*)style_ids, (const long long*)frame_ids, R, sigma_scale, tile7, out);
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}
