// 2-D style pass: patch embedding, the style transformer, the CNN decoder,
// the VGG-19 prefix, calc_mean_std / AdaIN and the trans_test.py post-processing.
//
// One MFMA GEMM kernel does all the heavy lifting: C = act(alpha * A * B^T + bias [+ residual]) on
// 128x128x32 workgroup tiles (4 waves, each a 64x64 sub-tile of 4x4 v_mfma_f32_16x16x32_f16 accumulators),
// operands staged global -> registers -> LDS as fp16 hi (+ lo) halves.  The A operand comes through a
// "row loader", which makes the same kernel a dense linear layer, a batched attention product, an 8x8
// patch embedding or a 3x3 convolution with reflection padding and nearest x2 upsampling folded into
// the gather (implicit GEMM over token-major / NHWC feature maps: a k-step is 32 consecutive channels of
// one tap, i.e. one 128-byte line per row).
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/tgtc_style2d.h"
#include "../../include/tgtc_train.h"
#include "common.h"
#include "mlp_core.h"

namespace tgtc {

constexpr int BK = 32, LDK = 40;  // LDK: 32 halves + 8 pad -> 80-byte rows, conflict-free b128 reads

// ------------------------------------------------------------------------------------------------ row loaders
// load4(ctx, k0, kq, v): v[j] = A(row, k0 + kq + j), zero outside the matrix.  k0 is the workgroup-uniform start of the
// 32-deep k block, kq the thread's quad inside it (a multiple of 4): loaders whose index math has a uniform part (the
// convolution's tap) can keep it in scalar registers.
struct DenseRows {  // A(m,k) = p[m*ld + k]
    const float* p;
    long long ld, batch_stride;
    int rows, K;
    // B operands that are network weights: the same matrix already split into fp16 hi / lo at handle creation (same
    // indexing as p), or null
    const half_t* h16 = nullptr;
    const half_t* l16 = nullptr;
    struct Ctx { const float* row; };
    __device__ Ctx prep(int m) const { return Ctx{m < rows ? p + (long long)m * ld : nullptr}; }
    __device__ void load4(const Ctx& c, int k0, int kq, float (&v)[4]) const {
        const int k = k0 + kq;
        if (c.row && k + 3 < K && ((reinterpret_cast<size_t>(c.row + k) & 15) == 0)) {
            const float4 t = *reinterpret_cast<const float4*>(c.row + k);
            v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (c.row && k + j < K) ? c.row[k + j] : 0.0f;
        }
    }
};

// A(m, k) = the k-th column of a concatenation of up to four segments that is never materialised (the layer inputs of the
// style trainer, include/tgtc_train.h).  A segment is a per-sample plane (row m) or a per-ray one (row m / n, n samples per
// ray).  The widths are not multiples of 4 (63, 95, 351, 607 columns in front of a segment): a quad may straddle two.
struct SegRows {
    struct Seg { const float* ptr; long long ld; int width, per_ray; };
    Seg seg[4];
    int nseg, rows, K, n;
    struct Ctx { int m, ray; };
    __device__ Ctx prep(int m) const { return m < rows ? Ctx{m, m / n} : Ctx{-1, 0}; }
    __device__ float at(const Ctx& c, int k) const {   // c.m >= 0, 0 <= k < K
        float v = 0.0f;
        int lo = k;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if (s < nseg && lo >= 0 && lo < seg[s].width) v = seg[s].ptr[(long long)(seg[s].per_ray ? c.ray : c.m) * seg[s].ld + lo];
            lo -= s < nseg ? seg[s].width : 0;
        }
        return v;
    }
    __device__ void load4(const Ctx& c, int k0, int kq, float (&v)[4]) const {
        const int k = k0 + kq;
        v[0] = v[1] = v[2] = v[3] = 0.0f;
        if (c.m < 0 || k >= K) return;
        int lo = k;                                    // the quad's first column, counted from the segment's first
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if (s < nseg && lo + 3 >= 0 && lo < seg[s].width) {
                const float* row = seg[s].ptr + (long long)(seg[s].per_ray ? c.ray : c.m) * seg[s].ld;
                if (lo >= 0 && lo + 3 < seg[s].width && ((reinterpret_cast<size_t>(row + lo) & 15) == 0)) {
                    const float4 t = *reinterpret_cast<const float4*>(row + lo);
                    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (lo + j >= 0 && lo + j < seg[s].width) v[j] = row[lo + j];
                }
            }
            lo -= s < nseg ? seg[s].width : 0;
        }
    }
};

__device__ __forceinline__ int reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

struct ConvNHWC {  // 3x3, stride 1, ReflectionPad(1); input token-major [Hs*Ws, C]; optional nearest x2 upsample first
    const float* p;
    long long batch_stride;
    int H, W, Hs, Ws, C, logC, up, rows, K;  // H,W: logical (post-upsample) = output size; k = tap*C + c
    struct Ctx { int y, x; };
    __device__ Ctx prep(int m) const { return m < rows ? Ctx{m / W, m % W} : Ctx{-1, 0}; }
    __device__ void load4(const Ctx& c, int k0, int kq, float (&v)[4]) const {
        const int k = k0 + kq;
        if (c.y < 0 || k >= K) {
            v[0] = v[1] = v[2] = v[3] = 0.0f;
            return;
        }
        // C is a power of two >= 32 (conv3x3 checks): a 32-deep k block lies inside one tap, so the tap and its (dy, dx) are
        // workgroup-uniform and stay in scalar registers
        const int tap = k0 >> logC, ch = k & (C - 1);
        const int dy = tap / 3 - 1, dx = tap - 3 * (tap / 3) - 1;
        int sy = reflect(c.y + dy, H), sx = reflect(c.x + dx, W);
        if (up) sy >>= 1, sx >>= 1;
        const float4 t = *reinterpret_cast<const float4*>(p + (((long long)sy * Ws + sx) << logC) + ch);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    }
};

struct ConvSmall {  // ksize x ksize (1 or 3), few input channels, arbitrary input strides; k = tap*C + c
    const float* p;
    long long batch_stride, s_pix, s_ch;
    int H, W, C, ksize, rows, K;
    struct Ctx { int y, x; };
    __device__ Ctx prep(int m) const { return m < rows ? Ctx{m / W, m % W} : Ctx{-1, 0}; }
    __device__ void load4(const Ctx& c, int k0, int kq, float (&v)[4]) const {
        const int k = k0 + kq;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int kk = k + j;
            float val = 0.0f;
            if (c.y >= 0 && kk < K) {
                const int tap = kk / C, ch = kk % C;
                int sy = c.y, sx = c.x;
                if (ksize == 3) sy = reflect(c.y + tap / 3 - 1, H), sx = reflect(c.x + tap % 3 - 1, W);
                val = p[((long long)sy * W + sx) * s_pix + ch * s_ch];
            }
            v[j] = val;
        }
    }
};

struct PatchRows {  // 8x8 stride-8 patches of an NCHW image [3,H,W]; k = c*64 + dy*8 + dx (Conv2d weight order)
    const float* p;
    long long batch_stride;
    int H, W, wt, rows, K;  // wt = W/8 tokens per row
    struct Ctx { int py, px; };
    __device__ Ctx prep(int m) const { return m < rows ? Ctx{m / wt, m % wt} : Ctx{-1, 0}; }
    __device__ void load4(const Ctx& c, int k0, int kq, float (&v)[4]) const {
        const int k = k0 + kq;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int kk = k + j;
            float val = 0.0f;
            if (c.py >= 0 && kk < K) {
                const int ch = kk >> 6, dy = (kk >> 3) & 7, dx = kk & 7;
                val = p[((long long)ch * H + (8 * c.py + dy)) * W + 8 * c.px + dx];
            }
            v[j] = val;
        }
    }
};

struct GemmOut {
    float* C;
    long long sm, sn, batch_stride;  // C[m*sm + n*sn]
    const float* bias;               // [N] or null
    const float* res;                // same layout as C, or null
    float alpha;
    int relu;
    long long bias_batch_stride = 0; // floats between the bias vectors of consecutive batches (blockIdx.z)
    const float* alpha_dev = nullptr; // optional second scale factor read from device memory (gradient rescaling)
    const float* row_alpha = nullptr; // optional third one per output row m, [M] in device memory (per-sample gradient rescaling)
};

// four fp32 values -> fp16 hi (+ lo) halves in LDS.  The lo halves come straight out of v_fma_mixlo/mixhi_f16
// (v * 1.0 - h in fp32, rounded once): two packed converts and four mixed FMAs instead of sixteen convert / subtract
// instructions -- the staging of these GEMMs is VALU-bound, not memory-bound.
template <bool SPLIT>
__device__ __forceinline__ void put4(half_t* hi, half_t* lo, const float (&v)[4]) {
    typedef _Float16 half2v __attribute__((ext_vector_type(2)));
    typedef float float2v __attribute__((ext_vector_type(2)));
    unsigned h[2], l[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        h[p] = __builtin_bit_cast(unsigned, __builtin_convertvector((float2v{v[2 * p], v[2 * p + 1]}), half2v));
        if constexpr (SPLIT) {
            asm("v_fma_mixlo_f16 %0, %1, 1.0, -%2 op_sel:[0,0,0] op_sel_hi:[0,0,1]" : "=v"(l[p]) : "v"(v[2 * p]), "v"(h[p]));
            asm("v_fma_mixhi_f16 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(l[p]) : "v"(v[2 * p + 1]), "v"(h[p]));
        }
    }
    *reinterpret_cast<uint2*>(hi) = uint2{h[0], h[1]};
    if constexpr (SPLIT) *reinterpret_cast<uint2*>(lo) = uint2{l[0], l[1]};
}

// B operand: either rows of W [N][K] (nn.Linear / conv weights, BL = DenseRows) or, with B_KMAJOR, a
// k-major matrix B[k][n] = p[k*ld + n] (the V operand of attention).
// WT = 16x16 accumulator tiles per wave and dimension: 4 -> 128x128 workgroup tiles, 2 -> 64x64, 1 -> 32x32 (launch_gemm
// picks; a [2500,512] projection is only 20x4 tiles of 128x128 on 256 CUs).
// B_PRE: the B rows come pre-split (DenseRows::h16 / l16, K a multiple of 4): two 8-byte loads per quad go straight to LDS,
// no conversion in the loop.
// A_PRE: the same for a DenseRows A operand whose halves the producer wrote (the training side's gradients).
template <class AL, bool SPLIT, bool B_KMAJOR, int WT, bool B_PRE = false, bool A_PRE = false>
__global__ void __launch_bounds__(256) gemm_kernel(AL al, DenseRows bl, GemmOut out, int M, int N, int K) {
    constexpr int NP = SPLIT ? 2 : 1;
    static_assert(!(B_PRE && B_KMAJOR), "pre-split weights are row operands");
    static_assert(!A_PRE || std::is_same<AL, DenseRows>::value, "pre-split A operands are dense rows");
    constexpr int BM = 32 * WT, BN = 32 * WT;
    static_assert(!B_KMAJOR || WT == 4, "the k-major B loader is written for 128-wide tiles");
    __shared__ __attribute__((aligned(16))) half_t sA[NP][BM][LDK];
    __shared__ __attribute__((aligned(16))) half_t sB[NP][BN][LDK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, n16 = lane & 15;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    if constexpr (!std::is_same<AL, SegRows>::value) al.p += (long long)blockIdx.z * al.batch_stride;   // (SegRows: one batch)
    bl.p += (long long)blockIdx.z * bl.batch_stride;
    if constexpr (B_PRE) bl.h16 += (long long)blockIdx.z * bl.batch_stride, bl.l16 += (long long)blockIdx.z * bl.batch_stride;
    if constexpr (A_PRE) al.h16 += (long long)blockIdx.z * al.batch_stride, al.l16 += (long long)blockIdx.z * al.batch_stride;
    out.C += (long long)blockIdx.z * out.batch_stride;
    if (out.res) out.res += (long long)blockIdx.z * out.batch_stride;
    if (out.bias) out.bias += (long long)blockIdx.z * out.bias_batch_stride;

    // staging map: 4 rows x one k-quad per thread
    const int srow = tid >> 3, skq = (tid & 7) * 4;
    typename AL::Ctx actx[WT];
    DenseRows::Ctx bctx[WT];
#pragma unroll
    for (int i = 0; i < WT; ++i) {
        actx[i] = al.prep(m0 + srow + 32 * i);
        if constexpr (!B_KMAJOR) bctx[i] = bl.prep(n0 + srow + 32 * i);
    }
    // k-major B: thread covers k = (tid>>5) + 8i, n-quad (tid&31)*4
    const int bk = tid >> 5, bnq = (tid & 31) * 4;

    float ra[A_PRE ? 1 : WT][4], rb[B_PRE ? 1 : WT][4];
    uint2 rbh[B_PRE ? WT : 1], rbl[B_PRE ? WT : 1], rah[A_PRE ? WT : 1], ral[A_PRE ? WT : 1];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < WT; ++i) {
            if constexpr (A_PRE) {
                const int row = m0 + srow + 32 * i, k = k0 + skq;
                const bool ok = row < al.rows && k < al.K;
                const long long o = (long long)row * al.ld + k;
                rah[i] = ok ? *reinterpret_cast<const uint2*>(al.h16 + o) : uint2{0u, 0u};
                if constexpr (SPLIT) ral[i] = ok ? *reinterpret_cast<const uint2*>(al.l16 + o) : uint2{0u, 0u};
            } else {
                al.load4(actx[i], k0, skq, ra[i]);
            }
            if constexpr (B_PRE) {
                const int row = n0 + srow + 32 * i, k = k0 + skq;
                const bool ok = row < bl.rows && k < bl.K;     // K % 4 == 0: a quad is inside or outside as a whole
                const long long o = (long long)row * bl.ld + k;
                rbh[i] = ok ? *reinterpret_cast<const uint2*>(bl.h16 + o) : uint2{0u, 0u};
                if constexpr (SPLIT) rbl[i] = ok ? *reinterpret_cast<const uint2*>(bl.l16 + o) : uint2{0u, 0u};
            } else if constexpr (!B_KMAJOR) {
                bl.load4(bctx[i], k0, skq, rb[i]);
            } else {
                const int k = k0 + bk + 8 * i;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    rb[i][j] = (k < K && n0 + bnq + j < N) ? bl.p[(long long)k * bl.ld + n0 + bnq + j] : 0.0f;
            }
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int i = 0; i < WT; ++i) {
            if constexpr (A_PRE) {
                *reinterpret_cast<uint2*>(&sA[0][srow + 32 * i][skq]) = rah[i];
                if constexpr (SPLIT) *reinterpret_cast<uint2*>(&sA[1][srow + 32 * i][skq]) = ral[i];
            } else {
                put4<SPLIT>(&sA[0][srow + 32 * i][skq], &sA[NP - 1][srow + 32 * i][skq], ra[i]);
            }
            if constexpr (B_PRE) {
                *reinterpret_cast<uint2*>(&sB[0][srow + 32 * i][skq]) = rbh[i];
                if constexpr (SPLIT) *reinterpret_cast<uint2*>(&sB[1][srow + 32 * i][skq]) = rbl[i];
            } else if constexpr (!B_KMAJOR) {
                put4<SPLIT>(&sB[0][srow + 32 * i][skq], &sB[NP - 1][srow + 32 * i][skq], rb[i]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const half_t h = (half_t)rb[i][j];
                    sB[0][bnq + j][bk + 8 * i] = h;
                    if constexpr (SPLIT) sB[1][bnq + j][bk + 8 * i] = (half_t)(rb[i][j] - (float)h);
                }
            }
        }
    };

    float4v acc[WT][WT];
#pragma unroll
    for (int i = 0; i < WT; ++i)
#pragma unroll
        for (int j = 0; j < WT; ++j) acc[i][j] = float4v{0.f, 0.f, 0.f, 0.f};

    const int KT = (K + BK - 1) / BK;
    fetch(0);
    for (int kt = 0; kt < KT; ++kt) {
        stash();
        __syncthreads();
        if (kt + 1 < KT) fetch((kt + 1) * BK);
        half8 ah[WT], al_[WT], bh[WT], bl_[WT];
#pragma unroll
        for (int i = 0; i < WT; ++i) {
            ah[i] = *reinterpret_cast<const half8*>(&sA[0][16 * WT * wm + 16 * i + n16][8 * g]);
            bh[i] = *reinterpret_cast<const half8*>(&sB[0][16 * WT * wn + 16 * i + n16][8 * g]);
            if constexpr (SPLIT) {
                al_[i] = *reinterpret_cast<const half8*>(&sA[1][16 * WT * wm + 16 * i + n16][8 * g]);
                bl_[i] = *reinterpret_cast<const half8*>(&sB[1][16 * WT * wn + 16 * i + n16][8 * g]);
            }
        }
#pragma unroll
        for (int i = 0; i < WT; ++i)
#pragma unroll
            for (int j = 0; j < WT; ++j) {
                acc[i][j] = mfma16(ah[i], bh[j], acc[i][j]);
                if constexpr (SPLIT) {
                    acc[i][j] = mfma16(al_[i], bh[j], acc[i][j]);
                    acc[i][j] = mfma16(ah[i], bl_[j], acc[i][j]);
                }
            }
        __syncthreads();
    }

    // epilogue: lane holds rows m = .. + 4g + r, column n = .. + (lane & 15)
    const float alpha = out.alpha_dev ? out.alpha * *out.alpha_dev : out.alpha;
#pragma unroll
    for (int i = 0; i < WT; ++i)
#pragma unroll
        for (int j = 0; j < WT; ++j) {
            const int n = n0 + 16 * WT * wn + 16 * j + n16;
            if (n >= N) continue;
            const float b = out.bias ? out.bias[n] : 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + 16 * WT * wm + 16 * i + 4 * g + r;
                if (m >= M) continue;
                const long long o = (long long)m * out.sm + (long long)n * out.sn;
                const float am = out.row_alpha ? alpha * out.row_alpha[m] : alpha;
                float v = am * acc[i][j][r] + b;
                if (out.res) v += out.res[o];
                if (out.relu) v = fmaxf(v, 0.0f);
                out.C[o] = v;
            }
        }
}

// ------------------------------------------------------------------------------------------------ attention
// nn.MultiheadAttention's softmax(q k^T / sqrt(64)) v for 8 heads of 64, never materialising the [8, L, S] scores
// (transformer.py:167-263 through torch's MultiheadAttention; 2 500 x 2 500 tokens at 400x400).
//
// attn_prep_kernel splits the projected q / k / v once into the fp16 hi / lo operands the MFMAs take (q scaled by
// 1/8, exact), v TRANSPOSED per feature ([512][S_pad]) and k / v zero-padded to a multiple of 64 keys.
// attn_kernel: one workgroup = one head x 64 queries, four waves of 16 queries, key tiles of 64 through LDS.
// Both products are evaluated transposed so that the QUERY sits on the MFMA lane:
//   S^T[key, q] = K[key, d] . Q^T[d, q]          (A = K tile rows from LDS, B = Q^T fragments held in registers)
//   O^T[d, q]  += V^T[d, key] . P^T[key, q]      (A = V^T tile rows from LDS, B = P^T)
// The accumulator tile of S^T (rows = keys 4g+r, column = query lane&15) is, after exp and conversion, exactly the B
// fragment of the second product (two 16-key tiles form one 32-deep k-step, CDNA guide "An accumulator tile as the
// next MFMA's operand"), so P never crosses lanes or LDS; a query's running maximum and sum need two shuffles
// (over the four lane groups) per key tile.  fp16x3: every product is hi*hi + lo*hi + hi*lo.
constexpr int kAttnLd = 72;   // LDS row stride in halves (64 + 8 pad: conflict-free 16-byte reads)

__global__ void __launch_bounds__(256) attn_prep_kernel(const float* __restrict__ q, long long ldq, int L,
                                                        const float* __restrict__ k, long long ldk,
                                                        const float* __restrict__ v, long long ldv, int S, int S_pad,
                                                        half_t* __restrict__ qh, half_t* __restrict__ ql,
                                                        half_t* __restrict__ kh, half_t* __restrict__ kl,
                                                        half_t* __restrict__ vth, half_t* __restrict__ vtl) {
    const long long nq = (long long)L * 512, nk = (long long)S_pad * 512;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    auto split = [](float x, half_t& h, half_t& l) {
        h = (half_t)x;
        l = (half_t)(x - (float)h);
    };
    if (i < nq) {
        const long long r = i >> 9;
        const int c = (int)(i & 511);
        split(q[r * ldq + c] * 0.125f, qh[i], ql[i]);
    } else if (i < nq + nk) {
        const long long j = i - nq, r = j >> 9;
        const int c = (int)(j & 511);
        split(r < S ? k[r * ldk + c] : 0.0f, kh[j], kl[j]);
    } else if (i < nq + 2 * nk) {
        // v^T: thread index walks [feature][key] so the stores are coalesced
        const long long j = i - nq - nk;
        const int c = (int)(j / S_pad);
        const long long r = j % S_pad;
        split(r < S ? v[r * ldv + c] : 0.0f, vth[j], vtl[j]);
    }
}

template <bool SPLIT>
__global__ void __launch_bounds__(256) attn_kernel(const half_t* __restrict__ qh, const half_t* __restrict__ ql,
                                                   const half_t* __restrict__ kh, const half_t* __restrict__ kl,
                                                   const half_t* __restrict__ vth, const half_t* __restrict__ vtl,
                                                   int L, int S, int S_pad, float* __restrict__ out,
                                                   float* __restrict__ part_o, float* __restrict__ part_ml) {
    constexpr int NP = SPLIT ? 2 : 1;
    __shared__ __attribute__((aligned(16))) half_t sK[NP][64][kAttnLd];
    __shared__ __attribute__((aligned(16))) half_t sV[NP][64][kAttnLd];   // [d][key]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, n = lane & 15;
    const int head = blockIdx.y;
    const int qi = blockIdx.x * 64 + wave * 16 + n;        // this lane's query
    const bool qok = qi < L;

    half8 Qh[2], Ql[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const long long o = (long long)(qok ? qi : 0) * 512 + head * 64 + 32 * ks + 8 * g;
        Qh[ks] = qok ? *reinterpret_cast<const half8*>(qh + o) : half8{};
        if constexpr (SPLIT) Ql[ks] = qok ? *reinterpret_cast<const half8*>(ql + o) : half8{};
    }
    float4v O[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) O[dt] = float4v{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, lsum = 0.0f;

    const int srow = tid >> 2, sc0 = (tid & 3) * 16;    // staging: 64 rows x 64 halves = 256 threads x 2 half8
    // the NEXT tile travels global -> registers while the current one is multiplied (one LDS buffer, two barriers a tile)
    half8 nk[NP][2], nv[NP][2];
    auto fetch = [&](int key0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int col = sc0 + 8 * i;
            const long long ko = (long long)(key0 + srow) * 512 + head * 64 + col;
            const long long vo = (long long)(head * 64 + srow) * S_pad + key0 + col;
            nk[0][i] = *reinterpret_cast<const half8*>(kh + ko);
            nv[0][i] = *reinterpret_cast<const half8*>(vth + vo);
            if constexpr (SPLIT) {
                nk[1][i] = *reinterpret_cast<const half8*>(kl + ko);
                nv[1][i] = *reinterpret_cast<const half8*>(vtl + vo);
            }
        }
    };
    // key split (gridDim.z > 1): this workgroup owns tiles [t0, t1) of the S_pad/64 key tiles and leaves an unnormalised
    // partial result (O, running max, running sum) for attn_combine_kernel -- 1 250 query waves alone are ~1.2 per SIMD
    const int n_tiles = S_pad / 64;
    const int key_begin = (int)((long long)blockIdx.z * n_tiles / gridDim.z) * 64;
    const int key_end = min(S, (int)((long long)(blockIdx.z + 1) * n_tiles / gridDim.z) * 64);
    fetch(key_begin);
    for (int key0 = key_begin; key0 < key_end; key0 += 64) {
        __syncthreads();   // the previous tile is consumed
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int col = sc0 + 8 * i;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                *reinterpret_cast<half8*>(&sK[p][srow][col]) = nk[p][i];
                *reinterpret_cast<half8*>(&sV[p][srow][col]) = nv[p][i];
            }
        }
        __syncthreads();
        if (key0 + 64 < key_end) fetch(key0 + 64);

        // S^T tiles: keys 16kt + 4g + r, query n
        float4v sc[4];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            sc[kt] = float4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const half8 ah = *reinterpret_cast<const half8*>(&sK[0][16 * kt + n][32 * ks + 8 * g]);
                sc[kt] = mfma16(ah, Qh[ks], sc[kt]);
                if constexpr (SPLIT) {
                    const half8 al = *reinterpret_cast<const half8*>(&sK[1][16 * kt + n][32 * ks + 8 * g]);
                    sc[kt] = mfma16(al, Qh[ks], sc[kt]);
                    sc[kt] = mfma16(ah, Ql[ks], sc[kt]);
                }
            }
        }
        // online softmax for query n: this lane holds 16 of the tile's 64 keys, the other lane groups the rest
        float tmax = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (key0 + 16 * kt + 4 * g + r >= S) sc[kt][r] = -INFINITY;   // padding keys
                tmax = fmaxf(tmax, sc[kt][r]);
            }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 16));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
        const float m_new = fmaxf(m, tmax);          // finite: every tile holds at least one real key
        const float alpha = expf(m - m_new);         // exp(-inf) = 0 on the first tile
        m = m_new;
        lsum *= alpha;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) O[dt] = O[dt] * alpha;
        half8 Ph[2], Pl[2];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = expf(sc[kt][r] - m);
                lsum += p;
                const half_t h = (half_t)p;
                Ph[kt >> 1][(kt & 1) * 4 + r] = h;
                if constexpr (SPLIT) Pl[kt >> 1][(kt & 1) * 4 + r] = (half_t)(p - (float)h);
            }
        // O^T tiles: features 16dt + 4g + r, query n;  k-step ks = keys 32ks + {4g..4g+3, 16+4g..16+4g+3}
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                typedef _Float16 half4 __attribute__((ext_vector_type(4)));
                const half4 a0 = *reinterpret_cast<const half4*>(&sV[0][16 * dt + n][32 * ks + 4 * g]);
                const half4 a1 = *reinterpret_cast<const half4*>(&sV[0][16 * dt + n][32 * ks + 16 + 4 * g]);
                const half8 ah = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
                O[dt] = mfma16(ah, Ph[ks], O[dt]);
                if constexpr (SPLIT) {
                    const half4 b0 = *reinterpret_cast<const half4*>(&sV[1][16 * dt + n][32 * ks + 4 * g]);
                    const half4 b1 = *reinterpret_cast<const half4*>(&sV[1][16 * dt + n][32 * ks + 16 + 4 * g]);
                    const half8 al = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
                    O[dt] = mfma16(al, Ph[ks], O[dt]);
                    O[dt] = mfma16(ah, Pl[ks], O[dt]);
                }
            }
    }
    lsum += __shfl_xor(lsum, 16);
    lsum += __shfl_xor(lsum, 32);
    if (gridDim.z > 1) {
        if (qok) {
            float* po = part_o + ((long long)blockIdx.z * L + qi) * 512 + head * 64;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                *reinterpret_cast<float4*>(po + 16 * dt + 4 * g) = float4{O[dt][0], O[dt][1], O[dt][2], O[dt][3]};
            if (g == 0) {
                float* pm = part_ml + (((long long)blockIdx.z * L + qi) * 8 + head) * 2;
                pm[0] = m, pm[1] = lsum;
            }
        }
        return;
    }
    if (qok) {
        const float inv = 1.0f / lsum;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            float4 o4{O[dt][0] * inv, O[dt][1] * inv, O[dt][2] * inv, O[dt][3] * inv};
            *reinterpret_cast<float4*>(out + (long long)qi * 512 + head * 64 + 16 * dt + 4 * g) = o4;
        }
    }
}

// out[q, head*64 + d] = sum_z O_z e^(m_z - M) / sum_z l_z e^(m_z - M),  M = max_z m_z   (the key splits of attn_kernel)
__global__ void __launch_bounds__(256) attn_combine_kernel(const float* __restrict__ part_o, const float* __restrict__ part_ml,
                                                           int L, int nsplit, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;     // one float4 of the output
    if (i >= (long long)L * 128) return;
    const long long q = i >> 7;
    const int c4 = (int)(i & 127), head = c4 >> 4;
    float M = -INFINITY;
    for (int z = 0; z < nsplit; ++z) M = fmaxf(M, part_ml[(((long long)z * L + q) * 8 + head) * 2]);
    float den = 0.0f;
    float4 acc{0.f, 0.f, 0.f, 0.f};
    for (int z = 0; z < nsplit; ++z) {
        const float* ml = part_ml + (((long long)z * L + q) * 8 + head) * 2;
        const float w = expf(ml[0] - M);
        den += ml[1] * w;
        const float4 o = *reinterpret_cast<const float4*>(part_o + ((long long)z * L + q) * 512 + 4 * c4);
        acc.x += o.x * w, acc.y += o.y * w, acc.z += o.z * w, acc.w += o.w * w;
    }
    const float inv = 1.0f / den;
    *reinterpret_cast<float4*>(out + q * 512 + 4 * c4) = float4{acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv};
}

// ------------------------------------------------------------------------------------------------ small kernels
// out[row] = LayerNorm(a[row] + b[row]) * w + bias over 512 features; one wavefront per row (eps 1e-5)
__global__ void __launch_bounds__(256) layernorm512_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                           const float* __restrict__ w, const float* __restrict__ bias,
                                                           float* __restrict__ out, int rows, long long lda) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float v[8], s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = lane + 64 * j;
        v[j] = a[(long long)row * lda + c] + (b ? b[(long long)row * 512 + c] : 0.0f);
        s += v[j];
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) s += __shfl_xor(s, off);
    const float mean = s * (1.0f / 512.0f);
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) q += (v[j] - mean) * (v[j] - mean);
#pragma unroll
    for (int off = 32; off; off >>= 1) q += __shfl_xor(q, off);
    const float rstd = 1.0f / sqrtf(q * (1.0f / 512.0f) + 1e-5f);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = lane + 64 * j;
        out[(long long)row * 512 + c] = (v[j] - mean) * rstd * w[c] + bias[c];
    }
}

// in-place softmax over rows of length S; one workgroup per row
__global__ void __launch_bounds__(256) softmax_rows_kernel(float* __restrict__ x, int S) {
    __shared__ float red[4];
    float* row = x + (long long)blockIdx.x * S;
    const int tid = threadIdx.x;
    float mx = -INFINITY;
    for (int i = tid; i < S; i += 256) mx = fmaxf(mx, row[i]);
#pragma unroll
    for (int off = 32; off; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float s = 0.f;
    for (int i = tid; i < S; i += 256) {
        const float e = expf(row[i] - mx);
        row[i] = e;
        s += e;
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) s += __shfl_xor(s, off);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    const float inv = 1.0f / (red[0] + red[1] + red[2] + red[3]);
    for (int i = tid; i < S; i += 256) row[i] *= inv;
}

__global__ void __launch_bounds__(256) add_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                  float* __restrict__ out, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = a[i] + b[i];
}

// MaxPool2d(2,2,ceil_mode=True) on token-major [H*W, C]
__global__ void __launch_bounds__(256) maxpool2_kernel(const float* __restrict__ in, int H, int W, int C,
                                                       float* __restrict__ out) {
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)Ho * Wo * C) return;
    const int c = (int)(i % C);
    const int p = (int)(i / C), y = p / Wo, x = p % Wo;
    float m = -INFINITY;
    for (int dy = 0; dy < 2; ++dy)
        for (int dx = 0; dx < 2; ++dx) {
            const int sy = 2 * y + dy, sx = 2 * x + dx;
            if (sy < H && sx < W) m = fmaxf(m, in[((long long)sy * W + sx) * C + c]);
        }
    out[i] = m;
}

// [n, C] -> [C, n] (to_nchw) or back
__global__ void __launch_bounds__(256) transpose_kernel(const float* __restrict__ in, int rows, int cols,
                                                        float* __restrict__ out) {
    __shared__ float tile[32][33];
    const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int j = ty; j < 32; j += 8)
        if (by + j < rows && bx + tx < cols) tile[j][tx] = in[(long long)(by + j) * cols + bx + tx];
    __syncthreads();
    for (int j = ty; j < 32; j += 8)
        if (bx + j < cols && by + tx < rows) out[(long long)(bx + j) * rows + by + tx] = tile[tx][j];
}

// ---- training-side dense layers (tgtc_s2d_linear_backward): helpers
// [rows, cols] -> [cols, ld_out] (ld_out >= rows; the pad columns are cleared by the caller)
// (`gate`, optional, same shape as `in`: elements whose gate is <= 0 read as zero -- the ReLU of the forward, applied to the
// incoming gradient on the fly)
__global__ void __launch_bounds__(256) transpose_ld_kernel(const float* __restrict__ in, long long rows, int cols,
                                                           float* __restrict__ out, long long ld_out,
                                                           const float* __restrict__ scale = nullptr,
                                                           const float* __restrict__ gate = nullptr) {
    __shared__ float tile[32][33];
    const long long by = (long long)blockIdx.y * 32;
    const int bx = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int j = ty; j < 32; j += 8)
        if (by + j < rows && bx + tx < cols) {
            const long long o = (by + j) * cols + bx + tx;
            tile[j][tx] = (gate && !(gate[o] > 0.0f)) ? 0.0f : in[o];
        }
    __syncthreads();
    for (int j = ty; j < 32; j += 8)
        if (bx + j < cols && by + tx < rows) out[(long long)(bx + j) * ld_out + by + tx] = tile[tx][j] * (scale ? *scale : 1.0f);
}
// out halves = split(gate ? in * scale : 0): the scaled, ReLU-gated gradient as a pre-split GEMM operand; the scale is the
// one of the element's row (row_inv [rows]: its reciprocal, a power of two), cols elements per row
__global__ void __launch_bounds__(256) scale_split_kernel(const float* __restrict__ in, long long n, int cols,
                                                          const float* __restrict__ row_inv, const float* __restrict__ gate,
                                                          half_t* __restrict__ hi, half_t* __restrict__ lo) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = (gate && !(gate[i] > 0.0f)) ? 0.0f : in[i] * (1.0f / row_inv[i / cols]);
    const half_t h = (half_t)v;
    hi[i] = h, lo[i] = (half_t)(v - (float)h);
}
// fp32 -> fp16 hi / lo halves (the GEMM's pre-split B operand)
__global__ void __launch_bounds__(256) split_kernel(const float* __restrict__ in, long long n, half_t* __restrict__ hi,
                                                    half_t* __restrict__ lo) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = in[i];
    const half_t h = (half_t)v;
    hi[i] = h, lo[i] = (half_t)(v - (float)h);
}
// transpose_ld_kernel writing the halves instead: [rows, cols] fp32 -> hi / lo [cols, ld_out] fp16
__global__ void __launch_bounds__(256) transpose_ld_half_kernel(const float* __restrict__ in, long long rows, int cols,
                                                                half_t* __restrict__ hi, half_t* __restrict__ lo, long long ld_out,
                                                                const float* __restrict__ scale = nullptr,
                                                                const float* __restrict__ gate = nullptr) {
    __shared__ float tile[32][33];
    const long long by = (long long)blockIdx.y * 32;
    const int bx = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int j = ty; j < 32; j += 8)
        if (by + j < rows && bx + tx < cols) {
            const long long o = (by + j) * cols + bx + tx;
            tile[j][tx] = (gate && !(gate[o] > 0.0f)) ? 0.0f : in[o];
        }
    __syncthreads();
    for (int j = ty; j < 32; j += 8)
        if (bx + j < cols && by + tx < rows) {
            const float v = tile[tx][j] * (scale ? *scale : 1.0f);
            const half_t h = (half_t)v;
            const long long o = (long long)(bx + j) * ld_out + by + tx;
            hi[o] = h, lo[o] = (half_t)(v - (float)h);
        }
}
// transpose_ld_half_kernel for the style trainer's segmented layer input: hi / lo [K, ld_out] fp16 straight from the segments
__global__ void __launch_bounds__(256) transpose_seg_half_kernel(SegRows al, half_t* __restrict__ hi, half_t* __restrict__ lo,
                                                                 long long ld_out) {
    __shared__ float tile[32][33];
    const int by = blockIdx.y * 32, bx = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int j = ty; j < 32; j += 8)
        if (by + j < al.rows && bx + tx < al.K) tile[j][tx] = al.at(al.prep(by + j), bx + tx);
    __syncthreads();
    for (int j = ty; j < 32; j += 8)
        if (bx + j < al.K && by + tx < al.rows) {
            const float v = tile[tx][j];
            const half_t h = (half_t)v;
            const long long o = (long long)(bx + j) * ld_out + by + tx;
            hi[o] = h, lo[o] = (half_t)(v - (float)h);
        }
}
// columns [0, cols) of in [rows, ld_in] -> out [cols, rows] fp32 and, with `hi`, its fp16 hi / lo halves (split_kernel's):
// a row sub-block of a transposed weight as the B operand of the dx GEMM
__global__ void __launch_bounds__(256) transpose_sub_kernel(const float* __restrict__ in, long long ld_in, int rows, int cols,
                                                            float* __restrict__ out, half_t* __restrict__ hi,
                                                            half_t* __restrict__ lo) {
    __shared__ float tile[32][33];
    const int by = blockIdx.y * 32, bx = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int j = ty; j < 32; j += 8)
        if (by + j < rows && bx + tx < cols) tile[j][tx] = in[(long long)(by + j) * ld_in + bx + tx];
    __syncthreads();
    for (int j = ty; j < 32; j += 8)
        if (bx + j < cols && by + tx < rows) {
            const float v = tile[tx][j];
            const long long o = (long long)(bx + j) * rows + by + tx;
            out[o] = v;
            if (hi) {
                const half_t h = (half_t)v;
                hi[o] = h, lo[o] = (half_t)(v - (float)h);
            }
        }
}
// out[r, c] = sum over the n samples of ray r of scale * gated dy[r*n + i, c]: what the ray's latent row sees of a layer's
// gradient (the latent columns of the weight multiply this sum once, not every sample)
__global__ void __launch_bounds__(256) ray_sum_kernel(const float* __restrict__ dy, const float* __restrict__ gate, long long R,
                                                      int n, int cols, const float* __restrict__ scale,
                                                      float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= R * cols) return;
    const long long r = i / cols;
    const int c = (int)(i - r * cols);
    const float sc = *scale;
    float s = 0.0f;
    for (int j = 0; j < n; ++j) {
        const long long o = (r * n + j) * cols + c;
        s += (gate && !(gate[o] > 0.0f)) ? 0.0f : dy[o] * sc;
    }
    out[i] = s;
}
// Gradients arrive many orders of magnitude below 1 (a mean over the batch sits in front of them), below the range in which
// an fp16 hi/lo split is exact.  They are rescaled by a power of two -- largest magnitude to ~2^10 -- on their way into the
// GEMM operands and the products scaled back; the factor never leaves the device.
//   sc[0] = bits of max |g| (atomicMax on the non-negative float's bits), then sc[1] = s, sc[2] = 1/s
__global__ void __launch_bounds__(256) absmax_kernel(const float* __restrict__ g, long long n, unsigned* __restrict__ sc,
                                                     const float* __restrict__ gate) {
    unsigned m = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        if (!gate || gate[i] > 0.0f) m = max(m, __float_as_uint(fabsf(g[i])));
#pragma unroll
    for (int off = 32; off; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(sc, m);
}
__global__ void grad_scale_kernel(float* __restrict__ sc) {
    const unsigned bits = reinterpret_cast<unsigned*>(sc)[0];
    const int e = (int)((bits >> 23) & 0xff) - 127;            // max |g| in [2^e, 2^(e+1))
    const bool ok = bits != 0 && ((bits >> 23) & 0xff) != 0xff;  // zero / inf / nan: leave the values alone
    const int k = ok ? max(-100, min(100, 10 - e)) : 0;
    sc[1] = ldexpf(1.0f, k), sc[2] = ldexpf(1.0f, -k);
}
__global__ void __launch_bounds__(256) scale_copy_kernel(const float* __restrict__ in, long long n, int cols,
                                                         const float* __restrict__ row_inv, float* __restrict__ out,
                                                         const float* __restrict__ gate) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (gate && !(gate[i] > 0.0f)) ? 0.0f : in[i] * (1.0f / row_inv[i / cols]);
}
// The scale of ONE sample's gradient row for dx = dy . W: a batch mixes rows of very different size (a sample behind a
// surface carries 2^-30 of its neighbour's gradient), and under one scale for the whole batch the small rows fall below the
// fp16 range of the split and come out with a few bits.  dx's rows do not mix samples, so each gets its own power of two --
// largest magnitude of the row (ungated, as absmax_kernel) to ~2^10 -- and the GEMM epilogue scales row m back by
// row_inv[m] = 2^-k.  |k| <= 126 keeps both factors normal floats; a zero / non-finite row keeps k = 0.  One wave per row.
__global__ void __launch_bounds__(256) row_scale_kernel(const float* __restrict__ g, long long rows, int cols,
                                                        float* __restrict__ row_inv) {
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;   // wave-uniform
    unsigned m = 0;
    for (int c = threadIdx.x & 63; c < cols; c += 64) m = max(m, __float_as_uint(fabsf(g[r * cols + c])));
#pragma unroll
    for (int off = 32; off; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off));
    if ((threadIdx.x & 63) == 0) {
        const int e = (int)((m >> 23) & 0xff) - 127;
        const bool ok = m != 0 && ((m >> 23) & 0xff) != 0xff;
        row_inv[r] = ldexpf(1.0f, ok ? -max(-126, min(126, 10 - e)) : 0);
    }
}
// out[i] = sum_s part[s][i]
__global__ void __launch_bounds__(256) sum_partials_kernel(const float* __restrict__ part, int nsplit, long long n,
                                                           float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.0f;
    for (int z = 0; z < nsplit; ++z) s += part[(long long)z * n + i];
    out[i] = s;
}
// out[row] += scale * sum of (hi + lo)[row][chunk]: one workgroup per (row, chunk of `mc` elements), out pre-zeroed
__global__ void __launch_bounds__(256) rowsum_kernel(const half_t* __restrict__ hi, const half_t* __restrict__ lo, long long n,
                                                     long long ld, long long mc, float* __restrict__ out,
                                                     const float* __restrict__ scale = nullptr) {
    __shared__ float red[4];
    const long long b = (long long)blockIdx.y * mc, e = min(n, b + mc);
    const long long r0 = (long long)blockIdx.x * ld;
    float s = 0.0f;
    for (long long i = b + threadIdx.x; i < e; i += 256) s += (float)hi[r0 + i] + (float)lo[r0 + i];
#pragma unroll
    for (int off = 32; off; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out + blockIdx.x, (red[0] + red[1] + red[2] + red[3]) * (scale ? *scale : 1.0f));
}
// mode 0: dx = dy * (y > 0) (ReLU);  mode 1: dx = dy * y * (1 - y) (sigmoid);  mode 2: y = sigmoid(dy) (forward, `y` unused)
__global__ void __launch_bounds__(256) act_kernel(const float* __restrict__ dy, const float* __restrict__ y, long long n,
                                                  int mode, float* __restrict__ dx) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float g = dy[i];
    if (mode == 0) dx[i] = y[i] > 0.0f ? g : 0.0f;
    else if (mode == 1) dx[i] = g * y[i] * (1.0f - y[i]);
    else dx[i] = 1.0f / (1.0f + expf(-g));
}

// per-channel mean and sqrt(unbiased var + eps) over HW; one workgroup per channel (function.py:4-12)
__global__ void __launch_bounds__(256) mean_std_kernel(const float* __restrict__ feat, long long HW, float eps,
                                                       float* __restrict__ mean, float* __restrict__ std_) {
    __shared__ double red[2][4];
    const float* row = feat + (long long)blockIdx.x * HW;
    double s = 0.0;
    for (long long i = threadIdx.x; i < HW; i += 256) s += row[i];
#pragma unroll
    for (int off = 32; off; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) red[0][threadIdx.x >> 6] = s;
    __syncthreads();
    const double mu = (red[0][0] + red[0][1] + red[0][2] + red[0][3]) / (double)HW;
    double q = 0.0;
    for (long long i = threadIdx.x; i < HW; i += 256) {
        const double d = row[i] - mu;
        q += d * d;
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) q += __shfl_xor(q, off);
    if ((threadIdx.x & 63) == 0) red[1][threadIdx.x >> 6] = q;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double var = (red[1][0] + red[1][1] + red[1][2] + red[1][3]) / (double)(HW - 1);
        mean[blockIdx.x] = (float)mu;
        std_[blockIdx.x] = sqrtf((float)var + eps);
    }
}

__global__ void __launch_bounds__(256) adain_kernel(const float* __restrict__ content, long long HW, int C,
                                                    const float* __restrict__ st, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= HW * C) return;
    const int c = (int)(i / HW);
    // st: [cm | cs | sm | ss], each C
    out[i] = (content[i] - st[c]) / st[C + c] * st[3 * C + c] + st[2 * C + c];
}

// nn.Upsample(mode='bilinear', align_corners=True)
__global__ void __launch_bounds__(256) resize_bilinear_kernel(const float* __restrict__ in, int C, int h, int w,
                                                              float* __restrict__ out, int H, int W) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)C * H * W) return;
    const int x = (int)(i % W), y = (int)((i / W) % H), c = (int)(i / ((long long)W * H));
    const float ry = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f, rx = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
    const float fy = ry * y, fx = rx * x;
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 + (y0 < h - 1), x1 = x0 + (x0 < w - 1);
    const float ly = fy - y0, lx = fx - x0;
    const float* p = in + (long long)c * h * w;
    out[i] = (1.f - ly) * ((1.f - lx) * p[y0 * w + x0] + lx * p[y0 * w + x1]) +
             ly * ((1.f - lx) * p[y1 * w + x0] + lx * p[y1 * w + x1]);
}

// trans_test.py:176.  hs token-major [n,512]; flat (c,p) order index f = r*512 + j -> c = f / n, p = f % n.
// One workgroup per output column j; float64 accumulation.
__global__ void __launch_bounds__(256) style_feature_kernel(const float* __restrict__ hs, int n,
                                                            float* __restrict__ feature) {
    __shared__ double red[2][4];
    const int j = blockIdx.x;
    double s = 0.0;
    for (int r = threadIdx.x; r < n; r += 256) {
        const long long f = (long long)r * 512 + j;
        s += hs[(f % n) * 512 + f / n];
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) red[0][threadIdx.x >> 6] = s;
    __syncthreads();
    const double mu = (red[0][0] + red[0][1] + red[0][2] + red[0][3]) / n;
    double q = 0.0;
    for (int r = threadIdx.x; r < n; r += 256) {
        const long long f = (long long)r * 512 + j;
        const double d = hs[(f % n) * 512 + f / n] - mu;
        q += d * d;
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) q += __shfl_xor(q, off);
    if ((threadIdx.x & 63) == 0) red[1][threadIdx.x >> 6] = q;
    __syncthreads();
    if (threadIdx.x == 0) {
        feature[j] = (float)mu;
        feature[512 + j] = (float)((red[1][0] + red[1][1] + red[1][2] + red[1][3]) / (n - 1));
    }
}

// ------------------------------------------------------------------------------------------------ host side
struct Bump {  // workspace carving
    char* base;
    size_t off, cap;
    bool ok = true;
    float* take(size_t floats) {
        const size_t bytes = (floats * sizeof(float) + 255) & ~(size_t)255;
        if (off + bytes > cap) {
            ok = false;
            return reinterpret_cast<float*>(base);
        }
        float* p = reinterpret_cast<float*>(base + off);
        off += bytes;
        return p;
    }
};

}  // namespace tgtc

using namespace tgtc;

struct tgtc_style2d {
    int precision;
    std::vector<float*> allocs;
    std::map<std::string, const float*> tr, emb, dec, vgg;  // device pointers by reference key name
    // every uploaded parameter group also as fp16 hi / lo halves (GEMM B operands skip the conversion): for a float pointer
    // p inside [base, base + n) the halves are hi16 + (p - base), lo16 + (p - base)
    struct Pre { const float* base; size_t n; const tgtc::half_t* hi16; const tgtc::half_t* lo16; };
    std::vector<Pre> pre;
    std::vector<void*> allocs16;
};

namespace tgtc {

// Tile choice by measurement (profiles/r2_kernel_variants.md section 8): these GEMMs are small (a [2500,512] projection is
// 1.3 GFLOP) and latency-bound, so they want workgroups, not big tiles.  64x64 tiles beat 128x128 everywhere, the 400x400
// VGG convolutions included; when even 64x64 leaves fewer than ~1.5 workgroups per CU (the 320-workgroup projections),
// 32x32 tiles quadruple the grid.  The k-major loader (attention's V operand) only exists at 128x128.
template <class AL, bool KM>
static int launch_gemm(const tgtc_style2d* h, AL al, DenseRows bl, GemmOut out, int M, int N, int K, int batch,
                       hipStream_t st) {
    if (M <= 0 || N <= 0) return TGTC_OK;
    const bool split = h->precision != TGTC_PREC_FP16;
    if constexpr (KM) {
        dim3 grid((M + 127) / 128, (N + 127) / 128, batch);
        if (split) gemm_kernel<AL, true, true, 4><<<grid, 256, 0, st>>>(al, bl, out, M, N, K);
        else gemm_kernel<AL, false, true, 4><<<grid, 256, 0, st>>>(al, bl, out, M, N, K);
    } else {
        // weights of this handle: take their pre-split halves (8-byte aligned quads need K, ld and the offset multiples of 4)
        bool pre = bl.h16 != nullptr && K % 4 == 0 && bl.ld % 4 == 0 && bl.batch_stride % 4 == 0;   // halves handed in by the caller
        if (!pre) bl.h16 = bl.l16 = nullptr;
        if constexpr (std::is_same<AL, DenseRows>::value || std::is_same<AL, ConvNHWC>::value) {
            if (!pre)
            for (const auto& r : h->pre)
                if (bl.p >= r.base && bl.p < r.base + r.n && K % 4 == 0 && bl.ld % 4 == 0 && bl.batch_stride % 4 == 0 && (bl.p - r.base) % 4 == 0) {
                    bl.h16 = r.hi16 + (bl.p - r.base), bl.l16 = r.lo16 + (bl.p - r.base), pre = true;
                    break;
                }
        }
        const long long mid = (long long)((M + 63) / 64) * ((N + 63) / 64) * batch;
        auto go = [&](auto wt_, auto pre_) {
            constexpr int WT = decltype(wt_)::value;
            constexpr bool PRE = decltype(pre_)::value;
            dim3 grid((M + 32 * WT - 1) / (32 * WT), (N + 32 * WT - 1) / (32 * WT), batch);
            if (split) gemm_kernel<AL, true, false, WT, PRE><<<grid, 256, 0, st>>>(al, bl, out, M, N, K);
            else gemm_kernel<AL, false, false, WT, PRE><<<grid, 256, 0, st>>>(al, bl, out, M, N, K);
        };
        if constexpr (std::is_same<AL, DenseRows>::value) {
            // both operands pre-split (the training side's backward GEMMs): nothing converts in the loop
            if (pre && al.h16 && K % 4 == 0 && al.ld % 4 == 0 && al.batch_stride % 4 == 0) {
                const dim3 grid1((M + 31) / 32, (N + 31) / 32, batch), grid2((M + 63) / 64, (N + 63) / 64, batch);
                if (mid < 400) {
                    if (split) gemm_kernel<AL, true, false, 1, true, true><<<grid1, 256, 0, st>>>(al, bl, out, M, N, K);
                    else gemm_kernel<AL, false, false, 1, true, true><<<grid1, 256, 0, st>>>(al, bl, out, M, N, K);
                } else {
                    if (split) gemm_kernel<AL, true, false, 2, true, true><<<grid2, 256, 0, st>>>(al, bl, out, M, N, K);
                    else gemm_kernel<AL, false, false, 2, true, true><<<grid2, 256, 0, st>>>(al, bl, out, M, N, K);
                }
                TGTC_LAUNCH_CHECK();
                return TGTC_OK;
            }
        }
        // (SegRows: the style trainer's layers take the tile and the B path of the same layer on DenseRows)
        if constexpr (std::is_same<AL, DenseRows>::value || std::is_same<AL, ConvNHWC>::value || std::is_same<AL, SegRows>::value) {
            if (pre) {
                if (mid < 400) go(ic<1>{}, std::true_type{});
                else go(ic<2>{}, std::true_type{});
            } else {
                if (mid < 400) go(ic<1>{}, std::false_type{});
                else go(ic<2>{}, std::false_type{});
            }
        } else {
            if (mid < 400) go(ic<1>{}, std::false_type{});
            else go(ic<2>{}, std::false_type{});
        }
    }
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

// y[M,N] (ld ldy) = act(x[M,K] (ld ldx) * W[N,K]^T + b)
static int linear(const tgtc_style2d* h, const float* x, long long ldx, int M, int K, const float* W, const float* b,
                  int N, float* y, long long ldy, const float* res, int relu, hipStream_t st) {
    DenseRows al{x, ldx, 0, M, K}, bl{W, K, 0, N, K};
    GemmOut out{y, ldy, 1, 0, b, res, 1.0f, relu};
    return launch_gemm<DenseRows, false>(h, al, bl, out, M, N, K, 1, st);
}

// out = LayerNorm(a + b); `lda` = row stride of a (the residual may be a 512-column slice of a wider projection)
static int layernorm(const float* a, const float* b, const float* w, const float* bias, float* out, int rows,
                     hipStream_t st, long long lda = 512) {
    layernorm512_kernel<<<(rows + 3) / 4, 256, 0, st>>>(a, b, w, bias, out, rows, lda);
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

static const float* need(const std::map<std::string, const float*>& m, const std::string& k) {
    auto it = m.find(k);
    return it == m.end() ? nullptr : it->second;
}

#define TGTC_TRY(expr)          \
    do {                        \
        int rc__ = (expr);      \
        if (rc__) return rc__;  \
    } while (0)

// nn.MultiheadAttention forward (batch 1): q_in [L,512] ld ldq, k_in / v_in [S,512] -> out [L,512]
static int mha(const tgtc_style2d* h, const std::string& p, const float* q_in, long long ldq, int L, const float* k_in,
               long long ldk, const float* v_in, long long ldv, int S, Bump& ws, float* out, hipStream_t st) {
    const float* w = need(h->tr, p + "in_proj_weight");
    const float* b = need(h->tr, p + "in_proj_bias");
    const float* ow = need(h->tr, p + "out_proj.weight");
    const float* ob = need(h->tr, p + "out_proj.bias");
    if (!w || !b || !ow || !ob) return fail(TGTC_ERR_ARG, "style2d: missing attention parameters '%s*'", p.c_str());
    const int S_pad = (S + 63) / 64 * 64;
    float* Q = ws.take((size_t)L * 512);
    float* Kp = ws.take((size_t)S * 512);
    float* V = ws.take((size_t)S * 512);
    float* O = ws.take((size_t)L * 512);
    // fp16 hi / lo operands of the attention kernel (two halves per float slot)
    half_t* qh = reinterpret_cast<half_t*>(ws.take((size_t)L * 512));
    half_t* ql = qh + (size_t)L * 512;
    half_t* kh = reinterpret_cast<half_t*>(ws.take((size_t)S_pad * 512));
    half_t* kl = kh + (size_t)S_pad * 512;
    half_t* vth = reinterpret_cast<half_t*>(ws.take((size_t)S_pad * 512));
    half_t* vtl = vth + (size_t)S_pad * 512;
    if (!ws.ok) return fail(TGTC_ERR_ARG, "style2d: workspace too small for attention (L=%d, S=%d)", L, S);
    // in_proj: three [*,512] x [512,512] products.  Alone each is 20 x 4 tiles of 128 on 256 CUs; batch what can be:
    long long ldK = 512, ldV = 512;
    auto batched = [&](const float* a, long long lda, long long a_stride, int rows, int first, int count, float* y) {
        DenseRows al{a, lda, a_stride, rows, 512}, bl{w + (size_t)first * 512 * 512, 512, 512 * 512, 512, 512};
        GemmOut o{y, 512, 1, (long long)rows * 512, b + first * 512, nullptr, 1.0f, 0};
        o.bias_batch_stride = 512;
        return launch_gemm<DenseRows, false>(h, al, bl, o, rows, 512, 512, count, st);
    };
    const bool same_ld = ldq == ldk && ldk == ldv, step_qk = L == S && ldq == ldk;
    if (L == S && same_ld && k_in - q_in == v_in - k_in && Kp == Q + (size_t)L * 512 && V == Kp + (size_t)S * 512) {
        TGTC_TRY(batched(q_in, ldq, k_in - q_in, L, 0, 3, Q));                     // encoder without pos: q | k | v slices
    } else if (k_in == v_in && ldk == ldv) {
        TGTC_TRY(linear(h, q_in, ldq, L, 512, w, b, 512, Q, 512, nullptr, 0, st));  // decoder: k and v share the memory
        float* KV = ws.take((size_t)S * 1024);
        if (!ws.ok) return fail(TGTC_ERR_ARG, "style2d: workspace too small for attention (L=%d, S=%d)", L, S);
        TGTC_TRY(linear(h, k_in, ldk, S, 512, w + 512 * 512, b + 512, 1024, KV, 1024, nullptr, 0, st));
        Kp = KV, V = KV + 512, ldK = ldV = 1024;
    } else if (step_qk && Kp == Q + (size_t)L * 512) {
        TGTC_TRY(batched(q_in, ldq, k_in - q_in, L, 0, 2, Q));                     // encoder with pos: q | k slices, v = src
        TGTC_TRY(linear(h, v_in, ldv, S, 512, w + 2 * 512 * 512, b + 1024, 512, V, 512, nullptr, 0, st));
    } else {
        TGTC_TRY(linear(h, q_in, ldq, L, 512, w, b, 512, Q, 512, nullptr, 0, st));
        TGTC_TRY(linear(h, k_in, ldk, S, 512, w + 512 * 512, b + 512, 512, Kp, 512, nullptr, 0, st));
        TGTC_TRY(linear(h, v_in, ldv, S, 512, w + 2 * 512 * 512, b + 1024, 512, V, 512, nullptr, 0, st));
    }
    {
        const long long total = (long long)L * 512 + 2LL * S_pad * 512;
        attn_prep_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(Q, 512, L, Kp, ldK, V, ldV, S, S_pad, qh, ql, kh, kl,
                                                                             vth, vtl);
        TGTC_LAUNCH_CHECK();
        // key splits: enough of them for ~4 query-waves per SIMD (1 024 SIMDs), at most one per key tile
        // (measured at 2 500 tokens, whole 2-D pass: 1 split 6.00 ms, 2: 5.52, 4: 5.43, 8: 5.40)
        const long long waves = (long long)((L + 15) / 16) * 8;
        int nsplit = (int)std::min<long long>(8, (4096 + waves - 1) / waves);
        nsplit = std::max(1, std::min(nsplit, S_pad / 64));
        float *part_o = nullptr, *part_ml = nullptr;
        if (nsplit > 1) {
            part_o = ws.take((size_t)nsplit * L * 512);
            part_ml = ws.take((size_t)nsplit * L * 16);
            if (!ws.ok) return fail(TGTC_ERR_ARG, "style2d: workspace too small for attention (L=%d, S=%d)", L, S);
        }
        const dim3 grid((L + 63) / 64, 8, nsplit);
        if (h->precision == TGTC_PREC_FP16)
            attn_kernel<false><<<grid, 256, 0, st>>>(qh, ql, kh, kl, vth, vtl, L, S, S_pad, O, part_o, part_ml);
        else
            attn_kernel<true><<<grid, 256, 0, st>>>(qh, ql, kh, kl, vth, vtl, L, S, S_pad, O, part_o, part_ml);
        TGTC_LAUNCH_CHECK();
        if (nsplit > 1) {
            attn_combine_kernel<<<(unsigned)(((long long)L * 128 + 255) / 256), 256, 0, st>>>(part_o, part_ml, L, nsplit, O);
            TGTC_LAUNCH_CHECK();
        }
    }
    return linear(h, O, 512, L, 512, ow, ob, 512, out, 512, nullptr, 0, st);
}

static int ffn_norm(const tgtc_style2d* h, const std::string& p, const std::string& norm, const float* x, int rows,
                    Bump& ws, float* out, hipStream_t st) {
    const float *w1 = need(h->tr, p + "linear1.weight"), *b1 = need(h->tr, p + "linear1.bias");
    const float *w2 = need(h->tr, p + "linear2.weight"), *b2 = need(h->tr, p + "linear2.bias");
    const float *nw = need(h->tr, p + norm + ".weight"), *nb = need(h->tr, p + norm + ".bias");
    if (!w1 || !b1 || !w2 || !b2 || !nw || !nb) return fail(TGTC_ERR_ARG, "style2d: missing FFN parameters '%s*'", p.c_str());
    float* hid = ws.take((size_t)rows * 2048);
    float* y = ws.take((size_t)rows * 512);
    if (!ws.ok) return fail(TGTC_ERR_ARG, "style2d: workspace too small for the feed-forward block");
    TGTC_TRY(linear(h, x, 512, rows, 512, w1, b1, 2048, hid, 2048, nullptr, 1, st));
    TGTC_TRY(linear(h, hid, 2048, rows, 2048, w2, b2, 512, y, 512, nullptr, 0, st));
    return layernorm(x, y, nw, nb, out, rows, st);
}

// transformer.py:167-184
static int encoder_layer(const tgtc_style2d* h, const std::string& p, const float* src, int S, bool has_pos, Bump ws,
                         float* out, hipStream_t st) {
    const float* n1w = need(h->tr, p + "norm1.weight");
    const float* n1b = need(h->tr, p + "norm1.bias");
    if (!n1w || !n1b) return fail(TGTC_ERR_ARG, "style2d: missing '%snorm1.*'", p.c_str());
    const int width = has_pos ? 1024 : 1536;
    const float* pw = need(h->tr, p + (has_pos ? "qk.weight" : "qkv.weight"));
    if (!pw) return fail(TGTC_ERR_ARG, "style2d: missing '%sqk(v).weight'", p.c_str());
    float* proj = ws.take((size_t)S * width);
    float* attn = ws.take((size_t)S * 512);
    float* x1 = ws.take((size_t)S * 512);
    if (!ws.ok) return fail(TGTC_ERR_ARG, "style2d: workspace too small for an encoder layer (S=%d)", S);
    TGTC_TRY(linear(h, src, 512, S, 512, pw, nullptr, width, proj, width, nullptr, 0, st));
    // without pos the value AND the residual are the third chunk of the projection (transformer.py:173-174)
    const float* val = has_pos ? src : proj + 1024;
    const long long ldv = has_pos ? 512 : width;
    TGTC_TRY(mha(h, p + "self_attn.", proj, width, S, proj + 512, width, val, ldv, S, ws, attn, st));
    if (has_pos) {
        TGTC_TRY(layernorm(src, attn, n1w, n1b, x1, S, st));
    } else {
        // the residual operand is the third 512-column chunk of the projection (row stride 1536): read in place
        TGTC_TRY(layernorm(val, attn, n1w, n1b, x1, S, st, width));
    }
    return ffn_norm(h, p, "norm2", x1, S, ws, out, st);
}

// transformer.py:236-263 with pos = None
static int decoder_layer(const tgtc_style2d* h, const std::string& p, const float* tgt, int L, const float* memory,
                         int S, const float* qpos, Bump ws, float* out, hipStream_t st) {
    const float *n1w = need(h->tr, p + "norm1.weight"), *n1b = need(h->tr, p + "norm1.bias");
    const float *n2w = need(h->tr, p + "norm2.weight"), *n2b = need(h->tr, p + "norm2.bias");
    if (!n1w || !n1b || !n2w || !n2b) return fail(TGTC_ERR_ARG, "style2d: missing '%snorm*'", p.c_str());
    float* q = ws.take((size_t)L * 512);
    float* a = ws.take((size_t)L * 512);
    float* t1 = ws.take((size_t)L * 512);
    float* t2 = ws.take((size_t)L * 512);
    if (!ws.ok) return fail(TGTC_ERR_ARG, "style2d: workspace too small for a decoder layer (L=%d)", L);
    const long long n = (long long)L * 512;
    add_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(tgt, qpos, q, n);
    TGTC_LAUNCH_CHECK();
    {
        Bump inner = ws;
        TGTC_TRY(mha(h, p + "self_attn.", q, 512, L, memory, 512, memory, 512, S, inner, a, st));
    }
    TGTC_TRY(layernorm(tgt, a, n1w, n1b, t1, L, st));
    add_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(t1, qpos, q, n);
    TGTC_LAUNCH_CHECK();
    {
        Bump inner = ws;
        TGTC_TRY(mha(h, p + "multihead_attn.", q, 512, L, memory, 512, memory, 512, S, inner, a, st));
    }
    TGTC_TRY(layernorm(t1, a, n2w, n2b, t2, L, st));
    return ffn_norm(h, p, "norm3", t2, L, ws, out, st);
}

static size_t layer_ws_floats(size_t L, size_t S) {
    // generous upper bound for one encoder / decoder layer incl. attention scratch (256-byte rounding included)
    return 1536 * S + 24 * 512 * (L + S + 64) + 2048 * (L + S) + 64 * 64;
}

static int conv3x3(const tgtc_style2d* h, const float* w, const float* b, const float* in, int Hs, int Ws, int up,
                   int Cin, int Cout, int relu, float* out, long long sm, long long sn, hipStream_t st) {
    int logC = 0;
    while ((1 << logC) < Cin) ++logC;
    if ((1 << logC) != Cin || Cin < 32) return fail(TGTC_ERR_UNSUPPORTED, "conv3x3: C_in=%d must be a power of two >= 32", Cin);
    const int H = up ? 2 * Hs : Hs, W = up ? 2 * Ws : Ws, M = H * W, K = 9 * Cin;
    ConvNHWC al{in, 0, H, W, Hs, Ws, Cin, logC, up, M, K};
    DenseRows bl{w, K, 0, Cout, K};
    GemmOut o{out, sm, sn, 0, b, nullptr, 1.0f, relu};
    return launch_gemm<ConvNHWC, false>(h, al, bl, o, M, Cout, K, 1, st);
}

}  // namespace tgtc

// ------------------------------------------------------------------------------------------------ C ABI
static int upload_group(tgtc_style2d* h, const tgtc_named_tensor* t, int n, std::map<std::string, const float*>& dst,
                        bool repack_conv3) {
    if (!t || n <= 0) return TGTC_OK;
    size_t total = 0;
    for (int i = 0; i < n; ++i) {
        if (!t[i].name || !t[i].data || t[i].numel <= 0) return fail(TGTC_ERR_ARG, "style2d_create: bad tensor #%d", i);
        total += ((size_t)t[i].numel + 63) & ~(size_t)63;
    }
    std::vector<float> host(total, 0.0f);
    std::vector<size_t> offs(n);
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        offs[i] = off;
        const std::string name = t[i].name;
        const bool is_w = name.size() > 7 && name.compare(name.size() - 7, 7, ".weight") == 0;
        // 3x3 conv weights [N][C][3][3] -> [N][tap][C] (k = tap*C + c, the implicit-GEMM k order)
        if (repack_conv3 && is_w && t[i].numel % 9 == 0 && name != "0.weight") {
            // identify (N, C): conv weights of the decoder / vgg are [N][C][3][3] with known N from the bias
            // tensor that follows; derive C from numel once N is known
            long long N = -1;
            const std::string bname = name.substr(0, name.size() - 7) + ".bias";
            for (int j = 0; j < n; ++j)
                if (bname == t[j].name) N = t[j].numel;
            if (N <= 0 || t[i].numel % (9 * N)) return fail(TGTC_ERR_ARG, "style2d_create: cannot shape conv '%s'", t[i].name);
            const long long C = t[i].numel / (9 * N);
            for (long long nn = 0; nn < N; ++nn)
                for (long long c = 0; c < C; ++c)
                    for (int tap = 0; tap < 9; ++tap)
                        host[off + (nn * 9 + tap) * C + c] = t[i].data[(nn * C + c) * 9 + tap];
        } else {
            std::memcpy(host.data() + off, t[i].data, (size_t)t[i].numel * sizeof(float));
        }
        off += ((size_t)t[i].numel + 63) & ~(size_t)63;
    }
    float* dev = nullptr;
    TGTC_HIP_CHECK(hipMalloc((void**)&dev, total * sizeof(float)));
    h->allocs.push_back(dev);
    TGTC_HIP_CHECK(hipMemcpy(dev, host.data(), total * sizeof(float), hipMemcpyHostToDevice));
    for (int i = 0; i < n; ++i) dst[t[i].name] = dev + offs[i];
    // fp16 hi / lo copies of the whole group (weights are what the GEMMs read as B operands)
    std::vector<half_t> h16(2 * total);
    for (size_t i = 0; i < total; ++i) {
        const half_t hi = (half_t)host[i];
        h16[i] = hi, h16[total + i] = (half_t)(host[i] - (float)hi);
    }
    half_t* dev16 = nullptr;
    TGTC_HIP_CHECK(hipMalloc((void**)&dev16, 2 * total * sizeof(half_t)));
    h->allocs16.push_back(dev16);
    TGTC_HIP_CHECK(hipMemcpy(dev16, h16.data(), 2 * total * sizeof(half_t), hipMemcpyHostToDevice));
    h->pre.push_back({dev, total, dev16, dev16 + total});
    return TGTC_OK;
}

extern "C" int tgtc_s2d_create(const tgtc_named_tensor* transformer, int n_transformer,
                               const tgtc_named_tensor* embedding, int n_embedding, const tgtc_named_tensor* decoder,
                               int n_decoder, const tgtc_named_tensor* vgg, int n_vgg, int precision,
                               tgtc_style2d** out) {
    TGTC_REQUIRE(out, "style2d_create: null output");
    TGTC_REQUIRE(precision == TGTC_PREC_FP16 || precision == TGTC_PREC_FP16X3, "style2d_create: unknown precision %d", precision);
    tgtc_style2d* h = new tgtc_style2d();
    h->precision = precision;
    int rc = upload_group(h, transformer, n_transformer, h->tr, false);
    if (!rc) rc = upload_group(h, embedding, n_embedding, h->emb, false);
    if (!rc) rc = upload_group(h, decoder, n_decoder, h->dec, true);
    if (!rc) rc = upload_group(h, vgg, n_vgg, h->vgg, true);
    if (rc) {
        tgtc_s2d_destroy(h);
        return rc;
    }
    *out = h;
    return TGTC_OK;
}

extern "C" int tgtc_s2d_destroy(tgtc_style2d* h) {
    if (!h) return TGTC_OK;
    for (float* p : h->allocs) (void)hipFree(p);
    for (void* p : h->allocs16) (void)hipFree(p);
    delete h;
    return TGTC_OK;
}

extern "C" int tgtc_s2d_patch_embed(const tgtc_style2d* h, const float* img, int H, int W, float* tokens,
                                    void* stream) {
    TGTC_REQUIRE(h && H >= 8 && W >= 8, "patch_embed: bad argument");
    TGTC_REQUIRE(img && tokens, "patch_embed: null pointer");
    const float *w = need(h->emb, "proj.weight"), *b = need(h->emb, "proj.bias");
    if (!w || !b) return fail(TGTC_ERR_ARG, "patch_embed: embedding parameters were not given to tgtc_s2d_create");
    const int ht = H / 8, wt = W / 8, M = ht * wt;
    PatchRows al{img, 0, H, W, wt, M, 192};
    DenseRows bl{w, 192, 0, 512, 192};
    GemmOut o{tokens, 512, 1, 0, b, nullptr, 1.0f, 0};
    return launch_gemm<PatchRows, false>(h, al, bl, o, M, 512, 192, 1, as_stream(stream));
}

extern "C" size_t tgtc_s2d_transformer_workspace_bytes(int ns, int nc) {
    if (ns <= 0 || nc <= 0) return 0;
    const size_t big = (size_t)(ns > nc ? ns : nc);
    return (layer_ws_floats(big, big) + 4 * 512 * big) * sizeof(float);
}

extern "C" int tgtc_s2d_mha(const tgtc_style2d* h, const char* prefix, const float* query, int L, const float* key,
                            const float* value, int S, void* workspace, size_t workspace_bytes, float* out,
                            void* stream) {
    TGTC_REQUIRE(h && prefix && L > 0 && S > 0 && query && key && value && workspace && out, "mha: bad argument");
    Bump ws{static_cast<char*>(workspace), 0, workspace_bytes};
    return mha(h, prefix, query, 512, L, key, 512, value, 512, S, ws, out, as_stream(stream));
}

extern "C" int tgtc_s2d_encoder_layer(const tgtc_style2d* h, const char* prefix, const float* src, int S, int has_pos,
                                      void* workspace, size_t workspace_bytes, float* out, void* stream) {
    TGTC_REQUIRE(h && prefix && S > 0 && src && workspace && out, "encoder_layer: bad argument");
    Bump ws{static_cast<char*>(workspace), 0, workspace_bytes};
    return encoder_layer(h, prefix, src, S, has_pos != 0, ws, out, as_stream(stream));
}

extern "C" int tgtc_s2d_decoder_layer(const tgtc_style2d* h, const char* prefix, const float* tgt, int L,
                                      const float* memory, int S, const float* query_pos, void* workspace,
                                      size_t workspace_bytes, float* out, void* stream) {
    TGTC_REQUIRE(h && prefix && L > 0 && S > 0 && tgt && memory && query_pos && workspace && out, "decoder_layer: bad argument");
    Bump ws{static_cast<char*>(workspace), 0, workspace_bytes};
    return decoder_layer(h, prefix, tgt, L, memory, S, query_pos, ws, out, as_stream(stream));
}

extern "C" int tgtc_s2d_transformer_forward(const tgtc_style2d* h, const float* style_tokens, int ns,
                                            const float* content_tokens, int nc, void* workspace,
                                            size_t workspace_bytes, float* hs, void* stream) {
    TGTC_REQUIRE(h && ns > 0 && nc > 0 && style_tokens && content_tokens && workspace && hs, "transformer_forward: bad argument");
    TGTC_REQUIRE(workspace_bytes >= tgtc_s2d_transformer_workspace_bytes(ns, nc), "transformer_forward: workspace too small");
    hipStream_t st = as_stream(stream);
    Bump ws{static_cast<char*>(workspace), 0, workspace_bytes};
    float* s[2] = {ws.take((size_t)ns * 512), ws.take((size_t)ns * 512)};
    float* c[2] = {ws.take((size_t)nc * 512), ws.take((size_t)nc * 512)};
    const float* cur = style_tokens;
    for (int i = 0; i < 3; ++i) {  // transformer.py:62
        TGTC_TRY(encoder_layer(h, "encoder_s.layers." + std::to_string(i) + ".", cur, ns, false, ws, s[i & 1], st));
        cur = s[i & 1];
    }
    const float* style_enc = cur;
    cur = content_tokens;
    for (int i = 0; i < 3; ++i) {  // transformer.py:63 (pos = content embedding is only a switch, transformer.py:172-176)
        TGTC_TRY(encoder_layer(h, "encoder_c.layers." + std::to_string(i) + ".", cur, nc, true, ws, c[i & 1], st));
        cur = c[i & 1];
    }
    // decoder: tgt = encoded content, memory = encoded style, query_pos = content embedding (transformer.py:64-65)
    const float* tgt = cur;             // c[0] after three layers
    float* pp[2] = {c[1], c[0]};        // ping-pong; layer 0 reads c[0] writes c[1], layer 1 reads c[1] writes c[0], ...
    for (int i = 0; i < 3; ++i) {
        TGTC_TRY(decoder_layer(h, "decoder.layers." + std::to_string(i) + ".", tgt, nc, style_enc, ns, content_tokens,
                               ws, pp[i & 1], st));
        tgt = pp[i & 1];
    }
    const float *nw = need(h->tr, "decoder.norm.weight"), *nb = need(h->tr, "decoder.norm.bias");
    if (!nw || !nb) return fail(TGTC_ERR_ARG, "transformer_forward: missing decoder.norm.*");
    return layernorm(tgt, nullptr, nw, nb, hs, nc, st);  // transformer.py:131-132
}

// ---- CNN decoder (tctrans.py:36-66)
extern "C" size_t tgtc_s2d_decode_workspace_bytes(int h, int w) {
    if (h <= 0 || w <= 0) return 0;
    // largest pair of live maps: [8h*8w, 64] twice
    return 2 * ((size_t)64 * h * w * 64 * sizeof(float) + 256);
}

extern "C" int tgtc_s2d_cnn_decode(const tgtc_style2d* hd, const float* tokens, int h, int w, void* workspace,
                                   size_t workspace_bytes, float* image, void* stream) {
    TGTC_REQUIRE(hd && h > 0 && w > 0 && tokens && workspace && image, "cnn_decode: bad argument");
    // ReflectionPad(1) mirrors row -1 onto row 1: a map one token high or wide has no such row (PyTorch refuses it too)
    TGTC_REQUIRE(h >= 2 && w >= 2, "cnn_decode: %d x %d tokens, reflection padding needs h >= 2 and w >= 2", h, w);
    TGTC_REQUIRE(workspace_bytes >= tgtc_s2d_decode_workspace_bytes(h, w), "cnn_decode: workspace too small");
    hipStream_t st = as_stream(stream);
    const size_t half = workspace_bytes / 2 & ~(size_t)255;
    float* buf[2] = {static_cast<float*>(workspace), reinterpret_cast<float*>(static_cast<char*>(workspace) + half)};
    struct L { int idx, cin, cout, relu, up_before; };
    static const L layers[9] = {{1, 512, 256, 1, 0},  {5, 256, 256, 1, 1},  {8, 256, 256, 1, 0}, {11, 256, 256, 1, 0},
                                {14, 256, 128, 1, 0}, {18, 128, 128, 1, 1}, {21, 128, 64, 1, 0}, {25, 64, 64, 1, 1},
                                {28, 64, 3, 0, 0}};
    const float* cur = tokens;
    int Hs = h, Ws = w;
    for (int i = 0; i < 9; ++i) {
        const L& l = layers[i];
        const float* wt = need(hd->dec, std::to_string(l.idx) + ".weight");
        const float* bs = need(hd->dec, std::to_string(l.idx) + ".bias");
        if (!wt || !bs) return fail(TGTC_ERR_ARG, "cnn_decode: decoder parameter %d.* missing", l.idx);
        const int H = l.up_before ? 2 * Hs : Hs, W = l.up_before ? 2 * Ws : Ws;
        const bool last = i == 8;
        float* dst = last ? image : buf[i & 1];
        // last conv writes NCHW [3, H*W]; the others token-major [H*W, C]
        TGTC_TRY(conv3x3(hd, wt, bs, cur, Hs, Ws, l.up_before, l.cin, l.cout, l.relu, dst, last ? 1 : l.cout,
                         last ? (long long)H * W : 1, st));
        cur = dst, Hs = H, Ws = W;
    }
    return TGTC_OK;
}

// ---- VGG-19 prefix (tctrans.py:68-99, :161-166)
extern "C" size_t tgtc_s2d_vgg_workspace_bytes(int H, int W) {
    if (H <= 0 || W <= 0) return 0;
    return 3 * ((size_t)H * W * 64 * sizeof(float) + 256);
}

extern "C" int tgtc_s2d_vgg_encode(const tgtc_style2d* h, const float* img, int H, int W, void* workspace,
                                   size_t workspace_bytes, float* relu1_1, float* relu2_1, float* relu3_1,
                                   float* relu4_1, void* stream) {
    TGTC_REQUIRE(h && H > 0 && W > 0 && img && workspace, "vgg_encode: bad argument");
    // every 3x3 convolution up to relu4_1 must see at least 2 rows and columns: ceil(ceil(ceil(H/2)/2)/2) >= 2
    TGTC_REQUIRE(H >= 9 && W >= 9, "vgg_encode: %d x %d image, reflection padding at relu4_1 needs H >= 9 and W >= 9", H, W);
    TGTC_REQUIRE(workspace_bytes >= tgtc_s2d_vgg_workspace_bytes(H, W), "vgg_encode: workspace too small");
    hipStream_t st = as_stream(stream);
    const size_t third = workspace_bytes / 3 & ~(size_t)255;
    float* buf[3];
    for (int i = 0; i < 3; ++i) buf[i] = reinterpret_cast<float*>(static_cast<char*>(workspace) + i * third);
    auto par = [&](int idx, const char* what) { return need(h->vgg, std::to_string(idx) + what); };
    for (int idx : {0, 2, 5, 9, 12, 16, 19, 22, 25, 29})
        if (!par(idx, ".weight") || !par(idx, ".bias")) return fail(TGTC_ERR_ARG, "vgg_encode: vgg parameter %d.* missing", idx);
    const int HW = H * W;
    {   // vgg.0: Conv2d(3,3,1x1) on the NCHW image -> NCHW scratch
        ConvSmall al{img, 0, 1, HW, H, W, 3, 1, HW, 3};
        DenseRows bl{par(0, ".weight"), 3, 0, 3, 3};
        GemmOut o{buf[0], 1, HW, 0, par(0, ".bias"), nullptr, 1.0f, 0};
        TGTC_TRY((launch_gemm<ConvSmall, false>(h, al, bl, o, HW, 3, 3, 1, st)));
    }
    {   // vgg.2: pad + Conv2d(3,64,3x3) + relu -> relu1_1, token-major [HW,64].
        // The 3x3 weights of this layer were repacked to [N][tap][c] like every other 3x3 conv.
        ConvSmall al{buf[0], 0, 1, HW, H, W, 3, 3, HW, 27};
        DenseRows bl{par(2, ".weight"), 27, 0, 64, 27};
        GemmOut o{buf[1], 64, 1, 0, par(2, ".bias"), nullptr, 1.0f, 1};
        TGTC_TRY((launch_gemm<ConvSmall, false>(h, al, bl, o, HW, 64, 27, 1, st)));
    }
    auto emit = [&](const float* tok, int n, int C, float* dst) -> int {
        if (!dst) return TGTC_OK;
        dim3 grid((C + 31) / 32, (n + 31) / 32);
        transpose_kernel<<<grid, 256, 0, st>>>(tok, n, C, dst);
        TGTC_LAUNCH_CHECK();
        return TGTC_OK;
    };
    auto pool = [&](const float* in, int Hh, int Ww, int C, float* out) -> int {
        const long long n = (long long)((Hh + 1) / 2) * ((Ww + 1) / 2) * C;
        maxpool2_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(in, Hh, Ww, C, out);
        TGTC_LAUNCH_CHECK();
        return TGTC_OK;
    };
    auto conv = [&](int idx, const float* in, int Hh, int Ww, int cin, int cout, float* out) -> int {
        return conv3x3(h, par(idx, ".weight"), par(idx, ".bias"), in, Hh, Ww, 0, cin, cout, 1, out, cout, 1, st);
    };
    TGTC_TRY(emit(buf[1], HW, 64, relu1_1));
    TGTC_TRY(conv(5, buf[1], H, W, 64, 64, buf[2]));                 // relu1_2
    int H2 = (H + 1) / 2, W2 = (W + 1) / 2;
    TGTC_TRY(pool(buf[2], H, W, 64, buf[0]));
    TGTC_TRY(conv(9, buf[0], H2, W2, 64, 128, buf[1]));              // relu2_1
    TGTC_TRY(emit(buf[1], H2 * W2, 128, relu2_1));
    TGTC_TRY(conv(12, buf[1], H2, W2, 128, 128, buf[2]));            // relu2_2
    int H3 = (H2 + 1) / 2, W3 = (W2 + 1) / 2;
    TGTC_TRY(pool(buf[2], H2, W2, 128, buf[0]));
    TGTC_TRY(conv(16, buf[0], H3, W3, 128, 256, buf[1]));            // relu3_1
    TGTC_TRY(emit(buf[1], H3 * W3, 256, relu3_1));
    TGTC_TRY(conv(19, buf[1], H3, W3, 256, 256, buf[2]));            // relu3_2
    TGTC_TRY(conv(22, buf[2], H3, W3, 256, 256, buf[0]));            // relu3_3
    TGTC_TRY(conv(25, buf[0], H3, W3, 256, 256, buf[1]));            // relu3_4
    int H4 = (H3 + 1) / 2, W4 = (W3 + 1) / 2;
    TGTC_TRY(pool(buf[1], H3, W3, 256, buf[2]));
    TGTC_TRY(conv(29, buf[2], H4, W4, 256, 512, buf[0]));            // relu4_1
    return emit(buf[0], H4 * W4, 512, relu4_1);
}

extern "C" int tgtc_s2d_linear(const float* x, int64_t M, int K, const float* W, const float* b, int N, int relu,
                               int precision, float* y, void* stream) {
    TGTC_REQUIRE(M >= 0 && M < 0x7fffffffLL && K > 0 && N > 0, "s2d_linear: bad shape");
    TGTC_REQUIRE(precision == TGTC_PREC_FP16 || precision == TGTC_PREC_FP16X3, "s2d_linear: unknown precision %d", precision);
    if (M == 0) return TGTC_OK;
    TGTC_REQUIRE(x && W && y, "s2d_linear: null pointer");
    tgtc_style2d h;
    h.precision = precision;
    return linear(&h, x, K, (int)M, K, W, b, N, y, N, nullptr, relu, as_stream(stream));
}

// The same layer with the weight also given as fp16 hi / lo halves (tgtc_s2d_split; K a multiple of 4), which the GEMM
// loads without converting: for callers that apply one weight to many batches (the training side re-splits after each
// optimiser step).
extern "C" int tgtc_s2d_split(const float* w, int64_t n, void* hi, void* lo, void* stream) {
    TGTC_REQUIRE(n >= 0, "s2d_split: bad size");
    if (n == 0) return TGTC_OK;
    TGTC_REQUIRE(w && hi && lo, "s2d_split: null pointer");
    split_kernel<<<(unsigned)((n + 255) / 256), 256, 0, as_stream(stream)>>>(w, n, static_cast<half_t*>(hi), static_cast<half_t*>(lo));
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

extern "C" int tgtc_s2d_linear_pre(const float* x, int64_t M, int K, const float* W, const void* W_hi, const void* W_lo,
                                   const float* b, int N, int relu, int precision, float* y, void* stream) {
    TGTC_REQUIRE(M >= 0 && M < 0x7fffffffLL && K > 0 && N > 0, "s2d_linear_pre: bad shape");
    TGTC_REQUIRE(precision == TGTC_PREC_FP16 || precision == TGTC_PREC_FP16X3, "s2d_linear_pre: unknown precision %d", precision);
    if (M == 0) return TGTC_OK;
    TGTC_REQUIRE(x && W && y, "s2d_linear_pre: null pointer");
    tgtc_style2d h;
    h.precision = precision;
    DenseRows al{x, K, 0, (int)M, K}, bl{W, K, 0, N, K};
    if (W_hi && W_lo && K % 4 == 0) bl.h16 = static_cast<const half_t*>(W_hi), bl.l16 = static_cast<const half_t*>(W_lo);
    GemmOut out{y, N, 1, 0, b, nullptr, 1.0f, relu};
    return launch_gemm<DenseRows, false>(&h, al, bl, out, (int)M, N, K, 1, as_stream(stream));
}

// split of the sample dimension for dW = dy^T . x: enough batches to fill the chip with 64x64 tiles, 32-aligned
static void backward_split(int64_t M, int K, int N, int& nsplit, int64_t& mc) {
    const long long tiles = (long long)((N + 63) / 64) * ((K + 63) / 64);
    nsplit = (int)std::max<long long>(1, std::min<long long>(std::min<long long>(64, (512 + tiles - 1) / tiles), (M + 1023) / 1024));
    mc = ((M + nsplit - 1) / nsplit + 31) / 32 * 32;
}

extern "C" size_t tgtc_s2d_linear_backward_workspace_bytes(int64_t M, int K, int N) {
    int nsplit;
    int64_t mc;
    backward_split(M, K, N, nsplit, mc);
    const size_t mpad = (size_t)nsplit * mc;
    return ((size_t)N * mpad + (size_t)K * mpad + (size_t)nsplit * N * K + (size_t)K * N + (size_t)M * N + (size_t)M + 8 * 64) * sizeof(float);
}

extern "C" int tgtc_s2d_linear_backward(const float* x, const float* dy, const float* relu_y, const float* W, int64_t M, int K,
                                        int N, int precision, void* workspace, size_t workspace_bytes, float* dx, float* dW,
                                        float* db, void* stream) {
    TGTC_REQUIRE(M >= 0 && M < 0x7fffffffLL && K > 0 && N > 0, "s2d_linear_backward: bad shape");
    TGTC_REQUIRE(precision == TGTC_PREC_FP16 || precision == TGTC_PREC_FP16X3, "s2d_linear_backward: unknown precision %d", precision);
    if (M == 0) return TGTC_OK;
    TGTC_REQUIRE(dy && (!dx || W) && (!dW || x), "s2d_linear_backward: null pointer");
    TGTC_REQUIRE(workspace && workspace_bytes >= tgtc_s2d_linear_backward_workspace_bytes(M, K, N), "s2d_linear_backward: workspace too small");
    hipStream_t st = as_stream(stream);
    tgtc_style2d h;
    h.precision = precision;
    int nsplit;
    int64_t mc;
    backward_split(M, K, N, nsplit, mc);
    const long long mpad = (long long)nsplit * mc, mn = (long long)M * N;
    Bump ws{static_cast<char*>(workspace), 0, workspace_bytes};
    float* sc = ws.take(64);                       // [0] bits of max |dy|, [1] scale s (a power of two), [2] 1/s
    float* dyT = ws.take((size_t)N * mpad);        // (s * dy)^T, zero padded to nsplit * mc samples
    float* xT = ws.take((size_t)K * mpad);
    float* part = ws.take((size_t)nsplit * N * K);
    float* WT = ws.take((size_t)K * N);
    float* dys = ws.take((size_t)mn);              // s_m * dy, row m at its own scale (dx only)
    float* row_inv = ws.take((size_t)M);           // 1 / s_m
    if (!ws.ok) return fail(TGTC_ERR_ARG, "s2d_linear_backward: workspace too small");
    TGTC_HIP_CHECK(hipMemsetAsync(sc, 0, 16, st));
    absmax_kernel<<<(unsigned)std::min<long long>(1024, (mn + 255) / 256), 256, 0, st>>>(dy, mn, reinterpret_cast<unsigned*>(sc), nullptr);   // ungated maximum >= gated one: as good a scale, half the bytes
    TGTC_LAUNCH_CHECK();
    grad_scale_kernel<<<1, 1, 0, st>>>(sc);
    TGTC_LAUNCH_CHECK();
    if (dx) {   // dx[M,K] = dy[M,N] . W[N,K]: a linear layer on s_m*dy whose weight is W^T [K,N], row m scaled back by 1/s_m
        half_t* dyh = reinterpret_cast<half_t*>(dys);      // s_m * gated dy as halves: [M,N] hi, then lo
        half_t* dyl = dyh + (size_t)mn;
        const bool a_pre = N % 4 == 0;
        row_scale_kernel<<<(unsigned)((M + 3) / 4), 256, 0, st>>>(dy, M, N, row_inv);
        TGTC_LAUNCH_CHECK();
        if (a_pre) scale_split_kernel<<<(unsigned)((mn + 255) / 256), 256, 0, st>>>(dy, mn, N, row_inv, relu_y, dyh, dyl);
        else scale_copy_kernel<<<(unsigned)((mn + 255) / 256), 256, 0, st>>>(dy, mn, N, row_inv, dys, relu_y);
        TGTC_LAUNCH_CHECK();
        const dim3 g((K + 31) / 32, (N + 31) / 32);
        transpose_ld_kernel<<<g, 256, 0, st>>>(W, N, K, WT, N);
        TGTC_LAUNCH_CHECK();
        DenseRows al{dys, N, 0, (int)M, N}, bl{WT, N, 0, K, N};
        if (a_pre) al.h16 = dyh, al.l16 = dyl;
        if (N % 4 == 0) {   // the weight as pre-split halves (no conversion in the GEMM loop)
            half_t* w16 = reinterpret_cast<half_t*>(part);   // (>= N*K floats; the dW partials come later on the stream)
            split_kernel<<<(unsigned)(((long long)K * N + 255) / 256), 256, 0, st>>>(WT, (long long)K * N, w16, w16 + (size_t)K * N);
            TGTC_LAUNCH_CHECK();
            bl.h16 = w16, bl.l16 = w16 + (size_t)K * N;
        }
        GemmOut out{dx, K, 1, 0, nullptr, nullptr, 1.0f, 0};
        out.row_alpha = row_inv;
        TGTC_TRY((launch_gemm<DenseRows, false>(&h, al, bl, out, (int)M, K, N, 1, st)));
    }
    half_t* dth = reinterpret_cast<half_t*>(dyT);      // (s * gated dy)^T as halves [N, mpad] each, zero padded
    half_t* dtl = dth + (size_t)N * mpad;
    if (dW || db) {
        if (mpad > M) {   // only the pad columns: the transpose writes the rest
            TGTC_HIP_CHECK(hipMemset2DAsync(dth + M, (size_t)mpad * sizeof(half_t), 0, (size_t)(mpad - M) * sizeof(half_t), N, st));
            TGTC_HIP_CHECK(hipMemset2DAsync(dtl + M, (size_t)mpad * sizeof(half_t), 0, (size_t)(mpad - M) * sizeof(half_t), N, st));
        }
        const dim3 g((N + 31) / 32, (unsigned)((M + 31) / 32));
        transpose_ld_half_kernel<<<g, 256, 0, st>>>(dy, M, N, dth, dtl, mpad, sc + 1, relu_y);
        TGTC_LAUNCH_CHECK();
    }
    if (dW) {   // dW[N,K] = sum over sample chunks of (s*dy)^T[N, chunk] . xT[K, chunk]^T, chunks as GEMM batches, times 1/s
        // x^T straight into fp16 hi / lo halves [K, mpad] each (the GEMM's pre-split B operand), pad columns cleared
        half_t* xh = reinterpret_cast<half_t*>(xT);
        half_t* xl = xh + (size_t)K * mpad;
        if (mpad > M) {
            TGTC_HIP_CHECK(hipMemset2DAsync(xh + M, (size_t)mpad * sizeof(half_t), 0, (size_t)(mpad - M) * sizeof(half_t), K, st));
            TGTC_HIP_CHECK(hipMemset2DAsync(xl + M, (size_t)mpad * sizeof(half_t), 0, (size_t)(mpad - M) * sizeof(half_t), K, st));
        }
        const dim3 g((K + 31) / 32, (unsigned)((M + 31) / 32));
        transpose_ld_half_kernel<<<g, 256, 0, st>>>(x, M, K, xh, xl, mpad);
        TGTC_LAUNCH_CHECK();
        DenseRows al{dyT, mpad, mc, N, (int)mc}, bl{xT, mpad, mc, K, (int)mc};
        al.h16 = dth, al.l16 = dtl;
        bl.h16 = xh, bl.l16 = xl;
        GemmOut out{nsplit > 1 ? part : dW, K, 1, (long long)N * K, nullptr, nullptr, 1.0f, 0};
        out.alpha_dev = sc + 2;
        TGTC_TRY((launch_gemm<DenseRows, false>(&h, al, bl, out, N, K, (int)mc, nsplit, st)));
        if (nsplit > 1) {
            const long long n = (long long)N * K;
            sum_partials_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(part, nsplit, n, dW);
            TGTC_LAUNCH_CHECK();
        }
    }
    if (db) {   // column sums of dy = row sums of its transpose (scaled by s when dW shares the buffer)
        TGTC_HIP_CHECK(hipMemsetAsync(db, 0, (size_t)N * sizeof(float), st));
        rowsum_kernel<<<dim3(N, nsplit), 256, 0, st>>>(dth, dtl, M, mpad, mc, db, sc + 2);
        TGTC_LAUNCH_CHECK();
    }
    return TGTC_OK;
}

// ------------------------------------------------------------------------------------------------ style trainer
// include/tgtc_train.h: the 13 linears of the two style MLPs as a chain of the per-layer GEMMs above.  Forward: one GEMM per
// layer on a SegRows A operand.  Backward, per layer from the head down: the scales of tgtc_s2d_linear_backward, dx for the
// hidden columns only (a row sub-block of W^T), the ray-summed gradient times the latent columns, dW from the transposed
// gradient and the transposed segments, db.
namespace tgtc {

enum ChainSrc { SRC_X, SRC_REMAP, SRC_LAT, SRC_H };   // SRC_H: the previous layer's output plane
struct ChainLayer {
    int K, N, relu, nseg, src[4];
    int h_col, lat_col;   // first column of the hidden / latent segment in the weight (h_col -1: no hidden input)
};
constexpr int kChainLayers = 13, kChainPlanes = 12, kChainConcat = 5, kChainWRows = 288;   // W^T rows kept: 256 hidden + 32 latent
#define TGTC_CHAIN_HL {288, 256, 1, 2, {SRC_H, SRC_LAT, 0, 0}, 0, 256}
#define TGTC_CHAIN_HLX {351, 256, 1, 3, {SRC_H, SRC_LAT, SRC_X, 0}, 0, 256}
static const ChainLayer kChain[kChainLayers] = {
    {95, 256, 1, 2, {SRC_X, SRC_LAT, 0, 0}, -1, 63}, TGTC_CHAIN_HL, TGTC_CHAIN_HL, TGTC_CHAIN_HL, TGTC_CHAIN_HLX,        // concat
    {607, 256, 1, 4, {SRC_REMAP, SRC_H, SRC_X, SRC_LAT}, 256, 575}, TGTC_CHAIN_HL, TGTC_CHAIN_HL, TGTC_CHAIN_HL,         // style
    TGTC_CHAIN_HLX, TGTC_CHAIN_HL, TGTC_CHAIN_HL, {288, 3, 0, 2, {SRC_H, SRC_LAT, 0, 0}, 0, 256}};
#undef TGTC_CHAIN_HL
#undef TGTC_CHAIN_HLX

struct ChainCall {   // what a backward needs to know of its forward
    const float *x, *remap, *lat_c, *lat_s;
    int64_t R;
    int n, precision;
};

struct ChainLayout {   // byte offsets into the workspace
    size_t plane[kChainPlanes], rgb;                         // kept from forward to backward
    size_t g[2], dpre, sc, dyT, xT, part, WT, w16, dys, row_inv, dsum, dsums, ray_inv, total;
};
static ChainLayout chain_layout(int64_t R, int n) {
    ChainLayout L{};
    const size_t M = (size_t)R * n;
    size_t off = 0;
    auto take = [&](size_t floats) {
        const size_t o = off;
        off += (floats * sizeof(float) + 255) & ~(size_t)255;
        return o;
    };
    for (int i = 0; i < kChainPlanes; ++i) L.plane[i] = take(M * 256);
    L.rgb = take(M * 3);
    size_t dyT = 0, xT = 0, part = 0;
    for (const ChainLayer& l : kChain) {
        int nsplit;
        int64_t mc;
        backward_split((int64_t)M, l.K, l.N, nsplit, mc);
        const size_t mpad = (size_t)nsplit * mc;
        dyT = std::max(dyT, l.N * mpad), xT = std::max(xT, l.K * mpad), part = std::max(part, (size_t)nsplit * l.N * l.K);
    }
    L.g[0] = take(M * 256), L.g[1] = take(M * 256), L.dpre = take(M * 3), L.sc = take(64);
    L.dyT = take(dyT), L.xT = take(xT), L.part = take(part);
    L.WT = take((size_t)kChainWRows * 256), L.w16 = take((size_t)kChainWRows * 256);   // w16: hi, then lo, halves
    L.dys = take(M * 256), L.row_inv = take(M);
    L.dsum = take((size_t)R * 256), L.dsums = take((size_t)R * 256), L.ray_inv = take((size_t)R);
    L.total = off;
    return L;
}

static SegRows chain_rows(int g, const ChainCall& c, char* ws, const ChainLayout& L) {
    const ChainLayer& l = kChain[g];
    SegRows a{};
    a.nseg = l.nseg, a.rows = (int)(c.R * c.n), a.K = l.K, a.n = c.n;
    for (int s = 0; s < l.nseg; ++s) {
        switch (l.src[s]) {
            case SRC_X: a.seg[s] = {c.x, 63, 63, 0}; break;
            case SRC_REMAP: a.seg[s] = {c.remap, 256, 256, 0}; break;
            case SRC_LAT: a.seg[s] = {g < kChainConcat ? c.lat_c : c.lat_s, 32, 32, 1}; break;
            default: a.seg[s] = {reinterpret_cast<const float*>(ws + L.plane[g - 1]), 256, 256, 0}; break;
        }
    }
    return a;
}

// M = R * n samples at most 65 535 x 32: the transposes of the weight-gradient operands put 32 samples on each grid.y block
constexpr int64_t kChainMaxSamples = 65535LL * 32;
static bool chain_shape_ok(int64_t R, int n) { return R >= 0 && n > 0 && R <= kChainMaxSamples / n; }

// one layer's backward; dy [M,N] is the gradient of the layer's output, `gate` that output (ReLU layers) or null
static int chain_layer_backward(const tgtc_style2d& h, int g, const ChainCall& c, char* ws, const ChainLayout& L, const float* W,
                                const float* dy, const float* gate, float* dx, float* dW, float* db, float* d_lat,
                                hipStream_t st) {
    const ChainLayer& l = kChain[g];
    const int K = l.K, N = l.N;
    const int64_t M = c.R * c.n;
    auto f = [&](size_t o) { return reinterpret_cast<float*>(ws + o); };
    int nsplit;
    int64_t mc;
    backward_split(M, K, N, nsplit, mc);
    const long long mpad = (long long)nsplit * mc, mn = (long long)M * N;
    float *sc = f(L.sc), *WT = f(L.WT), *dys = f(L.dys), *row_inv = f(L.row_inv), *part = f(L.part);
    TGTC_HIP_CHECK(hipMemsetAsync(sc, 0, 16, st));
    absmax_kernel<<<(unsigned)std::min<long long>(1024, (mn + 255) / 256), 256, 0, st>>>(dy, mn, reinterpret_cast<unsigned*>(sc), nullptr);
    TGTC_LAUNCH_CHECK();
    grad_scale_kernel<<<1, 1, 0, st>>>(sc);
    TGTC_LAUNCH_CHECK();
    // rows of W^T: the hidden columns in rows 0..255, the latent columns in rows 256..287, as fp32 and as pre-split halves
    const bool pre = N % 4 == 0;
    half_t* wh = reinterpret_cast<half_t*>(f(L.w16));
    half_t* wl = wh + (size_t)kChainWRows * 256;
    auto w_rows = [&](int col0, int cols, int row0) {
        const dim3 grid((cols + 31) / 32, (N + 31) / 32);
        const size_t o = (size_t)row0 * N;
        transpose_sub_kernel<<<grid, 256, 0, st>>>(W + col0, K, N, cols, WT + o, pre ? wh + o : nullptr, pre ? wl + o : nullptr);
    };
    if (dx && d_lat && l.lat_col == l.h_col + 256) {
        w_rows(l.h_col, 288, 0);
    } else {
        if (dx) w_rows(l.h_col, 256, 0);
        if (d_lat) w_rows(l.lat_col, 32, 256);
    }
    TGTC_LAUNCH_CHECK();
    if (dx) {   // dx[M,256] = (s_m * gated dy)[M,N] . W[:, hidden columns], row m scaled back by 1/s_m
        half_t* dyh = reinterpret_cast<half_t*>(dys);
        half_t* dyl = dyh + (size_t)mn;
        row_scale_kernel<<<(unsigned)((M + 3) / 4), 256, 0, st>>>(dy, M, N, row_inv);
        TGTC_LAUNCH_CHECK();
        if (pre) scale_split_kernel<<<(unsigned)((mn + 255) / 256), 256, 0, st>>>(dy, mn, N, row_inv, gate, dyh, dyl);
        else scale_copy_kernel<<<(unsigned)((mn + 255) / 256), 256, 0, st>>>(dy, mn, N, row_inv, dys, gate);
        TGTC_LAUNCH_CHECK();
        DenseRows al{dys, N, 0, (int)M, N}, bl{WT, N, 0, 256, N};
        if (pre) al.h16 = dyh, al.l16 = dyl, bl.h16 = wh, bl.l16 = wl;
        GemmOut out{dx, 256, 1, 0, nullptr, nullptr, 1.0f, 0};
        out.row_alpha = row_inv;
        TGTC_TRY((launch_gemm<DenseRows, false>(&h, al, bl, out, (int)M, 256, N, 1, st)));
    }
    if (d_lat) {   // d_lat[R,32] += (sum over the ray's samples of s * gated dy)[R,N] . W[:, latent columns] / s
        const long long rn = (long long)c.R * N;
        float *dsum = f(L.dsum), *dsums = f(L.dsums), *ray_inv = f(L.ray_inv);
        half_t* sh = reinterpret_cast<half_t*>(dsums);
        half_t* sl = sh + (size_t)rn;
        ray_sum_kernel<<<(unsigned)((rn + 255) / 256), 256, 0, st>>>(dy, gate, c.R, c.n, N, sc + 1, dsum);
        TGTC_LAUNCH_CHECK();
        row_scale_kernel<<<(unsigned)((c.R + 3) / 4), 256, 0, st>>>(dsum, c.R, N, ray_inv);
        TGTC_LAUNCH_CHECK();
        if (pre) scale_split_kernel<<<(unsigned)((rn + 255) / 256), 256, 0, st>>>(dsum, rn, N, ray_inv, nullptr, sh, sl);
        else scale_copy_kernel<<<(unsigned)((rn + 255) / 256), 256, 0, st>>>(dsum, rn, N, ray_inv, dsums, nullptr);
        TGTC_LAUNCH_CHECK();
        const size_t o = (size_t)256 * N;
        DenseRows al{dsums, N, 0, (int)c.R, N}, bl{WT + o, N, 0, 32, N};
        if (pre) al.h16 = sh, al.l16 = sl, bl.h16 = wh + o, bl.l16 = wl + o;
        GemmOut out{d_lat, 32, 1, 0, nullptr, d_lat, 1.0f, 0};
        out.row_alpha = ray_inv, out.alpha_dev = sc + 2;
        TGTC_TRY((launch_gemm<DenseRows, false>(&h, al, bl, out, (int)c.R, 32, N, 1, st)));
    }
    // dW, db: tgtc_s2d_linear_backward's, with x^T written from the segments
    half_t* dth = reinterpret_cast<half_t*>(f(L.dyT));
    half_t* dtl = dth + (size_t)N * mpad;
    half_t* xh = reinterpret_cast<half_t*>(f(L.xT));
    half_t* xl = xh + (size_t)K * mpad;
    if (mpad > M) {   // only the pad columns: the transposes write the rest
        const size_t pitch = (size_t)mpad * sizeof(half_t), wide = (size_t)(mpad - M) * sizeof(half_t);
        TGTC_HIP_CHECK(hipMemset2DAsync(dth + M, pitch, 0, wide, N, st));
        TGTC_HIP_CHECK(hipMemset2DAsync(dtl + M, pitch, 0, wide, N, st));
        TGTC_HIP_CHECK(hipMemset2DAsync(xh + M, pitch, 0, wide, K, st));
        TGTC_HIP_CHECK(hipMemset2DAsync(xl + M, pitch, 0, wide, K, st));
    }
    transpose_ld_half_kernel<<<dim3((N + 31) / 32, (unsigned)((M + 31) / 32)), 256, 0, st>>>(dy, M, N, dth, dtl, mpad, sc + 1, gate);
    TGTC_LAUNCH_CHECK();
    transpose_seg_half_kernel<<<dim3((K + 31) / 32, (unsigned)((M + 31) / 32)), 256, 0, st>>>(chain_rows(g, c, ws, L), xh, xl, mpad);
    TGTC_LAUNCH_CHECK();
    DenseRows al{f(L.dyT), mpad, mc, N, (int)mc}, bl{f(L.xT), mpad, mc, K, (int)mc};
    al.h16 = dth, al.l16 = dtl;
    bl.h16 = xh, bl.l16 = xl;
    GemmOut out{nsplit > 1 ? part : dW, K, 1, (long long)N * K, nullptr, nullptr, 1.0f, 0};
    out.alpha_dev = sc + 2;
    TGTC_TRY((launch_gemm<DenseRows, false>(&h, al, bl, out, N, K, (int)mc, nsplit, st)));
    if (nsplit > 1) {
        const long long nk = (long long)N * K;
        sum_partials_kernel<<<(unsigned)((nk + 255) / 256), 256, 0, st>>>(part, nsplit, nk, dW);
        TGTC_LAUNCH_CHECK();
    }
    TGTC_HIP_CHECK(hipMemsetAsync(db, 0, (size_t)N * sizeof(float), st));
    rowsum_kernel<<<dim3(N, nsplit), 256, 0, st>>>(dth, dtl, M, mpad, mc, db, sc + 2);
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

}  // namespace tgtc

struct tgtc_style_trainer {
    std::mutex mu;
    std::map<const void*, ChainCall> calls;   // by workspace: the forward it holds
};

extern "C" int tgtc_style_trainer_create(tgtc_style_trainer** out) {
    TGTC_REQUIRE(out, "style_trainer_create: null argument");
    *out = new tgtc_style_trainer();
    return TGTC_OK;
}

extern "C" int tgtc_style_trainer_destroy(tgtc_style_trainer* tr) {
    delete tr;
    return TGTC_OK;
}

extern "C" size_t tgtc_style_trainer_workspace_bytes(int64_t R, int n) {
    return chain_shape_ok(R, n) && R > 0 ? chain_layout(R, n).total : 0;
}

extern "C" int tgtc_style_trainer_forward(tgtc_style_trainer* tr, const float* const* params, const float* x,
                                          const float* base_remap, const float* lat_c, const float* lat_s, int64_t R, int n,
                                          int precision, void* workspace, size_t workspace_bytes, float* rgb, void* stream) {
    TGTC_REQUIRE(tr, "style_trainer_forward: null trainer");
    TGTC_REQUIRE(chain_shape_ok(R, n), "style_trainer_forward: bad shape (R >= 0, n > 0, R * n <= 2 097 120)");
    TGTC_REQUIRE(precision == TGTC_PREC_FP16 || precision == TGTC_PREC_FP16X3, "style_trainer_forward: precision %d (fp16x3 or fp16)", precision);
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(params && x && base_remap && lat_c && lat_s && rgb && workspace, "style_trainer_forward: null pointer");
    for (int i = 0; i < 2 * kChainLayers; ++i) TGTC_REQUIRE(params[i], "style_trainer_forward: params[%d] is null", i);
    const ChainLayout L = chain_layout(R, n);
    TGTC_REQUIRE(workspace_bytes >= L.total, "style_trainer_forward: workspace of %zu bytes, needs %zu", workspace_bytes, L.total);
    hipStream_t st = as_stream(stream);
    tgtc_style2d h;
    h.precision = precision;
    char* ws = static_cast<char*>(workspace);
    const ChainCall c{x, base_remap, lat_c, lat_s, R, n, precision};
    const int M = (int)(R * n);
    half_t* wh = reinterpret_cast<half_t*>(ws + L.w16);
    for (int g = 0; g < kChainLayers; ++g) {
        const ChainLayer& l = kChain[g];
        DenseRows bl{params[2 * g], l.K, 0, l.N, l.K};
        if (l.K % 4 == 0) {   // the weight as pre-split halves, as tgtc_s2d_split hands them to tgtc_s2d_linear_pre
            const long long nk = (long long)l.N * l.K;
            split_kernel<<<(unsigned)((nk + 255) / 256), 256, 0, st>>>(params[2 * g], nk, wh, wh + nk);
            TGTC_LAUNCH_CHECK();
            bl.h16 = wh, bl.l16 = wh + nk;
        }
        float* y = reinterpret_cast<float*>(ws + (g < kChainPlanes ? L.plane[g] : L.dpre));
        GemmOut out{y, l.N, 1, 0, params[2 * g + 1], nullptr, 1.0f, l.relu};
        TGTC_TRY((launch_gemm<SegRows, false>(&h, chain_rows(g, c, ws, L), bl, out, M, l.N, l.K, 1, st)));
    }
    const long long m3 = (long long)M * 3;
    act_kernel<<<(unsigned)((m3 + 255) / 256), 256, 0, st>>>(reinterpret_cast<const float*>(ws + L.dpre), nullptr, m3, 2, rgb);
    TGTC_LAUNCH_CHECK();
    TGTC_HIP_CHECK(hipMemcpyAsync(ws + L.rgb, rgb, (size_t)m3 * sizeof(float), hipMemcpyDeviceToDevice, st));
    std::lock_guard<std::mutex> lock(tr->mu);
    tr->calls[workspace] = c;
    return TGTC_OK;
}

extern "C" int tgtc_style_trainer_backward(tgtc_style_trainer* tr, const float* const* params, const float* d_rgb, int64_t R,
                                           int n, void* workspace, size_t workspace_bytes, float* const* grads, float* d_lat_c,
                                           float* d_lat_s, void* stream) {
    TGTC_REQUIRE(tr, "style_trainer_backward: null trainer");
    TGTC_REQUIRE(chain_shape_ok(R, n), "style_trainer_backward: bad shape (R >= 0, n > 0, R * n <= 2 097 120)");
    TGTC_REQUIRE(grads, "style_trainer_backward: null pointer");
    for (int i = 0; i < 2 * kChainLayers; ++i) TGTC_REQUIRE(grads[i], "style_trainer_backward: grads[%d] is null", i);
    hipStream_t st = as_stream(stream);
    if (R == 0) {   // an empty batch: every gradient is zero
        for (int g = 0; g < kChainLayers; ++g) {
            TGTC_HIP_CHECK(hipMemsetAsync(grads[2 * g], 0, (size_t)kChain[g].N * kChain[g].K * sizeof(float), st));
            TGTC_HIP_CHECK(hipMemsetAsync(grads[2 * g + 1], 0, (size_t)kChain[g].N * sizeof(float), st));
        }
        return TGTC_OK;
    }
    TGTC_REQUIRE(params && d_rgb && workspace, "style_trainer_backward: null pointer");
    for (int i = 0; i < 2 * kChainLayers; ++i) TGTC_REQUIRE(params[i], "style_trainer_backward: params[%d] is null", i);
    const ChainLayout L = chain_layout(R, n);
    TGTC_REQUIRE(workspace_bytes >= L.total, "style_trainer_backward: workspace of %zu bytes, needs %zu", workspace_bytes, L.total);
    ChainCall c;
    {
        std::lock_guard<std::mutex> lock(tr->mu);
        const auto it = tr->calls.find(workspace);
        TGTC_REQUIRE(it != tr->calls.end() && it->second.R == R && it->second.n == n,
                     "style_trainer_backward: this workspace holds no forward of %lld rays x %d samples", (long long)R, n);
        c = it->second;
        tr->calls.erase(it);
    }
    tgtc_style2d h;
    h.precision = c.precision;
    char* ws = static_cast<char*>(workspace);
    auto f = [&](size_t o) { return reinterpret_cast<float*>(ws + o); };
    const long long m3 = (long long)R * n * 3;
    act_kernel<<<(unsigned)((m3 + 255) / 256), 256, 0, st>>>(d_rgb, f(L.rgb), m3, 1, f(L.dpre));   // through the sigmoid
    TGTC_LAUNCH_CHECK();
    if (d_lat_c) TGTC_HIP_CHECK(hipMemsetAsync(d_lat_c, 0, (size_t)R * 32 * sizeof(float), st));
    if (d_lat_s) TGTC_HIP_CHECK(hipMemsetAsync(d_lat_s, 0, (size_t)R * 32 * sizeof(float), st));
    const float* dy = f(L.dpre);
    for (int g = kChainLayers - 1, flip = 0; g >= 0; --g) {
        float* dx = kChain[g].h_col >= 0 ? f(L.g[flip]) : nullptr;
        TGTC_TRY(chain_layer_backward(h, g, c, ws, L, params[2 * g], dy, g < kChainPlanes ? f(L.plane[g]) : nullptr, dx,
                                      grads[2 * g], grads[2 * g + 1], g < kChainConcat ? d_lat_c : d_lat_s, st));
        dy = dx, flip ^= 1;
    }
    return TGTC_OK;
}

// mode 0: ReLU backward dx = dy * (y > 0); 1: sigmoid backward dx = dy * y * (1 - y); 2: sigmoid forward dx = sigmoid(dy)
extern "C" int tgtc_s2d_activation(const float* dy, const float* y, int64_t n, int mode, float* dx, void* stream) {
    TGTC_REQUIRE(n >= 0 && mode >= 0 && mode <= 2, "s2d_activation: bad argument");
    if (n == 0) return TGTC_OK;
    TGTC_REQUIRE(dy && dx && (mode == 2 || y), "s2d_activation: null pointer");
    act_kernel<<<(unsigned)((n + 255) / 256), 256, 0, as_stream(stream)>>>(dy, y, n, mode, dx);
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

extern "C" int tgtc_s2d_mean_std(const float* feat, int C, int64_t HW, float eps, float* mean, float* std_,
                                 void* stream) {
    TGTC_REQUIRE(feat && mean && std_ && C > 0 && HW > 1, "mean_std: bad argument (needs HW > 1 for the unbiased variance)");
    mean_std_kernel<<<C, 256, 0, as_stream(stream)>>>(feat, HW, eps, mean, std_);
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

extern "C" int tgtc_s2d_adain(const float* content, int64_t HWc, const float* style, int64_t HWs, int C, float* stats,
                              float* out, void* stream) {
    TGTC_REQUIRE(content && style && stats && out && C > 0 && HWc > 1 && HWs > 1, "adain: bad argument");
    hipStream_t st = as_stream(stream);
    mean_std_kernel<<<C, 256, 0, st>>>(content, HWc, 1e-5f, stats, stats + C);
    mean_std_kernel<<<C, 256, 0, st>>>(style, HWs, 1e-5f, stats + 2 * C, stats + 3 * C);
    const long long n = HWc * C;
    adain_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(content, HWc, C, stats, out);
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

extern "C" int tgtc_s2d_resize_bilinear(const float* in, int C, int h, int w, float* out, int H, int W, void* stream) {
    TGTC_REQUIRE(in && out && C > 0 && h > 0 && w > 0 && H > 0 && W > 0, "resize_bilinear: bad argument");
    const long long n = (long long)C * H * W;
    resize_bilinear_kernel<<<(unsigned)((n + 255) / 256), 256, 0, as_stream(stream)>>>(in, C, h, w, out, H, W);
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

extern "C" int tgtc_s2d_style_feature(const float* hs_tokens, int n_tokens, float* feature, void* stream) {
    TGTC_REQUIRE(hs_tokens && feature && n_tokens > 1, "style_feature: bad argument");
    style_feature_kernel<<<512, 256, 0, as_stream(stream)>>>(hs_tokens, n_tokens, feature);
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

extern "C" int tgtc_s2d_tokens_to_nchw(const float* tokens, int n, int C, float* out, void* stream) {
    TGTC_REQUIRE(tokens && out && n > 0 && C > 0, "tokens_to_nchw: bad argument");
    dim3 grid((C + 31) / 32, (n + 31) / 32);
    transpose_kernel<<<grid, 256, 0, as_stream(stream)>>>(tokens, n, C, out);
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

extern "C" int tgtc_s2d_nchw_to_tokens(const float* in, int n, int C, float* tokens, void* stream) {
    TGTC_REQUIRE(in && tokens && n > 0 && C > 0, "nchw_to_tokens: bad argument");
    dim3 grid((n + 31) / 32, (C + 31) / 32);
    transpose_kernel<<<grid, 256, 0, as_stream(stream)>>>(in, C, n, tokens);
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}
