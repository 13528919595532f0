// Stylised path, K latent sets per ray in one launch (reference rendering.py:122-142 under K latents).
//
// In the stylised chain the latent z enters only the concat MLP and the style MLP; positions, the positional encoding,
// the NeRF trunk (sigma, base_remap) are functions of the ray alone.  styled_rays_multi_kernel is styled_rays_kernel
// (mlp_style.hip) with the tile's work reordered so that this part runs once per tile:
//
//   per tile of samples:
//       positions, positional encoding                                   (once)
//       NeRF trunk -> sigma (stored once), base_remap                    (once)   stream: NeRF trunk
//       park base_remap in slab region B                                 (once)
//       for k in 0 .. K-1:
//           z_k, mean(z_k) of the tile's rays
//           concat MLP(pe, z_k) -> concat_features in registers                   stream: concat
//           base_remap <- slab region B
//           style layer 0 on [base_remap | concat_features | pe | mean z_k]       stream: style
//               (k-step order as in styled_rays_kernel: 8 remap, 8 concat, 2 pe, 1 z); outputs stream to slab region A
//           style layers 1..7 -> sigmoid -> rgb[k, sample]
//
// Per latent the MFMA sequence and its operands are those of styled_rays_kernel: which 256-feature set passes through
// the slab differs (there concat_features, here base_remap), but a parked set is the same fp16 hi/lo pairs the
// registers held, so rgb[k] and sigma carry the bits of tgtc_styled_forward_rays(..., z[k]).
//
// Weight ring: two static maps over the same LDS ring, the NeRF trunk (one segment; the colour head behind it is never
// fetched into a consumed fragment) and concat | style (two segments).  The ring is restarted (s_barrier + prologue() +
// start()) once for the trunk and once per latent; styled_rays_kernel restarts it once per tile.  The restart is also
// where z_k is fetched: its global loads are retired BEFORE any LDS-DMA is issued, as in styled_rays_kernel (a vmcnt
// wait for them would otherwise drain the whole look-ahead).  Both bias tables stay in LDS for the whole kernel.
//
// Slab: two regions of kStashBytesPerWG per workgroup, both owned by the style handle (tgtc_style_create): region A
// carries style layer 0's outputs as in styled_rays_kernel, region B holds base_remap across the K iterations.
#include "mlp_core.h"
#include "mlp_layouts.h"
#include "mlp_pack.h"
#include "mlp_style_chain.h"

namespace tgtc {

struct StyledMultiArgs {
    const char* nerf_bias;
    const char* nerf_stream;
    const char* pair_bias;
    const char* concat_stream;
    const char* style_stream;
    char* stash;            // region A: gridDim.x * kStashBytesPerWG
    long long stash2_delta;  // region B of a workgroup lies this many bytes behind its region A
    long long M;   // R * N samples (per latent)
    long long R;
    int N;
    int K;
    const double* rays_o;
    const double* rays_d;
    const float* ts;
    const float* z;  // [K,R,32]
    float* rgb;      // [K,R,N,3]
    float* sigma;    // [R,N] or null
};

// concat | style, both chunk aligned (kConcatFrags is a whole number of chunks in both modes)
template <class C>
struct PairMap {
    static constexpr int F_CONCAT = 0;
    static constexpr int F_STYLE = kConcatFrags;
    static constexpr int NFRAG = F_STYLE + kStyleFrags;
    static constexpr int NSEG = 2;
    static constexpr int chunk0(int i) { return i == 0 ? 0 : i == 1 ? F_STYLE / C::FPC : (1 << 30); }
    static_assert(kConcatFrags % C::FPC == 0, "concat stream must end on a chunk boundary");
};

template <class C>
__global__ void __launch_bounds__(C::NWAVES * 64, C::NWAVES / 4) styled_rays_multi_kernel(StyledMultiArgs a) {
    constexpr int NCT = C::NCT;
    constexpr bool SPLIT = C::SPLIT;
    using Map = PairMap<C>;
    using L = NerfLayout;
    __shared__ __attribute__((aligned(16))) char smem[kRingBytes + kNerfBiasBytes + kStylePairBiasBytes];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, n = lane & 15;
    char* slab = a.stash + (size_t)blockIdx.x * kStashBytesPerWG + (size_t)tid * 16;    // this lane's 16-byte column, region A
    // (region B's column is slab + a.stash2_delta, formed where it is used: one address pair live, not two)

    // the two streams share the ring and its lane addresses
    WeightStream<C, SingleStreamMap<kTrunkFrags>> wt;
    WeightStream<C, Map> ws;
    const char* const trunk_streams[1] = {a.nerf_stream};
    wt.init(trunk_streams, smem, wave, lane);
    ws.src[0] = ws.lane_src(a.concat_stream, wave, lane);
    ws.src[1] = ws.lane_src(a.style_stream, wave, lane);
    ws.voff = wt.voff, ws.lds_wave = wt.lds_wave, ws.lane_lo = wt.lane_lo, ws.lane_hi = wt.lane_hi;
    // bias tables: loaded once per workgroup (LDS-DMA), visible after the first ring barrier
#pragma unroll
    for (int j = 0; j < kNerfBiasBytes / (C::NWAVES * 1024); ++j)
        __builtin_amdgcn_global_load_lds(TGTC_GPTR(a.nerf_bias + (j * C::NWAVES + wave) * 1024 + lane * 16),
                                         TGTC_LPTR(smem + kRingBytes + (j * C::NWAVES + wave) * 1024), 16, 0, 0);
#pragma unroll
    for (int j = 0; j < kStylePairBiasBytes / (C::NWAVES * 1024); ++j)
        __builtin_amdgcn_global_load_lds(TGTC_GPTR(a.pair_bias + (j * C::NWAVES + wave) * 1024 + lane * 16),
                                         TGTC_LPTR(smem + kRingBytes + kNerfBiasBytes + (j * C::NWAVES + wave) * 1024), 16, 0, 0);
    const lds_cptr nerf_bias = opaque((lds_cptr)smem + kRingBytes + 16 * g);
    const lds_cptr pair_bias = opaque((lds_cptr)smem + kRingBytes + kNerfBiasBytes + 16 * g);

    const long long n_tiles = (a.M + C::SAMPLES_PER_WG - 1) / C::SAMPLES_PER_WG;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        // ---- inputs
        const long long s_wave = tile * C::SAMPLES_PER_WG + wave * C::SAMPLES_PER_WAVE;
        double pos[NCT][3];
        unsigned sidx[NCT];   // M < 2^31
#pragma unroll
        for (int c = 0; c < NCT; ++c) {
            long long s = s_wave + c * 16 + n;
            sidx[c] = (unsigned)s;
            if (s >= a.M) s = a.M - 1;
            const long long r = (unsigned)s / (unsigned)a.N;
            const double t = (double)a.ts[s];
#pragma unroll
            for (int k = 0; k < 3; ++k) pos[c][k] = a.rays_o[r * 3 + k] + t * a.rays_d[r * 3 + k];
            // retire the loads before any LDS-DMA is issued (their wait would drain the whole prefetch)
#pragma unroll
            for (int k = 0; k < 3; ++k) asm volatile("" : "+v"(pos[c][k]));
        }
        // previous tile: every wave must be done with the ring before it is refilled
        __builtin_amdgcn_s_barrier();
        wt.prologue();

        half8 pe_h[2][NCT], pe_l[2][NCT];
        // the encoder's band / coordinate selectors are functions of the lane group alone: seen as loop invariants they are
        // hoisted out of the tile loop (8 bands, 16 lane masks) and spilled; an opaque copy keeps them inside the tile
        int g_enc = g;
        asm volatile("" : "+v"(g_enc));
#pragma unroll
        for (int c = 0; c < NCT; ++c) {
            half8 h2[2], l2[2];
            encode_point<SPLIT, SPLIT>(pos[c], g_enc, h2, l2, nullptr);
            pe_h[0][c] = h2[0], pe_h[1][c] = h2[1], pe_l[0][c] = l2[0], pe_l[1][c] = l2[1];
        }
        wt.start();

        half8 Xh[8][NCT], Xl[8][NCT], Yh[8][NCT], Yl[8][NCT];
        auto to_Y = [&](auto rt_, auto c_, auto h_, const float4v& acc) {
            constexpr int rt = decltype(rt_)::value, c = decltype(c_)::value;
            store_act<C, rt, decltype(h_)::value>(acc, Yh[rt / 2][c], Yl[rt / 2][c]);
        };
        auto to_X = [&](auto rt_, auto c_, auto h_, const float4v& acc) {
            constexpr int rt = decltype(rt_)::value, c = decltype(c_)::value;
            store_act<C, rt, decltype(h_)::value>(acc, Xh[rt / 2][c], Xl[rt / 2][c]);
        };
        // ---- NeRF trunk (models.py:95-101), once per tile
        dense_layer<C, L::frag0(0), 2, 16, L::bias0(0)>(wt, nerf_bias, pe_h, pe_l, to_Y);
        dense_layer<C, L::frag0(1), 8, 16, L::bias0(1)>(wt, nerf_bias, Yh, Yl, to_X);
        dense_layer<C, L::frag0(2), 8, 16, L::bias0(2)>(wt, nerf_bias, Xh, Xl, to_Y);
        dense_layer<C, L::frag0(3), 8, 16, L::bias0(3)>(wt, nerf_bias, Yh, Yl, to_X);
        dense_layer<C, L::frag0(4), 8, 16, L::bias0(4)>(wt, nerf_bias, Xh, Xl, to_Y);
        {
            half8 Bh[10][NCT], Bl[10][NCT];
#pragma unroll
            for (int k = 0; k < 8; ++k) append<C>(Bh, Bl, k, Yh[k], Yl[k]);
            append<C>(Bh, Bl, 8, pe_h[0], pe_l[0]);
            append<C>(Bh, Bl, 9, pe_h[1], pe_l[1]);
            dense_layer<C, L::frag0(5), 10, 16, L::bias0(5)>(wt, nerf_bias, Bh, Bl, to_X);
        }
        dense_layer<C, L::frag0(6), 8, 16, L::bias0(6)>(wt, nerf_bias, Xh, Xl, to_Y);
        dense_layer<C, L::frag0(7), 8, 16, L::bias0(7)>(wt, nerf_bias, Yh, Yl, to_X);
        dense_layer<C, L::frag0(8), 8, 1, L::bias0(8)>(wt, nerf_bias, Xh, Xl, [&](auto, auto c_, auto h_, const float4v& acc) {
            constexpr int c = decltype(c_)::value;
            if constexpr (decltype(h_)::value == 0)
                if (g == 0 && a.sigma && sidx[c] < a.M) a.sigma[(size_t)sidx[c]] = acc[0];
        });
        // base_remap: streams to slab region B as it is produced, where it stays for the K iterations
        {
            half8 Th[NCT], Tl[NCT];
            dense_layer<C, L::frag0(9), 8, 16, L::bias0(9)>(wt, nerf_bias, Xh, Xl, [&](auto rt_, auto c_, auto h_, const float4v& acc) {
                constexpr int rt = decltype(rt_)::value, c = decltype(c_)::value, hf = decltype(h_)::value;
                store_act<C, rt, hf>(acc, Th[c], Tl[c]);
                if constexpr ((rt & 1) && hf == 1) stash_store<C>(slab + a.stash2_delta, rt / 2, c, Th[c], Tl[c]);
            });
        }

        for (int k = 0; k < a.K; ++k) {
            // ---- latent k of the tile's rays
            float zsum[NCT];
            half8 z_h[NCT], z_l[NCT], zb_h[NCT], zb_l[NCT];
#pragma unroll
            for (int c = 0; c < NCT; ++c) {
                const long long s = sidx[c] < a.M ? sidx[c] : a.M - 1;
                const long long r = (unsigned)s / (unsigned)a.N;
                const float* zr = a.z + ((long long)k * a.R + r) * 32;
                float part = 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) part += zr[8 * g + j];
                load_vec32<SPLIT>(zr, g, z_h[c], z_l[c]);
                zsum[c] = part;
                // retired before the ring is restarted, as the tile's inputs are
                asm volatile("" : "+v"(zsum[c]), "+v"(z_h[c]));
                if constexpr (SPLIT) asm volatile("" : "+v"(z_l[c]));
            }
            // every wave must be done with the previous stream before the ring is refilled
            __builtin_amdgcn_s_barrier();
            ws.prologue();
#pragma unroll
            for (int c = 0; c < NCT; ++c) {
                // rendering.py:126: mean over the 32 latent channels, broadcast back to 32 (rendering.py:139)
                float zs = zsum[c];
                zs += __shfl_xor(zs, 16);
                zs += __shfl_xor(zs, 32);
                splat8<SPLIT>(zs * (1.0f / 32.0f), zb_h[c], zb_l[c]);
            }
            ws.start();

            // ---- concat MLP -> Y
            concat_mlp<C, Map::F_CONCAT, 0>(ws, pair_bias, pe_h, pe_l, z_h, z_l, Xh, Xl, Yh, Yl);
            // ---- style layer 0 on [remap (slab B -> X) | concat_features (Y) | pe | mean z]; outputs stream to slab A
            stash_load<C>(slab + a.stash2_delta, Xh, Xl);
            {
                half8 Bh[19][NCT], Bl[19][NCT];
#pragma unroll
                for (int i = 0; i < 8; ++i) append<C>(Bh, Bl, i, Xh[i], Xl[i]);
#pragma unroll
                for (int i = 0; i < 8; ++i) append<C>(Bh, Bl, 8 + i, Yh[i], Yl[i]);
                append<C>(Bh, Bl, 16, pe_h[0], pe_l[0]);
                append<C>(Bh, Bl, 17, pe_h[1], pe_l[1]);
                append<C>(Bh, Bl, 18, zb_h, zb_l);
                half8 Th[NCT], Tl[NCT];
                dense_layer<C, Map::F_STYLE + style_frag0(0), 19, 16, kConcatBiasFloats + style_bias0(0)>(
                    ws, pair_bias, Bh, Bl, [&](auto rt_, auto c_, auto h_, const float4v& acc) {
                        constexpr int rt = decltype(rt_)::value, c = decltype(c_)::value, hf = decltype(h_)::value;
                        store_act<C, rt, hf>(acc, Th[c], Tl[c]);
                        if constexpr ((rt & 1) && hf == 1) stash_store<C>(slab, rt / 2, c, Th[c], Tl[c]);
                    });
            }
            stash_load<C>(slab, Xh, Xl);
            // ---- style layers 1..7 -> rgb[k] (models.py:172-179)
            float* rgb_k = a.rgb + (long long)k * a.M * 3;
            style_tail<C, Map::F_STYLE, kConcatBiasFloats>(ws, pair_bias, pe_h, pe_l, zb_h, zb_l, Xh, Xl, Yh, Yl,
                                                           [&](auto c_, auto h_, const float4v& acc) {
                                                               constexpr int c = decltype(c_)::value, hf = decltype(h_)::value;
                                                               if (g == 0 && sidx[c] < a.M) {
#pragma unroll
                                                                   for (int r = 2 * hf; r < (hf ? 3 : 2); ++r)
                                                                       rgb_k[(size_t)sidx[c] * 3 + r] = 1.0f / (1.0f + expf(-acc[r]));
                                                               }
                                                           });
        }
    }
}

using CfgFast = MlpCfg<8, 2, false, 4>;  // the geometry of styled_rays_kernel (mlp_style.hip)
using CfgExact = MlpCfg<8, 1, true, 4>;

// The fp16 instance is compiled in a translation unit of its own (this source with -DTGTC_TU_FP16_ONLY) so that the two
// kernels build in parallel.
template <class C>
void launch_styled_rays_multi(unsigned grid, const StyledMultiArgs& a, hipStream_t st) {
    styled_rays_multi_kernel<C><<<grid, C::NWAVES * 64, 0, st>>>(a);
}
#ifdef TGTC_TU_FP16_ONLY
template void launch_styled_rays_multi<CfgFast>(unsigned, const StyledMultiArgs&, hipStream_t);
}  // namespace tgtc
#else
extern template void launch_styled_rays_multi<CfgFast>(unsigned, const StyledMultiArgs&, hipStream_t);

int styled_forward_rays_multi_impl(const tgtc_net* nerf, const tgtc_net* style, const double* rays_o, const double* rays_d,
                                   const float* ts, const float* z, int K, int64_t R, int N, float* rgb, float* sigma,
                                   hipStream_t st) {
    if (nerf->precision != style->precision)
        return fail(TGTC_ERR_ARG, "styled_forward_rays_multi: NeRF and style nets were packed with different precisions");
    // (style handles are fp16x3 or fp16 only, so the precisions are one of the two the kernel is built for)
    constexpr int64_t kLimit = (int64_t)1 << 31;
    if (R >= kLimit || R * (int64_t)N >= kLimit || R * (int64_t)N * K >= kLimit)
        return fail(TGTC_ERR_UNSUPPORTED, "styled_forward_rays_multi: K x R x N >= 2^31 in one launch (chunk the rays)");
    StyledMultiArgs a{};
    a.nerf_bias = nerf->dev, a.nerf_stream = nerf->dev + nerf->bias_bytes;
    a.pair_bias = style->dev, a.concat_stream = style->dev + style->bias_bytes;
    a.style_stream = style->dev + style->stream2_off;
    a.stash = style->dev + style->stash_off, a.stash2_delta = (long long)(style->stash2_off - style->stash_off);
    a.M = R * (int64_t)N, a.R = R, a.N = N, a.K = K;
    a.rays_o = rays_o, a.rays_d = rays_d, a.ts = ts, a.z = z, a.rgb = rgb, a.sigma = sigma;
    if (nerf->precision == TGTC_PREC_FP16) {
        const long long tiles = (a.M + CfgFast::SAMPLES_PER_WG - 1) / CfgFast::SAMPLES_PER_WG;
        launch_styled_rays_multi<CfgFast>((unsigned)(tiles < style->n_wg ? tiles : style->n_wg), a, st);
    } else {
        const long long tiles = (a.M + CfgExact::SAMPLES_PER_WG - 1) / CfgExact::SAMPLES_PER_WG;
        launch_styled_rays_multi<CfgExact>((unsigned)(tiles < style->n_wg ? tiles : style->n_wg), a, st);
    }
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

}  // namespace tgtc

using namespace tgtc;

extern "C" int tgtc_styled_forward_rays_multi(const tgtc_net* nerf, const tgtc_net* style, const double* rays_o,
                                              const double* rays_d, const float* ts, const float* z, int K, int64_t R,
                                              int N, float* rgb, float* sigma, void* stream) {
    TGTC_REQUIRE(nerf && nerf->kind == 0 && style && style->kind == 1 && K >= 1 && R >= 0 && N >= 1,
                 "styled_forward_rays_multi: bad argument");
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d && ts && z && rgb, "styled_forward_rays_multi: null pointer");
    return styled_forward_rays_multi_impl(nerf, style, rays_o, rays_d, ts, z, K, R, N, rgb, sigma, as_stream(stream));
}
#endif  // TGTC_TU_FP16_ONLY
