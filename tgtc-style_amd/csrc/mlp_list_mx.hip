// The stylised list kernel of the fp16x3+fp16mx pair without a plane (tgtc_styled_forward_list_folded_mx,
// tgtc_render_rays_styled_sparse_folded_mx, tgtc_restyle_rays_folded_mx, render.hip): the NeRF trunk of an fp16mx handle and
// the K latents of an fp16x3 style handle's fp16mx streams, tile after tile, in one persistent launch.
//
// styled_list_mx_kernel is trunk_plane_mx_kernel (mlp_trunk_mx.hip) followed by the latent loop of restyle_trunk_mx_kernel
// (mlp_style_mx.hip) per 128-entry tile: the two share the tile (8 waves, one column tile per wave), the ring and dense_mx, and
// the consumer's thread tid reads exactly the 16-byte columns the producer's thread tid wrote.  So base_remap's hi / lo fp16
// fragments are parked in the workgroup's tile of slab region B of the style handle (stash2_off, idle in the plane path)
// instead of the list's tile of a plane: the same stash_store / stash_load at blockIdx.x * kStashBytesPerWG + tid * 16, the
// same half8 values through memory, the same dense_mx sequences on the same operands -- a live sample's colours carry the bits
// of tgtc_geometry_trunk_mx + tgtc_restyle_rays_trunk_folded_mx.  Both translation units are restated here, not cut into a
// header (the two kernels keep their source and their register counts; profiles/list_mx_resources.txt); StylePairMxMap and
// mx_from_frags are the only shared pieces and live in mlp_mx.h.
//
// LDS: ring (128 KiB) | ONE table region (16 KiB) | the style row exponents (8 KiB) = 152 KiB.  The NeRF bias / row-exponent
// table (kNerfBiasBytes) and latent k's pair bias table (kStylePairBiasBytes) share the table region -- side by side they
// would need 168 KiB of a CU's 160.  The NeRF table is brought in behind the barrier that opens every tile, latent k's table
// behind the barrier that opens every latent iteration, also for K = 1 (the trunk phase has overwritten the region): the
// table swap restyle_trunk_mx_kernel makes per latent.  Both are requested in front of the ring prologue of their stream, so
// that stream's first counted wait and ring barrier cover them.  The style row exponents are loaded once per workgroup.
//
// COMPACT: the list's length is a host number, ts_live holds the list's depths, rgb is [K,count,3] at the list position
// (tgtc_restyle_rays_folded_mx).  Otherwise the length is a device word, the depth is ts[live[i]] and rgb[k, live[i]] is
// scattered into dense planes the caller has zero-filled (tgtc_render_rays_styled_sparse_folded_mx), as
// styled_rays_sparse_kernel<*, false, true> does.
//
// DESIGN.md section 3.1 facts this kernel depends on: (a) dense_mx drains the MFMA pipe behind a layer's last
// v_mfma_scale_* before the final epilogue; (b) every LDS-DMA here is the asm flavour (TGTC_ASM_DMA: lds_dma16 for the three
// tables, the rings' own through MxReader); (c) the tile's gather is retired before the tile's first LDS-DMA.  Each reader is
// walked to the last chunk of its stream (the last boundary waits for the last chunk), and a barrier stands between the last
// read of one stream and the prologue of the next: no LDS-DMA of one stream is in flight when the other stream's prologue
// starts, and none when the workgroup ends.  A workgroup without a tile returns before its first LDS-DMA.
#define TGTC_ASM_DMA 1  // see mlp_core.h lds_dma16
#include "common.h"

#include "mlp_layouts.h"
#include "mlp_mx.h"
#include "mlp_nerf_mx_chain.h"
#include "mlp_pack.h"
#include "mlp_style_chain.h"
#include "mlp_style_mx.h"

namespace tgtc {

using CfgMx = MlpCfg<8, 1, false, 4>;    // the geometry of nerf_mx_kernel (mlp_nerf_mx.hip)
using CfgSlab = MlpCfg<8, 1, true, 4>;   // layout of the two slab tiles (hi then lo per k-step), the fp16x3 plane's
static_assert(CfgMx::SAMPLES_PER_WG == CfgSlab::SAMPLES_PER_WG && CfgMx::NWAVES == CfgSlab::NWAVES, "one tile geometry");

struct ListMxArgs {
    const char* nerf_bias;       // the NeRF handle's bias / row-exponent table (kNerfBiasBytes)
    const char* nerf_stream;     // its group stream (kNerfMxTable)
    const char* concat_stream;   // segment 0 of kStylePairMxTable
    const char* style_stream;    // segment 1
    const char* row_exp;         // kStylePairMxExpBytes
    const char* folded;          // [K] pair bias tables of kStylePairBiasBytes (tgtc_style_fold_latents)
    char* stash;                 // slab region A: gridDim.x * kStashBytesPerWG (style layer 0's round trip)
    long long stash2_delta;      // slab region B - slab region A (base_remap of the workgroup's tile)
    const double* rays_o;
    const double* rays_d;
    const unsigned* live;        // ascending sample indices
    const unsigned* n_live;      // scattered form: the list's length, a device word
    const float* ts;             // scattered form: [R,N]
    const float* ts_live;        // compact form: [count] depths of the list's samples
    float* rgb;                  // scattered: [K,R,N,3], zero-filled by the caller; compact: [K,count,3], every entry written
    long long M;                 // entries of one colour plane: R * N, or count
    unsigned count;              // compact form: the list's length
    int N;
    int K;
};

template <bool COMPACT>
__global__ void __launch_bounds__(CfgMx::NWAVES * 64, CfgMx::NWAVES / 4) styled_list_mx_kernel(ListMxArgs a) {
    using C = CfgMx;
    using L = NerfLayout;
    constexpr const MxTable& TN = kNerfMxTable;
    constexpr const MxTable& T = kStylePairMxTable;
    constexpr int NQN = TN.first[10];                          // layers 0-7, sigma, base_remap
    constexpr int NUNITS = mx_bytes_upto(TN, NQN) / 1024;
    constexpr int NQ = T.n;
    constexpr int kTableBytes = 16384;
    static_assert(kNerfBiasBytes == kTableBytes && kStylePairBiasBytes == kTableBytes, "the two tables share one region");
    constexpr int kTableAt = kRingBytes, kExpAt = kRingBytes + kTableBytes;
    constexpr int SB = kConcatBiasFloats;   // the style MLP's biases (and row exponents) lie behind the concat MLP's
    // ring | NeRF bias + row exponents, or latent k's pair bias table | style row exponents
    __shared__ __attribute__((aligned(16))) char smem[kExpAt + kStylePairMxExpBytes];

    // a workgroup without a tile leaves before any LDS-DMA is issued (none may be in flight when it ends), which is also what
    // keeps live[n_live - 1] from being read when nothing is live
    unsigned n_live;
    if constexpr (COMPACT) n_live = a.count;
    else n_live = *a.n_live;
    const unsigned n_tiles = (n_live + C::SAMPLES_PER_WG - 1) / C::SAMPLES_PER_WG;   // n_live < 2^31
    if (blockIdx.x >= n_tiles) return;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, n = lane & 15;
    // this lane's 16-byte column of the workgroup's tile of slab region A, and of region B
    char* slab = a.stash + (size_t)blockIdx.x * kStashBytesPerWG + (size_t)tid * 16;
    char* remap = slab + a.stash2_delta;

    // two readers on one ring: the style pair's takes the lane addresses, the trunk's copies them
    MxReader<C, StylePairMxMap, kStylePairMxTable> rd;
    MxReader<C, SingleStreamMap<NUNITS>, kNerfMxTable> rt;
    {
        const char* const streams[2] = {a.concat_stream, a.style_stream};
        rd.init(streams, smem, wave, lane);
        rt.ring.src[0] = rt.lane_src(a.nerf_stream, wave, lane);
        rt.ring.voff = rd.ring.voff, rt.ring.lds_wave = rd.ring.lds_wave;
        rt.ring.lane_lo = rd.ring.lane_lo, rt.ring.lane_hi = rd.ring.lane_hi;
        rt.b8_lo = rd.b8_lo, rt.b8_hi = rd.b8_hi;
    }
    // the style row exponents: requested before the first ring prologue, whose counted wait and ring barrier cover them
    static_assert(kStylePairMxExpBytes == C::NWAVES * 1024, "one LDS-DMA per wave");
    lds_dma16(a.row_exp + wave * 1024 + lane * 16, smem + kExpAt + wave * 1024);
    const lds_cptr bias_lane = opaque((lds_cptr)smem + kTableAt + 16 * g);
    const lds_cptr rs_nerf = opaque((lds_cptr)smem + kTableAt + kNerfMxScaleOff + 2 * n);
    const lds_cptr rs_lane = opaque((lds_cptr)smem + kExpAt + 2 * n);

    for (unsigned tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        // ---- inputs, gathered through the list: once per tile, kept for the style phase
        const unsigned i_wave = tile * C::SAMPLES_PER_WG + wave * C::SAMPLES_PER_WAVE;
        unsigned i = i_wave + n;
        const bool own = i < n_live;   // a live sample of this tile, not a clamped copy of the last one
        if (!own) i = n_live - 1;
        const unsigned sidx = a.live[i];   // dense sample index (< R N < 2^31)
        double pos[3];
        {
            const long long r = sidx / (unsigned)a.N;
            const double t = (double)(COMPACT ? a.ts_live[i] : a.ts[sidx]);
#pragma unroll
            for (int k = 0; k < 3; ++k) pos[k] = a.rays_o[r * 3 + k] + t * a.rays_d[r * 3 + k];
            // retire the loads before any LDS-DMA is issued (their wait would drain the whole prefetch)
#pragma unroll
            for (int k = 0; k < 3; ++k) asm volatile("" : "+v"(pos[k]));
        }
        const unsigned at = COMPACT ? i_wave + n : sidx;   // the column's place in a colour plane

        // ---- trunk phase.  Every wave must be done with the previous tile's last stream and with its last latent's bias table
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int j = 0; j < kNerfBiasBytes / (C::NWAVES * 1024); ++j)
            lds_dma16(a.nerf_bias + (j * C::NWAVES + wave) * 1024 + lane * 16, smem + kTableAt + (j * C::NWAVES + wave) * 1024);
        rt.ring.prologue();

        half8 Ph[2], Pl[2];
        {
            // (an opaque copy keeps the encoder's selectors inside the tile, as in styled_rays_multi_kernel)
            int g_enc = g;
            asm volatile("" : "+v"(g_enc));
            encode_point<true, true>(pos, g_enc, Ph, Pl, nullptr);
        }
        rt.template start<0, NQN>();
        {
            // the trunk (trunk_plane_mx_kernel: nerf_chain_mx's calls up to base_remap)
            MxAct<2> X, Y;
            MxAct<1> none;  // layer 0 has no activation input
            half8 l16[4];
            const half8 nop[1] = {};
            auto to_Y = [&](auto rt_, auto h_, const float4v& acc) { mx_store_act<decltype(rt_)::value, decltype(h_)::value>(acc, Y, l16); };
            auto to_X = [&](auto rt_, auto h_, const float4v& acc) { mx_store_act<decltype(rt_)::value, decltype(h_)::value>(acc, X, l16); };
            dense_mx<C, TN.first[0], NQN, 16, 0, 2, L::bias0(0)>(rt, bias_lane, rs_nerf, none, Ph, Pl, to_Y);
            dense_mx<C, TN.first[1], NQN, 16, 2, 0, L::bias0(1)>(rt, bias_lane, rs_nerf, Y, nop, nop, to_X);
            dense_mx<C, TN.first[2], NQN, 16, 2, 0, L::bias0(2)>(rt, bias_lane, rs_nerf, X, nop, nop, to_Y);
            dense_mx<C, TN.first[3], NQN, 16, 2, 0, L::bias0(3)>(rt, bias_lane, rs_nerf, Y, nop, nop, to_X);
            dense_mx<C, TN.first[4], NQN, 16, 2, 0, L::bias0(4)>(rt, bias_lane, rs_nerf, X, nop, nop, to_Y);
            // skip layer: k order [h | pe]
            dense_mx<C, TN.first[5], NQN, 16, 2, 2, L::bias0(5)>(rt, bias_lane, rs_nerf, Y, Ph, Pl, to_X);
            dense_mx<C, TN.first[6], NQN, 16, 2, 0, L::bias0(6)>(rt, bias_lane, rs_nerf, X, nop, nop, to_Y);
            dense_mx<C, TN.first[7], NQN, 16, 2, 0, L::bias0(7)>(rt, bias_lane, rs_nerf, Y, nop, nop, to_X);
            // sigma layer: one row tile, walked for its place in the stream; sigma came from the sigma pass
            dense_mx<C, TN.first[8], NQN, 1, 2, 0, L::bias0(8)>(rt, bias_lane, rs_nerf, X, nop, nop, [&](auto, auto h_, const float4v& acc) {
                if constexpr (decltype(h_)::value == 0) asm volatile("" ::"v"(acc[0]));
            });
            // base_remap: ReLU, hi / lo split, and out to the workgroup's tile of slab region B with every second row tile
            half8 Th, Tl;
            dense_mx<C, TN.first[9], NQN, 16, 2, 0, L::bias0(9)>(rt, bias_lane, rs_nerf, X, nop, nop, [&](auto rt_, auto h_, const float4v& acc) {
                constexpr int r = decltype(rt_)::value, hf = decltype(h_)::value;
                unsigned hpk, lpk;
                split_pair(acc[2 * hf], acc[2 * hf + 1], hpk, lpk);
                set_pair(Th, (r & 1) * 4 + 2 * hf, hpk);
                set_pair(Tl, (r & 1) * 4 + 2 * hf, lpk);
                if constexpr ((r & 1) && hf == 1) stash_store<CfgSlab>(remap, r / 2, 0, Th, Tl);
            });
        }

        // ---- style phase (the latent loop of restyle_trunk_mx_kernel, base_remap from slab region B)
        for (int k = 0; k < a.K; ++k) {
            // every wave must be done with the previous stream (the trunk's, or the latent's before), and with its table
            __builtin_amdgcn_s_barrier();
            {
                const char* table = a.folded + (size_t)k * kStylePairBiasBytes;
#pragma unroll
                for (int j = 0; j < kStylePairBiasBytes / (C::NWAVES * 1024); ++j)
                    lds_dma16(table + (j * C::NWAVES + wave) * 1024 + lane * 16, smem + kTableAt + (j * C::NWAVES + wave) * 1024);
            }
            rd.ring.prologue();
            rd.template start<0, NQ>();

            MxAct<2> X, Y;
            MxAct<1> none;   // concat layer 0 has no activation input
            half8 l16[4];
            const half8 nop[1] = {};
            auto to_Y = [&](auto rt_, auto h_, const float4v& acc) { mx_store_act<decltype(rt_)::value, decltype(h_)::value>(acc, Y, l16); };
            auto to_X = [&](auto rt_, auto h_, const float4v& acc) { mx_store_act<decltype(rt_)::value, decltype(h_)::value>(acc, X, l16); };

            // ---- concat MLP -> Y (concat_mlp_folded: [pe] / [h] x 3 / [h | pe])
            dense_mx<C, T.first[0], NQ, 16, 0, 2, 256 * 0>(rd, bias_lane, rs_lane, none, Ph, Pl, to_Y);
            dense_mx<C, T.first[1], NQ, 16, 2, 0, 256 * 1>(rd, bias_lane, rs_lane, Y, nop, nop, to_X);
            dense_mx<C, T.first[2], NQ, 16, 2, 0, 256 * 2>(rd, bias_lane, rs_lane, X, nop, nop, to_Y);
            dense_mx<C, T.first[3], NQ, 16, 2, 0, 256 * 3>(rd, bias_lane, rs_lane, Y, nop, nop, to_X);
            dense_mx<C, T.first[4], NQ, 16, 2, 2, 256 * 4>(rd, bias_lane, rs_lane, X, Ph, Pl, to_Y);

            // ---- style layer 0 on [remap (slab B) | concat_features (Y) | pe]; its row tiles stream to slab region A
            {
                MxAct<4> B;
                {
                    half8 Rh[8][1], Rl[8][1];
                    stash_load<CfgSlab>(remap, Rh, Rl);
                    mx_from_frags<0>(Rh, Rl, B);
                }
#pragma unroll
                for (int s = 0; s < 8; ++s) B.h[8 + s] = Y.h[s];
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) B.h6[2 + kb] = Y.h6[kb], B.l6[2 + kb] = Y.l6[kb], B.sc[2 + kb] = Y.sc[kb];
                half8 Th, Tl;
                dense_mx<C, T.first[5], NQ, 16, 4, 2, SB + style_bias0(0)>(
                    rd, bias_lane, rs_lane, B, Ph, Pl, [&](auto rt_, auto h_, const float4v& acc) {
                        constexpr int r = decltype(rt_)::value, hf = decltype(h_)::value;
                        unsigned hpk, lpk;
                        split_pair(acc[2 * hf], acc[2 * hf + 1], hpk, lpk);
                        set_pair(Th, (r & 1) * 4 + 2 * hf, hpk);
                        set_pair(Tl, (r & 1) * 4 + 2 * hf, lpk);
                        if constexpr ((r & 1) && hf == 1) stash_store<CfgSlab>(slab, r / 2, 0, Th, Tl);
                    });
            }
            {
                half8 Rh[8][1], Rl[8][1];
                stash_load<CfgSlab>(slab, Rh, Rl);
                mx_from_frags<0>(Rh, Rl, X);
            }

            // ---- style layers 1..7 -> rgb[k] at the column's place (style_tail_folded)
            dense_mx<C, T.first[6], NQ, 16, 2, 0, SB + style_bias0(1)>(rd, bias_lane, rs_lane, X, nop, nop, to_Y);
            dense_mx<C, T.first[7], NQ, 16, 2, 0, SB + style_bias0(2)>(rd, bias_lane, rs_lane, Y, nop, nop, to_X);
            dense_mx<C, T.first[8], NQ, 16, 2, 0, SB + style_bias0(3)>(rd, bias_lane, rs_lane, X, nop, nop, to_Y);
            dense_mx<C, T.first[9], NQ, 16, 2, 2, SB + style_bias0(4)>(rd, bias_lane, rs_lane, Y, Ph, Pl, to_X);
            dense_mx<C, T.first[10], NQ, 16, 2, 0, SB + style_bias0(5)>(rd, bias_lane, rs_lane, X, nop, nop, to_Y);
            dense_mx<C, T.first[11], NQ, 16, 2, 0, SB + style_bias0(6)>(rd, bias_lane, rs_lane, Y, nop, nop, to_X);
            float* rgb_k = a.rgb + (size_t)k * (size_t)a.M * 3;
            dense_mx<C, T.first[12], NQ, kStyleRT[7], 2, 0, SB + style_bias0(7)>(
                rd, bias_lane, rs_lane, X, nop, nop, [&](auto, auto h_, const float4v& acc) {
                    constexpr int hf = decltype(h_)::value;
                    if (g == 0 && own) {
#pragma unroll
                        for (int r = 2 * hf; r < (hf ? 3 : 2); ++r) rgb_k[(size_t)at * 3 + r] = 1.0f / (1.0f + expf(-acc[r]));
                    }
                });
        }
    }
}

// ------------------------------------------------------------------------------------------------ host
// (render.hip has checked sizes, handle kinds and precisions, and that the style handle has mx streams)
static ListMxArgs list_mx_args(const tgtc_net* nerf, const tgtc_net* style, const double* rays_o, const double* rays_d,
                               const void* folded, int K, int N, const uint32_t* live, float* rgb) {
    ListMxArgs a{};
    a.nerf_bias = nerf->dev, a.nerf_stream = nerf->dev + nerf->bias_bytes;
    a.concat_stream = style->mx->dev, a.style_stream = style->mx->dev + kStylePairMxStyleOff;
    a.row_exp = style->mx->dev + style->mx->exp_off;
    a.folded = static_cast<const char*>(folded);
    a.stash = style->dev + style->stash_off, a.stash2_delta = (long long)(style->stash2_off - style->stash_off);
    a.rays_o = rays_o, a.rays_d = rays_d, a.live = live, a.rgb = rgb;
    a.N = N, a.K = K;
    return a;
}

// rgb[k, live[i]] for the samples of a list whose length is a device word; the caller has zero-filled rgb.  The grid is sized
// for the dense plane and workgroups without a tile leave at once.
int styled_forward_list_folded_mx_impl(const tgtc_net* nerf, const tgtc_net* style, const double* rays_o, const double* rays_d,
                                       const float* ts, const void* folded, int K, int64_t R, int N, const uint32_t* live,
                                       const uint32_t* n_live, float* rgb, hipStream_t st) {
    ListMxArgs a = list_mx_args(nerf, style, rays_o, rays_d, folded, K, N, live, rgb);
    a.M = R * (int64_t)N, a.ts = ts, a.n_live = n_live;
    const long long tiles = (a.M + CfgMx::SAMPLES_PER_WG - 1) / CfgMx::SAMPLES_PER_WG;
    styled_list_mx_kernel<false><<<(unsigned)(tiles < style->n_wg ? tiles : style->n_wg), CfgMx::NWAVES * 64, 0, st>>>(a);
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

// rgb_live[k, i] for the `count` >= 1 entries of a cached list: the compact form, its grid sized from the host count
int styled_restyle_live_folded_mx_impl(const tgtc_net* nerf, const tgtc_net* style, const double* rays_o, const double* rays_d,
                                       const void* folded, int K, int64_t R, int N, const uint32_t* live, const float* ts_live,
                                       int64_t count, float* rgb_live, hipStream_t st) {
    (void)R;
    ListMxArgs a = list_mx_args(nerf, style, rays_o, rays_d, folded, K, N, live, rgb_live);
    a.M = count, a.ts_live = ts_live, a.count = (unsigned)count;
    const long long tiles = (count + CfgMx::SAMPLES_PER_WG - 1) / CfgMx::SAMPLES_PER_WG;
    styled_list_mx_kernel<true><<<(unsigned)(tiles < style->n_wg ? tiles : style->n_wg), CfgMx::NWAVES * 64, 0, st>>>(a);
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

}  // namespace tgtc
