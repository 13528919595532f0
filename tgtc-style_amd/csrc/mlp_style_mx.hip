// The folded plane consumer with the style networks in fp16mx (tgtc_restyle_rays_trunk_folded_mx, render.hip): the concat MLP
// and the style MLP of styled_rays_sparse_kernel<CfgExact, true, true, kPlaneRead> (mlp_style_sparse.hip) on dense_mx
// (mlp_mx.h) -- per 128-deep block four fp16 MFMAs and two block-scaled e2m3 MFMAs instead of twelve fp16 MFMAs; the
// encoding k-steps keep their three fp16 products.
//
// Shared with the sibling, as source text or as the same expression: 8 waves, one column tile per wave, 128 list entries per
// workgroup tile; the gather through the list (clamped past its end, `own` masking every store), o + t d and its float64
// encoding; the fp16x3 plane and its addressing (read with the sibling's stash_load); the latent loop with latent k's bias
// table swapped in place behind the barrier that opens the iteration; style layer 0's row tiles streamed to slab region A
// and reloaded; rgb[k, i] at the LIST position, through the same sigmoid.
// Its own: the group streams of tgtc_style_enable_mx (kStylePairMxTable: one table, two stream segments) through an MxReader on
// the draining ring; the row-exponent table in LDS behind the bias table, loaded once per workgroup (it does not depend on
// the latent); and the e2m3 blocks of the two operand sets that come out of memory, not out of an accumulator -- base_remap
// (the plane) and style layer 0's output (the slab): their hi fragments are the fp16 operand and the source of Ah6, their lo
// fragments the source of Al6, block exponents from the running maximum of the hi values as in mx_store_act.  That
// conversion runs once per LATENT, like the sibling's plane reload: a third MxAct<2> kept over the concat MLP would put 59 more
// registers beside the two live sets (177 + encodings 16 + reader 28 + staging 16 + accumulators of 256), and the four
// conversions cost ~400 of a latent's ~60 000 cycles.
// Style layer 0 holds [remap | concat_features] as one MxAct<4> (117 registers) and produces into half8 pairs that leave for
// the slab with every second row tile, so the third operand set never exists in registers.
//
// DESIGN.md section 3.1 facts this kernel depends on: (a) dense_mx drains the MFMA pipe behind a layer's last
// v_mfma_scale_* before the final epilogue; (b) every LDS-DMA here is the asm flavour (TGTC_ASM_DMA: lds_dma16 for the three
// tables, the ring's own through MxReader) -- one compiler-visible global_load_lds would turn every counted lgkmcnt wait into a
// full one; (c) the tile's gather is retired before the tile's first LDS-DMA.
#define TGTC_ASM_DMA 1  // see mlp_core.h lds_dma16
#include "mlp_style_mx.h"

#include "mlp_layouts.h"
#include "mlp_mx.h"
#include "mlp_mx_pack.h"
#include "mlp_style_chain.h"

namespace tgtc {

using CfgMx = MlpCfg<8, 1, false, 4>;    // the geometry of nerf_mx_kernel (mlp_nerf_mx.hip)
using CfgSlab = MlpCfg<8, 1, true, 4>;   // the fp16x3 consumer's: layout of the plane and of the slab (hi then lo per k-step)
static_assert(CfgMx::SAMPLES_PER_WG == CfgSlab::SAMPLES_PER_WG && CfgMx::NWAVES == CfgSlab::NWAVES, "one tile geometry");

struct StyleMxArgs {
    const char* concat_stream;   // segment 0 of kStylePairMxTable
    const char* style_stream;    // segment 1
    const char* row_exp;         // kStylePairMxExpBytes
    const char* folded;          // [K] pair bias tables of kStylePairBiasBytes (tgtc_style_fold_latents)
    char* stash;                 // slab region A: gridDim.x * kStashBytesPerWG
    const char* plane;           // ceil(count / 128) tiles of kStashBytesPerWG, base_remap as fp16x3 operand fragments
    const double* rays_o;
    const double* rays_d;
    const unsigned* live;        // [count] ascending sample indices
    const float* ts_live;        // [count] depths of the list's samples
    float* rgb;                  // [K,count,3], every entry written
    unsigned count;
    int N;
    int K;
};

// (StylePairMxMap and mx_from_frags, shared with styled_list_mx_kernel of mlp_list_mx.hip, are in mlp_mx.h)
__global__ void __launch_bounds__(CfgMx::NWAVES * 64, CfgMx::NWAVES / 4) restyle_trunk_mx_kernel(StyleMxArgs a) {
    using C = CfgMx;
    constexpr const MxTable& T = kStylePairMxTable;
    constexpr int NQ = T.n;
    constexpr int kBiasAt = kRingBytes, kExpAt = kRingBytes + kStylePairBiasBytes;
    constexpr int SB = kConcatBiasFloats;   // the style MLP's biases (and row exponents) lie behind the concat MLP's
    // ring | pair bias table (latent k's) | row exponents
    __shared__ __attribute__((aligned(16))) char smem[kExpAt + kStylePairMxExpBytes];

    // a workgroup without a tile leaves before any LDS-DMA is issued (none may be in flight when it ends)
    const unsigned n_live = a.count;
    const unsigned n_tiles = (n_live + C::SAMPLES_PER_WG - 1) / C::SAMPLES_PER_WG;   // n_live < 2^31
    if (blockIdx.x >= n_tiles) return;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, n = lane & 15;
    char* slab = a.stash + (size_t)blockIdx.x * kStashBytesPerWG + (size_t)tid * 16;

    MxReader<C, StylePairMxMap, kStylePairMxTable> rd;
    const char* const streams[2] = {a.concat_stream, a.style_stream};
    rd.init(streams, smem, wave, lane);
    // tables: requested before the first ring prologue, so that stream's first counted wait and ring barrier cover them
    static_assert(kStylePairMxExpBytes == C::NWAVES * 1024, "one LDS-DMA per wave");
    lds_dma16(a.row_exp + wave * 1024 + lane * 16, smem + kExpAt + wave * 1024);
#pragma unroll
    for (int j = 0; j < kStylePairBiasBytes / (C::NWAVES * 1024); ++j)
        lds_dma16(a.folded + (j * C::NWAVES + wave) * 1024 + lane * 16, smem + kBiasAt + (j * C::NWAVES + wave) * 1024);
    const lds_cptr bias_lane = opaque((lds_cptr)smem + kBiasAt + 16 * g);
    const lds_cptr rs_lane = opaque((lds_cptr)smem + kExpAt + 2 * n);

    for (unsigned tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        // ---- inputs, gathered through the list
        const unsigned i_wave = tile * C::SAMPLES_PER_WG + wave * C::SAMPLES_PER_WAVE;
        unsigned i = i_wave + n;
        const bool own = i < n_live;   // a live sample of this tile, not a clamped copy of the last one
        if (!own) i = n_live - 1;
        double pos[3];
        {
            const long long r = a.live[i] / (unsigned)a.N;
            const double t = (double)a.ts_live[i];
#pragma unroll
            for (int k = 0; k < 3; ++k) pos[k] = a.rays_o[r * 3 + k] + t * a.rays_d[r * 3 + k];
            // retire the loads before any LDS-DMA is issued (their wait would drain the whole prefetch)
#pragma unroll
            for (int k = 0; k < 3; ++k) asm volatile("" : "+v"(pos[k]));
        }
        half8 Ph[2], Pl[2];
        {
            // (an opaque copy keeps the encoder's selectors inside the tile, as in styled_rays_multi_kernel)
            int g_enc = g;
            asm volatile("" : "+v"(g_enc));
            encode_point<true, true>(pos, g_enc, Ph, Pl, nullptr);
        }
        // this lane's 16-byte column of the tile's base_remap (64-bit: a frame's plane passes 2^32 bytes)
        char* remap = const_cast<char*>(a.plane) + (size_t)tile * kStashBytesPerWG + (size_t)tid * 16;

        for (int k = 0; k < a.K; ++k) {
            // every wave must be done with the previous stream (of the latent or the tile before), and with its bias table
            __builtin_amdgcn_s_barrier();
            if (a.K > 1) {
                const char* table = a.folded + (size_t)k * kStylePairBiasBytes;
#pragma unroll
                for (int j = 0; j < kStylePairBiasBytes / (C::NWAVES * 1024); ++j)
                    lds_dma16(table + (j * C::NWAVES + wave) * 1024 + lane * 16, smem + kBiasAt + (j * C::NWAVES + wave) * 1024);
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

            // ---- style layer 0 on [remap (plane) | concat_features (Y) | pe]; its row tiles stream to slab region A
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
                        constexpr int rt = decltype(rt_)::value, hf = decltype(h_)::value;
                        unsigned hpk, lpk;
                        split_pair(acc[2 * hf], acc[2 * hf + 1], hpk, lpk);
                        set_pair(Th, (rt & 1) * 4 + 2 * hf, hpk);
                        set_pair(Tl, (rt & 1) * 4 + 2 * hf, lpk);
                        if constexpr ((rt & 1) && hf == 1) stash_store<CfgSlab>(slab, rt / 2, 0, Th, Tl);
                    });
            }
            {
                half8 Rh[8][1], Rl[8][1];
                stash_load<CfgSlab>(slab, Rh, Rl);
                mx_from_frags<0>(Rh, Rl, X);
            }

            // ---- style layers 1..7 -> rgb[k] at the column's list position (style_tail_folded)
            dense_mx<C, T.first[6], NQ, 16, 2, 0, SB + style_bias0(1)>(rd, bias_lane, rs_lane, X, nop, nop, to_Y);
            dense_mx<C, T.first[7], NQ, 16, 2, 0, SB + style_bias0(2)>(rd, bias_lane, rs_lane, Y, nop, nop, to_X);
            dense_mx<C, T.first[8], NQ, 16, 2, 0, SB + style_bias0(3)>(rd, bias_lane, rs_lane, X, nop, nop, to_Y);
            dense_mx<C, T.first[9], NQ, 16, 2, 2, SB + style_bias0(4)>(rd, bias_lane, rs_lane, Y, Ph, Pl, to_X);
            dense_mx<C, T.first[10], NQ, 16, 2, 0, SB + style_bias0(5)>(rd, bias_lane, rs_lane, X, nop, nop, to_Y);
            dense_mx<C, T.first[11], NQ, 16, 2, 0, SB + style_bias0(6)>(rd, bias_lane, rs_lane, Y, nop, nop, to_X);
            float* rgb_k = a.rgb + (size_t)k * a.count * 3;
            dense_mx<C, T.first[12], NQ, kStyleRT[7], 2, 0, SB + style_bias0(7)>(
                rd, bias_lane, rs_lane, X, nop, nop, [&](auto, auto h_, const float4v& acc) {
                    constexpr int hf = decltype(h_)::value;
                    if (g == 0 && own) {
#pragma unroll
                        for (int r = 2 * hf; r < (hf ? 3 : 2); ++r) rgb_k[(size_t)(i_wave + n) * 3 + r] = 1.0f / (1.0f + expf(-acc[r]));
                    }
                });
        }
    }
}

// ------------------------------------------------------------------------------------------------ host
int style_mx_pack(const std::vector<LayerSpec>& concat, const std::vector<LayerSpec>& style, std::vector<char>& stream,
                  std::vector<char>& row_exp) {
    const MxTable& T = kStylePairMxTable;
    if (concat.size() != 5 || style.size() != 8) return fail(TGTC_ERR_UNSUPPORTED, "style_enable_mx: expected 5 + 8 layers");
    stream.assign((size_t)T.bytes, 0);
    row_exp.assign(kStylePairMxExpBytes, 0);
    int qi = 0;
    for (int l = 0; l < 13; ++l) {
        // row exponents at the layer's place in the pair bias table; the biases themselves are the folded tables'
        const int b0 = l < 5 ? 256 * l : kConcatBiasFloats + style_bias0(l - 5);
        if (qi != T.first[l] || !mx_pack_layer(l < 5 ? concat[l] : style[l - 5], kStylePairMxShape[l], T, qi, b0, stream.data(),
                                               reinterpret_cast<unsigned short*>(row_exp.data()), nullptr))
            return fail(TGTC_ERR_UNSUPPORTED, "style_enable_mx: internal fp16+fp6 layout mismatch at layer %d", l);
    }
    if (qi != T.n) return fail(TGTC_ERR_UNSUPPORTED, "style_enable_mx: internal fp16+fp6 group count mismatch");
    return TGTC_OK;
}

int styled_restyle_plane_mx_impl(const tgtc_net* style, const double* rays_o, const double* rays_d, const void* folded, int K,
                                 int64_t R, int N, const uint32_t* live, const float* ts_live, int64_t count, const void* plane,
                                 float* rgb_live, hipStream_t st) {
    (void)R;
    StyleMxArgs a{};
    a.concat_stream = style->mx->dev, a.style_stream = style->mx->dev + kStylePairMxStyleOff;
    a.row_exp = style->mx->dev + style->mx->exp_off;
    a.folded = static_cast<const char*>(folded);
    a.stash = style->dev + style->stash_off;
    a.plane = static_cast<const char*>(plane);
    a.rays_o = rays_o, a.rays_d = rays_d, a.live = live, a.ts_live = ts_live, a.rgb = rgb_live;
    a.count = (unsigned)count, a.N = N, a.K = K;
    const long long tiles = (count + CfgMx::SAMPLES_PER_WG - 1) / CfgMx::SAMPLES_PER_WG;
    restyle_trunk_mx_kernel<<<(unsigned)(tiles < style->n_wg ? tiles : style->n_wg), CfgMx::NWAVES * 64, 0, st>>>(a);
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

}  // namespace tgtc
