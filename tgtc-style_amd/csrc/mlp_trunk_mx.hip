// The trunk plane from an fp16mx NeRF handle (tgtc_geometry_trunk_mx, render.hip), and the read-back of a plane
// (tgtc_geometry_trunk_read).
//
// trunk_plane_mx_kernel is the producer half of styled_rays_sparse_kernel<CfgExact, true, false, kPlaneBuild>
// (mlp_style_sparse.hip) on dense_mx (mlp_mx.h): the gather through the cached list (clamped past its end), o + t d in
// float64 and its encoding, the NeRF trunk -- layers 0-7, the sigma layer's groups (walked, result dropped: they lie in the
// stream between layer 7 and base_remap), base_remap_layer -- and base_remap's ReLU-ed hi / lo fp16 fragments stored to the
// tile's tile of an fp16x3 plane with the sibling's stash_store.  The ten dense_mx calls are those of nerf_chain_mx
// (mlp_nerf_mx_chain.h) in its HIP form, same template arguments but the group count the reader stops at, which only decides
// what is prefetched: a column's accumulators are the ones nerf_mx_kernel<*, true> hands to its remap callback.
//
// Launch shape: one workgroup per 128-entry tile, as nerf_mx_kernel (512 threads, two waves per SIMD; ring + table fill the
// CU's LDS, so one workgroup is resident per CU either way).  Nothing survives a tile: the bias / row-exponent table, the
// ring prologue and the reader start with the workgroup.
//
// DESIGN.md section 3.1 facts this kernel depends on: (a) dense_mx drains the MFMA pipe behind a layer's last
// v_mfma_scale_* before the final epilogue; (b) every LDS-DMA here is the asm flavour (TGTC_ASM_DMA: lds_dma16 for the
// table, the ring's own through MxReader); (c) the tile's gather is retired before the tile's first LDS-DMA.  The reader is
// walked to the last chunk of its cut (first[10] groups; the last boundary waits for the last chunk), so no LDS-DMA is in
// flight when the workgroup ends.
#define TGTC_ASM_DMA 1  // see mlp_core.h lds_dma16
#include "common.h"

#include "mlp_layouts.h"
#include "mlp_mx.h"
#include "mlp_nerf_mx_chain.h"
#include "mlp_pack.h"
#include "mlp_style_chain.h"

namespace tgtc {

using CfgMx = MlpCfg<8, 1, false, 4>;    // the geometry of nerf_mx_kernel (mlp_nerf_mx.hip)
using CfgSlab = MlpCfg<8, 1, true, 4>;   // the fp16x3 plane's: hi then lo per k-step (mlp_style_sparse.hip, CfgExact)
using CfgFast = MlpCfg<8, 2, false, 4>;  // the fp16 plane's: two column tiles per wave, hi only
static_assert(CfgMx::SAMPLES_PER_WG == CfgSlab::SAMPLES_PER_WG && CfgMx::NWAVES == CfgSlab::NWAVES, "one tile geometry");

struct TrunkMxArgs {
    const char* bias;        // the handle's bias / row-exponent table (kNerfBiasBytes)
    const char* stream;      // its group stream (kNerfMxTable)
    char* plane;             // ceil(count / 128) tiles of kStashBytesPerWG, every byte written
    const double* rays_o;
    const double* rays_d;
    const unsigned* live;    // [count] ascending sample indices
    const float* ts_live;    // [count] depths of the list's samples
    unsigned count;          // >= 1
    int N;
};

__global__ void __launch_bounds__(CfgMx::NWAVES * 64, CfgMx::NWAVES / 4) trunk_plane_mx_kernel(TrunkMxArgs a) {
    using C = CfgMx;
    using L = NerfLayout;
    constexpr const MxTable& T = kNerfMxTable;
    constexpr int NQ = T.first[10];                            // layers 0-7, sigma, base_remap
    constexpr int NUNITS = mx_bytes_upto(T, NQ) / 1024;
    // ring | biases + row exponents
    __shared__ __attribute__((aligned(16))) char smem[C::RING_BYTES + kNerfBiasBytes];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, n = lane & 15;
    const unsigned tile = blockIdx.x;                          // the grid is the tiles: tile * 128 < count

    // ---- 1. inputs, gathered through the list; a slot behind the list's end is the last live sample again and is stored
    //         like any other (every byte of the tile is written)
    double pos[3];
    {
        unsigned i = tile * C::SAMPLES_PER_WG + wave * C::SAMPLES_PER_WAVE + n;   // count < 2^31
        if (i >= a.count) i = a.count - 1;
        const long long r = a.live[i] / (unsigned)a.N;
        const double t = (double)a.ts_live[i];
#pragma unroll
        for (int k = 0; k < 3; ++k) pos[k] = a.rays_o[r * 3 + k] + t * a.rays_d[r * 3 + k];
        // retire the loads before any LDS-DMA is issued (their wait would drain the whole prefetch)
#pragma unroll
        for (int k = 0; k < 3; ++k) asm volatile("" : "+v"(pos[k]));
    }

    // ---- 2. bias / row-exponent table, then the first 8 chunks of the weight stream
    MxReader<C, SingleStreamMap<NUNITS>, kNerfMxTable> rd;
    const char* const streams[1] = {a.stream};
    rd.init(streams, smem, wave, lane);
#pragma unroll
    for (int j = 0; j < kNerfBiasBytes / (C::NWAVES * 1024); ++j)
        lds_dma16(a.bias + (j * C::NWAVES + wave) * 1024 + lane * 16, smem + C::RING_BYTES + (j * C::NWAVES + wave) * 1024);
    rd.ring.prologue();

    // ---- 3. positional encoding (the trunk does not see the direction)
    half8 Ph[2], Pl[2];
    encode_point<true, true>(pos, g, Ph, Pl, nullptr);

    const lds_cptr bias_lane = opaque((lds_cptr)smem + C::RING_BYTES + 16 * g);
    const lds_cptr rs_lane = opaque((lds_cptr)smem + C::RING_BYTES + kNerfMxScaleOff + 2 * n);
    rd.template start<0, NQ>();

    // ---- 4. the trunk (nerf_chain_mx's calls up to base_remap)
    MxAct<2> X, Y;
    MxAct<1> none;  // layer 0 has no activation input
    half8 l16[4];
    const half8 nop[1] = {};
    auto to_Y = [&](auto rt_, auto h_, const float4v& acc) { mx_store_act<decltype(rt_)::value, decltype(h_)::value>(acc, Y, l16); };
    auto to_X = [&](auto rt_, auto h_, const float4v& acc) { mx_store_act<decltype(rt_)::value, decltype(h_)::value>(acc, X, l16); };
    dense_mx<C, T.first[0], NQ, 16, 0, 2, L::bias0(0)>(rd, bias_lane, rs_lane, none, Ph, Pl, to_Y);
    dense_mx<C, T.first[1], NQ, 16, 2, 0, L::bias0(1)>(rd, bias_lane, rs_lane, Y, nop, nop, to_X);
    dense_mx<C, T.first[2], NQ, 16, 2, 0, L::bias0(2)>(rd, bias_lane, rs_lane, X, nop, nop, to_Y);
    dense_mx<C, T.first[3], NQ, 16, 2, 0, L::bias0(3)>(rd, bias_lane, rs_lane, Y, nop, nop, to_X);
    dense_mx<C, T.first[4], NQ, 16, 2, 0, L::bias0(4)>(rd, bias_lane, rs_lane, X, nop, nop, to_Y);
    // skip layer: k order [h | pe]
    dense_mx<C, T.first[5], NQ, 16, 2, 2, L::bias0(5)>(rd, bias_lane, rs_lane, Y, Ph, Pl, to_X);
    dense_mx<C, T.first[6], NQ, 16, 2, 0, L::bias0(6)>(rd, bias_lane, rs_lane, X, nop, nop, to_Y);
    dense_mx<C, T.first[7], NQ, 16, 2, 0, L::bias0(7)>(rd, bias_lane, rs_lane, Y, nop, nop, to_X);
    // sigma layer: one row tile, walked for its place in the stream; sigma came from the sigma pass
    dense_mx<C, T.first[8], NQ, 1, 2, 0, L::bias0(8)>(rd, bias_lane, rs_lane, X, nop, nop, [&](auto, auto h_, const float4v& acc) {
        if constexpr (decltype(h_)::value == 0) asm volatile("" ::"v"(acc[0]));
    });
    // base_remap: ReLU, hi / lo split, and out with every second row tile -- k-step ks = rt / 2 of the consumers' operand:
    // this lane's fragment holds features 32 ks + 16 (e >> 2) + 4 g + (e & 3), e = 0..7, of list entry tile * 128 + wave * 16 + n
    // (act_col; mx_from_frags in mlp_style_mx.hip is the way back).  The tile's byte offset is 64-bit: a frame's plane passes
    // 2^32 bytes.
    {
        char* remap = a.plane + (size_t)tile * kStashBytesPerWG + (size_t)tid * 16;
        half8 Th, Tl;
        dense_mx<C, T.first[9], NQ, 16, 2, 0, L::bias0(9)>(rd, bias_lane, rs_lane, X, nop, nop, [&](auto rt_, auto h_, const float4v& acc) {
            constexpr int rt = decltype(rt_)::value, hf = decltype(h_)::value;
            unsigned hpk, lpk;
            split_pair(acc[2 * hf], acc[2 * hf + 1], hpk, lpk);
            set_pair(Th, (rt & 1) * 4 + 2 * hf, hpk);
            set_pair(Tl, (rt & 1) * 4 + 2 * hf, lpk);
            if constexpr ((rt & 1) && hf == 1) stash_store<CfgSlab>(remap, rt / 2, 0, Th, Tl);
        });
    }
}

// base_remap[i, f] of a plane, as floats: one workgroup per list entry, one thread per feature.  This is the plane's layout
// said once in code: tile = i / S (S = 128 entries in fp16x3, 256 in fp16); inside the tile, wave = (i % S) / (16 NCT), column
// tile c = (i % S) / 16 % NCT, column n = i % 16; feature f = 32 ks + 16 eh + 4 g + el lies in k-step ks, element e = 4 eh + el of
// the fragment of lane 16 g + n; fragment (ks, c, part p) of thread tid = 64 wave + lane starts at byte
// ((ks * NCT + c) * P + p) * 8192 + tid * 16 of the tile (P = 2 parts, hi then lo, in fp16x3; P = 1 in fp16).
template <class C>
__global__ void __launch_bounds__(256) trunk_plane_read_kernel(const char* plane, float* hi, float* lo) {
    constexpr int P = C::SPLIT ? 2 : 1;
    const size_t i = blockIdx.x;
    const int f = threadIdx.x;
    const int in_tile = (int)(i % C::SAMPLES_PER_WG);
    const int wave = in_tile / C::SAMPLES_PER_WAVE, c = in_tile / 16 % C::NCT, n = in_tile % 16;
    const int ks = f / 32, eh = f / 16 % 2, g = f / 4 % 4, el = f % 4;
    const int tid = wave * 64 + 16 * g + n;
    const char* frag = plane + (i / C::SAMPLES_PER_WG) * (size_t)kStashBytesPerWG + (size_t)((ks * C::NCT + c) * P) * 8192 +
                       (size_t)tid * 16 + (4 * eh + el) * 2;
    hi[i * 256 + f] = (float)*reinterpret_cast<const half_t*>(frag);
    if (C::SPLIT && lo) lo[i * 256 + f] = (float)*reinterpret_cast<const half_t*>(frag + 8192);
}

// ------------------------------------------------------------------------------------------------ host
// tgtc_geometry_trunk_mx (render.hip; count >= 1, sizes, the handle's kind and precision are checked there)
int styled_trunk_plane_mx_impl(const tgtc_net* nerf, const double* rays_o, const double* rays_d, int64_t R, int N,
                               const uint32_t* live, const float* ts_live, int64_t count, void* plane, hipStream_t st) {
    (void)R;
    TrunkMxArgs a{};
    a.bias = nerf->dev, a.stream = nerf->dev + nerf->bias_bytes;
    a.plane = static_cast<char*>(plane);
    a.rays_o = rays_o, a.rays_d = rays_d, a.live = live, a.ts_live = ts_live;
    a.count = (unsigned)count, a.N = N;
    const long long tiles = (count + CfgMx::SAMPLES_PER_WG - 1) / CfgMx::SAMPLES_PER_WG;
    trunk_plane_mx_kernel<<<(unsigned)tiles, CfgMx::NWAVES * 64, 0, st>>>(a);
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

// tgtc_geometry_trunk_read (render.hip; count >= 1 and the plane's size are checked there)
int trunk_plane_read_impl(bool fp16, const void* plane, int64_t count, float* hi, float* lo, hipStream_t st) {
    if (fp16) trunk_plane_read_kernel<CfgFast><<<(unsigned)count, 256, 0, st>>>(static_cast<const char*>(plane), hi, nullptr);
    else trunk_plane_read_kernel<CfgSlab><<<(unsigned)count, 256, 0, st>>>(static_cast<const char*>(plane), hi, lo);
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

}  // namespace tgtc
