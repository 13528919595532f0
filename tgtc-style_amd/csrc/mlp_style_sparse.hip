// Stylised path over a compact list of samples: the style networks only where the compositing weight can matter.
//
// In the stylised chain sigma depends on the ray alone, so the compositing weight w = alpha * T of every fine sample is
// known before any style network has run (tgtc_render_rays_styled_sparse, render.hip: sigma pass -> tgtc_composite weights).
// A sample with w == 0 enters rgb = sum w * c as exactly +0 whatever finite colour the style MLP would give it.
//
//   compact_count_kernel / compact_write_kernel   live[] = ascending sample indices s = r * N + i with w[s] > min_weight,
//                                                 n_live, both on the device; deterministic (no atomics): kCompactParts
//                                                 contiguous ranges are counted, then each range writes behind the sum of
//                                                 the counts in front of it, lanes in order through ballots.
//   styled_rays_sparse_kernel                     styled_rays_multi_kernel (mlp_style_multi.hip) with its samples gathered
//                                                 through the list: tile t owns live[t * SAMPLES_PER_WG ...], past the end
//                                                 clamped to the last live sample; r, ts[s], z[k,r] follow from the sample
//                                                 index as there; rgb[k,s] is scattered to its dense position (the caller
//                                                 zero-fills the planes); sigma is not written.  The number of tiles comes
//                                                 from n_live read on the device.
//   styled_rays_sparse_kernel<C, true>            the COMPACT form of the same body (tgtc_restyle_rays, render.hip): the list,
//                                                 the depth of every list entry (ts_live[i] = ts[live[i]]) and the list's
//                                                 length (a host value) come from a geometry cache; rgb[k,i] goes to the
//                                                 compact plane [K,count,3] at the sample's LIST position.  No dense plane is
//                                                 read or written.  Everything else -- r = live[i] / N, z[k,r], o + t d, the
//                                                 MFMA sequence, the clamped columns masked from every store -- is shared
//                                                 source, so a live sample has the bits it has in the scattered form.
//   styled_rays_sparse_kernel<C, COMPACT, true>   the FOLD form of either (tgtc_render_rays_styled_sparse_folded,
//                                                 tgtc_restyle_rays_folded): K latents that are the same for every sample.
//                                                 Their k-step in each of the 13 style layers is a per-latent bias table
//                                                 (tgtc_style_fold_latents, mlp_style.hip); the kernel walks the handle's
//                                                 streams packed without that k-step and swaps latent k's table into the
//                                                 LDS bias region at the top of each latent iteration.  With z = 0 the
//                                                 bits of the unfolded form with a zero latent.
//   styled_rays_sparse_kernel<C, true, false, kPlaneBuild>   the trunk PRODUCER (tgtc_geometry_trunk): the compact form's
//                                                 gather, encoding and NeRF trunk, with base_remap's operand fragments
//                                                 stored to the caller's trunk plane (one kStashBytesPerWG tile per tile of
//                                                 the list) instead of slab region B.  No style stream, no latent, no rgb.
//   styled_rays_sparse_kernel<C, true, FOLD, kPlaneRead>     the plane CONSUMER (tgtc_restyle_rays_trunk[_folded]): the compact
//                                                 form without its trunk -- no NeRF stream, no NeRF bias table -- reading
//                                                 the tile's fragments from the plane where the others read slab region B.
//                                                 The values make the same half8 round trip through memory, so the bits
//                                                 of the compact form on the same list.
//
// Per latent this is the MFMA sequence of styled_rays_multi_kernel on the same operands, and a column (sample) of an MFMA
// does not depend on the other columns of its tile, so a live sample carries the bits of the dense kernels.
#include "mlp_core.h"
#include "mlp_layouts.h"
#include "mlp_pack.h"
#include "mlp_style_chain.h"

namespace tgtc {

struct StyledSparseArgs {
    const char* nerf_bias;
    const char* nerf_stream;
    const char* pair_bias;
    const char* concat_stream;
    const char* style_stream;
    char* stash;             // region A: gridDim.x * kStashBytesPerWG
    long long stash2_delta;  // region B of a workgroup lies this many bytes behind its region A
    long long M;             // samples per colour plane: R * N (scattered form), the list's length (compact form)
    long long R;
    int N;
    int K;
    const double* rays_o;
    const double* rays_d;
    const float* ts;           // [R,N]; the compact form reads ts_live instead
    const float* z;            // [K,R,32]
    const unsigned* live;      // [n_live] ascending sample indices
    const unsigned* n_live;    // device scalar; the compact form takes `count`
    float* rgb;                // [K,R,N,3], zero-filled by the caller; compact form: [K,count,3], every entry written
    const float* ts_live;      // compact form: [count] depths of the list's samples
    unsigned count;            // compact form: the list's length
    const char* folded;        // folded forms: [K] pair bias tables of kStylePairBiasBytes (tgtc_style_fold_latents); z is not read
    char* plane;               // plane forms: ceil(count / SAMPLES_PER_WG) tiles of kStashBytesPerWG, base_remap in the slab's layout
};

// PLANE: where base_remap of a tile lives between the trunk and the latents.
constexpr int kPlaneNone = 0;   // slab region B of the style handle, written and read by the same launch
constexpr int kPlaneBuild = 1;  // the trunk alone, written to a.plane
constexpr int kPlaneRead = 2;   // no trunk, read from a.plane

// concat | style, both chunk aligned (as PairMap of mlp_style_multi.hip)
template <class C>
struct SparsePairMap {
    static constexpr int F_CONCAT = 0;
    static constexpr int F_STYLE = kConcatFrags;
    static constexpr int NFRAG = F_STYLE + kStyleFrags;
    static constexpr int NSEG = 2;
    static constexpr int chunk0(int i) { return i == 0 ? 0 : i == 1 ? F_STYLE / C::FPC : (1 << 30); }
    static_assert(kConcatFrags % C::FPC == 0, "concat stream must end on a chunk boundary");
};
// the same over the streams packed without the latent k-steps
template <class C>
struct SparsePairFoldMap {
    static constexpr int F_CONCAT = 0;
    static constexpr int F_STYLE = kConcatFoldFrags;
    static constexpr int NFRAG = F_STYLE + kStyleFoldFrags;
    static constexpr int NSEG = 2;
    static constexpr int chunk0(int i) { return i == 0 ? 0 : i == 1 ? F_STYLE / C::FPC : (1 << 30); }
    static_assert(kConcatFoldFrags % C::FPC == 0, "concat stream must end on a chunk boundary");
};

// FOLD: the latents are constant over the launch.  a.z is not read and no latent operand exists; a.concat_stream /
// a.style_stream are the handle's streams without the latent k-steps, and latent k's bias table a.folded[k] takes the place
// of the handle's pair bias table in LDS.  The LDS has room for one table (ring + NeRF bias + pair bias = 160 KiB), so with
// K > 1 table k is brought into the same region at the top of every latent iteration:
//   * behind the barrier that opens the iteration -- every wave has then finished the last bias read (style layer 7) of
//     the latent before, and of the tile before;
//   * in front of ws.prologue()'s chunk requests -- vmcnt retires loads in issue order, so every counted wait behind them
//     (start_ring: chunks 0 and 1 landed) finds the table's two requests landed as well, with the counts unchanged, and
//     the barrier of start_ring makes all waves' pieces visible before the first bias read of the concat MLP.
// With K = 1 the table loaded at the kernel's start stays.
//
// PLANE (compact form only): kPlaneBuild stops behind base_remap, which goes to tile `tile` of a.plane; kPlaneRead starts
// behind it and loads the tile from a.plane.  A plane tile is slab region B's bytes at another base: thread tid owns the 16
// bytes at tile * kStashBytesPerWG + ((ks * NCT + c) * P + p) * 8192 + tid * 16 (P = 2 parts, hi then lo, in split mode).  The
// tile's byte offset is 64-bit: a frame's plane passes 2^32 bytes.  Every column is stored, the clamped ones (copies of the
// last live sample) included, so a build writes every byte of every tile.
//   * kPlaneRead has no trunk stream to take the ring's lane addresses from: ws is initialised on its own (the same values).
//   * Its pair bias table is requested before the first ws.prologue(), so that stream's first counted wait and ring barrier
//     cover it as the trunk's did.
//   * Both forms end on a stream that has been walked to its last chunk: no LDS-DMA is in flight when a workgroup ends.
template <class C, bool COMPACT, bool FOLD = false, int PLANE = kPlaneNone>
__global__ void __launch_bounds__(C::NWAVES * 64, C::NWAVES / 4) styled_rays_sparse_kernel(StyledSparseArgs a) {
    static_assert(PLANE == kPlaneNone || COMPACT, "the plane belongs to a cached list");
    static_assert(PLANE != kPlaneBuild || !FOLD, "the trunk sees no latent");
    constexpr bool TRUNK = PLANE != kPlaneRead;    // the tile runs the NeRF trunk
    constexpr bool STYLE = PLANE != kPlaneBuild;   // ... and the style networks
    constexpr int NCT = C::NCT;
    constexpr bool SPLIT = C::SPLIT;
    using Map = std::conditional_t<FOLD, SparsePairFoldMap<C>, SparsePairMap<C>>;
    using L = NerfLayout;
    constexpr int kPairBiasAt = kRingBytes + (TRUNK ? kNerfBiasBytes : 0);
    __shared__ __attribute__((aligned(16))) char smem[kPairBiasAt + (STYLE ? kStylePairBiasBytes : 0)];

    // the list's length decides the tiles; a workgroup without one leaves before any LDS-DMA is issued (none may be in
    // flight when it ends), which is also what keeps live[n_live - 1] from being read when nothing is live
    unsigned n_live;
    if constexpr (COMPACT) n_live = a.count;
    else n_live = *a.n_live;
    const unsigned n_tiles = (n_live + C::SAMPLES_PER_WG - 1) / C::SAMPLES_PER_WG;   // n_live < 2^31
    if (blockIdx.x >= n_tiles) return;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, n = lane & 15;
    // this lane's 16-byte column of slab region A (the trunk producer has no style handle and no slab)
    char* slab = STYLE ? a.stash + (size_t)blockIdx.x * kStashBytesPerWG + (size_t)tid * 16 : nullptr;
    // ... and of the tile's base_remap: slab region B, or the tile's own tile of the plane
    auto remap_at = [&](unsigned tile) -> char* {
        if constexpr (PLANE == kPlaneNone) return slab + a.stash2_delta;
        else return a.plane + (size_t)tile * kStashBytesPerWG + (size_t)tid * 16;
    };

    WeightStream<C, SingleStreamMap<kTrunkFrags>> wt;
    WeightStream<C, Map> ws;
    if constexpr (TRUNK) {
        const char* const trunk_streams[1] = {a.nerf_stream};
        wt.init(trunk_streams, smem, wave, lane);
    }
    if constexpr (STYLE && TRUNK) {
        ws.src[0] = ws.lane_src(a.concat_stream, wave, lane);
        ws.src[1] = ws.lane_src(a.style_stream, wave, lane);
        ws.voff = wt.voff, ws.lds_wave = wt.lds_wave, ws.lane_lo = wt.lane_lo, ws.lane_hi = wt.lane_hi;
    } else if constexpr (STYLE) {
        const char* const pair_streams[2] = {a.concat_stream, a.style_stream};
        ws.init(pair_streams, smem, wave, lane);
    }
    // bias tables: loaded once per workgroup (LDS-DMA), visible after the first ring barrier
    if constexpr (TRUNK) {
#pragma unroll
        for (int j = 0; j < kNerfBiasBytes / (C::NWAVES * 1024); ++j)
            __builtin_amdgcn_global_load_lds(TGTC_GPTR(a.nerf_bias + (j * C::NWAVES + wave) * 1024 + lane * 16),
                                             TGTC_LPTR(smem + kRingBytes + (j * C::NWAVES + wave) * 1024), 16, 0, 0);
    }
    if constexpr (STYLE) {
        const char* const first_table = FOLD ? a.folded : a.pair_bias;
#pragma unroll
        for (int j = 0; j < kStylePairBiasBytes / (C::NWAVES * 1024); ++j)
            __builtin_amdgcn_global_load_lds(TGTC_GPTR(first_table + (j * C::NWAVES + wave) * 1024 + lane * 16),
                                             TGTC_LPTR(smem + kPairBiasAt + (j * C::NWAVES + wave) * 1024), 16, 0, 0);
    }
    const lds_cptr nerf_bias = opaque((lds_cptr)smem + kRingBytes + 16 * g);
    const lds_cptr pair_bias = opaque((lds_cptr)smem + kPairBiasAt + 16 * g);

    for (unsigned tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        // ---- inputs, gathered through the list
        const unsigned i_wave = tile * C::SAMPLES_PER_WG + wave * C::SAMPLES_PER_WAVE;
        double pos[NCT][3];
        unsigned sidx[NCT];     // dense sample index (< M < 2^31) of the column, clamped to the last live sample
        unsigned own = 0;       // bit c: column c is a live sample of this tile (not a clamped copy)
#pragma unroll
        for (int c = 0; c < NCT; ++c) {
            unsigned i = i_wave + c * 16 + n;
            if (i < n_live) own |= 1u << c;
            else i = n_live - 1;
            const unsigned s = a.live[i];
            sidx[c] = s;
            const long long r = s / (unsigned)a.N;
            const double t = (double)(COMPACT ? a.ts_live[i] : a.ts[s]);
#pragma unroll
            for (int k = 0; k < 3; ++k) pos[c][k] = a.rays_o[r * 3 + k] + t * a.rays_d[r * 3 + k];
            // retire the loads before any LDS-DMA is issued (their wait would drain the whole prefetch)
#pragma unroll
            for (int k = 0; k < 3; ++k) asm volatile("" : "+v"(pos[c][k]));
        }
        // previous tile: every wave must be done with the ring before it is refilled (without a trunk the barrier that opens
        // the first latent iteration is that barrier)
        if constexpr (TRUNK) {
            __builtin_amdgcn_s_barrier();
            wt.prologue();
        }

        half8 pe_h[2][NCT], pe_l[2][NCT];
        // (an opaque copy keeps the encoder's selectors inside the tile, as in styled_rays_multi_kernel)
        int g_enc = g;
        asm volatile("" : "+v"(g_enc));
#pragma unroll
        for (int c = 0; c < NCT; ++c) {
            half8 h2[2], l2[2];
            encode_point<SPLIT, SPLIT>(pos[c], g_enc, h2, l2, nullptr);
            pe_h[0][c] = h2[0], pe_h[1][c] = h2[1], pe_l[0][c] = l2[0], pe_l[1][c] = l2[1];
        }
        if constexpr (TRUNK) wt.start();

        half8 Xh[8][NCT], Xl[8][NCT], Yh[8][NCT], Yl[8][NCT];
        auto to_Y = [&](auto rt_, auto c_, auto h_, const float4v& acc) {
            constexpr int rt = decltype(rt_)::value, c = decltype(c_)::value;
            store_act<C, rt, decltype(h_)::value>(acc, Yh[rt / 2][c], Yl[rt / 2][c]);
        };
        auto to_X = [&](auto rt_, auto c_, auto h_, const float4v& acc) {
            constexpr int rt = decltype(rt_)::value, c = decltype(c_)::value;
            store_act<C, rt, decltype(h_)::value>(acc, Xh[rt / 2][c], Xl[rt / 2][c]);
        };
        if constexpr (TRUNK) {
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
        // sigma_layer: its fragments lie in the stream between layer 7's and base_remap's, so the layer is walked as in
        // styled_rays_multi_kernel (same windows, same ring timing); sigma came from the sigma pass and is not written again
        dense_layer<C, L::frag0(8), 8, 1, L::bias0(8)>(wt, nerf_bias, Xh, Xl, [&](auto, auto, auto h_, const float4v& acc) {
            if constexpr (decltype(h_)::value == 0) asm volatile("" ::"v"(acc[0]));
        });
        // base_remap: streams to slab region B (to the tile's tile of the plane) as it is produced, where it stays for the K
        // iterations (for the caller)
        {
            half8 Th[NCT], Tl[NCT];
            dense_layer<C, L::frag0(9), 8, 16, L::bias0(9)>(wt, nerf_bias, Xh, Xl, [&](auto rt_, auto c_, auto h_, const float4v& acc) {
                constexpr int rt = decltype(rt_)::value, c = decltype(c_)::value, hf = decltype(h_)::value;
                store_act<C, rt, hf>(acc, Th[c], Tl[c]);
                if constexpr ((rt & 1) && hf == 1) stash_store<C>(remap_at(tile), rt / 2, c, Th[c], Tl[c]);
            });
        }
        }   // TRUNK

        if constexpr (!STYLE) {
            // the trunk producer: next tile
        } else if constexpr (FOLD) {
            for (int k = 0; k < a.K; ++k) {
                // every wave must be done with the previous stream, and with the previous latent's bias table
                __builtin_amdgcn_s_barrier();
                if (a.K > 1) {
                    const char* table = a.folded + (size_t)k * kStylePairBiasBytes;
#pragma unroll
                    for (int j = 0; j < kStylePairBiasBytes / (C::NWAVES * 1024); ++j)
                        __builtin_amdgcn_global_load_lds(TGTC_GPTR(table + (j * C::NWAVES + wave) * 1024 + lane * 16),
                                                         TGTC_LPTR(smem + kPairBiasAt + (j * C::NWAVES + wave) * 1024),
                                                         16, 0, 0);
                }
                ws.prologue();
                ws.start();
                concat_mlp_folded<C, Map::F_CONCAT, 0>(ws, pair_bias, pe_h, pe_l, Xh, Xl, Yh, Yl);
                // ---- style layer 0 on [remap (slab B -> X) | concat_features (Y) | pe]; outputs stream to slab A
                stash_load<C>(remap_at(tile), Xh, Xl);
                {
                    half8 Bh[18][NCT], Bl[18][NCT];
#pragma unroll
                    for (int i = 0; i < 8; ++i) append<C>(Bh, Bl, i, Xh[i], Xl[i]);
#pragma unroll
                    for (int i = 0; i < 8; ++i) append<C>(Bh, Bl, 8 + i, Yh[i], Yl[i]);
                    append<C>(Bh, Bl, 16, pe_h[0], pe_l[0]);
                    append<C>(Bh, Bl, 17, pe_h[1], pe_l[1]);
                    half8 Th[NCT], Tl[NCT];
                    dense_layer<C, Map::F_STYLE + style_fold_frag0(0), 18, 16, kConcatBiasFloats + style_bias0(0)>(
                        ws, pair_bias, Bh, Bl, [&](auto rt_, auto c_, auto h_, const float4v& acc) {
                            constexpr int rt = decltype(rt_)::value, c = decltype(c_)::value, hf = decltype(h_)::value;
                            store_act<C, rt, hf>(acc, Th[c], Tl[c]);
                            if constexpr ((rt & 1) && hf == 1) stash_store<C>(slab, rt / 2, c, Th[c], Tl[c]);
                        });
                }
                stash_load<C>(slab, Xh, Xl);
                float* rgb_k = a.rgb + (long long)k * a.M * 3;
                style_tail_folded<C, Map::F_STYLE, kConcatBiasFloats>(ws, pair_bias, pe_h, pe_l, Xh, Xl, Yh, Yl,
                                                                      [&](auto c_, auto h_, const float4v& acc) {
                                                                          constexpr int c = decltype(c_)::value, hf = decltype(h_)::value;
                                                                          if (g == 0 && (own >> c & 1)) {
                                                                              const unsigned at = COMPACT ? i_wave + c * 16 + n : sidx[c];
#pragma unroll
                                                                              for (int r = 2 * hf; r < (hf ? 3 : 2); ++r)
                                                                                  rgb_k[(size_t)at * 3 + r] = 1.0f / (1.0f + expf(-acc[r]));
                                                                          }
                                                                      });
            }
        } else
        for (int k = 0; k < a.K; ++k) {
            // ---- latent k of the tile's rays
            float zsum[NCT];
            half8 z_h[NCT], z_l[NCT], zb_h[NCT], zb_l[NCT];
#pragma unroll
            for (int c = 0; c < NCT; ++c) {
                const long long r = sidx[c] / (unsigned)a.N;
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
            stash_load<C>(remap_at(tile), Xh, Xl);
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
            // ---- style layers 1..7 -> rgb[k], scattered to the sample's dense position (models.py:172-179); the compact
            //      form writes the column's list position, rebuilt from the tile (own masks the clamped columns)
            float* rgb_k = a.rgb + (long long)k * a.M * 3;
            style_tail<C, Map::F_STYLE, kConcatBiasFloats>(ws, pair_bias, pe_h, pe_l, zb_h, zb_l, Xh, Xl, Yh, Yl,
                                                           [&](auto c_, auto h_, const float4v& acc) {
                                                               constexpr int c = decltype(c_)::value, hf = decltype(h_)::value;
                                                               if (g == 0 && (own >> c & 1)) {
                                                                   const unsigned at = COMPACT ? i_wave + c * 16 + n : sidx[c];
#pragma unroll
                                                                   for (int r = 2 * hf; r < (hf ? 3 : 2); ++r)
                                                                       rgb_k[(size_t)at * 3 + r] = 1.0f / (1.0f + expf(-acc[r]));
                                                               }
                                                           });
        }
    }
}

using CfgFast = MlpCfg<8, 2, false, 4>;  // the geometries of styled_rays_multi_kernel
using CfgExact = MlpCfg<8, 1, true, 4>;

// Each of the four instances (fp16x3 / fp16, scattered / compact) is compiled in a translation unit of its own -- this
// source as it is, with -DTGTC_TU_FP16_ONLY, -DTGTC_TU_COMPACT or both -- so that the kernels build in parallel.  The four
// folded instances likewise, with -DTGTC_TU_FOLD in front of the same three combinations and of none.
// The six plane instances (producer: fp16x3 / fp16; consumer: those x unfolded / folded) likewise, with -DTGTC_TU_PLANE=1
// (kPlaneBuild) or =2 (kPlaneRead) in front of -DTGTC_TU_FP16_ONLY and -DTGTC_TU_FOLD.
template <class C, bool COMPACT, bool FOLD = false, int PLANE = kPlaneNone>
void launch_styled_rays_sparse(unsigned grid, const StyledSparseArgs& a, hipStream_t st) {
    styled_rays_sparse_kernel<C, COMPACT, FOLD, PLANE><<<grid, C::NWAVES * 64, 0, st>>>(a);
}
#if defined(TGTC_TU_PLANE)
#ifdef TGTC_TU_FP16_ONLY
using CfgPlane = CfgFast;
#else
using CfgPlane = CfgExact;
#endif
#ifdef TGTC_TU_FOLD
constexpr bool kPlaneFold = true;
#else
constexpr bool kPlaneFold = false;
#endif
template void launch_styled_rays_sparse<CfgPlane, true, kPlaneFold, TGTC_TU_PLANE>(unsigned, const StyledSparseArgs&, hipStream_t);
}  // namespace tgtc
#elif defined(TGTC_TU_FOLD)
#ifdef TGTC_TU_FP16_ONLY
using CfgFold = CfgFast;
#else
using CfgFold = CfgExact;
#endif
#ifdef TGTC_TU_COMPACT
constexpr bool kFoldCompact = true;
#else
constexpr bool kFoldCompact = false;
#endif
template void launch_styled_rays_sparse<CfgFold, kFoldCompact, true>(unsigned, const StyledSparseArgs&, hipStream_t);
}  // namespace tgtc
#elif defined(TGTC_TU_FP16_ONLY) && defined(TGTC_TU_COMPACT)
template void launch_styled_rays_sparse<CfgFast, true>(unsigned, const StyledSparseArgs&, hipStream_t);
}  // namespace tgtc
#elif defined(TGTC_TU_COMPACT)
template void launch_styled_rays_sparse<CfgExact, true>(unsigned, const StyledSparseArgs&, hipStream_t);
}  // namespace tgtc
#elif defined(TGTC_TU_FP16_ONLY)
template void launch_styled_rays_sparse<CfgFast, false>(unsigned, const StyledSparseArgs&, hipStream_t);
}  // namespace tgtc
#else
extern template void launch_styled_rays_sparse<CfgFast, false>(unsigned, const StyledSparseArgs&, hipStream_t);
extern template void launch_styled_rays_sparse<CfgExact, true>(unsigned, const StyledSparseArgs&, hipStream_t);
extern template void launch_styled_rays_sparse<CfgFast, true>(unsigned, const StyledSparseArgs&, hipStream_t);
extern template void launch_styled_rays_sparse<CfgExact, false, true>(unsigned, const StyledSparseArgs&, hipStream_t);
extern template void launch_styled_rays_sparse<CfgFast, false, true>(unsigned, const StyledSparseArgs&, hipStream_t);
extern template void launch_styled_rays_sparse<CfgExact, true, true>(unsigned, const StyledSparseArgs&, hipStream_t);
extern template void launch_styled_rays_sparse<CfgFast, true, true>(unsigned, const StyledSparseArgs&, hipStream_t);
extern template void launch_styled_rays_sparse<CfgExact, true, false, kPlaneBuild>(unsigned, const StyledSparseArgs&, hipStream_t);
extern template void launch_styled_rays_sparse<CfgFast, true, false, kPlaneBuild>(unsigned, const StyledSparseArgs&, hipStream_t);
extern template void launch_styled_rays_sparse<CfgExact, true, false, kPlaneRead>(unsigned, const StyledSparseArgs&, hipStream_t);
extern template void launch_styled_rays_sparse<CfgFast, true, false, kPlaneRead>(unsigned, const StyledSparseArgs&, hipStream_t);
extern template void launch_styled_rays_sparse<CfgExact, true, true, kPlaneRead>(unsigned, const StyledSparseArgs&, hipStream_t);
extern template void launch_styled_rays_sparse<CfgFast, true, true, kPlaneRead>(unsigned, const StyledSparseArgs&, hipStream_t);

// ------------------------------------------------------------------------------------------------ compaction
// The plane of M weights is cut into kCompactParts contiguous ranges of `span` samples (a multiple of the block size).
// Pass 1 counts the live samples of each range; pass 2 sums the counts in front of its range and writes the range's live
// indices behind them, 256 samples per step in lane order.  scratch: word 0 = n_live, words 64 .. 64 + kCompactParts the
// counts (every word is written by every call: nothing to initialise).
constexpr int kCompactParts = 1024;
constexpr int kCompactBlock = 256;
constexpr int kCompactCountWord = 64;

// CAND (the candidates of a density screen, render.hip): every sample that is NOT <= min_weight -- NaN included
template <bool CAND>
__device__ __forceinline__ bool is_live(float w, float min_weight) {
    if constexpr (CAND) return !(w <= min_weight);
    return w > min_weight;   // false for NaN
}

template <bool CAND>
__global__ void __launch_bounds__(kCompactBlock) compact_count_kernel(const float* __restrict__ w, unsigned M, unsigned span,
                                                                      float min_weight, unsigned* __restrict__ scratch) {
    __shared__ unsigned wave_n[kCompactBlock / 64];
    const unsigned long long b0 = (unsigned long long)blockIdx.x * span;
    const unsigned lo = b0 < M ? (unsigned)b0 : M;
    const unsigned hi = b0 + span < M ? (unsigned)(b0 + span) : M;
    unsigned cnt = 0;
    for (unsigned s = lo + threadIdx.x; s < hi; s += kCompactBlock) cnt += is_live<CAND>(w[s], min_weight) ? 1u : 0u;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d);
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned tot = 0;
#pragma unroll
        for (int i = 0; i < kCompactBlock / 64; ++i) tot += wave_n[i];
        scratch[kCompactCountWord + blockIdx.x] = tot;
    }
}

template <bool CAND>
__global__ void __launch_bounds__(kCompactBlock) compact_write_kernel(const float* __restrict__ w, unsigned M, unsigned span,
                                                                      float min_weight, const unsigned* __restrict__ counts,
                                                                      unsigned* __restrict__ live, unsigned* __restrict__ n_live,
                                                                      unsigned* __restrict__ live_count) {
    __shared__ unsigned red[kCompactBlock / 64];
    __shared__ unsigned wave_n[2][kCompactBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // samples live in the ranges in front of this one (and, for the last block, the total)
    unsigned before = 0, all = 0;
    for (unsigned p = threadIdx.x; p < kCompactParts; p += kCompactBlock) {
        const unsigned c = counts[p];
        all += c;
        if (p < blockIdx.x) before += c;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) before += __shfl_xor(before, d), all += __shfl_xor(all, d);
    if (lane == 0) red[wave] = before;
    __syncthreads();
    unsigned base = 0;
#pragma unroll
    for (int i = 0; i < kCompactBlock / 64; ++i) base += red[i];
    if (blockIdx.x == kCompactParts - 1) {
        __syncthreads();
        if (lane == 0) red[wave] = all;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned tot = 0;
#pragma unroll
            for (int i = 0; i < kCompactBlock / 64; ++i) tot += red[i];
            *n_live = tot;
            if (live_count) *live_count = tot;
        }
    }
    const unsigned long long b0 = (unsigned long long)blockIdx.x * span;
    const unsigned lo = b0 < M ? (unsigned)b0 : M;
    const unsigned hi = b0 + span < M ? (unsigned)(b0 + span) : M;
    // whole steps for every thread (the barrier inside is reached by all)
    int it = 0;
    for (unsigned s0 = lo; s0 < hi; s0 += kCompactBlock, ++it) {
        const unsigned s = s0 + threadIdx.x;
        const bool keep = s < hi && is_live<CAND>(w[s], min_weight);
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wave_n[it & 1][wave] = (unsigned)__popcll(m);
        __syncthreads();   // the buffer written two steps ago is free: every wave has passed the barrier in between
        unsigned at = base, step = 0;
#pragma unroll
        for (int i = 0; i < kCompactBlock / 64; ++i) {
            const unsigned c = wave_n[it & 1][i];
            if (i < wave) at += c;
            step += c;
        }
        if (keep) live[at + (unsigned)__popcll(m & ((1ull << lane) - 1ull))] = s;   // at + rank < n_live <= M
        base += step;
    }
}

template <bool CAND>
static int compact_launches(const float* w, int64_t M, float min_weight, uint32_t* live, uint32_t* scratch, uint32_t* live_count,
                            hipStream_t st) {
    // span: a multiple of the block size with kCompactParts * span >= M
    const int64_t per = (M + kCompactParts - 1) / kCompactParts;
    const unsigned span = (unsigned)((per + kCompactBlock - 1) / kCompactBlock * kCompactBlock);
    compact_count_kernel<CAND><<<kCompactParts, kCompactBlock, 0, st>>>(w, (unsigned)M, span, min_weight, scratch);
    TGTC_LAUNCH_CHECK();
    if (!live) return TGTC_OK;   // pass 1 alone: the counts of a statistic
    compact_write_kernel<CAND><<<kCompactParts, kCompactBlock, 0, st>>>(w, (unsigned)M, span, min_weight, scratch + kCompactCountWord,
                                                                        live, scratch, live_count);
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

int launch_compact_live(const float* w, int64_t M, float min_weight, uint32_t* live, uint32_t* scratch, uint32_t* live_count,
                        hipStream_t st) {
    return compact_launches<false>(w, M, min_weight, live, scratch, live_count, st);
}

// The candidates of a density screen: the ascending list of the samples whose screen density is not <= -margin (NaN and
// +inf are candidates), same scratch layout, same statistic words.
int launch_compact_candidates(const float* sigma, int64_t M, float margin, uint32_t* live, uint32_t* scratch, hipStream_t st) {
    return compact_launches<true>(sigma, M, -margin, live, scratch, nullptr, st);
}

// pass 1 of that alone (the candidate share of a pass that ran dense)
int launch_count_candidates(const float* sigma, int64_t M, float margin, uint32_t* scratch, hipStream_t st) {
    return compact_launches<true>(sigma, M, -margin, nullptr, scratch, nullptr, st);
}

static_assert((kCompactCountWord + kCompactParts) * sizeof(uint32_t) <= kSparseScratchBytes, "counts must fit the scratch");

// The live statistic of a plain chain render (render.hip): scratch words 2 and 3 = (number of samples with w > min_weight, M),
// the pair the render copies to the fine handle's pinned word.  launch_count_live is pass 1 of the compaction alone (a dense
// render has no use for the list); launch_live_stat sums the counts either form of pass 1 left behind.
constexpr int kCompactStatWord = 2;
static_assert(kCompactStatWord + 2 <= kCompactCountWord, "the statistic lies in front of the counts");

__global__ void __launch_bounds__(kCompactBlock) compact_stat_kernel(const unsigned* __restrict__ counts, unsigned M,
                                                                     unsigned* __restrict__ stat) {
    __shared__ unsigned red[kCompactBlock / 64];
    unsigned all = 0;
    for (unsigned p = threadIdx.x; p < kCompactParts; p += kCompactBlock) all += counts[p];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) all += __shfl_xor(all, d);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = all;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned tot = 0;
#pragma unroll
        for (int i = 0; i < kCompactBlock / 64; ++i) tot += red[i];
        stat[0] = tot, stat[1] = M;
    }
}

int launch_count_live(const float* w, int64_t M, float min_weight, uint32_t* scratch, hipStream_t st) {
    return compact_launches<false>(w, M, min_weight, nullptr, scratch, nullptr, st);
}

int launch_live_stat(uint32_t* scratch, int64_t M, const uint32_t** stat, hipStream_t st) {
    compact_stat_kernel<<<1, kCompactBlock, 0, st>>>(scratch + kCompactCountWord, (unsigned)M, scratch + kCompactStatWord);
    TGTC_LAUNCH_CHECK();
    *stat = scratch + kCompactStatWord;
    return TGTC_OK;
}

// rgb[k, s] for the samples of the list; the caller has zero-filled rgb.  n_live is read on the device: the grid is sized
// for the dense plane and workgroups without a tile leave at once.
int styled_forward_rays_sparse_impl(const tgtc_net* nerf, const tgtc_net* style, const double* rays_o, const double* rays_d,
                                    const float* ts, const float* z, int K, int64_t R, int N, const uint32_t* live,
                                    const uint32_t* n_live, float* rgb, hipStream_t st) {
    if (nerf->precision != style->precision)
        return fail(TGTC_ERR_ARG, "styled_forward_rays_sparse: NeRF and style nets were packed with different precisions");
    constexpr int64_t kLimit = (int64_t)1 << 31;
    if (R >= kLimit || R * (int64_t)N >= kLimit || R * (int64_t)N * K >= kLimit)
        return fail(TGTC_ERR_UNSUPPORTED, "styled_forward_rays_sparse: K x R x N >= 2^31 in one launch (chunk the rays)");
    StyledSparseArgs a{};
    a.nerf_bias = nerf->dev, a.nerf_stream = nerf->dev + nerf->bias_bytes;
    a.pair_bias = style->dev, a.concat_stream = style->dev + style->bias_bytes;
    a.style_stream = style->dev + style->stream2_off;
    a.stash = style->dev + style->stash_off, a.stash2_delta = (long long)(style->stash2_off - style->stash_off);
    a.M = R * (int64_t)N, a.R = R, a.N = N, a.K = K;
    a.rays_o = rays_o, a.rays_d = rays_d, a.ts = ts, a.z = z, a.live = live, a.n_live = n_live, a.rgb = rgb;
    if (nerf->precision == TGTC_PREC_FP16) {
        const long long tiles = (a.M + CfgFast::SAMPLES_PER_WG - 1) / CfgFast::SAMPLES_PER_WG;
        launch_styled_rays_sparse<CfgFast, false>((unsigned)(tiles < style->n_wg ? tiles : style->n_wg), a, st);
    } else {
        const long long tiles = (a.M + CfgExact::SAMPLES_PER_WG - 1) / CfgExact::SAMPLES_PER_WG;
        launch_styled_rays_sparse<CfgExact, false>((unsigned)(tiles < style->n_wg ? tiles : style->n_wg), a, st);
    }
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

// rgb_live[k, i] for the `count` samples of a cached list (count >= 1; K x count < 2^31 and the precisions are checked by the
// caller, tgtc_restyle_rays): the compact form, its grid sized from the host count.
int styled_restyle_live_impl(const tgtc_net* nerf, const tgtc_net* style, const double* rays_o, const double* rays_d,
                             const float* z, int K, int64_t R, int N, const uint32_t* live, const float* ts_live, int64_t count,
                             float* rgb_live, hipStream_t st) {
    StyledSparseArgs a{};
    a.nerf_bias = nerf->dev, a.nerf_stream = nerf->dev + nerf->bias_bytes;
    a.pair_bias = style->dev, a.concat_stream = style->dev + style->bias_bytes;
    a.style_stream = style->dev + style->stream2_off;
    a.stash = style->dev + style->stash_off, a.stash2_delta = (long long)(style->stash2_off - style->stash_off);
    a.M = count, a.R = R, a.N = N, a.K = K;
    a.rays_o = rays_o, a.rays_d = rays_d, a.z = z, a.live = live, a.ts_live = ts_live, a.count = (unsigned)count, a.rgb = rgb_live;
    if (nerf->precision == TGTC_PREC_FP16) {
        const long long tiles = (count + CfgFast::SAMPLES_PER_WG - 1) / CfgFast::SAMPLES_PER_WG;
        launch_styled_rays_sparse<CfgFast, true>((unsigned)(tiles < style->n_wg ? tiles : style->n_wg), a, st);
    } else {
        const long long tiles = (count + CfgExact::SAMPLES_PER_WG - 1) / CfgExact::SAMPLES_PER_WG;
        launch_styled_rays_sparse<CfgExact, true>((unsigned)(tiles < style->n_wg ? tiles : style->n_wg), a, st);
    }
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

// The two impls above over latents that are constant over the launch: `folded` holds the K bias tables of
// tgtc_style_fold_latents, the streams are the handle's folded pair, and no latent is read (tgtc_styled_forward_list_folded,
// tgtc_render_rays_styled_sparse_folded; tgtc_restyle_rays_folded).  The callers have checked the sizes and precisions.
static StyledSparseArgs folded_args(const tgtc_net* nerf, const tgtc_net* style, const double* rays_o, const double* rays_d,
                                    const void* folded, int K, int64_t R, int N, const uint32_t* live, float* rgb) {
    StyledSparseArgs a{};
    a.nerf_bias = nerf->dev, a.nerf_stream = nerf->dev + nerf->bias_bytes;
    a.pair_bias = style->dev, a.folded = static_cast<const char*>(folded);
    a.concat_stream = style->dev + style->fold_stream_off, a.style_stream = style->dev + style->fold_stream2_off;
    a.stash = style->dev + style->stash_off, a.stash2_delta = (long long)(style->stash2_off - style->stash_off);
    a.R = R, a.N = N, a.K = K, a.rays_o = rays_o, a.rays_d = rays_d, a.live = live, a.rgb = rgb;
    return a;
}

int styled_forward_list_folded_impl(const tgtc_net* nerf, const tgtc_net* style, const double* rays_o, const double* rays_d,
                                    const float* ts, const void* folded, int K, int64_t R, int N, const uint32_t* live,
                                    const uint32_t* n_live, float* rgb, hipStream_t st) {
    StyledSparseArgs a = folded_args(nerf, style, rays_o, rays_d, folded, K, R, N, live, rgb);
    a.M = R * (int64_t)N, a.ts = ts, a.n_live = n_live;
    if (nerf->precision == TGTC_PREC_FP16) {
        const long long tiles = (a.M + CfgFast::SAMPLES_PER_WG - 1) / CfgFast::SAMPLES_PER_WG;
        launch_styled_rays_sparse<CfgFast, false, true>((unsigned)(tiles < style->n_wg ? tiles : style->n_wg), a, st);
    } else {
        const long long tiles = (a.M + CfgExact::SAMPLES_PER_WG - 1) / CfgExact::SAMPLES_PER_WG;
        launch_styled_rays_sparse<CfgExact, false, true>((unsigned)(tiles < style->n_wg ? tiles : style->n_wg), a, st);
    }
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

int styled_restyle_live_folded_impl(const tgtc_net* nerf, const tgtc_net* style, const double* rays_o, const double* rays_d,
                                    const void* folded, int K, int64_t R, int N, const uint32_t* live, const float* ts_live,
                                    int64_t count, float* rgb_live, hipStream_t st) {
    StyledSparseArgs a = folded_args(nerf, style, rays_o, rays_d, folded, K, R, N, live, rgb_live);
    a.M = count, a.ts_live = ts_live, a.count = (unsigned)count;
    if (nerf->precision == TGTC_PREC_FP16) {
        const long long tiles = (count + CfgFast::SAMPLES_PER_WG - 1) / CfgFast::SAMPLES_PER_WG;
        launch_styled_rays_sparse<CfgFast, true, true>((unsigned)(tiles < style->n_wg ? tiles : style->n_wg), a, st);
    } else {
        const long long tiles = (count + CfgExact::SAMPLES_PER_WG - 1) / CfgExact::SAMPLES_PER_WG;
        launch_styled_rays_sparse<CfgExact, true, true>((unsigned)(tiles < style->n_wg ? tiles : style->n_wg), a, st);
    }
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

// ------------------------------------------------------------------------------------------------ trunk plane
// tgtc_geometry_trunk / tgtc_restyle_rays_trunk[_folded] (render.hip; count >= 1, sizes, precisions and handle kinds are
// checked there).  The producer needs no style handle and the consumers no NeRF handle.

// plane[tile] = base_remap's operand fragments of list entries [tile * S, (tile + 1) * S); grid: the tiles, at most one
// workgroup per CU
int styled_trunk_plane_impl(const tgtc_net* nerf, const double* rays_o, const double* rays_d, int64_t R, int N,
                            const uint32_t* live, const float* ts_live, int64_t count, void* plane, hipStream_t st) {
    int cus = 0;
    if (const int rc = cu_count(cus)) return rc;
    StyledSparseArgs a{};
    a.nerf_bias = nerf->dev, a.nerf_stream = nerf->dev + nerf->bias_bytes;
    a.M = count, a.R = R, a.N = N, a.rays_o = rays_o, a.rays_d = rays_d, a.live = live, a.ts_live = ts_live;
    a.count = (unsigned)count, a.plane = static_cast<char*>(plane);
    if (nerf->precision == TGTC_PREC_FP16) {
        const long long tiles = (count + CfgFast::SAMPLES_PER_WG - 1) / CfgFast::SAMPLES_PER_WG;
        launch_styled_rays_sparse<CfgFast, true, false, kPlaneBuild>((unsigned)(tiles < cus ? tiles : cus), a, st);
    } else {
        const long long tiles = (count + CfgExact::SAMPLES_PER_WG - 1) / CfgExact::SAMPLES_PER_WG;
        launch_styled_rays_sparse<CfgExact, true, false, kPlaneBuild>((unsigned)(tiles < cus ? tiles : cus), a, st);
    }
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

// rgb_live[k, i] from the plane: `folded` == nullptr takes z [K,R,32] and the handle's streams, otherwise the K bias tables
// and the streams packed without the latent k-steps.  The plane is only read.
int styled_restyle_plane_impl(const tgtc_net* style, const double* rays_o, const double* rays_d, const float* z,
                              const void* folded, int K, int64_t R, int N, const uint32_t* live, const float* ts_live,
                              int64_t count, const void* plane, float* rgb_live, hipStream_t st) {
    StyledSparseArgs a{};
    a.pair_bias = style->dev, a.folded = static_cast<const char*>(folded);
    a.concat_stream = style->dev + (folded ? style->fold_stream_off : style->bias_bytes);
    a.style_stream = style->dev + (folded ? style->fold_stream2_off : style->stream2_off);
    a.stash = style->dev + style->stash_off;
    a.M = count, a.R = R, a.N = N, a.K = K;
    a.rays_o = rays_o, a.rays_d = rays_d, a.z = z, a.live = live, a.ts_live = ts_live, a.count = (unsigned)count, a.rgb = rgb_live;
    a.plane = static_cast<char*>(const_cast<void*>(plane));
    const bool fast = style->precision == TGTC_PREC_FP16;
    const int per_wg = fast ? CfgFast::SAMPLES_PER_WG : CfgExact::SAMPLES_PER_WG;
    const long long tiles = (count + per_wg - 1) / per_wg;
    const unsigned grid = (unsigned)(tiles < style->n_wg ? tiles : style->n_wg);
    if (fast && folded) launch_styled_rays_sparse<CfgFast, true, true, kPlaneRead>(grid, a, st);
    else if (fast) launch_styled_rays_sparse<CfgFast, true, false, kPlaneRead>(grid, a, st);
    else if (folded) launch_styled_rays_sparse<CfgExact, true, true, kPlaneRead>(grid, a, st);
    else launch_styled_rays_sparse<CfgExact, true, false, kPlaneRead>(grid, a, st);
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

}  // namespace tgtc
#endif  // TGTC_TU_PLANE || TGTC_TU_FOLD || TGTC_TU_FP16_ONLY || TGTC_TU_COMPACT
