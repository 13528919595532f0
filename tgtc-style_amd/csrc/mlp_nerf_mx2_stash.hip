// The stashed form of the two-phase fine pass (render.hip fine_pass) for TGTC_PREC_FP16_FP6 handles: two kernels
// of the two-tile persistent geometry of mlp_nerf_mx2.hip, on two generated streams (tools/gen_mx2_asm.py stash ->
// mx2_stash_asm_nerf.inc, which the Makefile writes: it is a build product and not in git).
//   producer  nerf_mx2_stash_kernel: the density pass over rays (the sigma stream, instruction for instruction) that also
//             parks layer 7's output -- what REMAP reads -- of every sample with sigma > 0 in a caller-owned buffer in HBM;
//   consumer  nerf_mx2_heads_kernel: REMAP, C0 and C1 alone over the parked samples, sigmoid(rgb) scattered to rgb[sample].
// What is parked is the lane's share of activation set 1 as the stream holds it (gen_mx2_asm.py register map): 32 VGPRs of
// fp16 hi halves, 24 AGPRs of e2m3 copies, 2 block scales -- 58 dwords, all of the lane's own sample column (lane & 15) and
// k-group (lane >> 4).  A column moved to another column of another tile is multiplied by the same weights in the same
// order: the heads give the bits the full pass gives.
//
// The stash: kStashRegions regions of `cap` slots, region r = 4 * workgroup + wave owned by that wave of BOTH kernels (same
// grid).  A region is planes over its slots, so that the 16 lanes of a k-group move 16 consecutive slots = contiguous bytes:
//   plane d = 0..13 (h[0..7], a[0..5]): 16 B per (k-group, slot) at  (d * 4 + g) * cap * 16 + slot * 16
//   plane 14 (the two block scales):     8 B per (k-group, slot) at  14 * 64 * cap + (g * cap + slot) * 8
//   sample index:                        4 B per slot            at  928 * cap + slot * 4
// A wave gives its live columns consecutive slots from a cursor it keeps in a scalar (prefix over the tile's live mask: no
// atomics, no LDS) and leaves its live count in counts[r]; live samples beyond the region go to an overflow list
// (device counter, one vector atomic per sample: the rare path), which the caller runs through the list kernel.
#define TGTC_ASM_DMA 1  // see mlp_core.h lds_dma16
#include "mlp_nerf_mx.h"

#include "mlp_layouts.h"
#include "mlp_mx.h"
#include "mlp_nerf_mx_chain.h"

namespace tgtc {

struct Mx2Stash {
    half8 h[8];          // hreg(1, ct): fp16 hi halves
    half8 a[6];          // a6(1, ct): e2m3 copies h6 | l6
    unsigned sc[2];      // sc(1, ct, 0..1): block scales
};

#include "mx2_stash_asm_nerf.inc"

using CfgMx2 = MlpCfg<4, 2, false, 4>;
#ifndef TGTC_FRONT_ABL   // development switch, as TGTC_MX2_ABL of mlp_nerf_mx2.hip: what the HIP code in front of a pass costs
#define TGTC_FRONT_ABL 0
#endif
static_assert(CfgMx2::NWAVES * kNerfStashMaxGrid == kNerfStashRegions, "one region per wave of the largest grid");

__device__ __forceinline__ char* stash_region(const NerfStashArgs& s, int wave) {
    return s.base + (size_t)(blockIdx.x * CfgMx2::NWAVES + wave) * s.stride;
}

__global__ void __launch_bounds__(256, 1) nerf_mx2_stash_kernel(NerfArgs a, NerfStashArgs s, long long n_pass) {
    using C = CfgMx2;
    constexpr int NUNITS = nerf_mx_units(false);
    using Reader = MxReader<C, SingleStreamMap<NUNITS>, kNerfMxTable, true>;
    constexpr int kChunk = 16384, kSlots = C::RING_BYTES / kChunk, kLook = kSlots - 1, kPiece = kChunk / C::NWAVES;
    static_assert(C::RING_BYTES == 131072 && kPiece % 4096 == 0 && kChunkBytes == kChunk, "the generated stream was laid out for this ring");

    // ring | biases + row exponents
    __shared__ __attribute__((aligned(16))) char smem[C::RING_BYTES + kNerfBiasBytes];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    Reader rd;
    {
        const int lane = threadIdx.x & 63;
        const char* const streams[1] = {a.stream};
        rd.init(streams, smem, wave, lane);
#pragma unroll
        for (int j = 0; j < kNerfBiasBytes / (C::NWAVES * 1024); ++j)
            lds_dma16(a.bias + (j * C::NWAVES + wave) * 1024 + lane * 16, smem + C::RING_BYTES + (j * C::NWAVES + wave) * 1024);
        rd.ring.lds_wave = smem + wave * kPiece;
        rd.ring.voff = wave * kPiece + lane * 16;
        static_for<kLook * (kPiece / 1024)>([&](auto i_) {
            constexpr int i = decltype(i_)::value, ch = i / (kPiece / 1024), j = i % (kPiece / 1024);
            lds_dma16_s<(j % 4) * 1024>(rd.ring.src[0] + ch * kChunk + (j / 4) * 4096, rd.ring.voff, rd.ring.lds_wave + ch * kChunk + (j / 4) * 4096);
        });
    }

    unsigned cursor = 0;   // wave-uniform: live samples of this wave so far = the next free slot of its region
    for (long long p = blockIdx.x; p < n_pass; p += gridDim.x) {
        const long long s_wave = p * C::SAMPLES_PER_WG + wave * C::SAMPLES_PER_WAVE;
        half8 keep[2][4];
        {
            const int lane = fresh_lane_id();
            const int g = lane >> 4, n = lane & 15;
            double pos[2][3], dir[2][3];
            long long sidx[2];
            half8 pe_h[2][2], pe_l[2][2], de_h[1][2], de_l[1][2];
#if TGTC_FRONT_ABL & 1   // timing experiment: no sample loads, no encoding (results wrong by construction)
#pragma unroll
            for (int c = 0; c < 2; ++c) pe_h[0][c] = pe_h[1][c] = pe_l[0][c] = pe_l[1][c] = half8{(_Float16)(float)(g + n)};
#elif TGTC_FRONT_ABL & 4   // timing experiment: the sample loads (and their wait) without the encoders' arithmetic
            nerf_load_samples<2, IN_RAYS>(a, s_wave, n, pos, dir, sidx);
#pragma unroll
            for (int c = 0; c < 2; ++c)
                pe_h[0][c] = pe_h[1][c] = pe_l[0][c] = pe_l[1][c] = half8{(_Float16)(float)(pos[c][0] + pos[c][1] + pos[c][2])};
#else
            nerf_load_samples<2, IN_RAYS>(a, s_wave, n, pos, dir, sidx);
            nerf_encode<2, true, false>(a, pos, dir, sidx, g, pe_h, pe_l, de_h, de_l);
#endif
#pragma unroll
            for (int c = 0; c < 2; ++c) keep[c][0] = pe_h[0][c], keep[c][1] = pe_h[1][c], keep[c][2] = pe_l[0][c], keep[c][3] = pe_l[1][c];
        }
        // per-lane addresses from a lane id read HERE: nothing but them and the loop's scalars lives across the stream
        rd.relane(smem, wave);
        const int fl = fresh_lane_id();
        rd.ring.voff = wave * kPiece + fl * 16;
        const lds_cptr bias_lane = opaque((lds_cptr)smem + C::RING_BYTES + 16 * (fl >> 4));
        const lds_cptr rs_lane = opaque((lds_cptr)smem + C::RING_BYTES + kNerfMxScaleOff + 2 * (fl & 15));
        float sigma[2];
        Mx2Stash x[2];
        mx2_asm_nerf_sigma_stash_pass(rd, wave, bias_lane, rs_lane, keep, sigma, x);
        const int lane = fresh_lane_id();
        const unsigned g = (unsigned)lane >> 4, n = (unsigned)lane & 15u;
        char* const region = stash_region(s, wave);
        const size_t cap = s.cap;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const long long smp = s_wave + c * 16 + n;
            const bool col = lane < 16 && smp < a.M;       // sigma[c] is row 0 of the head's tile: lanes 0..15
            if (col) a.sigma[smp] = sigma[c];
            // the compaction's criterion with min_weight = 0 (mlp_style_sparse.hip is_live): false for NaN
            const unsigned m16 = __builtin_amdgcn_readfirstlane((unsigned)__ballot(col && sigma[c] > 0.0f)) & 0xffffu;
            if ((m16 >> n) & 1u) {
                const unsigned slot = cursor + (unsigned)__popc(m16 & ((1u << n) - 1u));
                if (slot < s.cap) {
                    char* const q = region + ((size_t)g * cap + slot) * 16;
#pragma unroll
                    for (int d = 0; d < 8; ++d) *reinterpret_cast<half8*>(q + (size_t)d * cap * 64) = x[c].h[d];
#pragma unroll
                    for (int d = 0; d < 6; ++d) *reinterpret_cast<half8*>(q + (size_t)(8 + d) * cap * 64) = x[c].a[d];
                    *reinterpret_cast<uint2*>(region + 896 * cap + ((size_t)g * cap + slot) * 8) = make_uint2(x[c].sc[0], x[c].sc[1]);
                    if (g == 0) *reinterpret_cast<unsigned*>(region + 928 * cap + (size_t)slot * 4) = (unsigned)smp;
                } else if (g == 0) {
                    s.ovf[atomicAdd(s.ovf_count, 1u)] = (unsigned)smp;   // (each sample once: the list has a word for every sample)
                }
            }
            cursor = __builtin_amdgcn_readfirstlane(cursor + (unsigned)__popc(m16));
        }
    }
    wait_vmcnt<0>();   // the look-ahead of a pass that will not run: its LDS-DMA must have landed before the workgroup ends
    if ((threadIdx.x & 63) == 0) s.counts[blockIdx.x * C::NWAVES + wave] = cursor;
}

// Wave w of workgroup b walks region (b, w) in passes of 2 x 16 slots; the ring is workgroup-lockstep, so the workgroup runs
// as many passes as its fullest region has, a wave that is out of slots repeating its last one with the stores masked.
__global__ void __launch_bounds__(256, 1) nerf_mx2_heads_kernel(NerfArgs a, NerfStashArgs s) {
    using C = CfgMx2;
    using Reader = MxReader<C, SingleStreamMap<kMx2HeadsUnits>, kNerfMxTable, true>;
    constexpr int kChunk = 16384, kSlots = C::RING_BYTES / kChunk, kLook = kSlots - 1, kPiece = kChunk / C::NWAVES;
    static_assert(C::RING_BYTES == 131072 && kPiece % 4096 == 0 && kChunkBytes == kChunk, "the generated stream was laid out for this ring");
    static_assert(kMx2HeadsPadChunks * kChunk == kNerfHeadsStreamBytes && kMx2HeadsPadChunks >= kLook, "the heads stream as the handle pads it");

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // scalar loads, issued before any LDS-DMA: what each wave of the producer's workgroup parked (its live count, capped)
    unsigned mine = 0, most = 0;
#pragma unroll
    for (int w = 0; w < C::NWAVES; ++w) {
        unsigned k = __builtin_amdgcn_readfirstlane(s.counts[blockIdx.x * C::NWAVES + w]);
        k = k < s.cap ? k : s.cap;
        most = k > most ? k : most;
        if (w == wave) mine = k;
    }
    const unsigned n_pass = (most + C::SAMPLES_PER_WAVE - 1) / C::SAMPLES_PER_WAVE;

    __shared__ __attribute__((aligned(16))) char smem[C::RING_BYTES + kNerfBiasBytes];
    Reader rd;
    {
        const int lane = threadIdx.x & 63;
        const char* const streams[1] = {a.stream};
        rd.init(streams, smem, wave, lane);
#pragma unroll
        for (int j = 0; j < kNerfBiasBytes / (C::NWAVES * 1024); ++j)
            lds_dma16(a.bias + (j * C::NWAVES + wave) * 1024 + lane * 16, smem + C::RING_BYTES + (j * C::NWAVES + wave) * 1024);
        rd.ring.lds_wave = smem + wave * kPiece;
        rd.ring.voff = wave * kPiece + lane * 16;
        static_for<kLook * (kPiece / 1024)>([&](auto i_) {
            constexpr int i = decltype(i_)::value, ch = i / (kPiece / 1024), j = i % (kPiece / 1024);
            lds_dma16_s<(j % 4) * 1024>(rd.ring.src[0] + ch * kChunk + (j / 4) * 4096, rd.ring.voff, rd.ring.lds_wave + ch * kChunk + (j / 4) * 4096);
        });
    }

    const size_t cap = s.cap;
    for (unsigned p = 0; p < n_pass; ++p) {
        const unsigned slot0 = p * C::SAMPLES_PER_WAVE;
        Mx2Stash x[2];
        half8 dkeep[2][2];
        {
            const int lane = fresh_lane_id();
            const unsigned g = (unsigned)lane >> 4, n = (unsigned)lane & 15u;
            const char* const region = stash_region(s, wave);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                unsigned slot = slot0 + c * 16 + n;
                slot = slot < mine ? slot : (mine ? mine - 1 : 0);   // out of slots: the last one again (cap >= 1: slot 0 exists)
                const char* const q = region + ((size_t)g * cap + slot) * 16;
#pragma unroll
                for (int d = 0; d < 8; ++d) x[c].h[d] = *reinterpret_cast<const half8*>(q + (size_t)d * cap * 64);
#pragma unroll
                for (int d = 0; d < 6; ++d) x[c].a[d] = *reinterpret_cast<const half8*>(q + (size_t)(8 + d) * cap * 64);
                const uint2 sc = *reinterpret_cast<const uint2*>(region + 896 * cap + ((size_t)g * cap + slot) * 8);
                x[c].sc[0] = sc.x, x[c].sc[1] = sc.y;
                const unsigned smp = *reinterpret_cast<const unsigned*>(region + 928 * cap + (size_t)slot * 4);
                nerf_encode_dir_late<IN_RAYS, true>(a, (long long)smp, (int)g, dkeep[c][0], dkeep[c][1]);
            }
        }
        rd.relane(smem, wave);
        const int fl = fresh_lane_id();
        rd.ring.voff = wave * kPiece + fl * 16;
        const lds_cptr bias_lane = opaque((lds_cptr)smem + C::RING_BYTES + 16 * (fl >> 4));
        const lds_cptr rs_lane = opaque((lds_cptr)smem + C::RING_BYTES + kNerfMxScaleOff + 2 * (fl & 15));
        float rgb[2][3];
        mx2_asm_nerf_heads_pass(rd, wave, bias_lane, rs_lane, dkeep, x, rgb);
        const int lane = fresh_lane_id();
        if (lane < 16) {
            const char* const region = stash_region(s, wave);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const unsigned slot = slot0 + c * 16 + lane;
                if (slot < mine) {
                    // the slot's sample is read again here: nothing but scalars lives across the stream
                    const unsigned smp = *reinterpret_cast<const unsigned*>(region + 928 * cap + (size_t)slot * 4);
                    if (smp < a.M) {   // (a stash its producer filled never fails this)
#pragma unroll
                        for (int r = 0; r < 3; ++r) a.rgb[(size_t)smp * 3 + r] = 1.0f / (1.0f + expf(-rgb[c][r]));   // models.py:111
                    }
                }
            }
        }
    }
    wait_vmcnt<0>();
}

// the REMAP / C0 / C1 groups of a packed full stream (mlp_mx_pack.h through nerf_mx_pack) in a stream of their own: each
// group's bytes as they are, at the offsets of the heads' own group table, padded to whole rings
void nerf_mx_heads_stream(const std::vector<char>& stream, std::vector<char>& heads) {
    static constexpr MxShape kHeadsShape[3] = {kNerfMxShape[9], kNerfMxShape[10], kNerfMxShape[11]};
    static constexpr MxTable H = mx_make_table(kHeadsShape, kRingBytes);
    constexpr const MxTable& T = kNerfMxTable;
    static_assert(H.n == T.first[12] - T.first[9] && H.bytes == kMx2HeadsUnits * 1024 && H.bytes <= kNerfHeadsStreamBytes, "heads table");
    heads.assign(kNerfHeadsStreamBytes, 0);
    for (int q = 0; q < H.n; ++q) {
        const int f = T.first[9] + q;
        const int size = T.npe[f] ? T.npe[f] * 2048 : kMxKGroupBytes;
        std::memcpy(heads.data() + H.off[q], stream.data() + T.off[f], (size_t)size);
    }
}

static int stash_grid(const NerfArgs& a, unsigned& nwg) {
    int cus = 0;
    if (const int rc = cu_count(cus)) return rc;
    const long long n_pass = (a.M + CfgMx2::SAMPLES_PER_WG - 1) / CfgMx2::SAMPLES_PER_WG;
    const long long most = cus < kNerfStashMaxGrid ? cus : kNerfStashMaxGrid;
    nwg = (unsigned)(n_pass < most ? n_pass : most);
    return TGTC_OK;
}

int nerf_mx2_stash_launch(const NerfArgs& a, const NerfStashArgs& s, hipStream_t st) {
    unsigned nwg = 0;
    if (const int rc = stash_grid(a, nwg)) return rc;
    const long long n_pass = (a.M + CfgMx2::SAMPLES_PER_WG - 1) / CfgMx2::SAMPLES_PER_WG;
    nerf_mx2_stash_kernel<<<nwg, dim3(CfgMx2::NWAVES * 64), 0, st>>>(a, s, n_pass);
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

int nerf_mx2_heads_launch(const NerfArgs& a, const NerfStashArgs& s, hipStream_t st) {
    unsigned nwg = 0;
    if (const int rc = stash_grid(a, nwg)) return rc;
    nerf_mx2_heads_kernel<<<nwg, dim3(CfgMx2::NWAVES * 64), 0, st>>>(a, s);
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

}  // namespace tgtc
