// The density screen's own kernel (DESIGN 3.1 "The screen"): the NeRF trunk + sigma head in TGTC_PREC_FP16, one MFMA product per
// weight, on FOUR column tiles per wave, one wave per SIMD: a persistent kernel (one workgroup of four waves per CU, 256 samples
// per pass, the weight ring never drains between passes) whose pass is ONE generated instruction stream (tools/gen_fp16s_asm.py
// -> fp16s_asm_nerf.inc).  Same arithmetic per sample, in the same order, as nerf_mlp_kernel<CfgFast, IN_RAYS, false>
// (mlp_nerf.hip): bit-identical densities wherever the sample's position is inside the screen's box, a quarter of the weight-side work per MFMA
// of a one-tile wave and half of CfgFast's.
// It reads the screen's packed form as it is: the TGTC_PREC_FP16 fragment stream of 1 KiB fragments and the bias table.
// The stream of a pass also carries, between its MFMAs, the front end of the wave's next pass (sample loads, float64 positions,
// point encodings); the same stream without it, behind the HIP front end, is compiled alongside as its yardstick.
#define TGTC_ASM_DMA 1  // see mlp_core.h lds_dma16
#include "mlp_nerf_mx.h"

#include <cstdlib>

#include "mlp_layouts.h"

namespace tgtc {

#ifndef TGTC_FP16S_INC   // (timing experiments build against streams generated with tools/gen_fp16s_asm.py abl_*=1)
#define TGTC_FP16S_INC "fp16s_asm_nerf.inc"
#endif
#include TGTC_FP16S_INC

using CfgFp16s = MlpCfg<4, kFp16sTiles, false, 4>;
#ifndef TGTC_FRONT_ABL   // development switch, as in mlp_nerf_x3s.hip: what the HIP code in front of a pass costs
#define TGTC_FRONT_ABL 0
#endif

// the reciprocal word of the exact 32-bit division the in-stream front end runs (sample -> ray): with it, mulhi(x, z) is the
// quotient x / n or falls short of it by at most two (the expansion hipcc itself emits for `x / n`: estimate, one Newton round)
__device__ __forceinline__ unsigned udiv_word(unsigned n) {
    unsigned z = (unsigned)(__builtin_amdgcn_rcpf((float)n) * 4294966784.0f);   // 0x4f7ffffe
    return z + __umulhi(z, (0u - n) * z);
}

// the HIP front end of one pass: the wave's 4 x 16 samples loaded and their points encoded (every pass of the serial-front
// kernel; a workgroup's first pass in the kernel whose stream carries the front end of the next)
template <int IN_MODE, int NCT>
__device__ __forceinline__ void fp16s_front(const NerfArgs& a, long long s_wave, half8 (&keep)[NCT][2], unsigned& bad) {
    const int lane = fresh_lane_id();
    const int g = lane >> 4, n = lane & 15;
    double pos[NCT][3], dir[NCT][3];
    long long sidx[NCT];
    half8 pe_h[2][NCT], pe_l[2][NCT], de_h[1][NCT], de_l[1][NCT];
    bad = 0;
#if TGTC_FRONT_ABL & 1   // timing experiment: no sample loads, no encoding (results wrong by construction)
#pragma unroll
    for (int c = 0; c < NCT; ++c) pe_h[0][c] = pe_h[1][c] = half8{(_Float16)(float)(g + n)};
#else
    nerf_load_samples<NCT, IN_MODE>(a, s_wave, n, pos, dir, sidx);
    nerf_encode<NCT, false, false>(a, pos, dir, sidx, g, pe_h, pe_l, de_h, de_l);
#pragma unroll
    for (int c = 0; c < NCT; ++c)
        if (!(__builtin_fabs(pos[c][0]) <= kScreenBox && __builtin_fabs(pos[c][1]) <= kScreenBox && __builtin_fabs(pos[c][2]) <= kScreenBox))
            bad |= 1u << c;
#endif
#pragma unroll
    for (int c = 0; c < NCT; ++c) keep[c][0] = pe_h[0][c], keep[c][1] = pe_h[1][c];
}

// FRONT: the stream of a pass computes the encodings of the wave's NEXT pass (p + gridDim.x) between its MFMAs and leaves them
// in a224..a255, where the next pass's stream takes them from (DESIGN 3.1 "The front end under the stream"); only a workgroup's
// first pass is encoded by the HIP front end.  !FRONT: the HIP front end in front of every pass (TGTC_SCREEN_SERIAL_FRONT=1,
// the yardstick the in-stream front end is held against).  The same bits either way.
template <int IN_MODE, bool FRONT>
__global__ void __launch_bounds__(256, 1) nerf_fp16s_kernel(NerfArgs a, long long n_pass) {
    using C = CfgFp16s;
    constexpr int NCT = C::NCT;
    using Ring = WeightStream<C, SingleStreamMap<NerfLayout::kFragsSigma>, true, true>;
    // the stream's ring: 128 KiB in chunks of kFp16sChunkBytes, every wave moves 1/4 of a chunk
    constexpr int kChunk = kFp16sChunkBytes, kSlots = C::RING_BYTES / kChunk, kLook = kSlots - 1, kPiece = kChunk / C::NWAVES;
    constexpr int kPad = ((NerfLayout::kFragsSigma * C::FRAG_BYTES + kChunk - 1) / kChunk + kSlots - 1) / kSlots * kSlots;
    static_assert(NerfLayout::kFragsSigma == kFp16sFrags && kPad == kFp16sPadChunks && C::RING_BYTES == 131072 && C::FRAG_BYTES == 1024 &&
                      kPiece % 4096 == 0 && kChunk == kChunkBytes,
                  "the generated stream was laid out for this ring");
    static_assert(kFp16sBox == kScreenBox, "the generated front end tests positions against the HIP front end's box");
    static_assert(!FRONT || IN_MODE == IN_RAYS, "the in-stream front end loads samples of rays");

    // ring | biases
    __shared__ __attribute__((aligned(16))) char smem[C::RING_BYTES + kNerfBiasBytes];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    Ring ring;
    {
        const int lane = threadIdx.x & 63;
        const char* const streams[1] = {a.stream};
        ring.init(streams, smem, wave, lane);
#pragma unroll
        for (int j = 0; j < kNerfBiasBytes / (C::NWAVES * 1024); ++j)
            lds_dma16(a.bias + (j * C::NWAVES + wave) * 1024 + lane * 16, smem + C::RING_BYTES + (j * C::NWAVES + wave) * 1024);
        // chunks 0 .. kLook-1 of the stream: the state every pass's entry expects (the first entry's counted wait also covers
        // the bias table: it is older than the chunks)
        ring.lds_wave = smem + wave * kPiece;
        ring.voff = wave * kPiece + lane * 16;
        static_for<kLook * (kPiece / 1024)>([&](auto i_) {
            constexpr int i = decltype(i_)::value, ch = i / (kPiece / 1024), j = i % (kPiece / 1024);
            lds_dma16_s<(j % 4) * 1024>(ring.src[0] + ch * kChunk + (j / 4) * 4096, ring.voff, ring.lds_wave + ch * kChunk + (j / 4) * 4096);
        });
    }

    // bit c: the lane's sample of tile c has a position outside the screen's box: a coordinate with not (|p| <= kScreenBox), a
    // NaN or an infinity included.  The margin is calibrated on the box and says nothing beyond it, and the ReLU of the fp16
    // layers (v_pk_max_f16 with zero) returns zero for a NaN, the finite density of an all-zero layer; such a sample gets
    // NaN instead, which the screened passes list as a candidate (render.hip): the exact kernels decide about it.
    unsigned bad = 0;
    half8 keep[NCT][2];
    if constexpr (FRONT) {
        fp16s_front<IN_MODE>(a, (long long)blockIdx.x * C::SAMPLES_PER_WG + wave * C::SAMPLES_PER_WAVE, keep, bad);
        fp16s_asm_first_keep(keep);   // into a224..a255, where every pass's stream finds its encodings and leaves the next pass's
    }
    // (M < 2^31 is checked at launch: sample indices, the first of a pass that does not exist included, fit 32 bits)
    const unsigned mm1 = (unsigned)(a.M - 1), zz = __builtin_amdgcn_readfirstlane(udiv_word((unsigned)a.N));

    for (long long p = blockIdx.x; p < n_pass; p += gridDim.x) {
        const long long s_wave = p * C::SAMPLES_PER_WG + wave * C::SAMPLES_PER_WAVE;
        if constexpr (!FRONT) fp16s_front<IN_MODE>(a, s_wave, keep, bad);
        // per-lane addresses from a lane id read HERE: nothing but them and the loop's scalars lives across the stream
        const int fl = fresh_lane_id();
        ring.voff = wave * kPiece + fl * 16;
        ring.lane_lo = opaque((lds_cptr)smem + fl * 16);
        ring.lane_hi = opaque((lds_cptr)smem + 65536 + fl * 16);
        const lds_cptr bias_lane = opaque((lds_cptr)smem + C::RING_BYTES + 16 * (fl >> 4));
        float sigma[NCT];
        unsigned nbad = 0;
        if constexpr (FRONT) {
            // the wave's samples of its next pass; beyond the last pass every index clamps to M - 1 inside the stream, as
            // nerf_load_samples clamps a ragged tail, and the encodings are never used
            const unsigned snext = (unsigned)(s_wave + (long long)gridDim.x * C::SAMPLES_PER_WG);
            fp16s_asm_nerf_sigma_pass_front(ring, bias_lane, sigma, nbad, a.ts, a.rays_o, a.rays_d, mm1, (unsigned)a.N, zz, snext);
        } else {
            fp16s_asm_nerf_sigma_pass(ring, bias_lane, keep, sigma);
        }
        const int lane = fresh_lane_id();
        if (lane < 16) {
#pragma unroll
            for (int c = 0; c < NCT; ++c) {
                const long long s = s_wave + c * 16 + lane;
                if (s < a.M) a.sigma[s] = (bad >> c & 1) ? __builtin_nanf("") : sigma[c];
            }
        }
        if constexpr (FRONT) bad = nbad;
    }
    wait_vmcnt<0>();   // the look-ahead of a pass that will not run: its LDS-DMA must have landed before the workgroup ends
}

// a.bias / a.stream: the TGTC_PREC_FP16 form of a handle; one workgroup per CU, never more than there are passes.
// TGTC_SCREEN_SERIAL_FRONT=1 in the environment (read at every call, as TGTC_SCREEN_CFGFAST is): the serial-front kernel.
int nerf_fp16s_launch(const NerfArgs& a, hipStream_t st) {
    using C = CfgFp16s;
    if (a.M <= 0) return TGTC_OK;
    if (a.M >= 0x7fffffffLL) return fail(TGTC_ERR_UNSUPPORTED, "nerf: too many samples in one launch (%lld)", a.M);
    int cus = 0;
    if (const int rc = cu_count(cus)) return rc;
    const long long n_pass = (a.M + C::SAMPLES_PER_WG - 1) / C::SAMPLES_PER_WG;
    const unsigned grid = (unsigned)(n_pass < cus ? n_pass : cus);
    const char* e = std::getenv("TGTC_SCREEN_SERIAL_FRONT");
    if (e && e[0] == '1') nerf_fp16s_kernel<IN_RAYS, false><<<grid, C::NWAVES * 64, 0, st>>>(a, n_pass);
    else nerf_fp16s_kernel<IN_RAYS, true><<<grid, C::NWAVES * 64, 0, st>>>(a, n_pass);
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

}  // namespace tgtc
