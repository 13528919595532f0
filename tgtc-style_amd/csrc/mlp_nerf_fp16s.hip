// The density screen's own kernel (DESIGN 3.1 "The screen"): the NeRF trunk + sigma head in TGTC_PREC_FP16, one MFMA product per
// weight, on FOUR column tiles per wave, one wave per SIMD: a persistent kernel (one workgroup of four waves per CU, 256 samples
// per pass, the weight ring never drains between passes) whose pass is ONE generated instruction stream (tools/gen_fp16s_asm.py
// -> fp16s_asm_nerf.inc).  Same arithmetic per sample, in the same order, as nerf_mlp_kernel<CfgFast, IN_RAYS, false>
// (mlp_nerf.hip): bit-identical densities wherever the sample's position is finite, a quarter of the weight-side work per MFMA
// of a one-tile wave and half of CfgFast's.
// It reads the screen's packed form as it is: the TGTC_PREC_FP16 fragment stream of 1 KiB fragments and the bias table.
#define TGTC_ASM_DMA 1  // see mlp_core.h lds_dma16
#include "mlp_nerf_mx.h"

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

template <int IN_MODE>
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

    for (long long p = blockIdx.x; p < n_pass; p += gridDim.x) {
        const long long s_wave = p * C::SAMPLES_PER_WG + wave * C::SAMPLES_PER_WAVE;
        half8 keep[NCT][2];
        // bit c: the lane's sample of tile c has a position that is not finite.  The ReLU of the fp16 layers (v_pk_max_f16 with
        // zero) returns zero for a NaN, so such a sample would come out with the finite density of an all-zero layer; it gets NaN
        // instead, which the screened passes list as a candidate (render.hip) -- as the exact kernels' density of it is.
        unsigned bad = 0;
        {
            const int lane = fresh_lane_id();
            const int g = lane >> 4, n = lane & 15;
            double pos[NCT][3], dir[NCT][3];
            long long sidx[NCT];
            half8 pe_h[2][NCT], pe_l[2][NCT], de_h[1][NCT], de_l[1][NCT];
#if TGTC_FRONT_ABL & 1   // timing experiment: no sample loads, no encoding (results wrong by construction)
#pragma unroll
            for (int c = 0; c < NCT; ++c) pe_h[0][c] = pe_h[1][c] = half8{(_Float16)(float)(g + n)};
#else
            nerf_load_samples<NCT, IN_MODE>(a, s_wave, n, pos, dir, sidx);
            nerf_encode<NCT, false, false>(a, pos, dir, sidx, g, pe_h, pe_l, de_h, de_l);
#pragma unroll
            for (int c = 0; c < NCT; ++c)
                if (!(__builtin_isfinite(pos[c][0]) && __builtin_isfinite(pos[c][1]) && __builtin_isfinite(pos[c][2]))) bad |= 1u << c;
#endif
#pragma unroll
            for (int c = 0; c < NCT; ++c) keep[c][0] = pe_h[0][c], keep[c][1] = pe_h[1][c];
        }
        // per-lane addresses from a lane id read HERE: nothing but them and the loop's scalars lives across the stream
        const int fl = fresh_lane_id();
        ring.voff = wave * kPiece + fl * 16;
        ring.lane_lo = opaque((lds_cptr)smem + fl * 16);
        ring.lane_hi = opaque((lds_cptr)smem + 65536 + fl * 16);
        const lds_cptr bias_lane = opaque((lds_cptr)smem + C::RING_BYTES + 16 * (fl >> 4));
        float sigma[NCT];
        fp16s_asm_nerf_sigma_pass(ring, bias_lane, keep, sigma);
        const int lane = fresh_lane_id();
        if (lane < 16) {
#pragma unroll
            for (int c = 0; c < NCT; ++c) {
                const long long s = s_wave + c * 16 + lane;
                if (s < a.M) a.sigma[s] = (bad >> c & 1) ? __builtin_nanf("") : sigma[c];
            }
        }
    }
    wait_vmcnt<0>();   // the look-ahead of a pass that will not run: its LDS-DMA must have landed before the workgroup ends
}

// a.bias / a.stream: the TGTC_PREC_FP16 form of a handle; one workgroup per CU, never more than there are passes
int nerf_fp16s_launch(const NerfArgs& a, hipStream_t st) {
    using C = CfgFp16s;
    if (a.M <= 0) return TGTC_OK;
    if (a.M >= 0x7fffffffLL) return fail(TGTC_ERR_UNSUPPORTED, "nerf: too many samples in one launch (%lld)", a.M);
    int cus = 0;
    if (const int rc = cu_count(cus)) return rc;
    const long long n_pass = (a.M + C::SAMPLES_PER_WG - 1) / C::SAMPLES_PER_WG;
    nerf_fp16s_kernel<IN_RAYS><<<(unsigned)(n_pass < cus ? n_pass : cus), C::NWAVES * 64, 0, st>>>(a, n_pass);
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

}  // namespace tgtc
