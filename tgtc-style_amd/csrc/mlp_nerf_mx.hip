// Fused positional encoding + NeRF MLP in TGTC_PREC_FP16_FP6 (see mlp_mx.h for the arithmetic, mlp_nerf.hip for
// the network: reference models.py:63-117 MLP_style inside :182-223 StyleNerf).
#define TGTC_ASM_DMA 1  // see mlp_core.h lds_dma16
#include "mlp_nerf_mx.h"

#include <algorithm>
#include <cstdlib>
#include <initializer_list>

#include "mlp_layouts.h"
#include "mlp_mx.h"
#include "mlp_mx_pack.h"
#include "mlp_nerf_mx_chain.h"

namespace tgtc {

using CfgMx = MlpCfg<8, 1, false, 4>;

template <int IN_MODE, bool FULL>
__global__ void __launch_bounds__(512, 2) nerf_mx_kernel(NerfArgs a) {
    using C = CfgMx;
    constexpr int NQ = nerf_mx_groups(FULL);
    constexpr int NUNITS = nerf_mx_units(FULL);

    // ring | biases + row exponents
    __shared__ __attribute__((aligned(16))) char smem[C::RING_BYTES + kNerfBiasBytes];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, n = lane & 15;
    const long long s_wave = (long long)blockIdx.x * C::SAMPLES_PER_WG + wave * C::SAMPLES_PER_WAVE;

    // ---- 1. inputs
    double pos[1][3], dir[1][3];
    long long sidx[1];
    nerf_load_samples<1, IN_MODE>(a, s_wave, n, pos, dir, sidx);
    half8 pe_h[2][1], pe_l[2][1], de_h[1][1], de_l[1][1];
    if constexpr (IN_MODE == IN_ENC) nerf_load_encoded<1, true, false>(a, sidx, g, pe_h, pe_l, de_h, de_l);

    // ---- 2. bias / row-exponent table, then the first 8 chunks of the weight stream
    MxReader<C, SingleStreamMap<NUNITS>, kNerfMxTable> rd;
    const char* const streams[1] = {a.stream};
    rd.init(streams, smem, wave, lane);
#pragma unroll
    for (int j = 0; j < kNerfBiasBytes / (C::NWAVES * 1024); ++j)
        lds_dma16(a.bias + (j * C::NWAVES + wave) * 1024 + lane * 16, smem + C::RING_BYTES + (j * C::NWAVES + wave) * 1024);
    rd.ring.prologue();

    // ---- 3. positional encoding (hi + lo fp16 B fragments)
    // (points only: the direction is encoded in front of the colour head, nerf_encode_dir_late)
    if constexpr (IN_MODE != IN_ENC) nerf_encode<1, true, false>(a, pos, dir, sidx, g, pe_h, pe_l, de_h, de_l);
    const half8 Ph[2] = {pe_h[0][0], pe_h[1][0]}, Pl[2] = {pe_l[0][0], pe_l[1][0]};

    const lds_cptr bias_lane = opaque((lds_cptr)smem + C::RING_BYTES + 16 * g);
    const lds_cptr rs_lane = opaque((lds_cptr)smem + C::RING_BYTES + kNerfMxScaleOff + 2 * n);
    rd.template start<0, NQ>();

    // ---- 4. the twelve layers
    nerf_chain_mx<C, FULL>(
        rd, bias_lane, rs_lane, Ph, Pl,
        [&](half8& dh, half8& dl) {
            nerf_encode_dir_late<IN_MODE, true>(a, sidx[0], g, de_h[0][0], de_l[0][0]);
            dh = de_h[0][0], dl = de_l[0][0];
        },
        [&](float sigma) {
            if (g == 0 && a.sigma && sidx[0] < a.M) a.sigma[sidx[0]] = sigma;
        },
        [&](auto rt_, auto h_, const float4v& acc) {
            constexpr int rt = decltype(rt_)::value, hf = decltype(h_)::value;
            if (a.remap && sidx[0] < a.M) {
                float* o = a.remap + sidx[0] * 256 + 16 * rt + 4 * g + 2 * hf;
                o[0] = relu(acc[2 * hf]), o[1] = relu(acc[2 * hf + 1]);
            }
        },
        [&](auto h_, const float4v& acc) {
            constexpr int hf = decltype(h_)::value;
            if (g == 0 && a.rgb && sidx[0] < a.M) {
#pragma unroll
                for (int r = 2 * hf; r < (hf ? 3 : 2); ++r) a.rgb[sidx[0] * 3 + r] = 1.0f / (1.0f + expf(-acc[r]));
            }
        });
}



// ------------------------------------------------------------------------------------------------ host
int nerf_mx_pack(const tgtc_linear* layers, std::vector<char>& bias_region, std::vector<char>& stream) {
    const std::vector<LayerSpec> specs = nerf_specs(layers);
    const MxTable& T = kNerfMxTable;
    bias_region.assign(kNerfBiasBytes, 0);
    stream.assign((size_t)T.bytes, 0);
    float* bias = reinterpret_cast<float*>(bias_region.data());
    unsigned short* rowexp = reinterpret_cast<unsigned short*>(bias_region.data() + kNerfMxScaleOff);
    static_assert(kNerfMxScaleOff >= NerfLayout::kBiasFloats * 4 && kNerfMxScaleOff + NerfLayout::kBiasFloats * 2 <= kNerfBiasBytes,
                  "row exponent table must fit behind the biases");
    int qi = 0, b0 = 0;
    for (size_t l = 0; l < specs.size(); ++l) {
        if (qi != T.first[l] || b0 != NerfLayout::bias0((int)l) ||
            !mx_pack_layer(specs[l], kNerfMxShape[l], T, qi, b0, stream.data(), rowexp, bias))
            return fail(TGTC_ERR_UNSUPPORTED, "nerf_create: internal fp16+fp6 layout mismatch at layer %zu", l);
        b0 += 16 * kNerfMxShape[l].rt;
    }
    if (qi != T.n) return fail(TGTC_ERR_UNSUPPORTED, "nerf_create: internal fp16+fp6 group count mismatch");
    return TGTC_OK;
}

// 1 (shipped): FULL launches that do not ask for base_remap go to the two-tile persistent kernel (mlp_nerf_mx2.hip)
#ifndef TGTC_MX2
#define TGTC_MX2 1
#endif

int nerf_mx_launch(int in_mode, bool full, const NerfArgs& a, hipStream_t st) {
    using C = CfgMx;
    if (TGTC_MX2 && full && !a.remap) return nerf_mx2_launch(in_mode, true, a, st);
    if (TGTC_MX2 && !full && in_mode == IN_RAYS && a.sigma && !a.remap && !a.out_pts_enc && !a.out_dirs_enc) return nerf_mx2_launch(in_mode, false, a, st);
    const unsigned nwg = (unsigned)((a.M + C::SAMPLES_PER_WG - 1) / C::SAMPLES_PER_WG);
    const dim3 block(C::NWAVES * 64);
    switch (in_mode * 2 + (full ? 1 : 0)) {
        case IN_RAYS * 2 + 0: nerf_mx_kernel<IN_RAYS, false><<<nwg, block, 0, st>>>(a); break;
        case IN_RAYS * 2 + 1: nerf_mx_kernel<IN_RAYS, true><<<nwg, block, 0, st>>>(a); break;
        case IN_PTS * 2 + 1: nerf_mx_kernel<IN_PTS, true><<<nwg, block, 0, st>>>(a); break;
        case IN_ENC * 2 + 1: nerf_mx_kernel<IN_ENC, true><<<nwg, block, 0, st>>>(a); break;
        default: return fail(TGTC_ERR_UNSUPPORTED, "nerf (fp16+fp6): no kernel for input mode %d, full %d", in_mode, (int)full);
    }
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

}  // namespace tgtc
