// Fused positional encoding + NeRF MLP (reference models.py:63-117 MLP_style inside :182-223 StyleNerf;
// D=8, W=256, skip at 4, view-dependent colour head).  One launch evaluates rgb / sigma for M samples;
// the [M,256] activations of the 11 dense layers never leave registers (mlp_core.h).
#include <cmath>
#include <cstdlib>

#include "mlp_core.h"
#include "mlp_pack.h"
#include "mlp_layouts.h"
#include "mlp_nerf_front.h"
#include "mlp_nerf_chain.h"
#include "mlp_nerf_mx.h"

namespace tgtc {

// ------------------------------------------------------------------------------------------------
// PARK geometry (MlpCfg::PARK): one wave per SIMD with the whole 512-register file.  The layer being produced is
// parked in AGPRs and copied into VGPRs at the layer boundary, where the previous input dies; every MFMA operand
// is an architectural VGPR.  Same arithmetic, same fragment stream and same results as the ping-pong path below.
template <class C>
struct ParkedAct {
    unsigned h[8][C::NCT][4];
    unsigned l[C::SPLIT ? 8 : 1][C::NCT][4];
};

template <class C, int KS>
__device__ __forceinline__ void unpark_act(const ParkedAct<C>& P, half8 (&Xh)[8][C::NCT], half8 (&Xl)[8][C::NCT]) {
#pragma unroll
    for (int k = 0; k < KS; ++k)
#pragma unroll
        for (int c = 0; c < C::NCT; ++c) {
            Xh[k][c] = unpark4(P.h[k][c]);
            if constexpr (C::SPLIT) Xl[k][c] = unpark4(P.l[k][c]);
        }
}

template <class C, int IN_MODE, bool FULL, class WS>
__device__ __forceinline__ void nerf_layers_parked(WS& ws, lds_cptr bias_lane, const NerfArgs& a, const long long (&sidx)[C::NCT],
                                                   int g, half8 (&pe_h)[2][C::NCT], half8 (&pe_l)[2][C::NCT],
                                                   half8 (&de_h)[1][C::NCT], half8 (&de_l)[1][C::NCT]) {
    constexpr int NCT = C::NCT;
    constexpr bool SPLIT = C::SPLIT;
    using L = NerfLayout;
    ParkedAct<C> P;
    half8 Xh[8][NCT], Xl[8][NCT];
    auto to_P = [&](auto rt_, auto c_, auto h_, const float4v& acc) {
        constexpr int rt = decltype(rt_)::value, c = decltype(c_)::value, hf = decltype(h_)::value;
        unsigned ph, pl = 0;
        if constexpr (kAbl & 8) ph = pl = __builtin_bit_cast(unsigned, acc[2 * hf]);
        else pack_act<SPLIT, hf>(acc, ph, pl);
        P.h[rt / 2][c][(rt & 1) * 2 + hf] = park(ph);
        if constexpr (SPLIT) P.l[rt / 2][c][(rt & 1) * 2 + hf] = park(pl);
    };
    dense_layer<C, L::frag0(0), 2, 16, L::bias0(0)>(ws, bias_lane, pe_h, pe_l, to_P);
    // the point encoding is needed again by the skip layer only: park it meanwhile
    unsigned pe_ph[2][NCT][4], pe_pl[2][NCT][4];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int c = 0; c < NCT; ++c) {
            park4(pe_h[k][c], pe_ph[k][c]);
            if constexpr (SPLIT) park4(pe_l[k][c], pe_pl[k][c]);
        }
    unpark_act<C, 8>(P, Xh, Xl);
    dense_layer<C, L::frag0(1), 8, 16, L::bias0(1)>(ws, bias_lane, Xh, Xl, to_P);
    unpark_act<C, 8>(P, Xh, Xl);
    dense_layer<C, L::frag0(2), 8, 16, L::bias0(2)>(ws, bias_lane, Xh, Xl, to_P);
    unpark_act<C, 8>(P, Xh, Xl);
    dense_layer<C, L::frag0(3), 8, 16, L::bias0(3)>(ws, bias_lane, Xh, Xl, to_P);
    unpark_act<C, 8>(P, Xh, Xl);
    dense_layer<C, L::frag0(4), 8, 16, L::bias0(4)>(ws, bias_lane, Xh, Xl, to_P);
    {
        // skip layer: reference input is cat(pe, h) (models.py:98-99); k order here is [h | pe]
        half8 Bh[10][NCT], Bl[10][NCT];
#pragma unroll
        for (int c = 0; c < NCT; ++c) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                Bh[k][c] = unpark4(P.h[k][c]);
                if constexpr (SPLIT) Bl[k][c] = unpark4(P.l[k][c]);
            }
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                Bh[8 + k][c] = unpark4(pe_ph[k][c]);
                if constexpr (SPLIT) Bl[8 + k][c] = unpark4(pe_pl[k][c]);
            }
        }
        dense_layer<C, L::frag0(5), 10, 16, L::bias0(5)>(ws, bias_lane, Bh, Bl, to_P);
    }
    unpark_act<C, 8>(P, Xh, Xl);
    dense_layer<C, L::frag0(6), 8, 16, L::bias0(6)>(ws, bias_lane, Xh, Xl, to_P);
    unpark_act<C, 8>(P, Xh, Xl);
    dense_layer<C, L::frag0(7), 8, 16, L::bias0(7)>(ws, bias_lane, Xh, Xl, to_P);
    unpark_act<C, 8>(P, Xh, Xl);
    dense_layer<C, L::frag0(8), 8, 1, L::bias0(8)>(ws, bias_lane, Xh, Xl, [&](auto, auto c_, auto h_, const float4v& acc) {
        constexpr int c = decltype(c_)::value;
        if constexpr (decltype(h_)::value == 0)
            if (g == 0 && a.sigma && sidx[c] < a.M) a.sigma[sidx[c]] = acc[0];
    });
    if constexpr (FULL) {
        dense_layer<C, L::frag0(9), 8, 16, L::bias0(9)>(ws, bias_lane, Xh, Xl, [&](auto rt_, auto c_, auto h_, const float4v& acc) {
            constexpr int rt = decltype(rt_)::value, c = decltype(c_)::value, hf = decltype(h_)::value;
            to_P(rt_, c_, h_, acc);
            if (a.remap && sidx[c] < a.M) {
                float* o = a.remap + sidx[c] * 256 + 16 * rt + 4 * g + 2 * hf;
                o[0] = relu(acc[2 * hf]), o[1] = relu(acc[2 * hf + 1]);
            }
        });
        {
            half8 Bh[9][NCT], Bl[9][NCT];
#pragma unroll
            for (int c = 0; c < NCT; ++c) {
                nerf_encode_dir_late<IN_MODE, SPLIT>(a, sidx[c], g, de_h[0][c], de_l[0][c]);
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    Bh[k][c] = unpark4(P.h[k][c]);
                    if constexpr (SPLIT) Bl[k][c] = unpark4(P.l[k][c]);
                }
                Bh[8][c] = de_h[0][c], Bl[8][c] = de_l[0][c];
            }
            dense_layer<C, L::frag0(10), 9, 8, L::bias0(10)>(ws, bias_lane, Bh, Bl, to_P);
        }
        half8 Zh[4][NCT], Zl[4][NCT];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < NCT; ++c) {
                Zh[k][c] = unpark4(P.h[k][c]);
                if constexpr (SPLIT) Zl[k][c] = unpark4(P.l[k][c]);
            }
        dense_layer<C, L::frag0(11), 4, 1, L::bias0(11)>(ws, bias_lane, Zh, Zl, [&](auto, auto c_, auto h_, const float4v& acc) {
            constexpr int c = decltype(c_)::value, hf = decltype(h_)::value;
            if (g == 0 && a.rgb && sidx[c] < a.M) {
#pragma unroll
                for (int r = 2 * hf; r < (hf ? 3 : 2); ++r) a.rgb[sidx[c] * 3 + r] = 1.0f / (1.0f + expf(-acc[r]));
            }
        });
    }
}

template <class C, int IN_MODE, bool FULL>
__global__ void __launch_bounds__(C::NWAVES * 64, C::NWAVES * C::WG_PER_CU / 4) nerf_mlp_kernel(NerfArgs a) {
    constexpr int NCT = C::NCT;
    constexpr bool SPLIT = C::SPLIT;
    constexpr int NFRAG = FULL ? NerfLayout::kFragsFull : NerfLayout::kFragsSigma;
    using L = NerfLayout;

    // ALL LDS in one array (a second __shared__ object makes hipcc drain vmcnt before LDS reads).
    __shared__ __attribute__((aligned(16))) char smem[C::RING_BYTES + kNerfBiasBytes];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, n = lane & 15;
    const long long s_wave = (long long)blockIdx.x * C::SAMPLES_PER_WG + wave * C::SAMPLES_PER_WAVE;

    // ---- 1. inputs (ordinary loads first: once LDS-DMA is in flight hipcc drains vmcnt(0) for them)
    double pos[NCT][3], dir[NCT][3];
    long long sidx[NCT];
    nerf_load_samples<NCT, IN_MODE>(a, s_wave, n, pos, dir, sidx);
    half8 pe_h[2][NCT], pe_l[2][NCT], de_h[1][NCT], de_l[1][NCT];
    if constexpr (IN_MODE == IN_ENC) nerf_load_encoded<NCT, SPLIT, false>(a, sidx, g, pe_h, pe_l, de_h, de_l);

    // ---- 2. start the weight stream: bias table, then the first 8 chunks
    WeightStream<C, SingleStreamMap<NFRAG>> ws;
    const char* const streams[1] = {a.stream};
    ws.init(streams, smem, wave, lane);
#pragma unroll
    for (int j = 0; j < kNerfBiasBytes / (C::NWAVES * 1024); ++j)
        lds_dma16(a.bias + (j * C::NWAVES + wave) * 1024 + lane * 16, smem + C::RING_BYTES + (j * C::NWAVES + wave) * 1024);
    ws.prologue();

    // ---- 3. positional encoding into B fragments (overlaps the prefetch latency)
    // (points only: the direction is encoded in front of the colour head, nerf_encode_dir_late -- eight to sixteen
    // registers that would otherwise sit idle through eleven layers)
    if constexpr (IN_MODE != IN_ENC) nerf_encode<NCT, SPLIT, false>(a, pos, dir, sidx, g, pe_h, pe_l, de_h, de_l);

    const lds_cptr bias_lane = opaque((lds_cptr)smem + C::RING_BYTES + 16 * g);
    ws.start();
    if constexpr (C::PARK) {
        nerf_layers_parked<C, IN_MODE, FULL>(ws, bias_lane, a, sidx, g, pe_h, pe_l, de_h, de_l);
        return;
    }

    // ---- 4. the twelve layers
    nerf_chain<C, FULL>(
        ws, bias_lane, pe_h, pe_l,
        [&](auto c_, half8& dh, half8& dl) {
            constexpr int c = decltype(c_)::value;
            nerf_encode_dir_late<IN_MODE, SPLIT>(a, sidx[c], g, de_h[0][c], de_l[0][c]);
            dh = de_h[0][c], dl = de_l[0][c];
        },
        [&](auto c_, float sigma) {
            constexpr int c = decltype(c_)::value;
            if (g == 0 && a.sigma && sidx[c] < a.M) a.sigma[sidx[c]] = sigma;
        },
        [&](auto rt_, auto c_, auto h_, const float4v& acc) {
            constexpr int rt = decltype(rt_)::value, c = decltype(c_)::value, hf = decltype(h_)::value;
            if (a.remap && sidx[c] < a.M) {
                float* o = a.remap + sidx[c] * 256 + 16 * rt + 4 * g + 2 * hf;
                o[0] = relu(acc[2 * hf]), o[1] = relu(acc[2 * hf + 1]);
            }
        },
        [&](auto c_, auto h_, const float4v& acc) {
            constexpr int c = decltype(c_)::value, hf = decltype(h_)::value;
            if (g == 0 && a.rgb && sidx[c] < a.M) {
#pragma unroll
                for (int r = 2 * hf; r < (hf ? 3 : 2); ++r) a.rgb[sidx[c] * 3 + r] = 1.0f / (1.0f + expf(-acc[r]));
            }
        });
}

// ------------------------------------------------------------------------------------------------ host
#ifndef TGTC_TU_FP16_ONLY
std::vector<LayerSpec> nerf_specs(const tgtc_linear* l) {
    std::vector<LayerSpec> v;
    auto add = [&](int idx, std::vector<Seg> segs) {
        v.push_back(LayerSpec{l[idx].weight, l[idx].bias, l[idx].out_features, l[idx].in_features, std::move(segs)});
    };
    add(0, {{SEG_PE63, 0, 2}});
    for (int i = 1; i <= 4; ++i) add(i, {{SEG_ACT, 0, 8}});
    add(5, {{SEG_ACT, 63, 8}, {SEG_PE63, 0, 2}});  // reference column order: [pe(63) | h(256)]
    add(6, {{SEG_ACT, 0, 8}});
    add(7, {{SEG_ACT, 0, 8}});
    add(8, {{SEG_ACT, 0, 8}});                       // sigma_layer
    add(9, {{SEG_ACT, 0, 8}});                       // base_remap_layer
    add(10, {{SEG_ACT, 0, 8}, {SEG_PE27, 256, 1}});  // rgb_layers.0 on [remap(256) | dirs(27)]
    add(11, {{SEG_ACT, 0, 4}});                      // rgb_layers.1
    return v;
}

#endif

template <class C, int IN_MODE, bool FULL>
int launch_nerf(const NerfArgs& a, hipStream_t st) {
    const long long nwg = (a.M + C::SAMPLES_PER_WG - 1) / C::SAMPLES_PER_WG;
    if (a.M >= 0x7fffffffLL) return fail(TGTC_ERR_UNSUPPORTED, "nerf: too many samples in one launch (%lld)", a.M);
    nerf_mlp_kernel<C, IN_MODE, FULL><<<(unsigned)nwg, C::NWAVES * 64, 0, st>>>(a);
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

// Geometry chosen by measurement (tools/bench_variants.sh, profiles/r1_kernel_variants.md): 8 waves per
// workgroup = 2 per SIMD, every MFMA operand in arch VGPRs (<= 256 registers per wave).  MFMAs whose B
// operand sits in the accumulator half of the register file issue ~25 % slower (tools/microbench/mfma_regs),
// which is what the 4-wave / 4-column-tile geometry (470-510 registers) ran into.
using CfgFast = MlpCfg<8, 2, false, 4>;
using CfgExact = MlpCfg<8, 1, true, 4>;

#define TGTC_NERF_FP16_INSTANCES(PREFIX)                                           \
    PREFIX template int launch_nerf<CfgFast, IN_RAYS, false>(const NerfArgs&, hipStream_t); \
    PREFIX template int launch_nerf<CfgFast, IN_RAYS, true>(const NerfArgs&, hipStream_t);  \
    PREFIX template int launch_nerf<CfgFast, IN_PTS, true>(const NerfArgs&, hipStream_t);   \
    PREFIX template int launch_nerf<CfgFast, IN_ENC, true>(const NerfArgs&, hipStream_t);
#ifdef TGTC_TU_FP16_ONLY
TGTC_NERF_FP16_INSTANCES()
}  // namespace tgtc
#else
#ifndef TGTC_DEV_VARIANT   // development builds compile their one configuration here and leave mlp_nerf_fp16.o out
TGTC_NERF_FP16_INSTANCES(extern)
#endif

// 1 (shipped): sigma-only fp16x3 launches over rays (the coarse pass of a render) go to the two-tile persistent kernel (mlp_nerf_x3s.hip)
#ifndef TGTC_X3S
#define TGTC_X3S 1
#endif

template <int IN_MODE, bool FULL>
static int dispatch_nerf(const tgtc_net* net, NerfArgs& a, hipStream_t st) {
    a.bias = net->dev;
    a.stream = net->dev + net->bias_bytes;
#ifdef TGTC_DEV_VARIANT   // development builds: only the hot-path kernels of one experimental configuration
    if constexpr (IN_MODE == IN_RAYS) {
        if (net->precision == (TGTC_DEV_VARIANT::SPLIT ? TGTC_PREC_FP16X3 : TGTC_PREC_FP16))
            return launch_nerf<TGTC_DEV_VARIANT, IN_MODE, FULL>(a, st);
    }
    return fail(TGTC_ERR_UNSUPPORTED, "development build: kernel not compiled");
#else
    if (net->precision == TGTC_PREC_FP16_FP6) {
        if (a.M >= 0x7fffffffLL) return fail(TGTC_ERR_UNSUPPORTED, "nerf: too many samples in one launch (%lld)", a.M);
        return nerf_mx_launch(IN_MODE, FULL, a, st);
    }
    if (net->precision == TGTC_PREC_FP16) return launch_nerf<CfgFast, IN_MODE, FULL>(a, st);
    if constexpr (TGTC_X3S && IN_MODE == IN_RAYS && !FULL) {   // the coarse pass: sigma only, no encodings out
        if (a.sigma && !a.out_pts_enc && !a.out_dirs_enc) {
            if (a.M >= 0x7fffffffLL) return fail(TGTC_ERR_UNSUPPORTED, "nerf: too many samples in one launch (%lld)", a.M);
            return nerf_x3s_launch(a, st);
        }
    }
    return launch_nerf<CfgExact, IN_MODE, FULL>(a, st);
#endif
}

int nerf_forward_rays_impl(const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts, int64_t R,
                           int N, float* rgb, float* sigma, hipStream_t st) {
    NerfArgs a{};
    a.M = R * (int64_t)N, a.N = N, a.rays_o = rays_o, a.rays_d = rays_d, a.ts = ts, a.rgb = rgb, a.sigma = sigma;
    return rgb ? dispatch_nerf<IN_RAYS, true>(net, a, st) : dispatch_nerf<IN_RAYS, false>(net, a, st);
}

// rgb[live[i]] -- and sigma[live[i]] where sigma is given -- for the *n_live samples of a device-side list (the caller has
// checked the precision and R x N < 2^31)
int nerf_forward_list_impl(const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts, int64_t R, int N,
                           const uint32_t* live, const uint32_t* n_live, float* rgb, float* sigma, hipStream_t st) {
    NerfArgs a{};
    a.M = R * (int64_t)N, a.N = N, a.rays_o = rays_o, a.rays_d = rays_d, a.ts = ts, a.rgb = rgb, a.sigma = sigma;
    a.live = live, a.n_live = n_live;
    a.bias = net->dev;
    a.stream = net->dev + net->bias_bytes;
    return nerf_mx_launch(IN_LIST, true, a, st);
}

// The same for fp16x3 handles (mlp_nerf_x3_list.hip): the bits of the dense full launch at the listed samples
// (the caller has checked the precision and R x N < 2^31)
int nerf_forward_list_x3_impl(const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts, int64_t R, int N,
                              const uint32_t* live, const uint32_t* n_live, float* rgb, float* sigma, hipStream_t st) {
    NerfArgs a{};
    a.M = R * (int64_t)N, a.N = N, a.rays_o = rays_o, a.rays_d = rays_d, a.ts = ts, a.rgb = rgb, a.sigma = sigma;
    a.live = live, a.n_live = n_live;
    a.bias = net->dev;
    a.stream = net->dev + net->bias_bytes;
    return nerf_x3_list_launch(a, st);
}

// sigma[live[i]] for the *n_live samples of a device-side list, fp16x3 handles: the bits of the sigma-only launch over rays
// (the caller has checked the precision and R x N < 2^31)
int nerf_sigma_list_impl(const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts, int64_t R, int N,
                         const uint32_t* live, const uint32_t* n_live, float* sigma, hipStream_t st) {
    NerfArgs a{};
    a.M = R * (int64_t)N, a.N = N, a.rays_o = rays_o, a.rays_d = rays_d, a.ts = ts, a.sigma = sigma;
    a.live = live, a.n_live = n_live;
    a.bias = net->dev;
    a.stream = net->dev + net->bias_bytes;
    return nerf_x3s_list_launch(a, st);
}

// The same for fp16mx handles: the bits of their sigma-only launch over rays and of the FULL kernels' sigma
// (mlp_nerf_mx2.hip, the <IN_LIST, false> instance; the caller has checked the precision and R x N < 2^31)
int nerf_sigma_list_mx_impl(const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts, int64_t R, int N,
                            const uint32_t* live, const uint32_t* n_live, float* sigma, hipStream_t st) {
    NerfArgs a{};
    a.M = R * (int64_t)N, a.N = N, a.rays_o = rays_o, a.rays_d = rays_d, a.ts = ts, a.sigma = sigma;
    a.live = live, a.n_live = n_live;
    a.bias = net->dev;
    a.stream = net->dev + net->bias_bytes;
    return nerf_mx2_launch(IN_LIST, false, a, st);
}

// The density screen: sigma of every sample from the handle's TGTC_PREC_FP16 form, one MFMA product per
// weight (the caller has checked that the screen is enabled).  Its kernel is the four-tile persistent stream of
// mlp_nerf_fp16s.hip; with TGTC_SCREEN_CFGFAST=1 in the environment (read at every call: the yardstick the stream is held
// against, in timing and in tests) it is the sigma-only launch an fp16 handle runs.  The densities are the same bits either
// way, but for samples whose position is outside the screen's box |p| <= kScreenBox or not finite: the stream gives them NaN (a
// candidate of every screened pass), CfgFast the density of its arithmetic, which is finite even for a NaN (the fp16 ReLU).
int nerf_screen_rays_impl(const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts, int64_t R, int N,
                          float* sigma, hipStream_t st) {
    NerfArgs a{};
    a.M = R * (int64_t)N, a.N = N, a.rays_o = rays_o, a.rays_d = rays_d, a.ts = ts, a.sigma = sigma;
    a.bias = net->screen->dev;
    a.stream = net->screen->dev + kNerfBiasBytes;
    const char* e = std::getenv("TGTC_SCREEN_CFGFAST");
    if (e && e[0] == '1') return launch_nerf<CfgFast, IN_RAYS, false>(a, st);
    return nerf_fp16s_launch(a, st);
}

// ---- the stashed two-phase fine pass (mlp_nerf_mx2_stash.hip).  scratch: kSparseScratchBytes laid out as the compaction's
// (word 0 the overflow list's length, the counts from kStashCountWord on: launch_live_stat sums them as they are)
constexpr int kStashCountWord = 64;
static_assert((kStashCountWord + kNerfStashRegions) * sizeof(uint32_t) <= kSparseScratchBytes, "counts must fit the scratch");

static NerfStashArgs stash_args(const tgtc_net* net, uint32_t* scratch, uint32_t* ovf) {
    return NerfStashArgs{net->stash, net->stash_cap, net->stash_stride, scratch + kStashCountWord, scratch, ovf};
}

// densities of all samples; layer 7's output of the live ones into the handle's stash, the rest of them into the list ovf
// (length scratch[0]); scratch is zeroed here
int nerf_stash_fill_impl(const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts, int64_t R, int N,
                         float* sigma, uint32_t* scratch, uint32_t* ovf, hipStream_t st) {
    NerfArgs a{};
    a.M = R * (int64_t)N, a.N = N, a.rays_o = rays_o, a.rays_d = rays_d, a.ts = ts, a.sigma = sigma;
    a.bias = net->dev;
    a.stream = net->dev + net->bias_bytes;
    TGTC_HIP_CHECK(hipMemsetAsync(scratch, 0, kSparseScratchBytes, st));
    return nerf_mx2_stash_launch(a, stash_args(net, scratch, ovf), st);
}

// rgb[s] of the samples the stash holds (scratch as nerf_stash_fill_impl left it)
int nerf_stash_heads_impl(const tgtc_net* net, const double* rays_o, const double* rays_d, int64_t R, int N, uint32_t* scratch,
                          float* rgb, hipStream_t st) {
    NerfArgs a{};
    a.M = R * (int64_t)N, a.N = N, a.rays_o = rays_o, a.rays_d = rays_d, a.rgb = rgb;
    a.bias = net->dev;
    a.stream = net->dev + net->heads_off;
    return nerf_mx2_heads_launch(a, stash_args(net, scratch, nullptr), st);
}

}  // namespace tgtc

using namespace tgtc;

extern "C" int tgtc_nerf_create(const tgtc_linear* layers, int n_layers, int precision, tgtc_net** out) {
    TGTC_REQUIRE(layers && out, "nerf_create: null argument");
    TGTC_REQUIRE(precision == TGTC_PREC_FP16 || precision == TGTC_PREC_FP16X3 || precision == TGTC_PREC_FP16_FP6,
                 "nerf_create: unknown precision %d", precision);
    static const int want[12][2] = {{256, 63},  {256, 256}, {256, 256}, {256, 256}, {256, 256}, {256, 319},
                                    {256, 256}, {256, 256}, {1, 256},   {256, 256}, {128, 283}, {3, 128}};
    if (n_layers != 12) return fail(TGTC_ERR_UNSUPPORTED, "nerf_create: expected the 12 linears of MLP_style (D=8), got %d", n_layers);
    for (int i = 0; i < 12; ++i) {
        TGTC_REQUIRE(layers[i].weight && layers[i].bias, "nerf_create: layer %d has a null pointer", i);
        if (layers[i].out_features != want[i][0] || layers[i].in_features != want[i][1])
            return fail(TGTC_ERR_UNSUPPORTED, "nerf_create: layer %d is %dx%d, kernels are built for %dx%d (D=8, W=256, PE 10/4, viewdirs)",
                        i, layers[i].out_features, layers[i].in_features, want[i][0], want[i][1]);
    }
    std::vector<char> bias_region, stream, heads;
    int n_frags = 0;
    // per-feature scales of the ReLU trunk balanced by powers of two first (mlp_pack.h, EqualisedNet): the same function,
    // numbers that every precision mode represents well.  base_remap's rows stay: it is an output of the operator.
    EqualisedNet eq;
    eq.copy(layers, 12);
    for (int l = 0; l < 7; ++l) eq.run(l, {{l + 1, l + 1 == 5 ? 63 : 0}});   // layer 5 reads cat(pe(63), h) (models.py:98-99)
    eq.run(7, {{8, 0}, {9, 0}});                                              // sigma_layer and base_remap_layer read h
    eq.run(10, {{11, 0}});                                                    // rgb_layers.0 -> rgb_layers.1
    layers = eq.lin.data();
    if (precision == TGTC_PREC_FP16_FP6) {
        const int rc = nerf_mx_pack(layers, bias_region, stream);
        if (rc != TGTC_OK) return rc;
        nerf_mx_heads_stream(stream, heads);
    } else {
        PackedNet p = pack_layers(nerf_specs(layers), precision == TGTC_PREC_FP16X3);
        if (p.n_frags != NerfLayout::kFragsFull || (int)p.bias.size() != NerfLayout::kBiasFloats)
            return fail(TGTC_ERR_UNSUPPORTED, "nerf_create: internal layout mismatch (%d frags, %zu bias)", p.n_frags, p.bias.size());
        for (int i = 0; i < 12; ++i)
            if (p.frag0[i] != NerfLayout::frag0(i) || p.bias0[i] != NerfLayout::bias0(i))
                return fail(TGTC_ERR_UNSUPPORTED, "nerf_create: internal layout mismatch at layer %d", i);
        bias_region.assign(kNerfBiasBytes, 0);
        std::memcpy(bias_region.data(), p.bias.data(), p.bias.size() * sizeof(float));
        stream.assign(reinterpret_cast<const char*>(p.stream.data()),
                      reinterpret_cast<const char*>(p.stream.data()) + p.stream.size() * sizeof(half_t));
        n_frags = p.n_frags;
    }
    tgtc_net* net = new tgtc_net();
    net->kind = 0, net->precision = precision;
    {
        void* word = nullptr;   // the pinned word of the live statistic (render.hip, fine_pass)
        hipError_t eh = hipHostMalloc(&word, sizeof(uint64_t), hipHostMallocDefault);
        if (eh != hipSuccess) {
            delete net;
            return fail(TGTC_ERR_HIP, "nerf_create: hipHostMalloc: %s", hipGetErrorString(eh));
        }
        *static_cast<uint64_t*>(word) = 0;
        net->cull = new tgtc_cull_state{TGTC_CULL_AUTO, static_cast<volatile uint64_t*>(word), 0, 0};
    }
    net->bias_bytes = kNerfBiasBytes;
    net->stream_bytes = stream.size();
    net->n_frags = n_frags;
    // + one ring of slack: the fused ray kernel rounds a pass up to a whole number of rings and fetches (never reads)
    // the chunks behind the stream's end (mlp_core.h, WeightStream PERSIST)
    // fp16mx: + the heads' own stream (REMAP / C0 / C1 again, whole rings: the stashed fine pass, mlp_nerf_mx2_stash.hip)
    net->heads_off = net->bias_bytes + net->stream_bytes + kRingBytes;
    size_t total = net->heads_off + heads.size();
    hipError_t e = hipMalloc((void**)&net->dev, total);
    if (e != hipSuccess) {
        (void)hipHostFree(const_cast<uint64_t*>(net->cull->landed));
        delete net->cull;
        delete net;
        return fail(TGTC_ERR_HIP, "nerf_create: hipMalloc(%zu): %s", total, hipGetErrorString(e));
    }
    std::vector<char> host(total, 0);
    std::memcpy(host.data(), bias_region.data(), bias_region.size());
    std::memcpy(host.data() + net->bias_bytes, stream.data(), net->stream_bytes);
    if (!heads.empty()) std::memcpy(host.data() + net->heads_off, heads.data(), heads.size());
    e = hipMemcpy(net->dev, host.data(), total, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(net->dev);
        (void)hipHostFree(const_cast<uint64_t*>(net->cull->landed));
        delete net->cull;
        delete net;
        return fail(TGTC_ERR_HIP, "nerf_create: hipMemcpy: %s", hipGetErrorString(e));
    }
    if (precision != TGTC_PREC_FP16) {
        // what tgtc_net_enable_screen packs from (vectors keep their buffers when moved: eq.lin still points into them)
        net->screen = new tgtc_screen_state();
        net->screen->eq = std::move(eq);
    }
    *out = net;
    return TGTC_OK;
}

// ---- the density screen of a handle
namespace {
// the calibration's rays: a fixed 64-bit generator (splitmix64), so that a handle's margin is a function of its weights alone
struct ScreenRng {
    uint64_t s;
    double uniform() {   // [0, 1)
        uint64_t z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        z ^= z >> 31;
        return (double)(z >> 11) * (1.0 / 9007199254740992.0);
    }
};
constexpr int kScreenCalRays = 256, kScreenCalDepths = 128;
constexpr float kScreenMarginFactor = 8.0f;

struct DeviceBuf {   // freed on every way out of the calibration
    void* p = nullptr;
    ~DeviceBuf() {
        if (p) (void)hipFree(p);
    }
};
}  // namespace

extern "C" int tgtc_net_enable_screen(tgtc_net* net, void* stream) {
    TGTC_REQUIRE(net, "net_enable_screen: null handle");
    if (net->kind != 0 || net->precision == TGTC_PREC_FP16 || !net->screen)
        return fail(TGTC_ERR_UNSUPPORTED, "net_enable_screen: built for NeRF handles in fp16x3 or fp16mx (an fp16 handle is its own screen)");
    tgtc_screen_state* const s = net->screen;
    if (s->dev) return TGTC_OK;
    // 1. the TGTC_PREC_FP16 form of the handle's equalised layers: tgtc_nerf_create's bias table and stream for that precision
    PackedNet p = pack_layers(nerf_specs(s->eq.lin.data()), false);
    if (p.n_frags != NerfLayout::kFragsFull || (int)p.bias.size() != NerfLayout::kBiasFloats)
        return fail(TGTC_ERR_UNSUPPORTED, "net_enable_screen: internal layout mismatch (%d frags, %zu bias)", p.n_frags, p.bias.size());
    const size_t stream_bytes = p.stream.size() * sizeof(half_t), total = kNerfBiasBytes + stream_bytes + kRingBytes;
    std::vector<char> host(total, 0);
    std::memcpy(host.data(), p.bias.data(), p.bias.size() * sizeof(float));
    std::memcpy(host.data() + kNerfBiasBytes, p.stream.data(), stream_bytes);
    DeviceBuf form;
    TGTC_HIP_CHECK(hipMalloc(&form.p, total));
    TGTC_HIP_CHECK(hipMemcpy(form.p, host.data(), total, hipMemcpyHostToDevice));
    // 2. the calibration: screen and exact densities of 256 fixed rays x 128 depths on [0, 1] that fill the screen's box --
    // every ray runs between two points uniform in it (both 2^-40 relative inside the faces: whatever o + t d rounds to is
    // inside), so the margin speaks for exactly the positions the screen's kernel accepts (kScreenBox, mlp_nerf_mx.h)
    constexpr int R = kScreenCalRays, N = kScreenCalDepths;
    constexpr double kHalf = kScreenBox * (1.0 - 0x1p-40);
    std::vector<double> rays(2 * R * 3);
    std::vector<float> ts((size_t)R * N);
    ScreenRng rng{0x7467746373637265ull};
    for (int r = 0; r < R; ++r) {
        double* o = &rays[r * 3], *d = &rays[(R + r) * 3];
        for (int k = 0; k < 3; ++k) o[k] = kHalf * (2.0 * rng.uniform() - 1.0);
        for (int k = 0; k < 3; ++k) d[k] = kHalf * (2.0 * rng.uniform() - 1.0) - o[k];
        for (int i = 0; i < N; ++i) ts[(size_t)r * N + i] = (float)i / (float)(N - 1);
    }
    DeviceBuf d_rays, d_ts, d_sigma;
    TGTC_HIP_CHECK(hipMalloc(&d_rays.p, rays.size() * sizeof(double)));
    TGTC_HIP_CHECK(hipMalloc(&d_ts.p, ts.size() * sizeof(float)));
    TGTC_HIP_CHECK(hipMalloc(&d_sigma.p, 2 * ts.size() * sizeof(float)));
    TGTC_HIP_CHECK(hipMemcpy(d_rays.p, rays.data(), rays.size() * sizeof(double), hipMemcpyHostToDevice));
    TGTC_HIP_CHECK(hipMemcpy(d_ts.p, ts.data(), ts.size() * sizeof(float), hipMemcpyHostToDevice));
    hipStream_t st = as_stream(stream);
    const double* const ro = static_cast<const double*>(d_rays.p);
    float* const sig = static_cast<float*>(d_sigma.p);
    s->dev = static_cast<char*>(form.p);   // (nerf_screen_rays_impl reads it; taken back below where the calibration fails)
    int rc = nerf_screen_rays_impl(net, ro, ro + R * 3, static_cast<const float*>(d_ts.p), R, N, sig, st);
    s->dev = nullptr;
    if (rc) return rc;
    rc = nerf_forward_rays_impl(net, ro, ro + R * 3, static_cast<const float*>(d_ts.p), R, N, nullptr, sig + ts.size(), st);
    if (rc) return rc;
    TGTC_HIP_CHECK(hipStreamSynchronize(st));
    std::vector<float> sigma(2 * ts.size());
    TGTC_HIP_CHECK(hipMemcpy(sigma.data(), sig, sigma.size() * sizeof(float), hipMemcpyDeviceToHost));
    float err = 0.0f;
    bool finite = true;
    for (size_t i = 0; i < ts.size(); ++i) {
        const float e = std::fabs(sigma[i] - sigma[ts.size() + i]);
        finite = finite && std::isfinite(e);
        err = std::fmax(err, e);
    }
    const float margin = kScreenMarginFactor * err;
    // a network whose two forms agree exactly (a constant density) or whose densities are not finite has no margin to
    // screen by: the screen stays disabled and the handle renders as it did
    if (!finite || !(err > 0.0f) || !std::isfinite(margin)) return TGTC_OK;
    if (!s->landed) {
        void* word = nullptr;
        TGTC_HIP_CHECK(hipHostMalloc(&word, sizeof(uint64_t), hipHostMallocDefault));
        *static_cast<uint64_t*>(word) = 0;
        s->landed = static_cast<volatile uint64_t*>(word);
    }
    s->margin = margin;
    s->dev = static_cast<char*>(form.p);
    form.p = nullptr;
    return TGTC_OK;
}

extern "C" float tgtc_net_screen_margin(const tgtc_net* net) {
    return net && net->screen && net->screen->dev ? net->screen->margin : -1.0f;
}

extern "C" int tgtc_net_set_screen(tgtc_net* net, int mode) {
    TGTC_REQUIRE(net && net->kind == 0, "net_set_screen: not a NeRF handle");
    TGTC_REQUIRE(mode == TGTC_SCREEN_AUTO || mode == TGTC_SCREEN_OFF || mode == TGTC_SCREEN_ON, "net_set_screen: bad mode %d", mode);
    if (!net->screen) return fail(TGTC_ERR_UNSUPPORTED, "net_set_screen: an fp16 handle has no screen");
    net->screen->mode = mode;
    return TGTC_OK;
}

extern "C" float tgtc_net_screen_fraction(const tgtc_net* net) {
    if (!net || !net->screen || !net->screen->landed) return -1.0f;
    const uint64_t word = *net->screen->landed;   // one aligned 8-byte read: never half of a copy
    const uint32_t cand = (uint32_t)word, total = (uint32_t)(word >> 32);
    if (total == 0 || cand > total) return -1.0f;
    return (float)((double)cand / (double)total);
}

extern "C" long long tgtc_net_screened_renders(const tgtc_net* net) { return net && net->screen ? net->screen->screened : -1; }

extern "C" int tgtc_nerf_screen_rays(const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts, int64_t R,
                                     int N, float* sigma, void* stream) {
    TGTC_REQUIRE(net && net->kind == 0 && R >= 0 && N >= 1, "nerf_screen_rays: bad argument");
    if (!(net->screen && net->screen->dev))
        return fail(TGTC_ERR_UNSUPPORTED, "nerf_screen_rays: the handle has no screen (tgtc_net_enable_screen)");
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d && ts && sigma, "nerf_screen_rays: null pointer");
    if (R >= ((int64_t)1 << 31) || R * (int64_t)N >= ((int64_t)1 << 31))
        return fail(TGTC_ERR_UNSUPPORTED, "nerf_screen_rays: R x N >= 2^31 (chunk the rays)");
    return nerf_screen_rays_impl(net, rays_o, rays_d, ts, R, N, sigma, as_stream(stream));
}

extern "C" int tgtc_nerf_sigma_list(const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts, int64_t R,
                                    int N, const uint32_t* live, const uint32_t* n_live, float* sigma, void* stream) {
    TGTC_REQUIRE(net && net->kind == 0 && R >= 0 && N >= 1, "nerf_sigma_list: bad argument");
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d && ts && live && n_live && sigma, "nerf_sigma_list: null pointer");
    if (net->precision != TGTC_PREC_FP16X3)
        return fail(TGTC_ERR_UNSUPPORTED, "nerf_sigma_list: built for fp16x3 handles only (got precision %d)", net->precision);
    if (R >= ((int64_t)1 << 31) || R * (int64_t)N >= ((int64_t)1 << 31))
        return fail(TGTC_ERR_UNSUPPORTED, "nerf_sigma_list: R x N >= 2^31 (chunk the rays)");
    return nerf_sigma_list_impl(net, rays_o, rays_d, ts, R, N, live, n_live, sigma, as_stream(stream));
}

extern "C" int tgtc_nerf_sigma_list_mx(const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts, int64_t R,
                                       int N, const uint32_t* live, const uint32_t* n_live, float* sigma, void* stream) {
    TGTC_REQUIRE(net && net->kind == 0 && R >= 0 && N >= 1, "nerf_sigma_list_mx: bad argument");
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d && ts && live && n_live && sigma, "nerf_sigma_list_mx: null pointer");
    if (net->precision != TGTC_PREC_FP16_FP6)
        return fail(TGTC_ERR_UNSUPPORTED, "nerf_sigma_list_mx: built for fp16+fp6 handles only (got precision %d)", net->precision);
    if (R >= ((int64_t)1 << 31) || R * (int64_t)N >= ((int64_t)1 << 31))
        return fail(TGTC_ERR_UNSUPPORTED, "nerf_sigma_list_mx: R x N >= 2^31 (chunk the rays)");
    return nerf_sigma_list_mx_impl(net, rays_o, rays_d, ts, R, N, live, n_live, sigma, as_stream(stream));
}

extern "C" int tgtc_net_destroy(tgtc_net* net) {
    if (!net) return TGTC_OK;
    hipError_t e = net->dev ? hipFree(net->dev) : hipSuccess;   // (waits for the device: no copy into the pinned word is left)
    if (net->cull) {
        (void)hipHostFree(const_cast<uint64_t*>(net->cull->landed));
        delete net->cull;
    }
    if (net->mx) {
        if (net->mx->dev) (void)hipFree(net->mx->dev);
        delete net->mx;
    }
    if (net->screen) {
        if (net->screen->dev) (void)hipFree(net->screen->dev);
        if (net->screen->landed) (void)hipHostFree(const_cast<uint64_t*>(net->screen->landed));
        delete net->screen;
    }
    delete net;
    if (e != hipSuccess) return fail(TGTC_ERR_HIP, "net_destroy: hipFree: %s", hipGetErrorString(e));
    return TGTC_OK;
}

extern "C" int tgtc_net_precision(const tgtc_net* net) { return net ? net->precision : TGTC_ERR_ARG; }

extern "C" int tgtc_net_set_cull(tgtc_net* net, int mode) {
    TGTC_REQUIRE(net && net->kind == 0 && net->cull, "net_set_cull: not a NeRF handle");
    TGTC_REQUIRE(mode == TGTC_CULL_AUTO || mode == TGTC_CULL_OFF || mode == TGTC_CULL_ON, "net_set_cull: bad mode %d", mode);
    net->cull->mode = mode;
    return TGTC_OK;
}

extern "C" size_t tgtc_net_stash_bytes(int64_t R, int nt, float share) {
    if (R <= 0 || nt <= 0 || !(share >= 0.0f)) return 0;
    // a wave of the producer sees 32 samples of every grid-th pass of 128: its region holds `share` of them
    int cus = 0;
    if (cu_count(cus) != TGTC_OK || cus > kNerfStashMaxGrid) cus = kNerfStashMaxGrid;
    const int64_t n_pass = (R * (int64_t)nt + 127) / 128;
    const int64_t grid = n_pass < cus ? n_pass : cus;
    const int64_t per_wave = (n_pass + grid - 1) / grid * 32;
    int64_t cap = (int64_t)std::ceil((double)(share > 1.0f ? 1.0f : share) * (double)per_wave);
    if (cap < 1) cap = 1;
    const size_t stride = (cap * kNerfStashSlotBytes + 15) & ~(size_t)15;
    return stride * kNerfStashRegions;
}

extern "C" int tgtc_net_set_stash(tgtc_net* net, void* ptr, size_t bytes) {
    TGTC_REQUIRE(net && net->kind == 0, "net_set_stash: not a NeRF handle");
    if (!ptr && bytes == 0) {
        net->stash = nullptr, net->stash_cap = 0, net->stash_stride = 0;
        return TGTC_OK;
    }
    if (net->precision != TGTC_PREC_FP16_FP6)
        return fail(TGTC_ERR_UNSUPPORTED, "net_set_stash: built for fp16+fp6 handles only (got precision %d)", net->precision);
    TGTC_REQUIRE(ptr && ((size_t)ptr & 255) == 0, "net_set_stash: the stash must be a device pointer aligned to 256 bytes");
    const size_t stride = bytes / kNerfStashRegions & ~(size_t)15;
    size_t cap = stride / kNerfStashSlotBytes;
    TGTC_REQUIRE(cap >= 1, "net_set_stash: %zu bytes hold no slot in each of the %d regions (need %zu)", bytes, kNerfStashRegions,
                 tgtc_net_stash_bytes(1, 1, 0.0f));
    if (cap > 0x40000000u) cap = 0x40000000u;
    net->stash = static_cast<char*>(ptr), net->stash_cap = (unsigned)cap, net->stash_stride = stride;
    return TGTC_OK;
}

extern "C" int tgtc_nerf_stash_fill(const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts, int64_t R,
                                    int N, float* sigma, uint32_t* scratch, uint32_t* overflow, void* stream) {
    TGTC_REQUIRE(net && net->kind == 0 && R >= 0 && N >= 1, "nerf_stash_fill: bad argument");
    TGTC_REQUIRE(net->stash, "nerf_stash_fill: no stash attached (tgtc_net_set_stash)");
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d && ts && sigma && scratch && overflow, "nerf_stash_fill: null pointer");
    if (R >= ((int64_t)1 << 31) || R * (int64_t)N >= ((int64_t)1 << 31))
        return fail(TGTC_ERR_UNSUPPORTED, "nerf_stash_fill: R x N >= 2^31 (chunk the rays)");
    return nerf_stash_fill_impl(net, rays_o, rays_d, ts, R, N, sigma, scratch, overflow, as_stream(stream));
}

extern "C" int tgtc_nerf_stash_heads(const tgtc_net* net, const double* rays_o, const double* rays_d, int64_t R, int N,
                                     uint32_t* scratch, float* rgb, void* stream) {
    TGTC_REQUIRE(net && net->kind == 0 && R >= 0 && N >= 1, "nerf_stash_heads: bad argument");
    TGTC_REQUIRE(net->stash, "nerf_stash_heads: no stash attached (tgtc_net_set_stash)");
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d && scratch && rgb, "nerf_stash_heads: null pointer");
    if (R >= ((int64_t)1 << 31) || R * (int64_t)N >= ((int64_t)1 << 31))
        return fail(TGTC_ERR_UNSUPPORTED, "nerf_stash_heads: R x N >= 2^31 (chunk the rays)");
    return nerf_stash_heads_impl(net, rays_o, rays_d, R, N, scratch, rgb, as_stream(stream));
}

extern "C" float tgtc_net_live_fraction(const tgtc_net* net) {
    if (!net || !net->cull) return -1.0f;
    const uint64_t word = *net->cull->landed;   // one aligned 8-byte read: never half of a copy
    const uint32_t live = (uint32_t)word, total = (uint32_t)(word >> 32);
    if (total == 0 || live > total) return -1.0f;
    return (float)((double)live / (double)total);
}

extern "C" long long tgtc_net_culled_renders(const tgtc_net* net) { return net && net->cull ? net->cull->culled : -1; }

extern "C" int tgtc_nerf_forward(const tgtc_net* net, const double* pts, const double* dirs, int64_t M, float* rgb,
                                 float* sigma, float* base_remap, float* pts_enc, float* dirs_enc, void* stream) {
    TGTC_REQUIRE(net && net->kind == 0 && M >= 0, "nerf_forward: bad argument");
    if (M == 0) return TGTC_OK;  // empty tensors carry null pointers
    TGTC_REQUIRE(pts && dirs, "nerf_forward: null input");
    NerfArgs a{};
    a.M = M, a.pts = pts, a.dirs = dirs, a.rgb = rgb, a.sigma = sigma, a.remap = base_remap;
    a.out_pts_enc = pts_enc, a.out_dirs_enc = dirs_enc;
    return dispatch_nerf<IN_PTS, true>(net, a, as_stream(stream));
}

extern "C" int tgtc_nerf_mlp_forward(const tgtc_net* net, const float* pts_enc, const float* dirs_enc, int64_t M,
                                     float* rgb, float* sigma, float* base_remap, void* stream) {
    TGTC_REQUIRE(net && net->kind == 0 && M >= 0, "nerf_mlp_forward: bad argument");
    if (M == 0) return TGTC_OK;
    TGTC_REQUIRE(pts_enc && dirs_enc, "nerf_mlp_forward: null input");
    NerfArgs a{};
    a.M = M, a.pts_enc = pts_enc, a.dirs_enc = dirs_enc, a.rgb = rgb, a.sigma = sigma, a.remap = base_remap;
    return dispatch_nerf<IN_ENC, true>(net, a, as_stream(stream));
}

extern "C" int tgtc_nerf_forward_rays(const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts,
                                      int64_t R, int N, float* rgb, float* sigma, void* stream) {
    TGTC_REQUIRE(net && net->kind == 0 && R >= 0 && N >= 1, "nerf_forward_rays: bad argument");
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d && ts && (rgb || sigma), "nerf_forward_rays: null input");
    return nerf_forward_rays_impl(net, rays_o, rays_d, ts, R, N, rgb, sigma, as_stream(stream));
}

extern "C" int tgtc_nerf_forward_list(const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts,
                                      int64_t R, int N, const uint32_t* live, const uint32_t* n_live, float* rgb, void* stream) {
    TGTC_REQUIRE(net && net->kind == 0 && R >= 0 && N >= 1, "nerf_forward_list: bad argument");
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d && ts && live && n_live && rgb, "nerf_forward_list: null pointer");
    if (net->precision != TGTC_PREC_FP16_FP6)
        return fail(TGTC_ERR_UNSUPPORTED, "nerf_forward_list: built for fp16+fp6 handles only (got precision %d)", net->precision);
    if (R >= ((int64_t)1 << 31) || R * (int64_t)N >= ((int64_t)1 << 31))
        return fail(TGTC_ERR_UNSUPPORTED, "nerf_forward_list: R x N >= 2^31 (chunk the rays)");
    return nerf_forward_list_impl(net, rays_o, rays_d, ts, R, N, live, n_live, rgb, nullptr, as_stream(stream));
}

extern "C" int tgtc_nerf_forward_list_sigma(const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts,
                                            int64_t R, int N, const uint32_t* live, const uint32_t* n_live, float* rgb,
                                            float* sigma, void* stream) {
    TGTC_REQUIRE(net && net->kind == 0 && R >= 0 && N >= 1, "nerf_forward_list_sigma: bad argument");
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d && ts && live && n_live && rgb && sigma, "nerf_forward_list_sigma: null pointer");
    if (net->precision != TGTC_PREC_FP16_FP6)
        return fail(TGTC_ERR_UNSUPPORTED, "nerf_forward_list_sigma: built for fp16+fp6 handles only (got precision %d)", net->precision);
    if (R >= ((int64_t)1 << 31) || R * (int64_t)N >= ((int64_t)1 << 31))
        return fail(TGTC_ERR_UNSUPPORTED, "nerf_forward_list_sigma: R x N >= 2^31 (chunk the rays)");
    return nerf_forward_list_impl(net, rays_o, rays_d, ts, R, N, live, n_live, rgb, sigma, as_stream(stream));
}

extern "C" int tgtc_nerf_forward_list_x3(const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts,
                                         int64_t R, int N, const uint32_t* live, const uint32_t* n_live, float* rgb,
                                         float* sigma, void* stream) {
    TGTC_REQUIRE(net && net->kind == 0 && R >= 0 && N >= 1, "nerf_forward_list_x3: bad argument");
    if (R == 0) return TGTC_OK;
    TGTC_REQUIRE(rays_o && rays_d && ts && live && n_live && rgb, "nerf_forward_list_x3: null pointer");
    if (net->precision != TGTC_PREC_FP16X3)
        return fail(TGTC_ERR_UNSUPPORTED, "nerf_forward_list_x3: built for fp16x3 handles only (got precision %d)", net->precision);
    if (R >= ((int64_t)1 << 31) || R * (int64_t)N >= ((int64_t)1 << 31))
        return fail(TGTC_ERR_UNSUPPORTED, "nerf_forward_list_x3: R x N >= 2^31 (chunk the rays)");
    return nerf_forward_list_x3_impl(net, rays_o, rays_d, ts, R, N, live, n_live, rgb, sigma, as_stream(stream));
}
#endif  // TGTC_TU_FP16_ONLY
