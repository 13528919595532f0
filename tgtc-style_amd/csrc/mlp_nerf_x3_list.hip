// The FULL NeRF network in TGTC_PREC_FP16X3 (trunk, sigma head, base_remap, colour head) over a device-side LIST of samples:
// the colour phase of the two-phase fine pass for a fine handle in fp16x3 (render.hip fine_pass).  A pass is the
// body of nerf_mlp_kernel<CfgExact, IN_RAYS, true> (mlp_nerf.hip) on 128 list slots -- the same geometry (eight waves, one
// column tile of 16 samples each, two waves per SIMD), the same nerf_chain<C, true> on SPLIT operands, the same late direction
// encoding, the same weight ring protocol, primed once per pass -- so a listed sample gets the bits the dense launch gives it:
// every sample is a column of the MFMA tiles and independent of its neighbours.  sigma of a FULL launch is the one-tile
// kernel's, which is the sigma-only stream's bit for bit (mlp_nerf_x3s.hip).
// Persistent: one workgroup per CU at most, workgroup b walks passes b, b + gridDim.x, ...; the list's length is read on the
// device.  Slots at or past the end repeat the last listed sample; stores are masked by SLOT.
#include "mlp_nerf_mx.h"

#include "mlp_layouts.h"
#include "mlp_nerf_chain.h"

namespace tgtc {

using CfgX3List = MlpCfg<8, 1, true, 4>;   // CfgExact of mlp_nerf.hip

__global__ void __launch_bounds__(CfgX3List::NWAVES * 64, CfgX3List::NWAVES * CfgX3List::WG_PER_CU / 4) nerf_x3_list_kernel(NerfArgs a) {
    using C = CfgX3List;
    constexpr int NCT = C::NCT;
    static_assert(NCT == 1 && C::SPLIT && C::SAMPLES_PER_WG == 128, "a pass is 128 list slots, one column tile per wave");

    // the list's length: a scalar load, issued (and waited for) before any LDS-DMA
    const unsigned n_live = __builtin_amdgcn_readfirstlane(*a.n_live);
    const long long n_pass = ((long long)n_live + C::SAMPLES_PER_WG - 1) / C::SAMPLES_PER_WG;

    // ALL LDS in one array (a second __shared__ object makes hipcc drain vmcnt before LDS reads).
    __shared__ __attribute__((aligned(16))) char smem[C::RING_BYTES + kNerfBiasBytes];

    const int wave_id = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    for (long long p = blockIdx.x; p < n_pass; p += gridDim.x) {
        // lane and wave ids are taken HERE, through volatile asm: what a pass derives from them (per-lane stream and LDS
        // addresses, the ring's M0 values) is computed in the pass as in the dense kernel, not hoisted out of the loop and
        // kept -- or spilled -- across the twelve layers
        const int lane = fresh_lane_id();
        int wave = wave_id;
        asm volatile("" : "+s"(wave));
        const int g = lane >> 4, n = lane & 15;
        const long long s_wave = p * C::SAMPLES_PER_WG + wave * C::SAMPLES_PER_WAVE;

        // ---- 1. inputs (ordinary loads first, as in the dense kernel); the store mask belongs to the SLOT
        double pos[NCT][3], dir[NCT][3];
        long long sidx[NCT];
        nerf_load_samples<NCT, IN_LIST>(a, s_wave, n, pos, dir, sidx, n_live);
        const bool write = (unsigned long long)(s_wave + n) < n_live && sidx[0] < a.M;   // (a list that keeps its promise never fails the second)
        half8 pe_h[2][NCT], pe_l[2][NCT], de_h[1][NCT], de_l[1][NCT];

        // ---- 2. the weight stream of this pass: bias table, then the first chunks.  The ring is primed per pass; every
        // LDS-DMA of the previous pass has landed (its last boundary waits for vmcnt(0)) and the barrier that ends a pass
        // proves every wave is done reading it.
        WeightStream<C, SingleStreamMap<NerfLayout::kFragsFull>> ws;
        const char* const streams[1] = {a.stream};
        ws.init(streams, smem, wave, lane);
#pragma unroll
        for (int j = 0; j < kNerfBiasBytes / (C::NWAVES * 1024); ++j)
            lds_dma16(a.bias + (j * C::NWAVES + wave) * 1024 + lane * 16, smem + C::RING_BYTES + (j * C::NWAVES + wave) * 1024);
        ws.prologue();

        // ---- 3. positional encoding of the points (the direction is encoded in front of the colour head)
        nerf_encode<NCT, true, false>(a, pos, dir, sidx, g, pe_h, pe_l, de_h, de_l);

        const lds_cptr bias_lane = opaque((lds_cptr)smem + C::RING_BYTES + 16 * g);
        ws.start();

        // ---- 4. the twelve layers
        nerf_chain<C, true>(
            ws, bias_lane, pe_h, pe_l,
            [&](auto c_, half8& dh, half8& dl) {
                constexpr int c = decltype(c_)::value;
                nerf_encode_dir_late<IN_LIST, true>(a, sidx[c], g, de_h[0][c], de_l[0][c]);
                dh = de_h[0][c], dl = de_l[0][c];
            },
            [&](auto c_, float sigma) {
                constexpr int c = decltype(c_)::value;
                if (g == 0 && a.sigma && write) a.sigma[sidx[c]] = sigma;
            },
            [&](auto, auto, auto, const float4v&) {},
            [&](auto c_, auto h_, const float4v& acc) {
                constexpr int c = decltype(c_)::value, hf = decltype(h_)::value;
                if (g == 0 && write) {
#pragma unroll
                    for (int r = 2 * hf; r < (hf ? 3 : 2); ++r) a.rgb[sidx[c] * 3 + r] = 1.0f / (1.0f + expf(-acc[r]));
                }
            });

        // every wave has read its last fragment and bias before the next pass re-fills the ring
        __builtin_amdgcn_s_barrier();
    }
    wait_vmcnt<0>();   // no LDS-DMA is in flight when the workgroup ends (an empty list issues none)
}

// the list's length is on the device: one workgroup per CU (never more than the dense plane has passes), each reads it
int nerf_x3_list_launch(const NerfArgs& a, hipStream_t st) {
    using C = CfgX3List;
    int cus = 0;
    if (const int rc = cu_count(cus)) return rc;
    const long long n_pass = (a.M + C::SAMPLES_PER_WG - 1) / C::SAMPLES_PER_WG;
    nerf_x3_list_kernel<<<(unsigned)(n_pass < cus ? n_pass : cus), C::NWAVES * 64, 0, st>>>(a);
    TGTC_LAUNCH_CHECK();
    return TGTC_OK;
}

}  // namespace tgtc
