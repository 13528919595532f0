// Interface between mlp_nerf.hip (C ABI, dispatch, timing hook) and mlp_nerf_mx.hip (the fp16+fp6 kernels).
#pragma once
#include <vector>

#include "mlp_nerf_front.h"
#include "mlp_pack.h"

namespace tgtc {

std::vector<LayerSpec> nerf_specs(const tgtc_linear* l);  // mlp_nerf.hip

// packs the 12 linears for TGTC_PREC_FP16_FP6: `bias` = the kNerfBiasBytes region (fp32 biases + row exponents),
// `stream` = the group stream (mlp_mx.h)
int nerf_mx_pack(const tgtc_linear* layers, std::vector<char>& bias, std::vector<char>& stream);
// launches the kernel for (in_mode, full); no event handling
int nerf_mx_launch(int in_mode, bool full, const NerfArgs& a, hipStream_t st);
// the FULL network without the base_remap output, or densities over rays: two column tiles per wave, one wave per SIMD, persistent
// (mlp_nerf_mx2.hip)
int nerf_mx2_launch(int in_mode, bool full, const NerfArgs& a, hipStream_t st);

// ---- the stashed two-phase fine pass (mlp_nerf_mx2_stash.hip; render.hip fine_pass)
constexpr int kNerfStashMaxGrid = 256;                  // workgroups of the producer and the consumer (one per CU at most)
constexpr int kNerfStashRegions = 4 * kNerfStashMaxGrid;   // one region per wave; = the parts of the live statistic's counts
constexpr size_t kNerfStashSlotBytes = 932;             // 58 dwords per lane x 4 k-groups + the sample index
constexpr int kNerfHeadsStreamBytes = 24 * 16384;       // REMAP / C0 / C1 as a stream of their own, padded to whole rings
struct NerfStashArgs {
    char* base;            // the stash: kNerfStashRegions regions, `stride` bytes apart
    unsigned cap;          // slots per region (>= 1)
    size_t stride;         // >= cap * kNerfStashSlotBytes, a multiple of 16
    unsigned* counts;      // [kNerfStashRegions] live samples each wave saw (zeroed by the caller); parked = min(count, cap)
    unsigned* ovf_count;   // live samples that found their region full (zeroed by the caller) ...
    unsigned* ovf;         // ... and their indices, in no order
};
void nerf_mx_heads_stream(const std::vector<char>& stream, std::vector<char>& heads);
// densities over rays into a.sigma, layer 7's output of the samples with sigma > 0 into the stash
int nerf_mx2_stash_launch(const NerfArgs& a, const NerfStashArgs& s, hipStream_t st);
// a.stream = the heads stream; sigmoid(rgb) of the parked samples into a.rgb
int nerf_mx2_heads_launch(const NerfArgs& a, const NerfStashArgs& s, hipStream_t st);
// fp16x3, rays in, sigma out (the coarse pass): two column tiles per wave, one wave per SIMD, persistent (mlp_nerf_x3s.hip)
int nerf_x3s_launch(const NerfArgs& a, hipStream_t st);
// the same over a device-side list (a.live, a.n_live): sigma[live[slot]], nothing else
int nerf_x3s_list_launch(const NerfArgs& a, hipStream_t st);
// fp16x3, the FULL network over a device-side list (a.live, a.n_live): rgb[live[slot]] and, where a.sigma is given,
// sigma[live[slot]] -- the bits of the dense full launch; one column tile per wave, persistent (mlp_nerf_x3_list.hip)
int nerf_x3_list_launch(const NerfArgs& a, hipStream_t st);
// fp16 (one product), rays in, sigma out (the density screen): four column tiles per wave, one wave per SIMD, persistent
// (mlp_nerf_fp16s.hip); a.bias / a.stream are a handle's TGTC_PREC_FP16 form
// The screen's declared domain (DESIGN 3.1 "The screen's domain"): a sample with a coordinate outside |p| <= kScreenBox, or not
// finite, gets NaN for its density, which the screened passes list as a candidate; the margin is calibrated on this box.
int nerf_fp16s_launch(const NerfArgs& a, hipStream_t st);
constexpr double kScreenBox = 2.0;

}  // namespace tgtc
