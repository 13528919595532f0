// Interface between mlp_style.hip (tgtc_style_enable_mx), render.hip (tgtc_restyle_rays_trunk_folded_mx) and mlp_style_mx.hip
// (the fp16mx packer of the folded style pair and the fp16mx plane consumer).
#pragma once
#include <vector>

#include "mlp_pack.h"

namespace tgtc {

// packs the 13 folded layers (no SEG_VEC32 segment left: without_latent) for kStylePairMxTable (mlp_mx.h):
// `stream` = the concat group stream followed, at kStylePairMxStyleOff, by the style group stream; `row_exp` = the
// kStylePairMxExpBytes table, one u16 per pair bias table entry (byte 0 = Wh6's exponent, byte 1 = Wl6's, both + 127)
int style_mx_pack(const std::vector<LayerSpec>& concat, const std::vector<LayerSpec>& style, std::vector<char>& stream,
                  std::vector<char>& row_exp);

// rgb_live[k, i] of the `count` >= 1 entries of a cached list from its fp16x3 trunk plane and the K bias tables `folded`,
// the style networks in fp16mx (the handle has mx streams; sizes and handle kind are checked by the caller, render.hip)
int styled_restyle_plane_mx_impl(const tgtc_net* style, const double* rays_o, const double* rays_d, const void* folded, int K,
                                 int64_t R, int N, const uint32_t* live, const float* ts_live, int64_t count, const void* plane,
                                 float* rgb_live, hipStream_t st);

// The same without a plane, behind the trunk of an fp16mx NeRF handle in the same launch (mlp_list_mx.hip; the callers in
// render.hip have checked sizes, kinds, precisions and the mx streams).  Scattered: rgb [K,R,N,3] zero-filled by the caller, the
// list's length a device word.  Compact: rgb_live [K,count,3], count >= 1.  Both slab regions of the style handle are used.
int styled_forward_list_folded_mx_impl(const tgtc_net* nerf, const tgtc_net* style, const double* rays_o, const double* rays_d,
                                       const float* ts, const void* folded, int K, int64_t R, int N, const uint32_t* live,
                                       const uint32_t* n_live, float* rgb, hipStream_t st);
int styled_restyle_live_folded_mx_impl(const tgtc_net* nerf, const tgtc_net* style, const double* rays_o, const double* rays_d,
                                       const void* folded, int K, int64_t R, int N, const uint32_t* live, const float* ts_live,
                                       int64_t count, float* rgb_live, hipStream_t st);

}  // namespace tgtc
