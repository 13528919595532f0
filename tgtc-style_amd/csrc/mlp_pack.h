// Host-side weight packer: turns nn.Linear weights ([out,in] row-major fp32) into the
// fragment-ordered fp16 (hi [+ lo]) stream the fused kernels consume through the LDS ring,
// plus a padded fp32 bias table.  The k-slot -> input-column maps live in mlp_core.h.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../../include/tgtc_hip.h"
#include "common.h"
#include "mlp_core.h"

namespace tgtc {

enum SegKind { SEG_ACT = 0, SEG_PE63 = 1, SEG_PE27 = 2, SEG_VEC32 = 3 };

struct Seg {
    SegKind kind;
    int col0;    // first column of this source inside the reference's concatenated input
    int ksteps;  // 32-deep k-steps this source occupies
};

struct LayerSpec {
    const float* W;
    const float* b;
    int out, in;
    std::vector<Seg> segs;
    int ksteps() const {
        int k = 0;
        for (auto& s : segs) k += s.ksteps;
        return k;
    }
    int row_tiles() const { return (out + 15) / 16; }
};

inline int seg_col(const Seg& s, int ks_in_seg, int g, int j) {
    int c = -1;
    switch (s.kind) {
        case SEG_ACT: c = act_col(ks_in_seg, g, j); break;
        case SEG_PE63: c = pe63_col(ks_in_seg, g, j); break;
        case SEG_PE27: c = pe27_col(g, j); break;
        case SEG_VEC32: c = vec32_col(g, j); break;
    }
    return c < 0 ? -1 : s.col0 + c;
}

// ------------------------------------------------------------------------------------------------
// Power-of-two cross-layer equalisation of ReLU layers before packing (every precision).
//
// fp16 operands have a 30-binade exponent range and the parity modes lean on its lower end: the lo halves of fp16x3 are
// 2^-11 of their values (an activation of 1e-3 has a lo of 5e-7, an fp16 subnormal with three significant bits; below
// 6e-8 it is gone), and the block-scaled corrections of fp16mx lose their benefit with the dynamic range inside a
// 32-value block (activations) or a weight row.  A network whose features live on very different scales -- what trained
// MLPs look like -- therefore loses accuracy in EVERY mode (tests/probes/emu_mx_e2e.py: log-normal per-feature scales
// put 6e-3 on a rendered ray in fp16x3, 4e-3 in fp16mx; equalised: 2e-6 / 2e-4).  A ReLU layer is positively
// homogeneous, so row i of layer l (and its bias) times 2^-k and column i of every consumer of that feature times 2^k is
// the SAME function -- exactly: powers of two commute with every rounding short of overflow -- and
// k_i = round(log2(rowmax_i / colmax_i) / 2), taken relative to the layer's median, balances the row's range against
// its consumers' column range feature by feature (cross-layer range equalisation, as used for integer quantisation).
// Layers whose outputs leave the operator (base_remap, concat_features, the heads) keep their rows.
// TGTC_NO_EQUALISE=1 packs the weights as given (development; tests/test_precision_robustness_gpu.py then fails).
struct EqualisedNet {
    std::vector<std::vector<float>> w, b;
    std::vector<tgtc_linear> lin;
    struct Cons {
        int layer, col0;
    };
    static bool enabled() {
        const char* e = std::getenv("TGTC_NO_EQUALISE");
        return !(e && e[0] == '1');
    }
    void copy(const tgtc_linear* layers, int n) {
        w.resize(n), b.resize(n), lin.resize(n);
        for (int l = 0; l < n; ++l) {
            w[l].assign(layers[l].weight, layers[l].weight + (size_t)layers[l].out_features * layers[l].in_features);
            b[l].assign(layers[l].bias, layers[l].bias + layers[l].out_features);
            lin[l] = tgtc_linear{w[l].data(), b[l].data(), layers[l].out_features, layers[l].in_features};
        }
    }
    // rows of ReLU layer l against columns [col0, col0 + rows) of its consumers
    void run(int l, std::initializer_list<Cons> cons) {
        if (!enabled()) return;
        const int n = lin[l].out_features, in = lin[l].in_features;
        std::vector<int> k(n, 0);
        for (int i = 0; i < n; ++i) {
            float r1 = 0.0f, r2 = 0.0f;
            for (int c = 0; c < in; ++c) r1 = std::fmax(r1, std::fabs(w[l][(size_t)i * in + c]));
            for (const Cons& q : cons)
                for (int r = 0; r < lin[q.layer].out_features; ++r)
                    r2 = std::fmax(r2, std::fabs(w[q.layer][(size_t)r * lin[q.layer].in_features + q.col0 + i]));
            if (r1 > 0.0f && r2 > 0.0f) k[i] = (int)std::nearbyint(0.5 * std::log2((double)r1 / (double)r2));
        }
        std::vector<int> sorted(k);
        std::nth_element(sorted.begin(), sorted.begin() + n / 2, sorted.end());
        const int med = sorted[n / 2];   // only the spread matters: the layer keeps its typical activation scale
        for (int i = 0; i < n; ++i) {
            const int ki = std::max(-8, std::min(8, k[i] - med));
            if (ki == 0) continue;
            const float down = std::ldexp(1.0f, -ki), up = std::ldexp(1.0f, ki);
            for (int c = 0; c < in; ++c) w[l][(size_t)i * in + c] *= down;
            b[l][i] *= down;
            for (const Cons& q : cons)
                for (int r = 0; r < lin[q.layer].out_features; ++r)
                    w[q.layer][(size_t)r * lin[q.layer].in_features + q.col0 + i] *= up;
        }
    }
};

struct PackedNet {
    std::vector<half_t> stream;  // fragments, chunk-padded
    std::vector<float> bias;     // 16 floats per row tile, layer after layer
    std::vector<int> frag0;      // first fragment of each layer
    std::vector<int> bias0;      // first bias float of each layer
    int n_frags = 0;
};

inline PackedNet pack_layers(const std::vector<LayerSpec>& layers, bool split) {
    PackedNet p;
    const int frag_halves = kFragHalves * (split ? 2 : 1);
    for (const LayerSpec& L : layers) {
        p.frag0.push_back(p.n_frags);
        p.bias0.push_back((int)p.bias.size());
        const int RT = L.row_tiles();
        for (int rt = 0; rt < RT; ++rt) {
            for (int r = 0; r < 16; ++r) {
                const int row = 16 * rt + r;
                p.bias.push_back(row < L.out ? L.b[row] : 0.0f);
            }
            int ks = 0;
            for (const Seg& s : L.segs) {
                for (int k = 0; k < s.ksteps; ++k, ++ks) {
                    const size_t base = p.stream.size();
                    p.stream.resize(base + frag_halves, (half_t)0.0f);
                    for (int lane = 0; lane < 64; ++lane) {
                        const int m = lane & 15, g = lane >> 4, row = 16 * rt + m;
                        for (int j = 0; j < 8; ++j) {
                            const int col = seg_col(s, k, g, j);
                            float w = 0.0f;
                            if (row < L.out && col >= 0 && col < L.in) w = L.W[(size_t)row * L.in + col];
                            const half_t hi = (half_t)w;
                            p.stream[base + lane * 8 + j] = hi;
                            if (split) p.stream[base + kFragHalves + lane * 8 + j] = (half_t)(w - (float)hi);
                        }
                    }
                    ++p.n_frags;
                }
            }
        }
    }
    const size_t chunk_halves = kChunkBytes / sizeof(half_t);
    p.stream.resize((p.stream.size() + chunk_halves - 1) / chunk_halves * chunk_halves, (half_t)0.0f);
    return p;
}

// The same layers without their latent segment (SEG_VEC32), the remaining k-steps in their order: the streams of the folded
// kernels, in which the latent's k-step is a per-latent bias (tgtc_style_fold_latents).
inline std::vector<LayerSpec> without_latent(std::vector<LayerSpec> layers) {
    for (LayerSpec& L : layers)
        L.segs.erase(std::remove_if(L.segs.begin(), L.segs.end(), [](const Seg& s) { return s.kind == SEG_VEC32; }), L.segs.end());
    return layers;
}

// The latent columns of the layers, one row of 32 floats per output row, appended to `out` layer after layer.
inline void append_latent_columns(const std::vector<LayerSpec>& layers, std::vector<float>& out) {
    for (const LayerSpec& L : layers)
        for (const Seg& s : L.segs) {
            if (s.kind != SEG_VEC32) continue;
            for (int row = 0; row < L.out; ++row)
                for (int j = 0; j < 32; ++j) out.push_back(L.W[(size_t)row * L.in + s.col0 + j]);
        }
}

}  // namespace tgtc

// What a NeRF handle keeps about the two-phase fine pass of the plain render (render.hip, tgtc_net_set_cull): the mode, one
// pinned host word that every chain render with this handle as its fine network ends in an asynchronous copy of
// (live count, R x (n_coarse + n_fine)) into, and how many of those renders took which branch.  Reached through a
// pointer: the render entry points take the handle as const.
struct tgtc_cull_state {
    int mode;                        // TGTC_CULL_*
    volatile uint64_t* landed;       // pinned: low word the live count, high word the sample count; 0 = nothing landed yet
    long long culled, dense;         // chain renders that took the two-phase fine pass / the dense one
};

// What a style handle keeps for its fp16mx streams (tgtc_style_enable_mx, mlp_style.hip): the equalised copy of the 13 linears
// every stream of the handle was packed from, and -- once enabled -- an allocation of its own
//   [concat group stream | style group stream (mlp_mx.h, kStylePairMxTable)][row exponents, kStylePairMxExpBytes]
// read by the fp16mx plane consumer (mlp_style_mx.hip).  Nothing inside tgtc_net::dev moves.
struct tgtc_style_mx {
    tgtc::EqualisedNet concat, style;
    char* dev = nullptr;     // nullptr: not enabled
    size_t exp_off = 0;      // the row-exponent table behind the streams
};

// What a NeRF handle in fp16x3 or fp16mx keeps for its density screen (tgtc_net_enable_screen, mlp_nerf.hip; render.hip,
// the screened passes): the equalised copy of the 12 linears the handle was packed from, and -- once enabled -- the
// TGTC_PREC_FP16 form of the same weights in an allocation of its own ([bias table][fp16 stream][one ring of slack], what
// tgtc_nerf_create packs for that precision), the calibrated margin, the policy and its pinned word: every chain render
// with this handle in a pass that can be screened ends in an asynchronous copy of (candidate count, samples of the pass).
// Nothing inside tgtc_net::dev moves.
struct tgtc_screen_state {
    tgtc::EqualisedNet eq;
    char* dev = nullptr;                   // nullptr: not enabled
    float margin = -1.0f;                  // 8 x the calibration's max |sigma_screen - sigma_exact|
    int mode = 0;                          // TGTC_SCREEN_*
    volatile uint64_t* landed = nullptr;   // pinned: low word the candidate count, high word the sample count; 0 = nothing yet
    long long screened = 0, dense = 0;     // chain renders whose pass with this handle was screened / was not
};

// The opaque handle of the C ABI.
struct tgtc_net {
    int kind;        // 0 = NeRF (StyleNerf), 1 = style pair (concat MLP + style MLP)
    int precision;   // TGTC_PREC_*
    char* dev;       // one device allocation: [bias table, padded][weight stream]
    size_t bias_bytes;
    size_t stream_bytes;
    int n_frags;
    // style pair only: second stream (the style MLP) inside the same allocation
    size_t bias2_off, bias2_bytes, stream2_off, stream2_bytes;
    int n_frags2;
    size_t stash_off;  // per-workgroup scratch slabs of the fused stylised kernel
    size_t stash2_off; // a second region of the same size (base_remap across the latents of mlp_style_multi.hip)
    int n_wg;          // persistent grid size (= CUs)
    // style pair only, behind the slabs: the two streams packed without the latent k-steps and the equalised fp32 latent
    // columns [kFoldRows, 32] of the 13 layers (tgtc_style_fold_latents and the folded kernels of mlp_style_sparse.hip)
    size_t fold_stream_off, fold_stream2_off, fold_wz_off;
    tgtc_cull_state* cull;  // NeRF handles only (tgtc_nerf_create)
    tgtc_style_mx* mx;      // style pairs only (tgtc_style_create)
    // fp16mx NeRF handles only: the REMAP / C0 / C1 stream behind the full stream's slack (mlp_nerf_mx2_stash.hip), and the
    // caller-owned stash of the two-phase fine pass (tgtc_net_set_stash; nullptr: none attached)
    size_t heads_off;
    char* stash;
    size_t stash_stride;    // bytes between the regions
    unsigned stash_cap;     // slots per region
    tgtc_screen_state* screen;   // NeRF handles in fp16x3 / fp16mx only (tgtc_nerf_create)
};
