// Host-side packer of the fp16mx group streams (mlp_mx.h): one layer at a time, for the NeRF nets (nerf_mx_pack,
// mlp_nerf_mx.hip) and for the folded style pair (style_mx_pack, mlp_style_mx.hip).
#pragma once
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

#include "mlp_mx.h"
#include "mlp_pack.h"

namespace tgtc {

// e2m3 code of x: round to nearest on the (piecewise linear) code axis, ties to even code, saturating at 7.5
inline int e2m3_encode(float x) {
    float a = std::fabs(x);
    if (!(a < 7.5f)) a = 7.5f;
    const float q = a < 1.0f ? a * 8.0f : (a < 2.0f ? 8.0f + (a - 1.0f) * 8.0f : (a < 4.0f ? 16.0f + (a - 2.0f) * 4.0f : 24.0f + (a - 4.0f) * 2.0f));
    int c = (int)std::nearbyint(q);  // default rounding mode: ties to even
    if (c > 31) c = 31;
    return c | (std::signbit(x) ? 32 : 0);
}

// Block exponent of one fp6 weight operand of a row, one per row over all activation columns and chosen independently for Wh6
// (the fp16 weights) and Wl6 (their rounding residuals, lo): the exponent of the operand's own largest magnitude puts the codes
// in [2,4) (no saturation), one below in [4,8) (finer steps, the few values above 7.5 saturate); whichever leaves the smaller
// squared error.  (Round 2 tied Wl6 to Wh6's exponent minus 11, which left the residuals two binades below the top of the
// code range: tests/probes/emu_mx_e2e.py, EMU_W_SHIFT=best, median end-to-end error 2.3e-5 -> 7.7e-6.)
inline int mx_row_exponent(const std::vector<float>& v, bool lo) {
    float mx = 0.0f;
    for (float x : v) mx = std::fmax(mx, std::fabs(x));
    if (!(mx > 0.0f)) return -14 - (lo ? 11 : 0);
    int e = 0;
    (void)std::frexp(mx, &e);   // mx = f * 2^e, f in [0.5, 1): the value's exponent is e - 1
    e -= 1;
    int pick = e - 1;
    double err_best = -1.0;
    for (int cand = e - 1; cand >= e - 2; --cand) {
        if (cand < -126) continue;
        const float inv = std::ldexp(1.0f, -cand), sc = std::ldexp(1.0f, cand);
        double err = 0.0;
        for (float x : v) {
            const double d = (double)e2m3_value(e2m3_encode(x * inv)) * sc - (double)x;
            err += d * d;
        }
        if (err_best < 0.0 || err < err_best) err_best = err, pick = cand;
    }
    return pick;
}

// Layer `Ls` as the groups T.first[..] = qi onwards of `stream` (qi is advanced), its row exponents (u16: byte 0 = Wh6's + 127,
// byte 1 = Wl6's) at rowexp[b0 ..] and, if `bias` is given, its biases at bias[b0 ..].  The layer's SEG_ACT segments, in their
// order, are the 4 * sh.nkb activation k-steps; its one other segment is the sh.npe encoding k-steps.  false: the layer does not
// have the shape `sh`.
inline bool mx_pack_layer(const LayerSpec& Ls, const MxShape& sh, const MxTable& T, int& qi, int b0, char* stream,
                          unsigned short* rowexp, float* bias) {
    std::vector<std::pair<const Seg*, int>> act_ks;   // (segment, k-step inside it)
    const Seg* pe = nullptr;
    for (const Seg& s : Ls.segs) {
        if (s.kind == SEG_ACT) {
            for (int k = 0; k < s.ksteps; ++k) act_ks.emplace_back(&s, k);
        } else if (!pe) {
            pe = &s;
        } else {
            return false;
        }
    }
    if (Ls.row_tiles() != sh.rt || (int)act_ks.size() != 4 * sh.nkb || (pe ? pe->ksteps : 0) != sh.npe) return false;
    auto weight = [&](int row, int col) -> float {
        return (row < Ls.out && col >= 0 && col < Ls.in) ? Ls.W[(size_t)row * Ls.in + col] : 0.0f;
    };
    for (int rt = 0; rt < sh.rt; ++rt) {
        int EH[16], EL[16];
        for (int r = 0; r < 16; ++r) {
            const int row = 16 * rt + r;
            if (bias) bias[b0 + 16 * rt + r] = row < Ls.out ? Ls.b[row] : 0.0f;
            std::vector<float> hi, lo;
            for (const auto& ks : act_ks)
                for (int c = 0; c < 32; ++c) {
                    const float w = weight(row, ks.first->col0 + 32 * ks.second + c);
                    const float h = (float)(half_t)w;
                    hi.push_back(h), lo.push_back(w - h);
                }
            EH[r] = mx_row_exponent(hi, false), EL[r] = mx_row_exponent(lo, true);
            rowexp[b0 + 16 * rt + r] = (unsigned short)((EH[r] + 127) | ((EL[r] + 127) << 8));
        }
        for (int kb = 0; kb < sh.nkb; ++kb, ++qi) {
            char* base = stream + T.off[qi];
            for (int lane = 0; lane < 64; ++lane) {
                const int m = lane & 15, g = lane >> 4, row = 16 * rt + m;
                unsigned long long bl[3] = {0, 0, 0}, bh[3] = {0, 0, 0};
                const float inv_l = std::ldexp(1.0f, -EL[m]);  // Wl6 = e2m3(wl / 2^EL)
                const float inv_h = std::ldexp(1.0f, -EH[m]);  // Wh6 = e2m3(wh / 2^EH)
                auto put = [](unsigned long long (&b)[3], int i, int code) {
                    const int bit = 6 * i;
                    b[bit / 64] |= (unsigned long long)code << (bit % 64);
                    if (bit % 64 > 58) b[bit / 64 + 1] |= (unsigned long long)code >> (64 - bit % 64);
                };
                for (int s = 0; s < 4; ++s) {
                    const auto& ks = act_ks[4 * kb + s];
                    for (int j = 0; j < 8; ++j) {
                        const float w = weight(row, seg_col(*ks.first, ks.second, g, j));
                        const half_t hi = (half_t)w;
                        std::memcpy(base + s * 1024 + lane * 16 + j * 2, &hi, 2);
                        put(bl, 8 * s + j, e2m3_encode((w - (float)hi) * inv_l));
                        put(bh, 8 * s + j, e2m3_encode((float)hi * inv_h));
                    }
                }
                // three 16-byte pieces per lane (mlp_mx.h): [Wl6 dwords 0-3] [Wl6 4-5 | Wh6 0-1] [Wh6 2-5]
                std::memcpy(base + 4096 + lane * 16, &bl[0], 16);
                std::memcpy(base + 5120 + lane * 16, &bl[2], 8);
                std::memcpy(base + 5120 + lane * 16 + 8, &bh[0], 8);
                std::memcpy(base + 6144 + lane * 16, &bh[1], 16);
            }
        }
        if (sh.npe) {
            char* base = stream + T.off[qi];
            for (int k = 0; k < sh.npe; ++k)
                for (int lane = 0; lane < 64; ++lane) {
                    const int m = lane & 15, g = lane >> 4, row = 16 * rt + m;
                    for (int j = 0; j < 8; ++j) {
                        const float w = weight(row, seg_col(*pe, k, g, j));
                        const half_t hi = (half_t)w, lo = (half_t)(w - (float)hi);
                        std::memcpy(base + (2 * k) * 1024 + lane * 16 + j * 2, &hi, 2);
                        std::memcpy(base + (2 * k + 1) * 1024 + lane * 16 + j * 2, &lo, 2);
                    }
                }
            ++qi;
        }
    }
    return true;
}

}  // namespace tgtc
