// The input-gradient chain of the fused trainer: the body of train_dgrad_kernel, included twice by mlp_train.hip (inside
// namespace tgtc::train, behind dgrad_epi) -- TGTC_DGRAD_SPARSE 0: train_dgrad_kernel(BwdArgs), the kernel as it always
// was, token for token; 1: train_dgrad_sparse_kernel(BwdArgs, LiveList), the instance of the sparse backward.  (A template
// parameter and a shared inline body cost the dense kernel its instruction schedule: the arguments then reach the body
// through a copy.)
#if TGTC_DGRAD_SPARSE
__global__ void __launch_bounds__(CfgT::NWAVES * 64, 2) train_dgrad_sparse_kernel(BwdArgs a, LiveList sp) {
#else
__global__ void __launch_bounds__(CfgT::NWAVES * 64, 2) train_dgrad_kernel(BwdArgs a) {
#endif
    using C = CfgT;
    __shared__ __attribute__((aligned(16))) char smem[C::RING_BYTES + kNerfBiasBytes];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, n = lane & 15;
    const long long tile = (long long)blockIdx.x * C::NWAVES + wave;
#if TGTC_DGRAD_SPARSE
    const unsigned count = __builtin_amdgcn_readfirstlane(*sp.count);
    if ((unsigned)blockIdx.x * (unsigned)kTileSamples >= count) return;
    const long long row = tile * 16 + n;          // of the dZ stash: the list slot
    const bool live = (unsigned)row < count;
    const long long s = live ? (long long)sp.list[row] : 0;   // (a dead lane reads sample 0's gates and multiplies them by zeros)
#else
    const long long s = tile * 16 + n;
    const bool live = s < a.M;
    const long long row = s;                      // of the dZ stash
#endif

    // ---- ordinary loads first: the ten gate words of this lane, the head gradients of its sample
    unsigned long long gw[kGateLayers];
#pragma unroll
#if TGTC_DGRAD_SPARSE
    for (int l = 0; l < kGateLayers; ++l) gw[l] = a.gates[((size_t)l * a.n_tiles + (s >> 4)) * 64 + 16 * g + (s & 15)];
#else
    for (int l = 0; l < kGateLayers; ++l) gw[l] = a.gates[((size_t)l * a.n_tiles + tile) * 64 + lane];
#endif
    float hd[4] = {0.f, 0.f, 0.f, 0.f};   // [d sigma, dz_r, dz_g, dz_b] (rgb = sigmoid(z): dz = d rgb * rgb * (1 - rgb), models.py:111)
    if (live) {
        hd[0] = a.d_sigma[s];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float y = a.rgb[s * 3 + k];
            hd[1 + k] = a.d_rgb[s * 3 + k] * y * (1.0f - y);
        }
    }
#pragma unroll
    for (int l = 0; l < kGateLayers; ++l) asm volatile("" : "+v"(gw[l]));
#pragma unroll
    for (int k = 0; k < 4; ++k) asm volatile("" : "+v"(hd[k]));

    WeightStream<C, SingleStreamMap<kDgradFrags>> ws;
    const char* const streams[1] = {a.stream};
    ws.init(streams, smem, wave, lane);
#pragma unroll
    for (int j = 0; j < kNerfBiasBytes / (C::NWAVES * 1024); ++j)
        lds_dma16(a.zero_bias + (j * C::NWAVES + wave) * 1024 + lane * 16, smem + C::RING_BYTES + (j * C::NWAVES + wave) * 1024);
    ws.prologue();

    const long long m_pad = a.n_tiles * 16;               // rows up to M_pad exist; dead samples carry zeros
    auto seg_row = [&](int col0, int width) { return a.dz + seg_at(col0, width, m_pad, row); };
    // heads: true values to the stash (16 floats: [d sigma, dz rgb, 0 ...]), tile maximum -> first scale
    *reinterpret_cast<float4v*>(seg_row(Z_HEADS, 16) + 4 * g) = g == 0 ? float4v{hd[0], hd[1], hd[2], hd[3]} : float4v{0.f, 0.f, 0.f, 0.f};
    // segment maxima of this wave's tile: kept (wave-uniform) until the chain is through and published then -- an atomic is
    // a vector-memory operation, and one per layer in front of the ring's counted waits stalled every layer's first chunks
    unsigned seg_max[12];
    // The two heads carry their own scales (and their own segment maxima, 10: colour, 11: sigma): d sigma and dz_rgb may be
    // orders of magnitude apart (compositing gives |d sigma| ~ 1e-3 |d rgb| early in training and the reverse is as legal),
    // and the smaller one at the larger one's scale loses its low bits to fp16.  The colour head's values enter at D0, the
    // sigma row at D2 -- two layers after the colour branch has shrunk its values and the lagged scale has grown: no scale up to
    // and including D2's outputs may exceed the one d sigma fits in, or d sigma (and the products it feeds) leave the fp16
    // range: hi = inf, lo = x - inf, and the layer sums to NaN without any inf left for the maxima to show (round 4).
    const float m_sig = wave_max(fabsf(hd[0]));
    float m = wave_max(fmaxf(fabsf(hd[1]), fmaxf(fabsf(hd[2]), fabsf(hd[3]))));
    seg_max[10] = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(unsigned, m));
    seg_max[11] = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(unsigned, m_sig));
    const int e_sig = scale_exp(m_sig, 100);   // (no sigma gradient in this tile: no constraint)
    int e_in = scale_exp(m, e_sig);            // (no colour gradient: the branch carries zeros, at the scale sigma will need)
    // natural order k = 8g + j: the four values sit in lane group 0; SIGMA: the sigma entry alone (D2), else the colour entries (D0)
    auto heads_frag = [&](auto sigma_, int e, half8& h, half8& l) {
        constexpr bool SIGMA = decltype(sigma_)::value;
        const float sc = pow2f(e);
        unsigned h01 = 0, l01 = 0, h23 = 0, l23 = 0;
        if (g == 0) {
            split_pair_signed(SIGMA ? hd[0] * sc : 0.f, SIGMA ? 0.f : hd[1] * sc, h01, l01);
            split_pair_signed(SIGMA ? 0.f : hd[2] * sc, SIGMA ? 0.f : hd[3] * sc, h23, l23);
        }
        h = __builtin_bit_cast(half8, u4{h01, h23, 0u, 0u});
        l = __builtin_bit_cast(half8, u4{l01, l23, 0u, 0u});
    };

    const lds_cptr bias_lane = opaque((lds_cptr)smem + C::RING_BYTES + 16 * g);
    ws.start();

    half8 Xh[8][1], Xl[8][1], Yh[8][1], Yl[8][1];
    float pend[2];
    // after a layer: the tile maximum of its gated outputs fixes the scale of the layer AFTER the next (the next layer's
    // operands were already produced at the scale derived one layer earlier); segment maxima feed the weight-gradient kernel
    auto close = [&](auto seg_, float& mm, int cur, int keep) {   // cur: the scale in force, keep: the answer for an all-zero tile
        const float t = wave_max(mm);
        seg_max[decltype(seg_)::value] = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(unsigned, t));
#ifdef TGTC_DGRAD_ATOMIC_PER_LAYER   // A/B build: the round's first form, one atomic per layer in front of the ring waits
        if (lane == 0) atomicMax(a.maxima + decltype(seg_)::value, __builtin_bit_cast(unsigned, t));
#endif
        mm = 0.f;
        return max(cur - 120, min(cur + 120, scale_exp(t, keep)));   // (s_op = 2^(difference of consecutive scales) stays a normal float)
    };

    // D0: rgb_layers.1^T.  inputs heads (scale e_in), outputs dz_f at the same scale (|W| < 1: the values shrink)
    int e_out = e_in, e_next;
    {
        half8 Bh[1][1], Bl[1][1];
        heads_frag(std::false_type{}, e_in, Bh[0][0], Bl[0][0]);
        half8 Zh[4][1], Zl[4][1];
        m = 0.f;
        {
            const float s_true = pow2f(-e_in), s_op = pow2f(e_out - e_in);
            float* const zrow = seg_row(Z_F, 128);
            dense_layer<C, dgrad_frag0(0), 1, 8, 0>(ws, bias_lane, Bh, Bl, [&](auto rt_, auto, auto h_, const float4v& acc) {
                constexpr int rt = decltype(rt_)::value, hf = decltype(h_)::value;
                dgrad_epi<rt, hf, true>(acc, gw[9], s_true, s_op, m, pend, zrow, g, Zh[rt / 2][0], Zl[rt / 2][0]);
            });
        }
        e_next = min(close(ic<9>{}, m, e_out, e_sig), e_sig);
        // D1: rgb_layers.0^T (activation columns): dz_f -> dz_remap
        e_in = e_out, e_out = e_next;
        {
            const float s_true = pow2f(-e_in), s_op = pow2f(e_out - e_in);
            float* const zrow = seg_row(Z_REMAP, 256);
            dense_layer<C, dgrad_frag0(1), 4, 16, 0>(ws, bias_lane, Zh, Zl, [&](auto rt_, auto, auto h_, const float4v& acc) {
                constexpr int rt = decltype(rt_)::value, hf = decltype(h_)::value;
                dgrad_epi<rt, hf, true>(acc, gw[8], s_true, s_op, m, pend, zrow, g, Yh[rt / 2][0], Yl[rt / 2][0]);
            });
        }
        e_next = min(close(ic<8>{}, m, e_out, e_sig), e_sig);
    }
    // D2: [base_remap^T | sigma^T]: [dz_remap | heads] -> dz_7
    e_in = e_out, e_out = e_next;
    {
        half8 Bh[9][1], Bl[9][1];
#pragma unroll
        for (int k = 0; k < 8; ++k) Bh[k][0] = Yh[k][0], Bl[k][0] = Yl[k][0];
        heads_frag(std::true_type{}, e_in, Bh[8][0], Bl[8][0]);
        const float s_true = pow2f(-e_in), s_op = pow2f(e_out - e_in);
        float* const zrow = seg_row(z_layer(7), 256);
        dense_layer<C, dgrad_frag0(2), 9, 16, 0>(ws, bias_lane, Bh, Bl, [&](auto rt_, auto, auto h_, const float4v& acc) {
            constexpr int rt = decltype(rt_)::value, hf = decltype(h_)::value;
            dgrad_epi<rt, hf, true>(acc, gw[7], s_true, s_op, m, pend, zrow, g, Xh[rt / 2][0], Xl[rt / 2][0]);
        });
    }
    e_next = close(ic<7>{}, m, e_out, e_out);
    // D3..D9: base_layers[7..1]^T: dz_l -> dz_{l-1}
    auto hidden = [&](auto d_, auto last_, const half8 (&Ih)[8][1], const half8 (&Il)[8][1], half8 (&Oh)[8][1], half8 (&Ol)[8][1]) {
        constexpr int d = decltype(d_)::value, l_out = 9 - d;          // D3 -> dz_6 ... D9 -> dz_0
        constexpr bool last = decltype(last_)::value;
        e_in = e_out, e_out = e_next;
        const float s_true = pow2f(-e_in), s_op = pow2f(e_out - e_in);
        float* const zrow = seg_row(z_layer(l_out), 256);
        dense_layer<C, dgrad_frag0(d), 8, 16, 0>(ws, bias_lane, Ih, Il, [&](auto rt_, auto, auto h_, const float4v& acc) {
            constexpr int rt = decltype(rt_)::value, hf = decltype(h_)::value;
            dgrad_epi<rt, hf, !last>(acc, gw[l_out], s_true, s_op, m, pend, zrow, g, Oh[rt / 2][0], Ol[rt / 2][0]);
        });
        e_next = close(ic<l_out>{}, m, e_out, e_out);
    };
    hidden(ic<3>{}, std::false_type{}, Xh, Xl, Yh, Yl);
    hidden(ic<4>{}, std::false_type{}, Yh, Yl, Xh, Xl);
    hidden(ic<5>{}, std::false_type{}, Xh, Xl, Yh, Yl);
    hidden(ic<6>{}, std::false_type{}, Yh, Yl, Xh, Xl);
    hidden(ic<7>{}, std::false_type{}, Xh, Xl, Yh, Yl);
    hidden(ic<8>{}, std::false_type{}, Yh, Yl, Xh, Xl);
    hidden(ic<9>{}, std::true_type{}, Xh, Xl, Yh, Yl);
    // a scaled operand beyond the fp16 range produces infinities, which reach the maxima (fmaxf drops a NaN, not an inf):
    // report instead of returning garbage
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 12; ++i) bad |= (seg_max[i] & 0x7f800000u) == 0x7f800000u;
    // lane i publishes segment i, and only if it raises the table (one coherent load + one masked atomic per wave; after the
    // first few tiles almost no lane has anything to add.  One unconditional atomic per wave and segment -- 90 000 on eleven
    // addresses -- cost 0.2 ms of the kernel wherever they were issued)
    unsigned mine = 0;
#pragma unroll
    for (int i = 0; i < 12; ++i) mine = lane == i ? seg_max[i] : mine;
    if (lane < 12 && mine > __hip_atomic_load(a.maxima + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(a.maxima + lane, mine);
    if (bad && lane == 0) atomicMax(a.status, 1u);
}
