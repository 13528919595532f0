"""CPU: what the GPU half of the training-kernel sweep (tests/test_train_kernel_shapes_gpu.py) takes for granted about its
cases (tests/train_kernel_cases.py): that the case lists reach every template instance and host branch they name, that the
input families have the properties claimed for them, and that the exactness conditions of the bit-for-bit checks hold."""
import numpy as np
import pytest
import torch

import train_kernel_cases as tc


# ----------------------------------------------------------------------------------------------- A. compositing
def test_composite_grid_reaches_every_instance_on_both_sides_of_its_boundary():
    inst = {N: tc.composite_instance(N) for N in tc.COMPOSITE_N}
    assert set(inst.values()) == {1, 2, 3, 4, 8}
    for edge in (64, 128, 192, 256):                     # last N of one instance, first of the next
        assert edge in inst and edge + 1 in inst and inst[edge] != inst[edge + 1]
    assert inst[193] == 4 and inst[257] == 8 and inst[512] == 8 and tc.composite_instance(513) is None
    assert tc.COMPOSITE_MAX_N == max(tc.COMPOSITE_N)
    # C = 8 with lanes that own no sample: lane l owns [8 l, 8 l + 8)
    assert 320 in inst and (320 + 7) // 8 < 64 and 449 in inst and (449 + 7) // 8 == 57 and (512 + 7) // 8 == 64
    assert tc.COMPOSITE_R == 5 and tc.COMPOSITE_R_EDGES == (193, [0, 1, 4])
    assert set(tc.FAMILY_N) <= set(tc.COMPOSITE_N) and {tc.composite_instance(N) for N in tc.FAMILY_N} == {2, 4, 8}
    assert {tc.composite_instance(N) for N in tc.POINTER_N} == {2, 8}
    cases = tc.composite_cases()
    assert len(cases) == len(set(cases))
    for fam in tc.FAMILIES:
        mine = [c for c in cases if c[0] == fam]
        assert {c[1] for c in mine} == set(tc.COMPOSITE_N if fam == "base" else tc.FAMILY_N)
        assert {c[2] for c in mine} == {0, 1}
        assert {c[3] for c in mine} == ({False} if fam in tc.NOISELESS else {True, False})


def _alpha32(sigma, ts, noise):
    delta = torch.cat([ts[:, 1:] - ts[:, :-1], torch.full_like(ts[:, :1], 1e10)], -1)
    dens = torch.relu(sigma if noise is None else sigma + noise)
    return 1.0 - torch.exp(-dens * delta), delta


@pytest.mark.parametrize("N", tc.FAMILY_N)
def test_composite_families_have_the_properties_claimed(N):
    R = tc.COMPOSITE_R
    for fam in tc.FAMILIES:
        for nz in ((False,) if fam in tc.NOISELESS else (True, False)):
            rgb, sigma, ts, noise = tc.composite_inputs(fam, R, N, nz)
            assert rgb.dtype == sigma.dtype == ts.dtype == torch.float32 and (noise is None) == (not nz)
            assert rgb.shape == (R, N, 3) and sigma.shape == ts.shape == (R, N)
            assert bool((ts[:, 1:] >= ts[:, :-1]).all()), fam               # depths stay sorted
            alpha, delta = _alpha32(sigma, ts, noise)
            if fam == "opaque":
                k = tc.opaque_index(N)
                assert 0 < k < N - 1 and bool((alpha[:, k] == 1.0).all()) and bool((delta[:, k] >= 0.0099).all())
                assert noise is None or bool((noise[:, k] == 0).all())
                w = tc.composite_reference(rgb, sigma, ts, noise, 0, dtype=torch.float32)["weights"]
                assert float(w[:, k + 1:].max()) < 1e-9 and float(w[:, :k + 1].sum(-1).min()) > 0.5
            if fam == "ties":
                even = torch.arange(0, N - 1, 2)
                assert bool((delta[:, even] == 0).all()) and bool((alpha[:, even] == 0).all())
                ref = tc.composite_reference(rgb, sigma, ts, noise, 1, *tc.composite_upstream(R, N))
                assert bool((ref["d_sigma"][:, even] == 0).all()) and float(ref["d_sigma"].abs().max()) > 0
            if fam == "gate":
                raw32 = sigma if noise is None else sigma + noise
                raw64 = sigma.double() if noise is None else sigma.double() + noise.double()
                assert np.array_equal(raw32.double().numpy(), raw64.numpy())          # the float32 sum is exact
                for t in ((sigma,) if noise is None else (sigma, noise)):
                    assert bool((t * 1024 == torch.round(t * 1024)).all())
                pos, neg, zero = [float(m.float().mean()) for m in (raw32 > 0, raw32 < 0, raw32 == 0)]
                assert min(pos, neg, zero) > 0.25, (pos, neg, zero)
                if noise is not None:        # the noise decides: the density alone has the other sign somewhere in each kind
                    assert bool(((sigma > 0) & (raw32 < 0)).any()) and bool(((sigma < 0) & (raw32 > 0)).any())
                    assert bool(((sigma != 0) & (raw32 == 0)).any())
            if fam == "dead":
                assert bool((sigma <= 0).all()) and bool((sigma == 0).any()) and bool((sigma < 0).any())
                for white in (0, 1):
                    ref = tc.composite_reference(rgb, sigma, ts, None, white, *tc.composite_upstream(R, N))
                    assert all(float(ref[k].abs().max()) == 0 for k in ("t_exp", "weights", "d_rgb", "d_sigma"))
                    assert bool((ref["rgb_exp"] == float(white)).all())
            if fam == "thin":
                # |sigma| 1e-4 x delta: below 1e-4 wherever |sigma| delta < 1, i.e. all but a few samples in front of a
                # wide gap of a short ray (1.2e-4 at N = 65); none reaches 1e-3 and the ray stays transparent
                assert 0 < float(alpha.max()) < 1e-3 and float((alpha < 1e-4).float().mean()) > 0.99
                assert float(alpha.sum(-1).max()) < 3e-3


def test_composite_base_inputs_are_the_existing_tests():
    rng = np.random.default_rng(164)
    rgb = tc.base_inputs(33, 64, 164)[0]
    assert np.array_equal(rgb.numpy(), rng.random((33, 64, 3)).astype(np.float32))
    a, b = tc.composite_inputs("base", 5, 65), tc.base_inputs(5, 65, 65 + 35)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_rows_error_sees_a_faint_ray_and_an_exact_zero():
    ref = torch.tensor([[1.0, 2.0], [1e-9, 2e-9], [0.0, 0.0], [0.0, 0.0]], dtype=torch.float64)
    got = ref.clone()
    got[1, 0] = 2e-9
    got[3, 1] = 1e-30
    e = tc.rows_error(got, ref)
    assert float(e[0]) == 0 and abs(float(e[1]) - 0.5) < 1e-12 and float(e[2]) == 0 and float(e[3]) == float("inf")
    assert float((got - ref).abs().max() / ref.abs().max()) < 1e-9          # the whole-tensor norm misses both
    got[0, 0] = float("nan")
    assert not bool(tc.rows_error(got, ref)[0] <= 1.0)


# ----------------------------------------------------------------------------------------------- B. dense layers
def test_linear_cases_reach_every_branch_of_the_backward():
    layer_shapes = {s for v in tc.LAYER_SHAPES.values() for s in v}
    split = {c: tc.backward_split(*c) for c in tc.LINEAR_CASES}
    for (M, K, N) in tc.LINEAR_CASES:
        assert (K, N) in layer_shapes, (K, N)
    kind = lambda c: (split[c][0], "pad" if split[c][0] * split[c][1] > c[0] else "full")
    of = lambda M: [kind(c) for c in tc.LINEAR_CASES if c[0] == M]
    assert (1, "pad") in of(1) and (1, "pad") in of(33) and (1, "full") in of(1024)
    assert (2, "pad") in of(1025) and (2, "full") in of(2048)
    assert split[(65537, 63, 256)][0] == 64 and (65537, 63, 256) in tc.LINEAR_CASES
    assert max(M * K * N for M, K, N in tc.LINEAR_CASES) == 65537 * 63 * 256
    for n in (1, 3):                                                   # float loads in the dx GEMM, with the samples split
        assert any(N == n and split[(M, K, N)][0] > 1 for M, K, N in tc.LINEAR_CASES)
    assert {63, 283, 319} <= {K for _, K, _ in tc.LINEAR_CASES} and all(k % 4 for k in (63, 283, 319))
    # the dx GEMM is [M, K] with inner dimension N: both workgroup tiles
    assert (6401, 256, 256) in tc.LINEAR_CASES and tc.gemm_mid(6401, 256) >= 400
    assert any(tc.gemm_mid(M, K) < 400 for M, K, _ in tc.LINEAR_CASES)
    assert set(tc.SUBSET_CASES) == {(1025, 256, 256), (33, 319, 256)} and len(tc.SUBSETS) == 7 and len(set(tc.SUBSETS)) == 7
    assert set(tc.FP16_CASES) == {(33, 319, 256), (1025, 256, 256), (1025, 256, 3)}
    assert tc.backward_split(1025, 256, 256) == (2, 544) and tc.backward_split(2048, 283, 128) == (2, 1024)
    assert tc.backward_split(1, 63, 256) == (1, 32) and tc.backward_split(65537, 63, 256) == (64, 1056)


def test_upstream_scales_stay_inside_the_exact_range():
    """The bit-for-bit check across 2^-100, 1, 2^100: grad_scale_kernel's exponent stays inside its clamp at all three, and no
    value of the float64 reference leaves the float32 normal range at either end (the ReLU gate is off in that check)."""
    M, K, N = tc.SCALE_CASE
    x, W, b, dy = tc.linear_inputs(M, K, N)
    dy = tc.scale_case_dy(dy)
    assert 1024 <= float(dy.abs().max()) < 2048
    ks = [tc.grad_scale_exponent(dy * 2.0 ** p) for p in tc.SCALES]
    assert ks == [100, 0, -100]
    assert tc.grad_scale_exponent(torch.zeros(3, 3)) == 0
    rows = [tc.row_scale_exponents(dy * 2.0 ** p) for p in tc.SCALES]          # dx: one exponent per row, clamped at +-126
    assert torch.equal(rows[0] - 100, rows[1]) and torch.equal(rows[2] + 100, rows[1]) and int(rows[0].max()) < 126 and int(rows[2].min()) > -126
    assert tc.row_scale_exponents(torch.tensor([[0.0, 0.0], [3.0, -1024.0], [2.0 ** -140, 0.0]])).tolist() == [0, 0, 126]
    ref = tc.linear_reference(x, W, b, dy, None)
    for k in ("dx", "dW", "db"):
        a = ref[k].abs()
        assert float(a.max()) * 2.0 ** 100 < 2.0 ** 120 and float(a[a > 0].min()) * 2.0 ** -100 > 2.0 ** -120
    un = tc.uneven_rows(dy)
    rows = un.abs().amax(1)
    assert float(rows[0] / rows[1]) > 2.0 ** 28 and float(rows[0] / rows[1]) < 2.0 ** 32


def test_fp16_model_is_a_product_of_once_rounded_operands():
    M, K, N = 33, 319, 256
    x, W, b, dy = tc.linear_inputs(M, K, N)
    gate = torch.from_numpy(np.random.default_rng(0).random((M, N)) > 0.5)
    m64, m32 = tc.fp16_model(x, W, b, dy, gate), tc.fp16_model(x, W, b, dy, gate, torch.float32)
    full = tc.linear_reference(x, W, b, dy, gate)
    for k in ("y", "dx", "dW"):
        scale = float(full[k].abs().max())
        rounding = float((m64[k] - full[k]).abs().max()) / scale
        yard = float((m32[k] - m64[k]).abs().max()) / scale
        assert 2e-5 < rounding < 2e-3, (k, rounding)        # fp16 operands: far above the 2e-6 the model is held to
        assert yard < 1e-6, (k, yard)
    assert float((m64["db"] - full["db"]).abs().max()) <= 1e-6 * float(full["db"].abs().max())      # both halves: 22 bits
    hi, lo = tc.split16(x)
    assert float((hi + lo - x).abs().max()) <= 2.0 ** -21 * float(x.abs().max())


def test_activation_inputs_hold_the_edges():
    assert tc.ACTIVATION_N == [1, 255, 256, 257]
    for n in tc.ACTIVATION_N:
        dy, y = tc.activation_inputs(0, n)
        assert bool((y == 0).any()) and (n == 1 or (bool((y > 0).any()) and bool((y < 0).any())))
        assert bool((tc.activation_reference(0, dy, y)[y == 0] == 0).all())
        x, _ = tc.activation_inputs(2, n)
        assert float(x.max()) == 100.0 and (n == 1 or float(x.min()) == -100.0)
        ref = tc.activation_reference(2, x, None)
        assert bool(torch.isfinite(ref).all()) and float(ref.max()) == 1.0 and (n == 1 or 0 < float(ref.min()) < 1e-43)


# ----------------------------------------------------------------------------------------------- C. latent gather
def test_latent_id_check_refuses_what_the_kernels_would_index_out_of_range():
    """The rule of StyleLatents_variational.forward, on the host and without a device: style ids in [0, style_num), frame ids
    >= 0, flat = sid * F + fid inside the table (x7 for llff)."""
    from tgtc_style_amd import models
    S, F = tc.LATENT_S, tc.LATENT_F
    # with one style the five pairs are (S, 0), (-1, F), (0, -1), (S - 1, 7 F) for llff and (0, F) for another type
    assert [(s, f) for s, f, _ in tc.bad_latent_ids(1, F)] == [(1, 0), (-1, F), (0, -1), (0, 7 * F), (0, F)]
    # the first two pass a check of flat alone: flat = rows < 7 rows, flat = 0
    assert 0 <= S * F + 0 < 7 * S * F and 0 <= -1 * F + F < 7 * S * F
    for styles in (1, S):
        for sid, fid, kind in tc.bad_latent_ids(styles, F):
            with pytest.raises(IndexError):
                models.check_latent_ids(torch.tensor([0, sid]), torch.tensor([0, fid]), styles, F, kind == "llff")
    models.check_latent_ids(torch.tensor([S - 1]), torch.tensor([7 * F]), S, F, True)        # a wrapped id, valid with S > 1
    models.check_latent_ids(torch.zeros(0, dtype=torch.long), torch.zeros(0, dtype=torch.long), S, F, True)
    for llff in (True, False):
        for R in tc.LATENT_R:
            sid, fid = tc.latent_ids(R, llff)
            models.check_latent_ids(sid, fid, S, F, llff)              # every id of the sweep is valid
    models.check_latent_ids(torch.tensor([S - 1]), torch.tensor([7 * S * F - 1 - (S - 1) * F]), S, F, True)
    models.check_latent_ids(torch.tensor([0]), torch.tensor([S * F - 1]), S, F, False)       # the reference's table[flat] too


def test_latent_sweep_ids():
    S, F, D = tc.LATENT_S, tc.LATENT_F, tc.LATENT_D
    assert tc.LATENT_R == [0, 1, 7, 8, 9, 257] and D == 32 and (S, F) == (3, 5)
    assert 7 * D < 256 and 8 * D == 256 and 9 * D > 256
    rows = S * F
    for llff in (True, False):
        limit = 7 * rows if llff else rows
        for R in tc.LATENT_R:
            sid, fid = tc.latent_ids(R, llff)
            assert sid.shape == fid.shape == (R,) and sid.dtype == fid.dtype == torch.int64
            if R:
                flat = sid * F + fid
                assert int(sid.min()) >= 0 and int(sid.max()) < S and int(fid.min()) >= 0
                assert int(flat.min()) >= 0 and int(flat.max()) == limit - 1
        sid, fid = tc.latent_ids(257, llff)
        s0, f0, n = tc.LATENT_CROWD
        assert int(((sid == s0) & (fid == f0)).sum()) >= n == 200
        lat, mu = tc.latent_tables()
        g = torch.ones(257, D)
        _, d_lat, d_mu = tc.latent_reference(lat, mu, sid, fid, 0.35, llff, g)
        touched = d_lat.abs().amax(-1) > 0
        assert 2 <= int(touched.sum()) <= 5 and bool(touched[s0, f0])          # every other row receives nothing
        assert abs(float(d_lat[s0, f0, 0]) - 0.35 * n) < 1e-9
    lat, mu = tc.latent_tables()
    # the tables keep one float32 rounding below the forward bound
    assert float(lat.abs().max()) < 1 and float(mu.abs().max()) < 1 and float((lat - mu[:, None]).abs().max()) < 2


# ----------------------------------------------------------------------------------------------- D. fused trainer
def test_enough_samples_survive_the_margin():
    from tgtc_style_amd import synth
    pts, dirs = tc.train_samples()
    print("%d of %d draws have every float64 pre-activation at least %g from zero" % (pts.shape[0], tc.TRAIN_DRAWS, tc.TRAIN_MARGIN))
    assert pts.shape[0] >= max(tc.TRAIN_M) == 385 and pts.shape[0] <= tc.TRAIN_DRAWS
    z = tc.float64_preactivations(synth.nerf_state(1), pts[:385], dirs[:385])
    assert z.shape == (385, 8 * 256 + 256 + 128) and float(z.abs().min()) >= tc.TRAIN_MARGIN
    assert tc.TRAIN_M == [1, 127, 128, 129, 385]


def test_uneven_upstream_cases():
    s1, s2, s3 = (tc.uneven_scales(c) for c in (1, 2, 3))
    assert s1.shape == (385,)
    assert bool((s1[:128] == 1).all()) and bool((s1[128:256] == 0).all()) and bool((s1[256:384] == 2.0 ** -80).all()) and float(s1[384]) == 1024
    assert bool((s2[:256] == 0).all()) and bool((s2[256:384] == 2.0 ** -80).all()) and float(s2[384]) == 0
    assert bool((s3[256:384] == 2.0 ** -110).all()) and float(s3.sum()) == 128 * 2.0 ** -110
    w_rgb, w_sig = tc.train_upstream(385, s2)
    base_rgb, base_sig = tc.train_upstream(385)
    # 2^-80 of the base gradients is still a normal float32, and exactly the power of two times it
    assert float(w_rgb[256:384].abs().min()) > 2.0 ** -126 and torch.equal(w_rgb[256:384] * 2.0 ** 80, base_rgb[256:384])
    assert torch.equal(w_sig[256:384] * 2.0 ** 80, base_sig[256:384]) and float(w_sig[:256].abs().max()) == 0
    assert 2.0 ** -110 < 2.0 ** -92 < 2.0 ** -80
