"""CPU half of the plain per-sample sweep (tests/test_nerf_kernel_shapes_gpu.py): what the GPU half takes for granted about its
own cases, checked without a GPU -- the case lists reach every tile edge and every family on every kernel, the weight
families are what they claim in float64, the direction patterns are what they claim, the fp16mx arithmetic model still
separates a lost correction product from the full scheme, and the conditions under which the GPU half's guards are in force
(4 y_mx <= 1e-3) hold, so that a change to the model or the families cannot silently switch a guard off."""
import numpy as np
import pytest
import torch

import nerf_kernel_cases as nk
import test_hip_style_shapes as S


def test_case_lists_cover_the_tile_edges():
    """If the kernels' geometry changes (MlpCfg in csrc/mlp_nerf.hip, the passes of mlp_nerf_x3s.hip / mlp_nerf_mx2.hip), update
    nk.TILES and the case lists with it."""
    for tile in nk.TILES:
        assert {tile - 1, tile, tile + 1} <= set(nk.M_LIST), tile
    for cases in (nk.PTS_CASES, nk.ENC_CASES):
        assert {c[0] for c in cases if c[1:] == (cases[0][1], "each", "base")} >= set(nk.M_LIST)
    assert nk.FAMILY_M in nk.M_LIST and nk.FAMILY_M % 256 == 1
    assert any(N % 16 and R * N > 256 for R, N in nk.RAY_SHAPES)                 # ragged rays over more than one workgroup
    assert {8, 24} <= {N for _, N in nk.RAY_SHAPES}                                # a tile straddling rays, N < 16 and N > 16
    assert nk.BITS_SHAPE in nk.RAY_SHAPES and nk.BITS_SHAPE[1] % 16 and (nk.BITS_SHAPE[0] * nk.BITS_SHAPE[1]) % 256
    assert set(nk.LIST_SHAPES) <= set(nk.RAY_SHAPES) and all(N != 192 for _, N in nk.LIST_SHAPES)
    assert any(N % 16 for _, N in nk.LIST_SHAPES)
    # every family at least once per kernel: each entry point's list holds them all, and the three lists reach A..E
    assert {pf for _, pf, _, _ in nk.PTS_CASES} == set(nk.POINT_FAMILIES)
    assert {ef for _, ef, _, _ in nk.ENC_CASES} == set(nk.ENC_FAMILIES)
    for cases in (nk.PTS_CASES, nk.ENC_CASES):
        assert {dp for _, _, dp, _ in cases} == set(nk.DIR_PATTERNS)
        assert {wf for *_, wf in cases} == set(nk.WEIGHT_FAMILIES)
        assert all(c[0] == nk.FAMILY_M for c in cases if c[1:] != (cases[0][1], "each", "base"))
    assert {rdk for _, _, rdk, _ in nk.RAY_CASES} == set(nk.RAY_DIRS)
    assert {wf for *_, wf in nk.RAY_CASES} == set(nk.WEIGHT_FAMILIES)
    assert {(R, N) for R, N, _, wf in nk.RAY_CASES if wf == "base"} == set(nk.RAY_SHAPES)
    for wf in nk.WEIGHT_FAMILIES:
        assert {(5, 37), (9, 100)} <= {(R, N) for R, N, _, w in nk.RAY_CASES if w == wf}
    assert set("".join(nk.REACHES.values())) == set(nk.KERNELS) == set("ABCDE")
    assert "B" in nk.REACHES["rays"] and "D" not in nk.REACHES["rays"]      # B is rays only; D through IN_PTS / IN_ENC
    assert len(set(nk.PTS_CASES)) == len(nk.PTS_CASES) and len(set(nk.RAY_CASES)) == len(nk.RAY_CASES)


@pytest.mark.parametrize("wf", ["rows", "outliers"])
def test_heavy_tailed_weights_compute_the_base_function(wf):
    """Asserted inside nk.states in float64 (so that the GPU half cannot skip it); here it runs on the CPU, and the scale spread
    that makes the family worth having is looked at once more."""
    sd, base = nk.states(wf), nk.states("base")
    spread = max(float(np.abs(sd["net.base_layers.%d.weight" % l]).max() / np.abs(base["net.base_layers.%d.weight" % l]).max())
                 for l in range(8))
    print("%s: largest weight grows %.0f x" % (wf, spread))
    assert spread >= 16
    for l in range(8):      # powers of two only: the float64 difference is exactly representable
        r = sd["net.base_layers.%d.bias" % l] / np.where(base["net.base_layers.%d.bias" % l] == 0, 1, base["net.base_layers.%d.bias" % l])
        assert np.array_equal(np.exp2(np.rint(np.log2(r))), r)


def test_dead_weights_are_dead_and_still_a_scene():
    sd, base = nk.states("dead"), nk.states("base")
    rows = sorted(set(nk.DEAD_ROWS) | set(nk.DEAD_BLOCK))
    assert len(nk.DEAD_BLOCK) == 32 and len(rows) == 35 and {7, 100} <= set(nk.DEAD_BLOCK)   # 7 = 4 + 3, 100 = 32 * 3 + 4
    assert nk.DEAD_BLOCK == [32 * s + 16 * h + 4 + r for s in range(4) for h in range(2) for r in range(4)]
    for l in nk.DEAD_LAYERS:
        assert not sd["net.base_layers.%d.weight" % l][rows].any() and not sd["net.base_layers.%d.bias" % l][rows].any()
    assert not sd["net.base_layers.4.weight"][:, nk.DEAD_COLS].any()
    assert not sd["net.base_layers.5.weight"][:, [63 + c for c in nk.DEAD_COLS]].any()
    assert sd["net.base_layers.5.weight"][:, nk.DEAD_COLS].any()                    # the pe columns below 63 stay
    assert not sd["net.rgb_layers.0.weight"][:, nk.DEAD_COLS].any() and not sd["net.rgb_layers.1.weight"][:, nk.DEAD_RGB1_COLS].any()
    # layer 7's dead rows: columns of both consumers that are nonzero and unread
    for name in ("net.sigma_layer.weight", "net.base_remap_layer.weight"):
        assert np.array_equal(sd[name], base[name]) and sd[name][:, rows].all()
    # every 32-value block of blocks() partitions the 256 features
    assert sorted(i for b in nk.blocks() for i in b) == list(range(256))
    mx, live, lo, hi = nk.dead_scene()
    print("dead: max|sigma| %.1f, sigma > 0 on %.1f %%, rgb in %.2f .. %.2f" % (mx, 100 * live, lo, hi))


def test_direction_patterns_are_what_they_claim():
    for M in (nk.FAMILY_M, 1000):
        one, lane = nk.directions("one", M), nk.directions("lane", M)
        i = torch.arange(M)
        assert bool((one == one[0]).all())
        differs = (lane != lane[0]).any(1)
        assert torch.equal(differs, i % 32 == 21) and bool(differs.any())
        assert float((lane[21] - lane[0]).abs().max()) > 0.25
        b16, b32, each = nk.directions("blocks16", M), nk.directions("blocks32", M), nk.directions("each", M)
        for r0 in range(0, M, 32):
            run32 = b32[r0:r0 + 32]
            assert bool((run32 == run32[0]).all())                                   # tile 1 = tile 0 in every wave
            if r0 + 32 < M:
                assert not torch.equal(b32[r0], b32[r0 + 32])                        # neighbouring waves differ
            if r0 + 16 < M:
                assert not torch.equal(b16[r0], b16[r0 + 16])                        # tile 1 != tile 0 in every wave
                assert bool((b16[r0:r0 + 16] == b16[r0]).all())
        assert len({tuple(r) for r in each.tolist()}) == M
    sp, sd = nk.pts_inputs((nk.FAMILY_M, "special", "each", "base"))
    assert not sp[0].any() and not sd[0].any()
    assert set(sp.flatten().tolist()) == set(nk.SPECIAL.tolist()) == set(sd.flatten().tolist())
    for pf, half in (("unit", 1.5), ("mid", 8.0), ("wide", 100.0)):
        p = nk.points(pf, 1000)
        assert 0.9 * half < float(p.abs().max()) <= half
    ro, rd, ts = nk.ray_inputs(9, 100, "parallel")
    assert bool((rd == rd[0]).all()) and len({tuple(r) for r in ro.tolist()}) == 9
    assert ts.dtype == torch.float32 and bool((ts[:, 1:] >= ts[:, :-1]).all())


def test_mx_model_separates_a_lost_correction():
    """The probe's own case (M = 1 000, nerf_state(1), U(-1, 1)).  All terms: at least 8 x below "fp16 only" on sigma, remap and
    rgb (measured 18.5, 15.3, 14.0); dropping either correction product: at least 4 x worse on each (measured 7.7 .. 11)."""
    errs = nk.probe_errors()
    full, fp16 = errs["fp16+fp6 (all terms)"], errs["fp16 only"]
    for name, e in errs.items():
        print("%-24s sigma %.2e  remap %.2e  rgb %.2e" % ((name,) + e))
    for i, t in enumerate(("sigma", "remap", "rgb")):
        assert fp16[i] >= 8 * full[i], (t, fp16[i], full[i])
        for dropped in ("no corr1 (Wl.Ah)", "no corr2 (Wh.Al)"):
            assert errs[dropped][i] >= 4 * full[i], (t, dropped, errs[dropped][i], full[i])


def guarded(case):
    return case[-1] in nk.MX_GUARDED_WEIGHTS


@pytest.mark.parametrize("case", [c for c in nk.PTS_CASES if guarded(c) and c[1] in nk.MX_GUARDED_POINTS], ids=nk.pts_id)
def test_mx_guard_is_in_force_on_points(case):
    """4 y_mx <= 1e-3 on every base / dead case at unit / mid: the GPU half asserts err <= 4 y_mx there."""
    (_, y), ymx = nk.pts_case_oracle(case), nk.pts_case_y_mx(case)
    for t, a, b in zip(nk.TENSORS, y, ymx):
        print("%-28s %-10s 16 y %.3e  4 y_mx %.3e" % (nk.pts_id(case), t, nk.K_X3 * a, nk.K_MX * b))
        assert nk.mx_guard(case[-1], b) is not None, (t, b)


@pytest.mark.parametrize("case", [c for c in nk.ENC_CASES + [r for r in nk.RAY_CASES if r[:2] in ((5, 37), (9, 100))] if guarded(c)],
                         ids=lambda c: "-".join(str(x) for x in c))
def test_mx_guard_is_in_force_on_encodings_and_rays(case):
    """The same on the encoded-input cases ('true' and 'free') and on the ragged ray shapes of the weight families."""
    if isinstance(case[1], str):                # (M, encoded family, ..) or (R, N, ..)
        (_, y), ymx = nk.enc_case_oracle(case), nk.enc_case_y_mx(case)
    else:
        (_, y), ymx = nk.ray_case_oracle(case), nk.ray_case_y_mx(case)
    for t, a, b in zip(nk.TENSORS, y, ymx):
        print("%-28s %-10s 16 y %.3e  4 y_mx %.3e" % ("-".join(str(x) for x in case), t, nk.K_X3 * a, nk.K_MX * b))
        assert nk.mx_guard(case[-1], b) is not None, (t, b)


def test_yardsticks_per_family():
    """Printed, not asserted (they are properties of the oracle, the bars that use them are in the GPU half): 16 y per point and
    encoded family, and the model's error where the guard is off (wide, rows, outliers)."""
    for case in nk.FAMILY_PTS_CASES[:4] + nk.FAMILY_PTS_CASES[-3:-1]:
        (_, y), ymx = nk.pts_case_oracle(case), nk.pts_case_y_mx(case)
        for t, a, b in zip(nk.TENSORS, y, ymx):
            print("%-28s %-10s 16 y %.3e  min(5e-5, 16 y) %.3e  4 y_mx %.3e" % (nk.pts_id(case), t, 16 * a, min(5e-5, 16 * a), 4 * b))
            assert a >= S.Y_FLOOR and np.isfinite(b)
