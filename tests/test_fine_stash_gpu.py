"""GPU: the stashed two-phase fine pass (csrc/mlp_nerf_mx2_stash.hip): the density launch parks layer 7's output
of every sample with sigma > 0 in a caller-owned stash, a heads-only launch (base_remap + colour head) reads it back, and
what found no room in its wave's region goes through the list kernel.

Every comparison is BIT IDENTITY (torch.equal): a parked column is multiplied by the same weights in the same order as in
the dense launch, wherever it is parked.  Outputs, workspace and stash have canary rows behind them.

Shapes.  One pass of the two kernels is 128 samples (4 waves x 2 tiles of 16).  At nt = 192 no ray count gives R x nt = 112,
128 or 129 (192 R is a multiple of 64), and below R = 4 the dead coarse planes cannot hold the overflow list, so the render
is dense.  The pass-edge counts therefore run at the call level, where N is free: (7, 16) = one sample tile short of a pass,
(8, 16) = exactly one pass, (3, 43) = one pass + 1 sample; the renders at nt = 192 take R = 4 (whole passes), 5 (a half pass
at the end) and 200 (300 passes: more than the CU count, every workgroup comes round again and some waves are out of slots
before their neighbours).  A stash of zero capacity cannot be attached (it is refused): "zero"
is the render with the stash detached."""
import numpy as np
import pytest
import torch

import nerf_kernel_cases as nk
from tgtc_style_amd import synth

pytestmark = pytest.mark.gpu

REGIONS = 1024
SLOT = 932
SCRATCH_WORDS = 2048
COUNT_WORD = 64
CANARY = -7.25
KINDS = ["base", "dead", "none", "all"]
CALL_SHAPES = [(7, 16), (8, 16), (3, 43), (200, 192)]
RENDER_SHAPES = [(4, 128, 64), (5, 128, 64), (200, 128, 64), (37, 24, 8)]


def T(sd):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}


class Args:
    use_viewdir, act_type = True, "relu"
    embed_freq_coor, embed_freq_dir = 10, 4
    netdepth = netdepth_fine = 8
    netwidth = netwidth_fine = 256
    precision = "fp16x3"


_nets = {}


def nets(kind, fine_precision="fp16mx"):
    """(coarse fp16x3, fine): 'base' / 'dead' of tests/nerf_kernel_cases.py, 'none' (sigma = -3 everywhere: no live sample at
    all) and 'all' (sigma = 8: every sample live, as tools/time_plain_cull.py --all-live)."""
    key = (kind, fine_precision)
    if key not in _nets:
        from tgtc_style_amd import models
        out = []
        for (seed, mode), prec in zip(((0, "coarse"), (1, "fine")), ("fp16x3", fine_precision)):
            m = models.StyleNerf(type("A", (Args,), {"precision": prec}), mode=mode)
            sd = T(synth.nerf_state(seed))
            if mode == "fine":
                if kind == "dead":
                    sd = T(nk.states("dead"))
                elif kind in ("none", "all"):
                    sd["net.sigma_layer.weight"] = torch.zeros_like(sd["net.sigma_layer.weight"])
                    sd["net.sigma_layer.bias"] = torch.full_like(sd["net.sigma_layer.bias"], -3.0 if kind == "none" else 8.0)
            m.load_state_dict(sd)
            out.append(m.cuda())
        _nets[key] = out
    return _nets[key]


def stash_bytes(cap):
    return REGIONS * ((SLOT * cap + 15) // 16 * 16)


def new_stash(cap=None, n=None):
    """(whole buffer, the part that is attached) for `cap` slots per region or n bytes: 4096 canary bytes behind the stash"""
    n = stash_bytes(cap) if n is None else n
    buf = torch.full((n + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf, buf[:n]


def stash_canary_ok(buf):
    return bool((buf[-4096:] == 0xA5).all())


_dense = {}


def dense_forward(kind, R, n):
    """(fine net, inputs, rgb [R*n,3], sigma [R*n]) of the full dense launch: computed once, never written again"""
    if (kind, R, n) not in _dense:
        from tgtc_style_amd import hip
        fine = nets(kind)[1]
        ro, rd, ts = (x.cuda() for x in nk.ray_inputs(R, n))
        rgb = torch.full((R * n, 3), float("nan"), device="cuda")
        sigma = torch.full((R * n,), float("nan"), device="cuda")
        hip.check(hip.load().tgtc_nerf_forward_rays(fine.packed().handle, hip.ptr(ro), hip.ptr(rd), hip.ptr(ts), R, n, hip.ptr(rgb),
                                                    hip.ptr(sigma), hip.stream()))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(sigma).all())
        _dense[(kind, R, n)] = (fine, (ro, rd, ts), rgb, sigma)
    return _dense[(kind, R, n)]


# ------------------------------------------------------------------------------------------------ 1: the two launches
def run_two_launches(kind, R, n, cap):
    """fill + heads + the list launch on the overflow, on canaried buffers; returns what the checks need"""
    from tgtc_style_amd import hip
    lib = hip.load()
    fine, (ro, rd, ts), rgb_dense, sigma_dense = dense_forward(kind, R, n)
    M = R * n
    net = fine.packed()
    buf, part = new_stash(cap)
    net.set_stash(part)
    try:
        sigma = torch.full((M + 64,), CANARY, device="cuda")
        scratch = torch.full((SCRATCH_WORDS + 64,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        ovf = torch.full((M + 64,), -1, dtype=torch.int32, device="cuda")
        hip.check(lib.tgtc_nerf_stash_fill(net.handle, hip.ptr(ro), hip.ptr(rd), hip.ptr(ts), R, n, hip.ptr(sigma), hip.ptr(scratch),
                                           hip.ptr(ovf), hip.stream()))
        heads = torch.full((M + 64, 3), CANARY, device="cuda")
        hip.check(lib.tgtc_nerf_stash_heads(net.handle, hip.ptr(ro), hip.ptr(rd), R, n, hip.ptr(scratch), hip.ptr(heads), hip.stream()))
        torch.cuda.synchronize()
        assert stash_canary_ok(buf)
        assert bool((scratch[SCRATCH_WORDS:] == 0x5a5a5a5a).all()) and bool((sigma[M:] == CANARY).all())
        # the producer's sigma: the density-only launch's bits (which are the full launch's, tests/test_plain_cull_gpu.py)
        ref = torch.full((M,), float("nan"), device="cuda")
        hip.check(lib.tgtc_nerf_forward_rays(net.handle, hip.ptr(ro), hip.ptr(rd), hip.ptr(ts), R, n, None, hip.ptr(ref), hip.stream()))
        torch.cuda.synchronize()
        assert torch.equal(sigma[:M], ref) and torch.equal(ref, sigma_dense)
        live = sigma_dense > 0
        counts = scratch[COUNT_WORD:COUNT_WORD + REGIONS].long()
        n_ovf = int(scratch[0])
        parked = int(torch.clamp(counts, max=cap).sum())
        print(kind, R, n, "cap", cap, "live", int(live.sum()), "parked", parked, "overflow", n_ovf)
        # every live sample exactly once: the counts add up, the list has no repeats, and no listed sample is parked
        assert int(counts.sum()) == int(live.sum()) == parked + n_ovf
        assert int(torch.clamp(counts - cap, min=0).sum()) == n_ovf
        listed = ovf[:n_ovf].long()
        assert bool((ovf[n_ovf:] == -1).all())
        assert listed.unique().numel() == n_ovf and (n_ovf == 0 or bool(live[listed].all()))
        wrote = (heads[:M] != CANARY).any(1)
        assert int(wrote.sum()) == parked and bool((heads[M:] == CANARY).all())
        assert not bool(wrote[listed].any()) and bool(live[wrote].all())
        # the heads kernel's colours: tgtc_nerf_forward_list on the same indices
        idx = torch.nonzero(wrote).flatten().int()
        if idx.numel():
            want = torch.full((M, 3), CANARY, device="cuda")
            n_idx = torch.tensor([idx.numel()], dtype=torch.int32, device="cuda")
            hip.check(lib.tgtc_nerf_forward_list(net.handle, hip.ptr(ro), hip.ptr(rd), hip.ptr(ts), R, n, hip.ptr(idx), hip.ptr(n_idx),
                                                 hip.ptr(want), hip.stream()))
            torch.cuda.synchronize()
            assert torch.equal(heads[:M], want)
            assert torch.equal(heads[:M][wrote], rgb_dense[wrote])
        return parked, n_ovf
    finally:
        net.set_stash(None)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("R,n", CALL_SHAPES)
def test_two_launches_generous_stash(kind, R, n):
    parked, n_ovf = run_two_launches(kind, R, n, 192)
    assert n_ovf == 0
    assert (parked == 0) == (kind == "none") and (parked == R * n or kind != "all")


@pytest.mark.parametrize("cap", [1, 40, 64])
def test_two_launches_regions_that_fill_up(cap):
    """all live, (200, 192): 300 passes over at most 256 workgroups, a wave sees 32 or 64 live samples.  One slot per region;
    a region that ends in the middle of a tile's live columns (40 = 32 + 8); exactly enough (64)."""
    parked, n_ovf = run_two_launches("all", 200, 192, cap)
    assert parked > 0 and (n_ovf == 0) == (cap == 64)
    parked, n_ovf = run_two_launches("base", 200, 192, cap)
    assert parked > 0


# ------------------------------------------------------------------------------------------------ 2: renders
def render(pair, ro, rd, jit, nc, nf, cull, stash):
    """tgtc_render_rays_plain on the chain with canaried outputs and workspace; stash: None or the attached part"""
    from tgtc_style_amd import hip
    lib = hip.load()
    R = ro.shape[0]
    fine = pair[1].packed()
    fine.set_cull(hip.CULL_ON if cull else hip.CULL_OFF)
    fine.set_stash(stash)
    need = lib.tgtc_render_workspace_bytes(R, nc, nf)
    ws = torch.full((need + 256,), 0x3C, dtype=torch.uint8, device="cuda")
    rgb = torch.full((R + 8, 3), CANARY, device="cuda")
    t = torch.full((R + 8,), CANARY, device="cuda")
    before = fine.culled_renders()
    hip.check(lib.tgtc_render_rays_plain(pair[0].packed().handle, fine.handle, hip.ptr(ro), hip.ptr(rd), R, nc, nf, 0.0, 1.0,
                                         hip.ptr(jit), hip.PATH_CHAIN, hip.ptr(ws), need, hip.ptr(rgb), hip.ptr(t), None, None,
                                         hip.stream()))
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0x3C).all()) and bool((rgb[R:] == CANARY).all()) and bool((t[R:] == CANARY).all())
    return rgb[:R].clone(), t[:R].clone(), fine.culled_renders() - before, fine.live_fraction()


def frame_rays(R, nc, seed=11):
    from tgtc_style_amd import utils
    o, d = utils.gen_rays(400, 400, synth.fern_intrinsics(400, 400), synth.spiral_pose(0))
    step = 160000 // R
    jit = torch.from_numpy(np.random.default_rng(seed).uniform(0, 1, (R, nc)).astype(np.float32)).cuda()
    return o[::step][:R].contiguous(), d[::step][:R].contiguous(), jit


_off = {}


def render_off(kind, R, nc, nf):
    if (kind, R, nc, nf) not in _off:
        ro, rd, jit = frame_rays(R, nc)
        rgb, t, culled, _ = render(nets(kind), ro, rd, jit, nc, nf, False, None)
        assert culled == 0 and bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(t).all())
        _off[(kind, R, nc, nf)] = (ro, rd, jit, rgb, t)
    return _off[(kind, R, nc, nf)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("R,nc,nf", RENDER_SHAPES)
def test_render_stash_bits_of_cull_off(kind, R, nc, nf):
    from tgtc_style_amd import hip
    ro, rd, jit, rgb_off, t_off = render_off(kind, R, nc, nf)
    # 6 x R x nc floats of dead coarse planes hold the overflow list and the scratch, or the pass is dense
    fits = 6 * R * nc * 4 >= R * (nc + nf) * 4 + 8192
    buf, part = new_stash(n=hip.load().tgtc_net_stash_bytes(R, nc + nf, 1.0))          # a region holds all its wave sees
    try:
        rgb, t, culled, share = render(nets(kind), ro, rd, jit, nc, nf, True, part)
        print(kind, R, nc, nf, "culled", culled, "live share", share)
        assert fits and culled == 1 and stash_canary_ok(buf)
        assert torch.equal(rgb, rgb_off) and torch.equal(t, t_off)
        if kind in ("none", "all"):
            assert share == (1.0 if kind == "all" else 0.0)
    finally:
        nets(kind)[1].packed().set_stash(None)


@pytest.mark.parametrize("kind", ["base", "all"])
def test_render_stash_capacities_and_state_between_launches(kind):
    """(200, 128 + 64) with the stash detached ("zero"), one slot per region, a region that ends inside a tile's live columns,
    exactly enough for the all-live net (64 per wave), generous; the same render twice without re-attaching; and a render
    with room for everything straight after one that overflowed, on the same scratch planes."""
    R, nc, nf = 200, 128, 64
    ro, rd, jit, rgb_off, t_off = render_off(kind, R, nc, nf)
    pair = nets(kind)
    try:
        for cap in (None, 1, 40, 64, 400):
            buf, part = (None, None) if cap is None else new_stash(cap)
            for again in range(2):
                rgb, t, culled, _ = render(pair, ro, rd, jit, nc, nf, True, part)
                assert culled == 1 and (buf is None or stash_canary_ok(buf))
                assert torch.equal(rgb, rgb_off) and torch.equal(t, t_off), (cap, again)
        small, big = new_stash(1), new_stash(400)
        for buf, part in (small, big, small, big):
            rgb, t, culled, _ = render(pair, ro, rd, jit, nc, nf, True, part)
            assert culled == 1 and stash_canary_ok(buf) and torch.equal(rgb, rgb_off) and torch.equal(t, t_off)
    finally:
        pair[1].packed().set_stash(None)


def test_ray_renderer_attaches_a_stash_as_its_default_says():
    from tgtc_style_amd import rendering
    R, nc, nf = 200, 128, 64
    ro, rd, jit, rgb_off, t_off = render_off("base", R, nc, nf)
    pair = nets("base")
    fine = pair[1].packed()
    try:
        for stash in (None, True, False):
            r = rendering.RayRenderer(pair[0], pair[1], fused=False, cull=True, stash=stash)
            out = r.render(ro, rd, nc, nf, jitter=jit)
            torch.cuda.synchronize()
            want = rendering.RayRenderer.STASH_DEFAULT if stash is None else stash
            assert (fine.stash is not None) == want
            assert torch.equal(out["rgb"], rgb_off) and torch.equal(out["t"], t_off)
        r = rendering.RayRenderer(pair[0], pair[1], fused=False, cull=False, stash=True)      # never with cull=False
        r.render(ro, rd, nc, nf, jitter=jit)
        torch.cuda.synchronize()
        assert fine.stash is None
    finally:
        fine.set_stash(None)


# ------------------------------------------------------------------------------------------------ 3: argument rules
def test_stash_argument_rules():
    from tgtc_style_amd import hip
    lib = hip.load()
    fine = nets("base")[1].packed()
    buf = torch.zeros(stash_bytes(2) + 512, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    assert p % 256 == 0
    one = stash_bytes(1)
    assert lib.tgtc_net_stash_bytes(1, 1, 0.0) == one
    assert lib.tgtc_net_set_stash(fine.handle, p, one) == 0
    assert lib.tgtc_net_set_stash(fine.handle, None, 0) == 0                      # detach
    ro, rd, ts = (x.cuda() for x in nk.ray_inputs(7, 16))
    sig = torch.zeros(7 * 16, device="cuda")
    scr = torch.zeros(SCRATCH_WORDS, dtype=torch.int32, device="cuda")
    ovf = torch.zeros(7 * 16, dtype=torch.int32, device="cuda")
    assert lib.tgtc_nerf_stash_fill(fine.handle, hip.ptr(ro), hip.ptr(rd), hip.ptr(ts), 7, 16, hip.ptr(sig), hip.ptr(scr), hip.ptr(ovf),
                                    hip.stream()) == -1                            # detached: nothing to fill
    assert lib.tgtc_net_set_stash(fine.handle, p, one - 16) == -1                 # too small for one slot per region
    assert lib.tgtc_net_set_stash(fine.handle, p + 16, one) == -1                 # misaligned
    assert lib.tgtc_net_set_stash(fine.handle, None, one) == -1 and lib.tgtc_net_set_stash(None, p, one) == -1
    for prec in ("fp16x3", "fp16"):                                               # other precisions are out of scope
        other = nets("base", prec)[1].packed()
        assert lib.tgtc_net_set_stash(other.handle, p, one) == -2
        assert lib.tgtc_net_set_stash(other.handle, None, 0) == 0
    torch.cuda.synchronize()


def test_case_lists_reach_the_shapes_named():
    assert [R * n for R, n in CALL_SHAPES] == [112, 128, 129, 38400] and 38400 // 128 > 256
    assert [(R * (nc + nf)) % 128 for R, nc, nf in RENDER_SHAPES[:3]] == [0, 64, 0] and (24, 8) == RENDER_SHAPES[3][1:]
