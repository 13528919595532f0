"""GPU: the culled stylised render (tgtc_render_rays_styled_sparse, csrc/mlp_style_sparse.hip, RayRenderer.render_latents /
render with min_weight, --cull_weight): sigma of every fine sample first, then the NeRF trunk + concat MLP + style MLP only
on the compact, ascending list of the samples whose compositing weight exceeds the threshold.

The parity statement at min_weight = 0 is BIT IDENTITY with the stylised chain and needs no tolerance: a dead sample has
weight exactly 0 and enters the pixel as +0 whatever its colour, and a live sample's colour does not depend on which samples
share its tile.  For a positive threshold the bound is the sum of the dropped weights (colours lie in [0,1]) plus the
rounding of an N-term float32 sum."""
import os

import numpy as np
import pytest
import torch

from tgtc_style_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def T(sd):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}


class Args:
    use_viewdir, act_type = True, "relu"
    embed_freq_coor, embed_freq_dir = 10, 4
    netdepth = netdepth_fine = 8
    netwidth = netwidth_fine = 256
    style_D, vae_latent = 8, 32
    precision = "fp16x3"


def make(precision, fine_sigma_bias=None, fine_sigma_const=None):
    """The nets of tests/test_multi_style_gpu.py; fine_sigma_bias is added to the fine net's sigma_layer.bias;
    fine_sigma_const makes the fine net's sigma that constant (sigma_layer.weight = 0, bias = the constant)."""
    from tgtc_style_amd import models
    a = type("A", (Args,), {"precision": precision})
    cm = models.StyleMLP_before_concat(a)
    cm.load_state_dict(T(synth.concat_state(2)))
    sm = models.StyleMLP_Wild_multilayers(a)
    sm.load_state_dict(T(synth.style_state(3)))
    nets = []
    for seed, mode in ((0, "coarse"), (1, "fine")):
        m = models.StyleNerf(a, mode=mode)
        sd = T(synth.nerf_state(seed))
        if mode == "fine" and fine_sigma_bias is not None:
            sd["net.sigma_layer.bias"] = sd["net.sigma_layer.bias"] + fine_sigma_bias
        if mode == "fine" and fine_sigma_const is not None:
            sd["net.sigma_layer.weight"] = torch.zeros_like(sd["net.sigma_layer.weight"])
            sd["net.sigma_layer.bias"] = torch.full_like(sd["net.sigma_layer.bias"], fine_sigma_const)
        m.load_state_dict(sd)
        nets.append(m.cuda())
    return cm.cuda(), sm.cuda(), nets


def sample_inputs(R, N, K, seed=5):
    rng = np.random.default_rng(seed)
    ro = torch.from_numpy(np.concatenate([rng.uniform(-1, 1, (R, 2)), -np.ones((R, 1))], 1))
    rd = torch.from_numpy(np.concatenate([rng.uniform(-.3, .3, (R, 2)), 2 * np.ones((R, 1))], 1))
    ts = torch.from_numpy(np.sort(rng.uniform(0, 1, (R, N)).astype(np.float32), -1))
    zs = torch.from_numpy(np.stack([rng.standard_normal((R, 32)).astype(np.float32) for _ in range(K)]))
    return ro, rd, ts, zs


def render_inputs(R, nc, K, seed=11):
    rng = np.random.default_rng(seed)
    ro = torch.from_numpy(np.concatenate([rng.uniform(-1, 1, (R, 2)), -np.ones((R, 1))], 1)).cuda()
    rd = torch.from_numpy(np.concatenate([rng.uniform(-.3, .3, (R, 2)), 2 * np.ones((R, 1))], 1)).cuda()
    zs = torch.from_numpy(rng.standard_normal((K, R, 32)).astype(np.float32)).cuda()
    jit = torch.from_numpy(rng.uniform(0, 1, (R, nc)).astype(np.float32)).cuda()
    return ro, rd, zs, jit


def renderers(precision, **kw):
    from tgtc_style_amd import models, rendering
    cm, sm, nets = make(precision, **kw)
    pair = models.StylePair(cm, sm)
    return rendering.RayRenderer(nets[0], nets[1], pair), rendering.RayRenderer(nets[0], nets[1], pair, fused=False), nets, pair


def workspace_planes(r, R, nc, nf, K):
    """The planes of the renderer's workspace by the layout include/tgtc_hip.h documents (each rounded up to 256 bytes):
    ts_c, sigma_c, w_c [R,nc]; ts_f, sigma_f [R,nt]; rgb_f [K,R,nt,3]; w_f [R,nt]; live uint32 [R*nt]; 8192 B scratch whose
    word 0 is the count."""
    torch.cuda.synchronize()
    ws, nt = r._ws_multi, nc + nf
    up = lambda words: (4 * words + 255) // 256 * 256
    out, off = {}, 0
    for name, words, shape in (("ts_c", R * nc, (R, nc)), ("sigma_c", R * nc, (R, nc)), ("w_c", R * nc, (R, nc)),
                               ("ts_f", R * nt, (R, nt)), ("sigma_f", R * nt, (R, nt)), ("rgb_f", K * R * nt * 3, (K, R, nt, 3)),
                               ("w_f", R * nt, (R, nt)), ("live", R * nt, (R * nt,)), ("scratch", 2048, (2048,))):
        out[name] = ws[off:off + 4 * words].view(torch.int32 if name in ("live", "scratch") else torch.float32).view(shape)
        off += up(words) if name != "scratch" else 8192
    from tgtc_style_amd import hip
    assert off == hip.load().tgtc_render_styled_sparse_workspace_bytes(R, nc, nf, K) and off <= ws.numel()
    return out


# ------------------------------------------------------------------------------------------------ 1: prerequisite
@pytest.mark.parametrize("precision", ["fp16x3", "fp16"])
@pytest.mark.parametrize("R,N", [(7, 192), (5, 37), (1, 1), (700, 192)])
def test_sigma_pass_bits_of_the_styled_kernel(precision, R, N):
    """The sigma pass is the sigma-only launch of tgtc_nerf_forward_rays on the fine net: its sigma is the sigma of
    tgtc_styled_forward_rays bit for bit (same packed stream, same dense_layer sequence for layers 0..8)."""
    from tgtc_style_amd import hip, models
    cm, sm, nets = make(precision)
    pair = models.StylePair(cm, sm)
    ro, rd, ts, zs = (t.cuda() for t in sample_inputs(R, N, 1))
    rgb = torch.empty(R, N, 3, device="cuda")
    s_styled = torch.full((R, N), float("nan"), device="cuda")
    s_pass = torch.full((R, N), float("nan"), device="cuda")
    lib = hip.load()
    hip.check(lib.tgtc_styled_forward_rays(nets[1].packed().handle, pair.packed().handle, hip.ptr(ro), hip.ptr(rd), hip.ptr(ts),
                                           hip.ptr(zs[0].contiguous()), R, N, hip.ptr(rgb), hip.ptr(s_styled), hip.stream()))
    hip.check(lib.tgtc_nerf_forward_rays(nets[1].packed().handle, hip.ptr(ro), hip.ptr(rd), hip.ptr(ts), R, N, None,
                                         hip.ptr(s_pass), hip.stream()))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(s_styled).all())
    assert torch.equal(s_pass, s_styled), float((s_pass - s_styled).abs().max())


# ------------------------------------------------------------------------------------------------ 2: bit identity at 0
RENDER_CASES = [(p, nc, nf) for p in ("fp16x3", "fp16") for nc, nf in ((128, 64), (64, 64), (100, 28))] + [("fp16mx+fp16x3", 128, 64)]


@pytest.mark.parametrize("precision,nc,nf", RENDER_CASES)
@pytest.mark.parametrize("K", [3, 1])
def test_cull_at_zero_bits_of_the_chain(precision, nc, nf, K):
    """render_latents(min_weight=0)["rgb"][k], ["t"] and render(z=zs[k], min_weight=0) = RayRenderer(fused=False).render(
    z=zs[k]), bit for bit, with and without jitter."""
    sparse, chain, _, _ = renderers(precision)
    R = 300
    ro, rd, zs, jit = render_inputs(R, nc, K)
    for jitter in (None, jit):
        out = sparse.render_latents(ro, rd, nc, nf, jitter=jitter, zs=zs, min_weight=0)
        assert out["rgb"].shape == (K, R, 3) and out["t"].shape == (R,) and out["live"].shape == ()
        n = int(out["live"])
        print(precision, nc, nf, K, "live", n, "of", R * (nc + nf))
        assert 0 < n < R * (nc + nf)
        for k in range(K):
            ref = chain.render(ro, rd, nc, nf, jitter=jitter, z=zs[k].contiguous())
            assert torch.equal(out["rgb"][k], ref["rgb"]), (k, float((out["rgb"][k] - ref["rgb"]).abs().max()))
            assert torch.equal(out["t"], ref["t"]), (k, float((out["t"] - ref["t"]).abs().max()))
            one = sparse.render(ro, rd, nc, nf, jitter=jitter, z=zs[k].contiguous(), min_weight=0)
            assert one["rgb"].shape == (R, 3) and torch.equal(one["rgb"], ref["rgb"]) and torch.equal(one["t"], ref["t"])
            assert int(one["live"]) == n
    with pytest.raises(ValueError):
        sparse.render(ro, rd, nc, nf, z=zs[0].contiguous(), min_weight=0, want_coarse=True)


# ------------------------------------------------------------------------------------------------ 3: the culling happened
@pytest.mark.parametrize("precision", ["fp16x3", "fp16"])
def test_the_list_is_what_the_header_says(precision):
    """live[:n] = the ascending indices where w_f > min_weight, n = out["live"] = word 0 of the scratch; w_f = the bits of
    tgtc_composite's weights on the workspace's sigma_f, ts_f; 0 < n < R*N at 0 and n(1e-4) < n(0)."""
    from tgtc_style_amd import hip
    sparse, _, _, _ = renderers(precision)
    R, nc, nf, K = 300, 128, 64, 2
    N = nc + nf
    ro, rd, zs, jit = render_inputs(R, nc, K)
    counts = {}
    for tau in (0., 1e-4):
        out = sparse.render_latents(ro, rd, nc, nf, jitter=jit, zs=zs, min_weight=tau)
        p = workspace_planes(sparse, R, nc, nf, K)
        n = int(out["live"])
        want = torch.nonzero(p["w_f"].reshape(-1) > tau).reshape(-1).to(torch.int32)
        assert n == want.numel() == int(p["scratch"][0])
        assert torch.equal(p["live"][:n], want)
        # the weights plane is the existing operator's
        w = torch.full((R, N), float("nan"), device="cuda")
        rgb_exp, t_exp = torch.empty(R, 3, device="cuda"), torch.empty(R, device="cuda")
        hip.check(hip.load().tgtc_composite(hip.ptr(p["rgb_f"][0]), hip.ptr(p["sigma_f"]), hip.ptr(p["ts_f"]), R, N, hip.ptr(rgb_exp),
                                            hip.ptr(t_exp), hip.ptr(w), hip.stream()))
        torch.cuda.synchronize()
        assert torch.equal(w, p["w_f"]) and torch.equal(t_exp, out["t"]) and torch.equal(rgb_exp, out["rgb"][0])
        # dead samples kept colour +0, live ones got one
        dead = torch.ones(R * N, dtype=torch.bool, device="cuda")
        dead[want.long()] = False
        flat = p["rgb_f"].reshape(K, R * N, 3)
        assert not bool(flat[:, dead].any()) and bool((flat[:, ~dead] > 0).all())
        counts[tau] = n
        print(precision, "tau", tau, "live", n, "of", R * N, "=", n / (R * N))
    assert 0 < counts[0.] < R * N and counts[1e-4] < counts[0.]


# ------------------------------------------------------------------------------------------------ 4: positive threshold
@pytest.mark.parametrize("precision", ["fp16x3", "fp16"])
def test_positive_threshold_moves_a_ray_by_at_most_its_dropped_weights(precision):
    sparse, _, _, _ = renderers(precision)
    R, nc, nf, K = 300, 128, 64, 2
    N = nc + nf
    ro, rd, zs, jit = render_inputs(R, nc, K)
    base = sparse.render_latents(ro, rd, nc, nf, jitter=jit, zs=zs, min_weight=0)
    rgb0, t0 = base["rgb"].clone(), base["t"].clone()
    for tau in (1e-5, 1e-4, 1e-3):
        out = sparse.render_latents(ro, rd, nc, nf, jitter=jit, zs=zs, min_weight=tau)
        w = workspace_planes(sparse, R, nc, nf, K)["w_f"].double()
        bound = torch.where((w > 0) & (w <= tau), w, torch.zeros_like(w)).sum(-1) + N * 2.0 ** -23          # [R]
        diff = (out["rgb"].double() - rgb0.double()).abs()                                                   # [K,R,3]
        print(precision, "tau", tau, "max diff", float(diff.max()), "max bound", float(bound.max()), "live", int(out["live"]))
        assert bool((diff <= bound[None, :, None]).all()), float((diff - bound[None, :, None]).max())
        assert torch.equal(out["t"], t0)


# ------------------------------------------------------------------------------------------------ 5: edges
def _same_as_chain(sparse, chain, ro, rd, nc, nf, zs, jitter=None, tau=0.):
    out = sparse.render_latents(ro, rd, nc, nf, jitter=jitter, zs=zs, min_weight=tau)
    assert bool(torch.isfinite(out["rgb"]).all()) and bool(torch.isfinite(out["t"]).all())
    assert float(out["rgb"].min()) >= 0 and float(out["rgb"].max()) <= 1 + 1e-5
    for k in range(zs.shape[0]):
        ref = chain.render(ro, rd, nc, nf, jitter=jitter, z=zs[k].contiguous())
        assert torch.equal(out["rgb"][k], ref["rgb"]) and torch.equal(out["t"], ref["t"]), k
    return out


@pytest.mark.parametrize("precision", ["fp16x3", "fp16"])
def test_edges_nothing_live_and_everything_live(precision):
    R, nc, nf, K = 40, 64, 64, 2
    ro, rd, zs, jit = render_inputs(R, nc, K)
    sparse, chain, _, _ = renderers(precision, fine_sigma_bias=-1e4)
    out = _same_as_chain(sparse, chain, ro, rd, nc, nf, zs, jit)
    assert int(out["live"]) == 0 and not bool(out["rgb"].any())
    # bias raised until every sigma is positive.  sigma of these nets spans about -180 .. +200 on these rays, so the bias that
    # lifts the lowest sigma above 0 puts the mean near 180: alpha is 1 to rounding from the first samples on, and the
    # transmittance (a product of factors >= 1e-10) underflows to exactly 0 part way down every ray.  A bias alone therefore
    # cannot make every weight positive with these nets (measured: 110 of 128 samples per ray live); this case checks the
    # chain's bits on rays whose every sigma is positive
    sparse, chain, _, _ = renderers(precision, fine_sigma_bias=1e3)
    out = _same_as_chain(sparse, chain, ro, rd, nc, nf, zs, jit)
    print(precision, "bias + 1e3: live", int(out["live"]), "of", R * (nc + nf))
    assert 0 < int(out["live"]) < R * (nc + nf)
    # everything live, n == R * N: sigma positive everywhere AND small enough for the transmittance to stay above 0 --
    # sigma_layer.weight = 0 and the bias raised to 8 (alpha ~ 0.1 per sample, T ~ e^-16 at the far end)
    sparse, chain, _, _ = renderers(precision, fine_sigma_const=8.0)
    out = _same_as_chain(sparse, chain, ro, rd, nc, nf, zs, jit)
    assert int(out["live"]) == R * (nc + nf)
    assert float(workspace_planes(sparse, R, nc, nf, K)["w_f"].min()) > 0


@pytest.mark.parametrize("precision", ["fp16x3", "fp16"])
def test_edges_one_ray_ragged_tile_and_many_tiles(precision):
    sparse, chain, _, _ = renderers(precision)
    # R = 1 and K = 1
    ro, rd, zs, jit = render_inputs(1, 128, 1)
    out = _same_as_chain(sparse, chain, ro, rd, 128, 64, zs, jit)
    print(precision, "R=1 live", int(out["live"]))
    # a live count that ends inside a tile (128 samples per workgroup in fp16x3, 256 in fp16), K = 1
    ro, rd, zs, jit = render_inputs(300, 128, 1)
    out = _same_as_chain(sparse, chain, ro, rd, 128, 64, zs, jit)
    n = int(out["live"])
    assert n % 256 != 0 and n % 128 != 0, n
    # more than one tile per CU: the persistent workgroups loop over the list
    ro, rd, zs, jit = render_inputs(6000, 128, 2)
    out = _same_as_chain(sparse, chain, ro, rd, 128, 64, zs, jit)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print(precision, "R=6000 live", int(out["live"]), "tiles per CU >=", int(out["live"]) / 256 / cus)
    assert int(out["live"]) > 256 * cus


# ------------------------------------------------------------------------------------------------ 6: the reference's own render
@pytest.mark.parametrize("precision", ["fp16x3", "fp16"])
@pytest.mark.parametrize("nc,nf", [(128, 64), (64, 64)])
def test_cull_at_zero_golden(golden, precision, nc, nf):
    """Golden g8_end_to_end by the recipe of test_render_latents_golden, at min_weight = 0, within that test's limits."""
    from tgtc_style_amd import models
    g = golden("g8_end_to_end")
    tag = "_%dc%df" % (nc, nf)
    r, _, _, _ = renderers(precision)
    lat = models.StyleLatents_variational(style_num=1, frame_num=20, latent_dim=32)
    lat.load_state_dict(T(synth.latents_state(4)))
    lat = lat.cuda()
    lat.sigma_scale = 1.0
    ro, rd = torch.from_numpy(g["rays_o" + tag]).cuda(), torch.from_numpy(g["rays_d" + tag]).cuda()
    R = ro.shape[0]
    z0 = lat(style_ids=torch.zeros(R, dtype=torch.long), frame_ids=torch.full((R,), 33, dtype=torch.long), type="llff")
    z1 = torch.from_numpy(np.random.default_rng(21).standard_normal((R, 32)).astype(np.float32)).cuda()
    zs = torch.stack([z0.float(), z1])
    lim = {"fp16x3": 1e-3, "fp16": 2e-2}[precision]
    for jt, jit in (("", None), ("_jit", torch.from_numpy(g["jit" + tag]).cuda())):
        out = r.render_latents(ro, rd, nc, nf, near=0., far=1., jitter=jit, zs=zs, min_weight=0)
        e = {"rgb": float((out["rgb"][0].cpu() - torch.from_numpy(g["styled_rgb" + jt + tag])).abs().max()),
             "t": float((out["t"].cpu() - torch.from_numpy(g["styled_t" + jt + tag])).abs().max())}
        print(precision, tag, jt, e, "live", int(out["live"]), "of", R * (nc + nf))
        assert max(e.values()) <= lim, e
        assert not torch.equal(out["rgb"][0], out["rgb"][1])


# ------------------------------------------------------------------------------------------------ 7: no state, no neighbours
@pytest.mark.parametrize("precision", ["fp16x3", "fp16"])
def test_no_state_between_latents_or_calls(precision):
    r, _, _, _ = renderers(precision)
    ro, rd, zs, jit = render_inputs(900, 128, 3)
    a = r.render_latents(ro, rd, 128, 64, jitter=jit, zs=zs, min_weight=0)
    perm = [2, 0, 1]
    b = r.render_latents(ro, rd, 128, 64, jitter=jit, zs=zs[perm].contiguous(), min_weight=0)
    assert torch.equal(b["rgb"], a["rgb"][perm]) and torch.equal(b["t"], a["t"]) and int(b["live"]) == int(a["live"])
    c = r.render_latents(ro, rd, 128, 64, jitter=jit, zs=zs, min_weight=0)
    assert torch.equal(c["rgb"], a["rgb"]) and torch.equal(c["t"], a["t"])
    assert not torch.equal(a["rgb"][0], a["rgb"][1]) and not torch.equal(a["rgb"][1], a["rgb"][2])


def test_a_ray_does_not_depend_on_its_neighbours_in_the_list():
    """Rays 3000:5000 of the 20-row strip of test_render_latents_full_size_properties rendered alone reproduce the strip's
    bits: compaction changes which samples share a tile, never a ray's result."""
    from tgtc_style_amd import models, utils
    H, W = 400, 400
    r, _, _, _ = renderers("fp16x3")
    lat = models.StyleLatents_variational(style_num=2, frame_num=20, latent_dim=32)
    lat.load_state_dict(T(synth.latents_state(4, style_num=2, frame_num=20)))
    lat = lat.cuda()
    lat.sigma_scale = 1.0
    ro, rd = utils.gen_rays(H, W, synth.fern_intrinsics(H, W), synth.spiral_pose(5), first_pixel=180 * W, n=20 * W)
    R = ro.shape[0]
    frame = torch.full((R,), 7, dtype=torch.long)
    zs = torch.stack([lat(style_ids=torch.full((R,), sid, dtype=torch.long), frame_ids=frame, type="llff").float()
                      for sid in range(2)]).cuda()
    a = r.render_latents(ro, rd, 128, 64, zs=zs, min_weight=0)
    a = {k: v.clone() for k, v in a.items()}
    assert bool(torch.isfinite(a["rgb"]).all()) and float(a["rgb"].min()) >= 0 and float(a["rgb"].max()) <= 1 + 1e-5
    print("strip live", int(a["live"]), "of", R * 192)
    b = r.render_latents(ro[3000:5000].contiguous(), rd[3000:5000].contiguous(), 128, 64, zs=zs[:, 3000:5000].contiguous(),
                         min_weight=0)
    assert torch.equal(a["rgb"][:, 3000:5000], b["rgb"]) and torch.equal(a["t"][3000:5000], b["t"])
    dense = r.render_latents(ro, rd, 128, 64, zs=zs)
    assert torch.equal(dense["rgb"], a["rgb"]) and torch.equal(dense["t"], a["t"]) and "live" not in dense


# ------------------------------------------------------------------------------------------------ 8: argument rules
def test_render_sparse_argument_rules():
    from tgtc_style_amd import hip, rendering
    lib = hip.load()
    r, _, nets, pair = renderers("fp16x3")
    R, nc, nf, K = 16, 64, 64, 2
    ro, rd, zs, _ = render_inputs(R, nc, K)
    need = lib.tgtc_render_styled_sparse_workspace_bytes(R, nc, nf, K)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    rgb, t = torch.empty(K, R, 3, device="cuda"), torch.empty(R, device="cuda")
    live = torch.zeros((), dtype=torch.int32, device="cuda")
    c, f, s = nets[0].packed().handle, nets[1].packed().handle, pair.packed().handle

    def call(coarse=c, fine=f, style=s, K=K, R=R, nc=nc, nf=nf, ws_bytes=need, z=zs, tau=0., count=live):
        return lib.tgtc_render_rays_styled_sparse(coarse, fine, style, hip.ptr(ro), hip.ptr(rd), hip.ptr(z), K, R, nc, nf, 0., 1.,
                                                  None, tau, hip.ptr(ws), ws_bytes, hip.ptr(rgb), hip.ptr(t), hip.ptr(count),
                                                  hip.stream())
    assert call() == 0 and call(count=None) == 0
    assert call(K=0) == -1 and call(R=-1) == -1 and call(nc=2) == -1 and call(nf=0) == -1 and call(z=None) == -1
    assert call(style=f) == -1 and call(fine=s) == -1 and call(ws_bytes=need - 1) == -1
    assert call(tau=-1e-6) == -1 and call(tau=float("nan")) == -1
    assert call(R=0) == 0
    _, _, nets16, _ = renderers("fp16")
    assert call(fine=nets16[1].packed().handle) == -1          # fine NeRF and style nets of different precisions
    assert call(K=1 << 20, R=1 << 10, ws_bytes=1 << 62) == -2   # K x R x N >= 2^31
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        r.render_latents(ro, rd, nc, nf, zs=zs, min_weight=-1.)
    with pytest.raises(ValueError):
        rendering.RayRenderer(nets[0], nets[1]).render(ro, rd, nc, nf, min_weight=0.)


# ------------------------------------------------------------------------------------------------ 9: CLI
def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


@pytest.mark.parametrize("share", [False, True])
def test_cli_cull_weight_zero_writes_the_same_files(tmp_path, share):
    """--render_valid_style --synthetic --cull_weight 0, with and without --share_geometry, writes PNGs byte-identical to
    the same command without the flag."""
    from tgtc_style_amd import train_tgtcs
    base = ["--config", os.path.join(ROOT, "configs", "fern.txt"), "--synthetic", "--synthetic_hw", "32", "--synthetic_frames", "2",
            "--synthetic_styles", "2", "--chunk", "1024", "--batch_size", "512", "--render_valid_style"]
    base += ["--share_geometry"] if share else []
    plain = _files(train_tgtcs.main(base + ["--basedir", str(tmp_path / "plain")]))
    culled = _files(train_tgtcs.main(base + ["--basedir", str(tmp_path / "culled"), "--cull_weight", "0"]))
    assert len(plain) == 8 and sorted(culled) == sorted(plain)
    for n in plain:
        assert culled[n] == plain[n], n


def test_cli_cull_weight_render_train_style(tmp_path):
    """--render_train_style --cull_weight 0 writes the file set of the run without the flag.  That run renders on the stylised
    ray kernel and this one on the chain's bits; the two differ by the compositing rounding between them (1.2e-7 on a pixel,
    as in test_cli_share_geometry), which can only flip a value that sits on an integer boundary: every image agrees to one
    8-bit level modulo 256 (to8b wraps), and a positive threshold leaves the depth images byte-identical to threshold 0."""
    from PIL import Image
    from tgtc_style_amd import train_tgtcs
    base = ["--config", os.path.join(ROOT, "configs", "fern.txt"), "--synthetic", "--synthetic_hw", "32", "--synthetic_frames", "2",
            "--chunk", "300", "--batch_size", "512", "--render_train_style"]
    plain = train_tgtcs.main(base + ["--basedir", str(tmp_path / "plain")])
    culled = train_tgtcs.main(base + ["--basedir", str(tmp_path / "culled"), "--cull_weight", "0"])
    some = train_tgtcs.main(base + ["--basedir", str(tmp_path / "some"), "--cull_weight", "1e-3"])
    names = sorted(os.listdir(plain))
    assert len(names) == 40 and sorted(os.listdir(culled)) == names and sorted(os.listdir(some)) == names
    img = lambda d, n: np.asarray(Image.open(os.path.join(d, n))).astype(np.int64)
    worst = 0
    for n in names:
        a, b = img(culled, n), img(plain, n)
        assert a.shape == b.shape
        d = (a - b) % 256
        worst = max(worst, int(np.minimum(d, 256 - d).max()))
        if "depth" in n:
            assert _files(some)[n] == _files(culled)[n], n
    print("levels between --cull_weight 0 and the default run:", worst)
    assert worst <= 1, worst


def _cli_rank(rank, world, port, argv):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), TGTC_DIST_BACKEND="gloo")
    from tgtc_style_amd import train_tgtcs
    train_tgtcs.main(argv)


@pytest.mark.parametrize("shard", ["frames", "rays"])
@pytest.mark.parametrize("share", [False, True])
def test_cli_cull_weight_two_ranks(tmp_path, shard, share):
    """--cull_weight 0 under two ranks (gloo rendezvous, both on one GPU) and both shardings: the files of the one-rank run."""
    import socket
    import torch.multiprocessing as mp
    from tgtc_style_amd import train_tgtcs
    common = ["--config", os.path.join(ROOT, "configs", "fern.txt"), "--synthetic", "--synthetic_hw", "20", "--synthetic_frames", "3",
              "--synthetic_styles", "2", "--chunk", "1024", "--batch_size", "128", "--render_valid_style", "--cull_weight", "0"]
    common += ["--share_geometry"] if share else []
    one = train_tgtcs.main(common + ["--basedir", str(tmp_path / "one")])
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = {k: os.environ.get(k) for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TGTC_DIST_BACKEND")}
    try:
        mp.spawn(_cli_rank, args=(2, port, common + ["--basedir", str(tmp_path / "two"), "--shard", shard]), nprocs=2, join=True)
    finally:
        for k, v in env.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    two = os.path.join(str(tmp_path / "two"), os.path.relpath(one, str(tmp_path / "one")))
    a, b = _files(one), _files(two)
    assert len(a) == 12 and sorted(b) == sorted(a)
    for n in a:
        assert a[n] == b[n], n
