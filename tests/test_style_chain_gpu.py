"""GPU: the style trainer (include/tgtc_train.h "Style trainer", style_chain.StyleTrainer) against the per-layer path
(autograd_ops.py: `.trainable()` modules on the expanded, concatenated inputs) and against float64 autograd on the oracle's
formulas: forward bits, the 26 parameter gradients and the two latent gradients, the edges of the C ABI, and
`training.style_train_iteration(chain=...)` on the synthetic scene."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

from origin_train_cases import FERN
from tgtc_style_amd import synth

pytestmark = pytest.mark.gpu

# (R, n): (5,7) rays straddle the 32-row tile, M = 35, pad columns in the transposed operands; (1,1) a single row; (100,7) the
# size of the per-layer path's own test; (9,128) M = 1152: the weight-gradient GEMM splits the samples over two batches;
# (9,129) the same split with pad columns (M = 1161 -> 2 x 608)
SHAPES = [(5, 7), (1, 1), (3, 64), (100, 7), (9, 128), (9, 129)]


def T(sd):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}


class Args:
    use_viewdir, act_type, embed_freq_coor, embed_freq_dir = True, "relu", 10, 4
    netdepth = netdepth_fine = 8
    netwidth = netwidth_fine = 256
    style_D, vae_latent, precision = 8, 32, "fp16x3"


CSD, SSD = synth.concat_state(2), synth.style_state(3)


def _models(precision="fp16x3"):
    from tgtc_style_amd import models
    cm, sm = models.StyleMLP_before_concat(Args), models.StyleMLP_Wild_multilayers(Args)
    cm.load_state_dict(T(CSD)), sm.load_state_dict(T(SSD))
    cm.precision = sm.precision = precision
    return cm.cuda().trainable(), sm.cuda().trainable()


@functools.lru_cache(maxsize=None)
def _inputs(R, n):
    rng = np.random.default_rng(1000 * R + n)
    M = R * n
    f = lambda a: torch.from_numpy(a.astype(np.float32))
    return {"x": f(rng.uniform(-1, 1, (R, n, 63))), "remap": f(np.maximum(rng.standard_normal((R, n, 256)), 0)),
            "z": f(rng.standard_normal((R, 32))), "zbar": f(np.repeat(rng.standard_normal((R, 1)), 32, axis=1)),
            "gt": f(rng.uniform(0, 1, (R, n, 3))), "M": M}


def _grads_of(cm, sm, z, zbar):
    g = {"c." + k: p.grad.detach().clone() for k, p in cm.state_dict(keep_vars=True).items()}
    g.update({"s." + k: p.grad.detach().clone() for k, p in sm.state_dict(keep_vars=True).items()})
    g["z"], g["zbar"] = z.grad.detach().clone(), zbar.grad.detach().clone()
    return g


@functools.lru_cache(maxsize=None)
def _per_layer(R, n, precision):
    """The per-layer path on the expanded inputs: rgb, the 12 traced activations, every gradient of mean((rgb - gt)^2)."""
    inp = _inputs(R, n)
    cm, sm = _models(precision)
    cm.act_trace, sm.act_trace = [], []
    x, remap, gt = inp["x"].cuda(), inp["remap"].cuda(), inp["gt"].cuda()
    z, zbar = inp["z"].cuda().requires_grad_(), inp["zbar"].cuda().requires_grad_()
    cf = cm(x=x, latent=z.unsqueeze(1).expand(R, n, 32))["concat_features"]
    rgb = sm(x=x, concated=torch.cat([remap, cf], -1), latent=zbar.unsqueeze(1).expand(R, n, 32))["rgb"]
    ((rgb - gt) ** 2).mean().backward()
    return {"rgb": rgb.detach(), "acts": [h.reshape(-1, 256) for h in cm.act_trace + sm.act_trace], "grads": _grads_of(cm, sm, z, zbar)}


@functools.lru_cache(maxsize=None)
def _chain(R, n, precision):
    from tgtc_style_amd import style_chain
    inp = _inputs(R, n)
    cm, sm = _models(precision)
    trainer = style_chain.StyleTrainer()
    trainer.trace_workspaces = []
    x, remap, gt = inp["x"].cuda(), inp["remap"].cuda(), inp["gt"].cuda()
    z, zbar = inp["z"].cuda().requires_grad_(), inp["zbar"].cuda().requires_grad_()
    rgb = trainer.apply(cm, sm, x, remap, z, zbar, n)
    assert rgb.shape == (R, n, 3)
    (ws, r_, n_), = trainer.trace_workspaces
    acts = [a.clone() for a in trainer.activations(ws, r_, n_)]            # copies: the workspace returns to the pool
    ((rgb - gt) ** 2).mean().backward()
    return {"rgb": rgb.detach(), "acts": acts, "grads": _grads_of(cm, sm, z, zbar)}


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ 1. forward bits
@pytest.mark.parametrize("precision", ["fp16x3", "fp16"])
@pytest.mark.parametrize("R,n", SHAPES)
def test_forward_bits_are_the_per_layer_path_s(R, n, precision):
    a, b = _chain(R, n, precision), _per_layer(R, n, precision)
    assert len(a["acts"]) == len(b["acts"]) == 12
    for i, (p, q) in enumerate(zip(a["acts"], b["acts"])):
        assert bool((q > 0).any()) or R * n == 1, i                          # a plane that is all zero would prove nothing
        assert _bits(p, q), "hidden activation %d" % i
    assert _bits(a["rgb"], b["rgb"])


# ------------------------------------------------------------------------------------------------ 2. gradients
def _oracle(R, n, gates, dtype):
    """The oracle's formulas (fields.concat_mlp / style_mlp) on one latent row per ray, each ReLU gate taken from the
    chain's forward (the recipe of test_style_mlp_gradients_match_the_oracle)."""
    inp = _inputs(R, n)
    M = inp["M"]
    cw = {k: v.clone().to(dtype).requires_grad_() for k, v in T(CSD).items()}
    sw = {k: v.clone().to(dtype).requires_grad_() for k, v in T(SSD).items()}
    z, zbar = inp["z"].clone().to(dtype).requires_grad_(), inp["zbar"].clone().to(dtype).requires_grad_()
    zz, zb = z.unsqueeze(1).expand(R, n, 32).reshape(M, 32), zbar.unsqueeze(1).expand(R, n, 32).reshape(M, 32)
    xx, remap, gt = inp["x"].reshape(M, 63).to(dtype), inp["remap"].reshape(M, 256).to(dtype), inp["gt"].reshape(M, 3).to(dtype)
    lin = lambda w, i, h: torch.nn.functional.linear(h, w["layers.%d.weight" % i], w["layers.%d.bias" % i])
    h = xx
    for i in range(5):
        h = torch.cat([h, zz], -1)
        h = torch.cat([h, xx], -1) if i == 4 else h
        h = lin(cw, i, h) * gates[i].to(dtype)
    h = torch.cat([remap, h, xx], -1)
    for i in range(7):
        h = torch.cat([h, zb], -1)
        h = torch.cat([h, xx], -1) if i == 4 else h
        h = lin(sw, i, h) * gates[5 + i].to(dtype)
    rgb = torch.sigmoid(lin(sw, 7, torch.cat([h, zb], -1)))
    ((rgb - gt) ** 2).mean().backward()
    g = {"c." + k: v.grad.double() for k, v in cw.items()}
    g.update({"s." + k: v.grad.double() for k, v in sw.items()})
    g["z"], g["zbar"] = z.grad.double(), zbar.grad.double()
    return g, rgb.detach()


@pytest.mark.parametrize("R,n", SHAPES)
def test_gradients_match_the_oracle_and_the_per_layer_path(R, n):
    """All 26 parameter gradients, d_lat_c (z) and d_lat_s (zbar): relative to the tensor's maximum, error <= max(2e-5, 3 x
    the error of the same formulas in float32), against float64 autograd and against the per-layer path."""
    a, b = _chain(R, n, "fp16x3"), _per_layer(R, n, "fp16x3")
    gates = [(h > 0).cpu() for h in a["acts"]]
    (g64, rgb64), (g32, _) = _oracle(R, n, gates, torch.float64), _oracle(R, n, gates, torch.float32)
    assert float((a["rgb"].double().cpu().reshape(-1, 3) - rgb64).abs().max()) <= 2e-5
    assert len(g64) == 28 and set(g64) == set(a["grads"]) == set(b["grads"])
    bad = []
    for k, ref in g64.items():
        scale = float(ref.abs().max()) + 1e-30
        yard = float((g32[k] - ref).abs().max()) / scale
        err = float((a["grads"][k].double().cpu() - ref).abs().max()) / scale
        err_pl = float((a["grads"][k].double() - b["grads"][k].double()).abs().max()) / scale
        print("%-22s max |ref| %.3e  chain vs float64 %.2e  chain vs per-layer %.2e  float32 yardstick %.2e" % (k, scale, err, err_pl, yard))
        if err > max(2e-5, 3 * yard) or err_pl > max(2e-5, 3 * yard):
            bad.append((k, err, err_pl, yard))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 3. edges
def _raw(R, n, precision="fp16x3"):
    """The pieces of one raw call: trainer, detached parameters, contiguous inputs on the device, upstream gradient."""
    from tgtc_style_amd import style_chain
    inp = _inputs(R, n)
    cm, sm = _models(precision)
    ps = [p.detach() for p in style_chain.chain_parameters(cm, sm)]
    M = inp["M"]
    dev = lambda k, w: inp[k].reshape(-1, w).cuda().contiguous()
    rgb = _chain(R, n, precision)["rgb"].reshape(M, 3).clone().requires_grad_()
    ((rgb - dev("gt", 3)) ** 2).mean().backward()                           # autograd's bits of the loss's gradient
    return style_chain.StyleTrainer(), ps, (dev("x", 63), dev("remap", 256), dev("z", 32), dev("zbar", 32)), rgb.grad.contiguous()


def _same(a, b, exact):
    """bit for bit; with the samples split over GEMM batches the bias gradient is summed by atomics in any order"""
    return _bits(a, b) if exact else bool((a - b).abs().max() <= 1e-6 * b.abs().max())


def test_null_latent_gradients():
    R, n = 5, 7
    trainer, ps, ins, d_rgb = _raw(R, n)
    ws = trainer.lease(R, n, "cuda")
    full = None
    for want_c, want_s in ((True, True), (False, True), (True, False), (False, False)):
        rgb = trainer.forward(ps, *ins, R, n, "fp16x3", ws)
        grads, d_c, d_s = trainer.backward(ps, d_rgb, R, n, ws, want_c, want_s)
        torch.cuda.synchronize()
        assert (d_c is None) == (not want_c) and (d_s is None) == (not want_s)
        if full is None:
            full = ([g.clone() for g in grads], d_c.clone(), d_s.clone())
            ref = _chain(R, n, "fp16x3")
            assert _bits(rgb, ref["rgb"].reshape(-1, 3)) and _bits(d_c, ref["grads"]["z"]) and _bits(d_s, ref["grads"]["zbar"])
            continue
        assert all(_bits(g, f) for g, f in zip(grads, full[0]))
        assert d_c is None or _bits(d_c, full[1])
        assert d_s is None or _bits(d_s, full[2])


def test_no_rays():
    from tgtc_style_amd import hip, style_chain
    from tgtc_style_amd.fused_train import _table
    cm, sm = _models()
    trainer = style_chain.StyleTrainer()
    e = lambda *s: torch.empty(*s, device="cuda")
    z, zbar = e(0, 32).requires_grad_(), e(0, 32).requires_grad_()
    rgb = trainer.apply(cm, sm, e(0, 7, 63), e(0, 7, 256), z, zbar, 7)
    assert rgb.shape == (0, 7, 3)
    rgb.sum().backward()
    torch.cuda.synchronize()
    for p in list(cm.parameters()) + list(sm.parameters()):
        assert p.grad is not None and bool((p.grad == 0).all())
    assert z.grad.shape == (0, 32)
    # the C ABI: R == 0 is TGTC_OK with NULL everything else; the backward zero-fills the gradients
    ps = [p.detach() for p in style_chain.chain_parameters(cm, sm)]
    grads = [torch.full_like(p, 7.0) for p in ps]
    lib = trainer.lib
    assert lib.tgtc_style_trainer_forward(trainer.handle, None, None, None, None, None, 0, 7, 0, None, 0, None, hip.stream()) == 0
    assert lib.tgtc_style_trainer_backward(trainer.handle, None, None, 0, 7, None, 0, _table(grads), None, None, hip.stream()) == 0
    torch.cuda.synchronize()
    assert all(bool((g == 0).all()) for g in grads)


def test_a_workspace_one_byte_short_is_refused_and_nothing_is_written():
    from tgtc_style_amd import hip
    from tgtc_style_amd.fused_train import _table
    R, n = 5, 7
    trainer, ps, ins, d_rgb = _raw(R, n)
    lib, need = trainer.lib, trainer.workspace_bytes(R, n)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    rgb = torch.full((R * n, 3), 7.0, device="cuda")
    fwd = lambda nbytes, prec=0, nn=n: lib.tgtc_style_trainer_forward(
        trainer.handle, _table(ps), *[hip.ptr(t) for t in ins], R, nn, prec, hip.ptr(ws), nbytes, hip.ptr(rgb), hip.stream())
    assert fwd(need - 1) == -1 and "workspace" in lib.tgtc_last_error().decode()
    assert fwd(need, prec=2) == -1 and fwd(need, nn=0) == -1                # fp16mx; no samples per ray
    torch.cuda.synchronize()
    assert bool((rgb == 7.0).all())
    grads = [torch.full_like(p, 7.0) for p in ps]
    d_c = torch.full((R, 32), 7.0, device="cuda")
    bwd = lambda nbytes: lib.tgtc_style_trainer_backward(trainer.handle, _table(ps), hip.ptr(d_rgb), R, n, hip.ptr(ws), nbytes,
                                                         _table(grads), hip.ptr(d_c), None, hip.stream())
    assert bwd(need) == -1 and "forward" in lib.tgtc_last_error().decode()   # no forward in this workspace yet
    assert fwd(need) == 0
    assert bwd(need - 1) == -1 and "workspace" in lib.tgtc_last_error().decode()
    torch.cuda.synchronize()
    assert all(bool((g == 7.0).all()) for g in grads) and bool((d_c == 7.0).all())
    assert bwd(need) == 0                                                    # the refused call did not consume the forward
    assert bwd(need) == -1                                                   # ... the accepted one did
    torch.cuda.synchronize()
    ref = _chain(R, n, "fp16x3")
    assert _bits(rgb, ref["rgb"].reshape(-1, 3)) and _bits(d_c, ref["grads"]["z"])
    assert _bits(grads[0], ref["grads"]["c.layers.0.weight"]) and _bits(grads[25], ref["grads"]["s.layers.7.bias"])


@pytest.mark.parametrize("R,n", [(5, 7), (9, 128), (9, 129)])
def test_a_workspace_of_ff_bytes_gives_the_same_results(R, n):
    """Every byte the calls read they wrote first: the pad columns of the transposed operands included ((5,7) and (9,129)
    have them; 0xFF halves are NaN)."""
    trainer, ps, ins, d_rgb = _raw(R, n)
    ws = trainer.lease(R, n, "cuda")
    ws.fill_(0xFF)
    rgb = trainer.forward(ps, *ins, R, n, "fp16x3", ws)
    grads, d_c, d_s = trainer.backward(ps, d_rgb, R, n, ws)
    torch.cuda.synchronize()
    ref = _chain(R, n, "fp16x3")
    exact = R * n < 1024                                                      # one GEMM batch: no atomics race
    assert _bits(rgb, ref["rgb"].reshape(-1, 3))
    names = ["c.layers.%d.%s" % (i, w) for i in range(5) for w in ("weight", "bias")] + \
            ["s.layers.%d.%s" % (i, w) for i in range(8) for w in ("weight", "bias")]
    for k, g in zip(names, grads):
        assert bool(torch.isfinite(g).all()), k
        assert _same(g, ref["grads"][k], exact or k.endswith("weight")), k
    assert _bits(d_c, ref["grads"]["z"]) and _bits(d_s, ref["grads"]["zbar"])


def test_two_forwards_before_one_backward_keep_their_own_stash():
    from tgtc_style_amd import style_chain
    (Ra, na), (Rb, nb) = (5, 7), (3, 64)
    cm, sm = _models()
    trainer = style_chain.StyleTrainer()
    trainer.trace_workspaces = []
    a, b = _inputs(Ra, na), _inputs(Rb, nb)
    za, zb_ = a["z"].cuda().requires_grad_(), b["z"].cuda().requires_grad_()
    ba, bb = a["zbar"].cuda().requires_grad_(), b["zbar"].cuda().requires_grad_()
    rgb_a = trainer.apply(cm, sm, a["x"].cuda(), a["remap"].cuda(), za, ba, na)
    rgb_b = trainer.apply(cm, sm, b["x"].cuda(), b["remap"].cuda(), zb_, bb, nb)
    assert trainer.trace_workspaces[0][0].data_ptr() != trainer.trace_workspaces[1][0].data_ptr()
    (((rgb_a - a["gt"].cuda()) ** 2).mean() + ((rgb_b - b["gt"].cuda()) ** 2).mean()).backward()
    ref_a, ref_b = _chain(Ra, na, "fp16x3"), _chain(Rb, nb, "fp16x3")
    assert _bits(rgb_a, ref_a["rgb"]) and _bits(rgb_b, ref_b["rgb"])
    assert _bits(za.grad, ref_a["grads"]["z"]) and _bits(zb_.grad, ref_b["grads"]["z"])
    assert _bits(ba.grad, ref_a["grads"]["zbar"]) and _bits(bb.grad, ref_b["grads"]["zbar"])
    for k, p in [("c." + k, p) for k, p in cm.state_dict(keep_vars=True).items()] + [("s." + k, p) for k, p in sm.state_dict(keep_vars=True).items()]:
        assert _bits(p.grad, ref_a["grads"][k] + ref_b["grads"][k]), k     # both under 1 024 samples: no atomics race
    assert len(trainer._pool) == 2                                           # both returned


# ------------------------------------------------------------------------------------------------ 4. the loop
N_S, N_F = 16, 16           # samples per ray: the same operators as fern's 64 + 64, a fraction of the time


def test_style_train_iteration_on_the_chain():
    """The synthetic scene at 16 x 16, batches of 64 + 64 rows, seeded draws: the first step's losses are those of the
    per-layer path (same forward bits), and ten steps on one batch reduce its pixel loss."""
    from tgtc_style_amd import config as cfg, models, style_chain, train_data, training
    args = cfg.parse_args(["--config", FERN, "--synthetic", "--synthetic_hw", "16", "--synthetic_styles", "2",
                           "--batch_size_style", "64", "--style_train", "--train_seed", "0"])
    data = train_data.StyleTrainRays.from_synthetic(args, "cuda")
    model, fine = models.StyleNerf(args, mode="coarse"), models.StyleNerf(args, mode="fine")
    model.load_state_dict(T(synth.nerf_state(0))), fine.load_state_dict(T(synth.nerf_state(1)))
    model, fine = model.cuda(), fine.cuda()
    model.set_enable_style(True), fine.set_enable_style(True)
    cm, sm = models.StyleMLP_before_concat(args), models.StyleMLP_Wild_multilayers(args)
    cm.load_state_dict(T(CSD)), sm.load_state_dict(T(SSD))
    lat = models.StyleLatents_variational(style_num=data.style_num, frame_num=data.frame_num, latent_dim=32)
    lat.load_state_dict(T(synth.latents_state(4, style_num=data.style_num, frame_num=data.frame_num)))
    cm, sm, lat = cm.cuda().trainable(), sm.cuda().trainable(), lat.cuda().trainable()
    B = 64
    index = torch.from_numpy(np.random.default_rng(0).permutation(data.data_num)[:B].astype(np.int64)).cuda()
    batch = data.batch(index, coh=(1, 2, 0, B))
    gen = torch.Generator(device="cuda")

    def run(cm_, sm_, lat_, chain, steps):
        opt_style = torch.optim.Adam(list(sm_.parameters()) + list(cm_.parameters()), lr=args.lrate)
        opt_lat = torch.optim.Adam([lat_.latents], lr=args.latent_lrate)
        coh, out = training.CoherenceState(data.frame_num), []
        for _ in range(steps):
            gen.manual_seed(5)                                                # the same draws at every step
            out.append(training.style_train_iteration(
                model, fine, cm_, sm_, lat_, opt_style, opt_lat, batch, B, N_S, N_F, data.near, data.far, coh, sigma_noise_std=1.0,
                logp_loss_lambda=0.1, loss_coh_lambda=100., coh_in_loss=False, generator=gen, check_ids=False, as_float=True, chain=chain))
        return out

    plain = run(copy.deepcopy(cm), copy.deepcopy(sm), copy.deepcopy(lat), None, 1)[0]
    steps = run(cm, sm, lat, style_chain.StyleTrainer(), 11)
    for k in ("loss", "loss_rgb", "loss_logp", "loss_coh", "total"):
        print("first step %-9s per-layer %.9g  chain %.9g" % (k, plain[k], steps[0][k]))
        assert np.isfinite(plain[k]) and abs(plain[k] - steps[0][k]) <= 1e-6 * abs(plain[k]), k
    print([s["loss_rgb"] for s in steps])
    assert all(np.isfinite(s["loss_rgb"]) for s in steps) and steps[10]["loss_rgb"] < steps[0]["loss_rgb"]
