"""GPU: `tgtc_style_train_batch` against `utils.gen_rays` and the tables bit for bit, the one-pass iteration against
`training.style_train_step`, and `train_tgtcs --style_train` end to end on the synthetic scene and on a fabricated
directory in the reference's layout: the loop learns, writes the reference's files, resumes, and its files render."""
import copy
import os

import numpy as np
import pytest
import torch

from origin_train_cases import FERN, llff_scene
from style_train_cases import style_inputs

pytestmark = pytest.mark.gpu

SV = "fern_style_style_nerf_relu_UseViewDir_ImgFactor4"          # train_tgtcs.py:19-20 for configs/fern.txt
S_, F_, H_, W_ = 2, 3, 5, 7
HW_ = H_ * W_
N_ = S_ * F_ * HW_


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.fixture(scope="module")
def scene():
    from tgtc_style_amd import synth
    rng = np.random.default_rng(11)
    cps = np.stack([synth.spiral_pose(k) for k in (2, 40, 90)])              # three distinct cameras
    images = rng.random((F_, H_, W_, 3), dtype=np.float32)
    stylized = rng.permutation(np.arange(N_ * 3) % 256).astype(np.uint8).reshape(S_, F_, H_, W_, 3)
    assert len(np.unique(stylized)) == 256                                    # every byte value is divided at least once
    return cps, images, stylized


def _data(scene, **kw):
    from tgtc_style_amd import synth, train_data
    cps, images, stylized = scene
    return train_data.StyleTrainRays(images, stylized, cps, [H_, W_, synth.fern_intrinsics(H_, W_)], "cuda", **kw)


def _indices(R):
    rng = np.random.default_rng(R)
    if R == 1:
        return [np.array([N_ - 1]), np.array([0]), np.array([F_ * HW_ + HW_ + 2 * W_ + 3])]
    idx = rng.integers(0, N_, R)
    idx[:4] = [0, N_ - 1, 17, 17]                                             # both ends and a duplicate
    idx[-1] = idx[5]
    return [idx]


def _reference(scene, data, pixel_alignment, ndc):
    """Per (frame, pixel): rays of utils.gen_rays; per (style, frame, pixel): float(table) / 255."""
    from tgtc_style_amd import utils
    cps, images, stylized = scene
    frames = [utils.gen_rays(H_, W_, data.f, cps[f], pixel_alignment=pixel_alignment, ndc=ndc) for f in range(F_)]
    ref_o = torch.stack([o for o, _ in frames]).reshape(-1, 3)
    ref_d = torch.stack([d for _, d in frames]).reshape(-1, 3)
    ref_gt = (torch.from_numpy(stylized).float() / 255).reshape(-1, 3).cuda()                # float32 division on the host
    assert np.array_equal(ref_gt.cpu().numpy().reshape(stylized.shape), np.float32(stylized) / 255)
    ref_org = torch.from_numpy(images).reshape(-1, 3).cuda()
    return ref_o, ref_d, ref_gt, ref_org


def _rows(idx, coh):
    """(style, frame, pixel) of every row of a batch, on the host."""
    s, rem = np.divmod(idx, F_ * HW_)
    f, p = np.divmod(rem, HW_)
    cs, cf, ca, n = coh
    i = np.arange(n)
    return (np.concatenate([s, np.full(n, cs)]), np.concatenate([f, np.full(n, cf)]), np.concatenate([p, (ca + i) % HW_]))


def _bits(a, b):
    v = torch.int64 if a.dtype == torch.float64 else torch.int32
    return torch.equal(a.view(v), b.view(v))


@pytest.mark.parametrize("ndc", [True, False])
@pytest.mark.parametrize("pixel_alignment", [False, True])
@pytest.mark.parametrize("R", [1, 64, 257])
def test_style_train_batch_bits(scene, R, pixel_alignment, ndc):
    data = _data(scene, ndc=ndc, pixel_alignment=pixel_alignment)
    ref_o, ref_d, ref_gt, ref_org = _reference(scene, data, pixel_alignment, ndc)
    for idx in _indices(R):
        index = torch.from_numpy(idx.astype(np.int64)).cuda()
        for n_coh in (0, 1, 40):                                              # 40 > H*W: the ordered rows wrap
            for coh_start in (0, 30, 70):                                     # 70 >= H*W: a window that left the frame
                coh = (1, 2, coh_start, n_coh) if coh_start else (0, 1, coh_start, n_coh)
                out = data.batch(index, coh=coh if n_coh else None)
                s, f, p = (torch.from_numpy(v).cuda() for v in _rows(idx, coh))
                T = R + n_coh
                assert out['rays_o'].shape == (T, 3) and out['rays_o'].dtype == torch.float64
                assert out['rgb_gt'].shape == (T, 3) and out['rgb_gt'].dtype == torch.float32
                assert out['style_id'].shape == (T,) and out['style_id'].dtype == torch.int64
                assert _bits(out['rays_o'], ref_o[f * HW_ + p]) and _bits(out['rays_d'], ref_d[f * HW_ + p])
                assert _bits(out['rgb_gt'], ref_gt[(s * F_ + f) * HW_ + p])
                assert _bits(out['rgb_origin'], ref_org[f * HW_ + p])
                assert torch.equal(out['style_id'], s) and torch.equal(out['frame_id'], f)


def _call(data, index, R, n_coh, outs, H=H_, W=W_, F=F_, S=S_, tab="c2w", images="images", stylized="stylized", coh=(1, 2, 30)):
    from tgtc_style_amd import hip
    p = lambda t: None if t is None else hip.ptr(t)
    get = lambda name: None if name is None else hip.ptr(getattr(data, name))
    return hip.load().tgtc_style_train_batch(H, W, data.f, data.f, 0.5 * W_, 0.5 * H_, get(tab), F, S, get(images), get(stylized),
                                             p(index), R, n_coh, coh[0], coh[1], coh[2], 0, 1, 1.0, *[p(t) for t in outs],
                                             hip.stream())


def _guards(T):
    mk = lambda dt: torch.full((T, 3), 5, device="cuda", dtype=dt)
    return [mk(torch.float64), mk(torch.float64), mk(torch.float32), mk(torch.float32),
            torch.full((T,), 5, device="cuda", dtype=torch.int64), torch.full((T,), 5, device="cuda", dtype=torch.int64)]


def test_null_outputs_leave_the_others_unchanged(scene):
    data = _data(scene)
    idx = _indices(64)[0]
    index = torch.from_numpy(idx.astype(np.int64)).cuda()
    full = data.batch(index, coh=(1, 2, 30, 40))
    names = ['rays_o', 'rays_d', 'rgb_gt', 'rgb_origin', 'style_id', 'frame_id']
    for drop in ([2], [3], [4], [5], [2, 3, 4, 5]):
        outs = _guards(104)
        passed = [None if k in drop else t for k, t in enumerate(outs)]
        assert _call(data, index, 64, 40, passed) == 0
        torch.cuda.synchronize()
        for k, t in enumerate(outs):
            if k in drop:
                assert bool((t == 5).all())
            else:
                assert _bits(t, full[names[k]]) if t.is_floating_point() else torch.equal(t, full[names[k]])
    # a colour output that is not asked for does not need its table
    outs = _guards(104)
    assert _call(data, index, 64, 40, [outs[0], outs[1], None, None, outs[4], outs[5]], images=None, stylized=None) == 0
    torch.cuda.synchronize()
    assert _bits(outs[0], full['rays_o']) and torch.equal(outs[5], full['frame_id'])


def test_empty_and_bad_arguments(scene):
    data = _data(scene)
    out = data.batch(torch.empty(0, dtype=torch.int64, device="cuda"))
    assert all(v.shape[0] == 0 for v in out.values()) and out['rays_o'].shape == (0, 3)
    only_coh = data.batch(torch.empty(0, dtype=torch.int64, device="cuda"), coh=(1, 0, 3, 5))     # index NULL with R == 0
    assert only_coh['frame_id'].tolist() == [0] * 5 and only_coh['style_id'].tolist() == [1] * 5
    index = torch.zeros(4, dtype=torch.int64, device="cuda")
    g = _guards(8)
    assert _call(data, index, 0, 0, g) == 0 and _call(data, None, 0, 0, g) == 0                   # TGTC_OK, nothing written
    bad = [_call(data, index, 4, 4, g, H=0), _call(data, index, 4, 4, g, W=0), _call(data, index, 4, 4, g, F=0),
           _call(data, index, 4, 4, g, S=0), _call(data, index, 4, 4, g, H=-3), _call(data, index, 4, 4, g, tab=None),
           _call(data, None, 4, 4, g), _call(data, index, 4, 4, [None] + g[1:]), _call(data, index, 4, 4, [g[0], None] + g[2:]),
           _call(data, index, 4, 4, g, coh=(S_, 0, 0)), _call(data, index, 4, 4, g, coh=(-1, 0, 0)),
           _call(data, index, 4, 4, g, coh=(0, F_, 0)), _call(data, index, 4, 4, g, coh=(0, -1, 0)),
           _call(data, index, 4, 4, g, coh=(0, 0, -1)), _call(data, index, 4, 4, g, stylized=None),
           _call(data, index, 4, 4, g, images=None), _call(data, index, -1, 4, g), _call(data, index, 4, -1, g)]
    assert bad == [-1] * len(bad)                                                                  # TGTC_ERR_ARG
    torch.cuda.synchronize()
    assert all(bool((t == 5).all()) for t in g)
    # the ordered batch's arguments are not looked at without ordered rows
    assert _call(data, index, 4, 0, g, coh=(S_, F_, -1)) == 0


def test_out_of_range_index_rows(scene):
    data = _data(scene)
    idx = np.array([3, -1, 100, N_, 7, 2 ** 40, -2 ** 62, N_ - 1], np.int64)
    out = data.batch(torch.from_numpy(idx).cuda(), coh=(1, 1, 4, 3))
    good = np.array([0, 2, 4, 7, 8, 9, 10])
    ok = data.batch(torch.from_numpy(idx[[0, 2, 4, 7]]).cuda(), coh=(1, 1, 4, 3))
    for k, v in out.items():
        assert torch.equal(v[good].view(torch.int64 if v.element_size() == 8 else torch.int32),
                           ok[k].view(torch.int64 if v.element_size() == 8 else torch.int32)), k
    for r in (1, 3, 5, 6):
        assert bool(torch.isnan(out['rays_o'][r]).all()) and bool(torch.isnan(out['rays_d'][r]).all())
        assert out['rgb_gt'][r].tolist() == [0, 0, 0] and out['rgb_origin'][r].tolist() == [0, 0, 0]
        assert int(out['style_id'][r]) == -1 and int(out['frame_id'][r]) == -1


# --------------------------------------------------------------------------------------------- the iteration
N_S, N_F = 16, 16           # samples per ray in the iteration tests: the same operators as 64 + 64, a fraction of the time


def _networks():
    from tgtc_style_amd import config as cfg, models, synth
    args = cfg.parse_args(["--config", FERN])
    t = lambda sd: {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}
    model, fine = models.StyleNerf(args, mode="coarse"), models.StyleNerf(args, mode="fine")
    model.load_state_dict(t(synth.nerf_state(0))), fine.load_state_dict(t(synth.nerf_state(1)))
    model, fine = model.cuda(), fine.cuda()
    model.set_enable_style(True), fine.set_enable_style(True)
    cm, sm = models.StyleMLP_before_concat(args), models.StyleMLP_Wild_multilayers(args)
    cm.load_state_dict(t(synth.concat_state(2))), sm.load_state_dict(t(synth.style_state(3)))
    lat = models.StyleLatents_variational(style_num=S_, frame_num=F_, latent_dim=32)
    lat.load_state_dict(t(synth.latents_state(4, style_num=S_, frame_num=F_)))
    return model, fine, cm.cuda().trainable(), sm.cuda().trainable(), lat.cuda().trainable()


def test_one_pass_iteration_agrees_with_style_train_step(scene):
    """Two iterations from the same state with given jitter, sigma_noise_std = 0 and learning rates of zero (the second one
    has a coherence term): the one-pass iteration against training.style_train_step batch by batch."""
    from tgtc_style_amd import training
    data = _data(scene)
    model, fine, cm, sm, lat = _networks()
    cm2, sm2, lat2 = copy.deepcopy(cm), copy.deepcopy(sm), copy.deepcopy(lat)
    R = B = 32
    opt = torch.optim.Adam(list(sm.parameters()) + list(cm.parameters()) + [lat.latents], lr=0.)
    opt_style = torch.optim.Adam(list(sm2.parameters()) + list(cm2.parameters()), lr=0.)
    opt_lat = torch.optim.Adam([lat2.latents], lr=0.)
    coh_a, coh_b = training.CoherenceState(F_), training.CoherenceState(F_)
    g = torch.Generator(device="cuda").manual_seed(5)
    common = dict(sigma_noise_std=0., rgb_loss_lambda=1.0, logp_loss_lambda=0.1, loss_coh_lambda=100., as_float=True)
    seen = []
    for it, coh in enumerate([(1, 0, 30), (1, 1, 30)]):
        index = torch.from_numpy(np.random.default_rng(it).permutation(N_)[:R].astype(np.int64)).cuda()
        batch = data.batch(index, coh=coh + (B,))
        jit = torch.rand(R + B, N_S, device="cuda", generator=g)
        a = training.style_train_step(
            model, fine, cm, sm, lat, opt, batch['rays_o'][:R], batch['rays_d'][:R], batch['rgb_gt'][:R], batch['style_id'][:R],
            batch['frame_id'][:R], N_S, N_F, 0., 1., jitter=jit[:R], coherence=coh_a,
            coh_batch={'rays_o': batch['rays_o'][R:], 'rays_d': batch['rays_d'][R:], 'rgb_origin': batch['rgb_origin'][R:],
                       'style_id': batch['style_id'][R:], 'frame_id': batch['frame_id'][R:], 'jitter': jit[R:]}, **common)
        b = training.style_train_iteration(model, fine, cm2, sm2, lat2, opt_style, opt_lat, batch, R, N_S, N_F, 0., 1., coh_b,
                                           jitter=jit, **common)
        for k in ('loss', 'loss_rgb', 'loss_logp', 'loss_coh'):
            print("iteration %d %-9s two passes %.9g  one pass %.9g" % (it, k, a[k], b[k]))
            assert np.isfinite(a[k]) and abs(a[k] - b[k]) <= 2e-5 * abs(a[k]), (it, k)
        assert abs(b['total'] - (b['loss'] + 100. * b['loss_coh'])) <= 1e-6 * abs(b['total'])
        seen.append(b)
    assert seen[0]['loss_coh'] == 0. and seen[1]['loss_coh'] > 0. and coh_a.cnt == coh_b.cnt == 2


def test_one_step_moves_what_the_two_optimisers_own(scene):
    from tgtc_style_amd import training
    data = _data(scene)
    model, fine, cm, sm, lat = _networks()
    before = {k: v.detach().clone() for k, v in list(lat.state_dict().items()) + [("sm." + k, v) for k, v in sm.state_dict().items()]}
    nerf_before = [p.detach().clone() for p in list(model.parameters()) + list(fine.parameters())]
    opt_style = torch.optim.Adam(list(sm.parameters()) + list(cm.parameters()), lr=5e-4)
    opt_lat = torch.optim.Adam([lat.latents], lr=1e-3)
    coh = training.CoherenceState(F_)
    R = B = 32
    # the shuffled rows name (style 0, frames 0 and 1) only; the ordered rows name (style 1, frames 1 and 2)
    index = torch.from_numpy(np.random.default_rng(1).integers(0, 2 * HW_, R).astype(np.int64)).cuda()
    g = torch.Generator(device="cuda")
    for it, frame in enumerate((1, 2)):
        g.manual_seed(it)
        batch = data.batch(index, coh=(1, frame, 0, B))
        r = training.style_train_iteration(model, fine, cm, sm, lat, opt_style, opt_lat, batch, R, N_S, N_F, 0., 1., coh,
                                           sigma_noise_std=1.0, logp_loss_lambda=0.1, loss_coh_lambda=100., generator=g,
                                           check_ids=False, as_float=True)
    assert r['loss_coh'] > 0 and np.isfinite(r['total'])
    grad = lat.latents.grad
    assert set(batch['frame_id'][:R].tolist()) == {0, 1} and set(batch['style_id'][:R].tolist()) == {0}
    assert bool((grad[0, 0] != 0).any()) and bool((grad[0, 1] != 0).any())
    assert bool((grad[0, 2] == 0).all()) and bool((grad[1] == 0).all())           # (1, 2) is named by the ordered rows
    now = lat.state_dict()
    assert torch.equal(now['style_latents_mu'], before['style_latents_mu'])
    assert torch.equal(now['style_latents_logvar'], before['style_latents_logvar'])
    assert not torch.equal(now['latents'][0, :2], before['latents'][0, :2])
    assert torch.equal(now['latents'][0, 2], before['latents'][0, 2]) and torch.equal(now['latents'][1], before['latents'][1])
    assert any(not torch.equal(v, before["sm." + k]) for k, v in sm.state_dict().items())
    for p, q in zip(list(model.parameters()) + list(fine.parameters()), nerf_before):
        assert torch.equal(p, q) and p.grad is None


# -------------------------------------------------------------------------------------------------- the loop
def _argv(basedir, *more):
    return ["--config", FERN, "--basedir", str(basedir), "--synthetic", "--synthetic_hw", "16", "--synthetic_styles", "2",
            "--batch_size_style", "64", "--style_train", "--train_seed", "0"] + list(more)


def _run(basedir, *more):
    from tgtc_style_amd import train_loop, train_tgtcs
    sv = train_tgtcs.main(_argv(basedir, *more))
    return sv, list(train_loop.last_log)


STEPS = 100


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """100 steps at the config's learning rates; the control: the same run (batches, draws) with both rates at 0; and the
    run whose style optimiser never sees the coherence term (--coh_until -1)."""
    a, b, c = (tmp_path_factory.mktemp(n) for n in ("trained", "control", "plain"))
    sv, log = _run(a, "--total_step", str(STEPS), "--i_print", "10")
    sv0, log0 = _run(b, "--total_step", str(STEPS), "--i_print", "10", "--lrate", "0", "--latent_lrate", "0")
    _, log1 = _run(c, "--total_step", str(STEPS), "--i_print", "10", "--coh_until", "-1")
    return {"basedir": a, "sv": sv, "log": log, "sv0": sv0, "log0": log0, "log1": log1}


def test_the_loop_learns(trained):
    """Measured on an MI355X, last 10-step window of 100 steps (trained / control with zero rates): mean of loss_rgb +
    loss_logp 6.356 / 6.730; mean pixel loss 0.517 / 0.328; mean of the style optimiser's loss 464.4 / 463.0.  With
    --coh_until -1: mean of loss_rgb + loss_logp 6.074, pixel loss of step 100 0.234 (control 0.336).  The window mean of a
    line is that of loss_rgb + loss_logp (train_loop.style_train says why)."""
    log, log0 = trained["log"], trained["log0"]
    assert [e["step"] for e in log] == list(range(0, 101, 10)) == [e["step"] for e in log0]
    assert [e["window"] for e in log] == [1] + [10] * 10
    for e in log + log0:
        print(e)
        assert all(np.isfinite(e[k]) for k in ("loss", "loss_coh", "only_loss", "loss_rgb", "loss_logp", "mean_loss",
                                               "mean_total", "mean_loss_rgb"))
        assert e["coh_in_loss"] is True and abs(e["loss"] - (e["loss_rgb"] + e["loss_logp"] + e["only_loss"])) <= 1e-5 * e["loss"]
    # step 0 runs before any update: same weights, same batches, same draws in both runs
    assert abs(log[0]["loss"] - log0[0]["loss"]) <= 1e-6 * log0[0]["loss"]
    assert log[-1]["mean_loss"] < log0[-1]["mean_loss"]
    # without the coherence term in the style optimiser's loss the pixel loss falls as well (with it, at fern's weight of
    # 1e2, the term's gradient on the scene's empty rays outweighs the pixel loss's: see train_loop.style_train)
    log1 = trained["log1"]
    print(log1[-1])
    assert all(e["coh_in_loss"] is False for e in log1) and log1[0]["loss"] == log0[0]["loss"] - log0[0]["only_loss"]
    assert log1[-1]["mean_loss_rgb"] < log0[-1]["mean_loss_rgb"] and log1[-1]["mean_loss"] < log0[-1]["mean_loss"]
    assert abs(log1[-1]["mean_total"] - log1[-1]["mean_loss"]) <= 1e-6 * log1[-1]["mean_loss"]
    # no coherence term at the first step, nor where the comparison restarts: every frame_num = 20 ordered batches
    # (train_tgtcs.py:396-403, :451-458); finite and positive everywhere else
    for lg in (log, log0):
        assert [e["loss_coh"] == 0. for e in lg] == [True, False] * 5 + [True]
        assert all(e["loss_coh"] > 0. for e in lg[1::2])
        assert abs(lg[1]["only_loss"] - 1e2 * lg[1]["loss_coh"]) <= 1e-6 * lg[1]["only_loss"]      # fern: loss_coh_lambda = 1e2


def test_the_files_of_a_run(trained):
    from tgtc_style_amd import checkpoints, config as cfg, models, synth
    sv = trained["sv"]
    assert sv == os.path.join(str(trained["basedir"]), SV)
    last = "%06d.tar" % STEPS
    assert sorted(f for f in os.listdir(sv) if f.endswith(".tar")) == ["latent_000000.tar", "latent_" + last,
                                                                       "style_000000.tar", "style_" + last]
    ck = torch.load(os.path.join(sv, "style_" + last), map_location="cpu")
    assert sorted(ck) == ["concat_model", "global_step", "model", "optimizer"] and ck["global_step"] == STEPS
    assert len(ck["optimizer"]["state"]) == 26 and all(int(s["step"]) == STEPS + 1 for s in ck["optimizer"]["state"].values())
    lk = torch.load(os.path.join(sv, "latent_" + last), map_location="cpu")
    assert sorted(lk) == ["global_step", "train_set_1"] and lk["global_step"] == STEPS
    assert sorted(lk["train_set_1"]) == ["latents", "style_latents_logvar", "style_latents_mu"]
    assert lk["train_set_1"]["latents"].shape == (2, 20, 32)
    args = cfg.parse_args(["--config", FERN])
    cm, sm = models.StyleMLP_before_concat(args), models.StyleMLP_Wild_multilayers(args)
    lat = models.StyleLatents_variational(style_num=2, frame_num=20, latent_dim=32)
    assert checkpoints.load_style(sv, sm, cm) == STEPS and checkpoints.load_latents(sv, lat)
    for got, want in ((sm.state_dict(), ck["model"]), (cm.state_dict(), ck["concat_model"]), (lat.state_dict(), lk["train_set_1"])):
        assert list(got) == list(want)
        for k, v in got.items():
            assert torch.equal(v.view(torch.int32), want[k].view(torch.int32)), k
    # trained: the style MLP and the latent table moved, mu / logvar did not; the control's files hold the initial values
    init = synth.latents_state(4, style_num=2, frame_num=20)
    assert not np.array_equal(ck["model"]["layers.0.weight"].numpy(), synth.style_state(3)["layers.0.weight"])
    assert not np.array_equal(lk["train_set_1"]["latents"].numpy(), init["latents"])
    assert np.array_equal(lk["train_set_1"]["style_latents_mu"].numpy(), init["style_latents_mu"])
    assert np.array_equal(lk["train_set_1"]["style_latents_logvar"].numpy(), init["style_latents_logvar"])
    ck0 = torch.load(os.path.join(trained["sv0"], "style_" + last), map_location="cpu")
    lk0 = torch.load(os.path.join(trained["sv0"], "latent_" + last), map_location="cpu")
    assert np.array_equal(ck0["concat_model"]["layers.0.weight"].numpy(), synth.concat_state(2)["layers.0.weight"])
    assert np.array_equal(lk0["train_set_1"]["latents"].numpy(), init["latents"])


def test_render_valid_style_picks_the_new_checkpoints_up(trained):
    from tgtc_style_amd import train_tgtcs
    out = train_tgtcs.main(["--config", FERN, "--basedir", str(trained["basedir"]), "--synthetic", "--synthetic_hw", "16",
                            "--synthetic_styles", "2", "--render_valid_style", "--synthetic_frames", "1"])
    assert out == os.path.join(trained["sv"], "render_valid_%d" % STEPS)
    assert len([f for f in os.listdir(out) if f.endswith(".png")]) >= 2


def test_resume_continues_the_run_and_prunes(tmp_path, capsys, monkeypatch):
    from tgtc_style_amd import train_loop
    monkeypatch.setattr(train_loop, "record_trace", True)
    more = ("--i_print", "10", "--i_weights", "5", "--ckp_num", "2")
    tars = lambda sv: sorted(f for f in os.listdir(sv) if f.endswith(".tar"))
    whole_sv, whole_log = _run(tmp_path / "whole", "--total_step", "20", *more)
    whole = {s: (i, c) for s, i, c in train_loop.last_trace}
    assert sorted(whole) == list(range(21)) and [e["step"] for e in whole_log] == [0, 10, 20]
    assert tars(whole_sv) == ["latent_000015.tar", "latent_000020.tar", "style_000015.tar", "style_000020.tar"]   # 0, 5, 10 pruned
    sv, log = _run(tmp_path / "parts", "--total_step", "10", *more)
    assert [e["step"] for e in log] == [0, 10] and tars(sv) == ["latent_000005.tar", "latent_000010.tar",
                                                                "style_000005.tar", "style_000010.tar"]
    capsys.readouterr()
    sv2, log2 = _run(tmp_path / "parts", "--total_step", "20", *more)
    said = capsys.readouterr().out
    assert sv2 == sv and "Resuming" in said and "step 10" in said and "[STYLE TRAIN] Iter: 11 " in said
    assert [e["step"] for e in log2] == [11, 20] and [e["window"] for e in log2] == [1, 9]
    assert log2[0]["loss_coh"] == 0. and log2[1]["loss_coh"] > 0.                # the coherence state restarts, as in the reference
    resumed = {s: (i, c) for s, i, c in train_loop.last_trace}
    assert sorted(resumed) == list(range(11, 21))
    for s in resumed:
        assert np.array_equal(resumed[s][0], whole[s][0]) and resumed[s][1] == whole[s][1], s
    assert len({c for _, c in whole.values()}) == 21 and whole[20][1] == (0, 0, 64)          # 20 frames, then the window moves
    assert tars(sv) == ["latent_000015.tar", "latent_000020.tar", "style_000015.tar", "style_000020.tar"]
    ck = torch.load(os.path.join(sv, "style_000020.tar"), map_location="cpu")
    assert ck["global_step"] == 20 and all(int(s["step"]) == 21 for s in ck["optimizer"]["state"].values())   # the Adam state was restored
    stamp = os.path.getmtime(os.path.join(sv, "style_000020.tar"))
    sv3, log3 = _run(tmp_path / "parts", "--total_step", "20", *more)
    assert sv3 == sv and log3 == log2 and "nothing to train" in capsys.readouterr().out
    assert os.path.getmtime(os.path.join(sv, "style_000020.tar")) == stamp


def test_a_nerf_checkpoint_short_of_origin_step_is_refused(tmp_path):
    from tgtc_style_amd import checkpoints, config as cfg, models
    args = cfg.parse_args(["--config", FERN])
    sv = os.path.join(str(tmp_path), SV)
    checkpoints.save_nerf(sv, 5, models.StyleNerf(args, mode="coarse"), models.StyleNerf(args, mode="fine"))
    with pytest.raises(SystemExit) as e:
        _run(tmp_path, "--origin_step", "100", "--total_step", "110")
    assert "step 5" in str(e.value) and "--origin_step 100" in str(e.value)
    assert not [f for f in os.listdir(sv) if "style" in f]
    sv2, log = _run(tmp_path, "--origin_step", "6", "--total_step", "8", "--i_print", "1")       # 5 + 1 >= 6: starts at step 6
    assert [e["step"] for e in log] == [6, 7, 8] and os.path.exists(os.path.join(sv2, "style_000008.tar"))


def test_the_whole_pipeline_from_a_fabricated_llff_directory(tmp_path):
    from tgtc_style_amd import checkpoints, models, train_loop, train_tgtcs
    base, _ = llff_scene(str(tmp_path / "scene"))
    common = ["--config", FERN, "--basedir", str(tmp_path / "logs"), "--datadir", base, "--origin_step", "2"]
    sv = train_tgtcs.main(common + ["--origin_train", "--batch_size", "32", "--i_print", "1"])
    # a latent table for the scene's one style and three frames (without a VAE file the latents come from a checkpoint)
    torch.manual_seed(3)
    checkpoints.save_latents(sv, 2, models.StyleLatents_variational(style_num=1, frame_num=3, latent_dim=32))
    gen = train_tgtcs.main(common + ["--render_train"])
    assert gen == os.path.join(sv, "nerf_gen_data2") and {"rgb_%05d.png" % i for i in range(3)} <= set(os.listdir(gen))
    with pytest.raises(SystemExit) as e:
        train_tgtcs.main(common + ["--style_train", "--total_step", "6"])
    assert "stylized_data.npz" in str(e.value)                                   # the 2-D pass has not run yet
    style_inputs(base, gen, rendered=True)
    sv2 = train_tgtcs.main(common + ["--style_train", "--total_step", "6", "--batch_size_style", "16", "--i_print", "1"])
    assert sv2 == sv
    assert [e["step"] for e in train_loop.last_log] == [3, 4, 5, 6] and all(np.isfinite(e["loss"]) for e in train_loop.last_log)
    tars = sorted(f for f in os.listdir(sv) if f.endswith(".tar") and ("style" in f or "latent" in f))
    assert tars == ["latent_000002.tar", "latent_000006.tar", "style_000006.tar"]
    assert torch.load(os.path.join(sv, "latent_000006.tar"), map_location="cpu")["train_set_1"]["latents"].shape == (1, 3, 32)
