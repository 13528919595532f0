"""GPU: `tgtc_train_batch` against `utils.gen_rays` bit for bit, and `train_tgtcs --origin_train` end to end on the
synthetic teacher scene and on a fabricated LLFF directory: the loop learns, writes the reference's checkpoint files,
resumes, and its checkpoint renders."""
import os

import numpy as np
import pytest
import torch

from origin_train_cases import FERN, llff_scene

pytestmark = pytest.mark.gpu

SV = "fern_style_style_nerf_relu_UseViewDir_ImgFactor4"          # train_tgtcs.py:19-20 for configs/fern.txt
KEYS = ["global_step", "model", "model_fine", "optimizer", "style_optimizer"]


def _argv(basedir, *more):
    return ["--config", FERN, "--basedir", str(basedir), "--synthetic", "--synthetic_hw", "16", "--batch_size", "256",
            "--origin_train", "--i_print", "10", "--train_seed", "0"] + list(more)


def _run(basedir, *more):
    from tgtc_style_amd import train_loop, train_tgtcs
    sv = train_tgtcs.main(_argv(basedir, *more))
    return sv, list(train_loop.last_log)


# ------------------------------------------------------------------------------------------------ the kernel
F_, H_, W_ = 3, 5, 7


@pytest.fixture(scope="module")
def scene():
    from tgtc_style_amd import synth
    rng = np.random.default_rng(11)
    cps = np.stack([synth.spiral_pose(k) for k in (2, 40, 90)])              # three distinct cameras
    images = rng.random((F_, H_, W_, 3), dtype=np.float32)
    return cps, images


def _indices(R):
    n = F_ * H_ * W_
    rng = np.random.default_rng(R)
    if R == 1:
        return [np.array([n - 1]), np.array([0]), np.array([H_ * W_ + 2 * W_ + 3])]
    idx = rng.integers(0, n, R)
    idx[:4] = [0, n - 1, 17, 17]                                              # both ends and a duplicate
    idx[-1] = idx[5]
    return [idx]


@pytest.mark.parametrize("ndc", [True, False])
@pytest.mark.parametrize("pixel_alignment", [False, True])
@pytest.mark.parametrize("R", [1, 64, 257])
def test_train_batch_bits(scene, R, pixel_alignment, ndc):
    from tgtc_style_amd import hip, synth, train_data, utils
    cps, images = scene
    focal = synth.fern_intrinsics(H_, W_)
    data = train_data.TrainRays(images, cps, [H_, W_, focal], "cuda", ndc=ndc, pixel_alignment=pixel_alignment)
    frames = [utils.gen_rays(H_, W_, focal, cps[f], pixel_alignment=pixel_alignment, ndc=ndc) for f in range(F_)]
    ref_o = torch.stack([o for o, _ in frames]).reshape(-1, 3)               # [F*H*W, 3] in index order
    ref_d = torch.stack([d for _, d in frames]).reshape(-1, 3)
    ref_c = torch.from_numpy(images).reshape(-1, 3).cuda()
    for idx in _indices(R):
        index = torch.from_numpy(idx.astype(np.int64)).cuda()
        o, d, c = data.batch(index)
        assert o.shape == (R, 3) and o.dtype == torch.float64 and c.dtype == torch.float32
        assert torch.equal(o.view(torch.int64), ref_o[index].view(torch.int64))
        assert torch.equal(d.view(torch.int64), ref_d[index].view(torch.int64))
        assert torch.equal(c.view(torch.int32), ref_c[index].view(torch.int32))
        # no images, no colour: the same rays
        o2 = torch.full((R, 3), -7.0, device="cuda", dtype=torch.float64)
        d2 = torch.full((R, 3), -7.0, device="cuda", dtype=torch.float64)
        hip.check(hip.load().tgtc_train_batch(H_, W_, focal, focal, 0.5 * W_, 0.5 * H_, hip.ptr(data.c2w), F_, None,
                                              hip.ptr(index), R, int(pixel_alignment), int(ndc), 1.0, hip.ptr(o2), hip.ptr(d2),
                                              None, hip.stream()))
        assert torch.equal(o2.view(torch.int64), o.view(torch.int64)) and torch.equal(d2.view(torch.int64), d.view(torch.int64))


def test_train_batch_empty_and_bad_arguments(scene):
    from tgtc_style_amd import hip, synth, train_data
    cps, images = scene
    focal = synth.fern_intrinsics(H_, W_)
    data = train_data.TrainRays(images, cps, [H_, W_, focal], "cuda")
    o, d, c = data.batch(torch.empty(0, dtype=torch.int64, device="cuda"))
    assert o.shape == (0, 3) and d.shape == (0, 3) and c.shape == (0, 3)
    lib = hip.load()
    guard = torch.full((4, 3), 5.0, device="cuda", dtype=torch.float64)
    index = torch.zeros(4, dtype=torch.int64, device="cuda")
    call = lambda H, W, F, tab, idx, out_o, out_d, R=0: lib.tgtc_train_batch(
        H, W, focal, focal, 0.5 * W_, 0.5 * H_, tab, F, hip.ptr(data.images), idx, R, 0, 1, 1.0, out_o, out_d, None, hip.stream())
    assert call(H_, W_, F_, hip.ptr(data.c2w), hip.ptr(index), hip.ptr(guard), hip.ptr(guard)) == 0       # R = 0: TGTC_OK
    torch.cuda.synchronize()
    assert bool((guard == 5.0).all())                                                                       # ... and nothing written
    for bad in (call(0, W_, F_, hip.ptr(data.c2w), hip.ptr(index), hip.ptr(guard), hip.ptr(guard), 4),
                call(H_, 0, F_, hip.ptr(data.c2w), hip.ptr(index), hip.ptr(guard), hip.ptr(guard), 4),
                call(H_, W_, 0, hip.ptr(data.c2w), hip.ptr(index), hip.ptr(guard), hip.ptr(guard), 4),
                call(H_, W_, F_, None, hip.ptr(index), hip.ptr(guard), hip.ptr(guard), 4),
                call(H_, W_, F_, hip.ptr(data.c2w), None, hip.ptr(guard), hip.ptr(guard), 4),
                call(H_, W_, F_, hip.ptr(data.c2w), hip.ptr(index), None, hip.ptr(guard), 4),
                call(H_, W_, F_, hip.ptr(data.c2w), hip.ptr(index), hip.ptr(guard), None, 4)):
        assert bad == -1                                                                                    # TGTC_ERR_ARG
    torch.cuda.synchronize()
    assert bool((guard == 5.0).all())


# -------------------------------------------------------------------------------------------------- the loop
@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """40 steps at the config's learning rate, and the control: the same run (batches, draws) with --lrate 0."""
    a, b = tmp_path_factory.mktemp("trained"), tmp_path_factory.mktemp("control")
    sv, log = _run(a, "--origin_step", "40")
    sv0, log0 = _run(b, "--origin_step", "40", "--lrate", "0")
    return {"basedir": a, "sv": sv, "log": log, "sv0": sv0, "log0": log0}


def test_the_loop_learns(trained):
    log, log0 = trained["log"], trained["log0"]
    assert [e["step"] for e in log] == [0, 10, 20, 30, 40] == [e["step"] for e in log0]      # 5 120 rays: 20 batches an epoch
    assert [e["window"] for e in log] == [1, 10, 10, 10, 10]
    for e in log + log0:
        print(e)
        assert all(np.isfinite(e[k]) for k in ("loss", "loss_rgb", "loss_rgb_fine", "mean_loss", "psnr", "psnr_fine"))
        assert e["overflows"] == 0
    # step 0 runs before any update: same weights, same batch, same draws in both runs
    assert abs(log[0]["loss"] - log0[0]["loss"]) <= 1e-6 * log0[0]["loss"]
    assert log[-1]["mean_loss"] < log0[-1]["mean_loss"]


def test_the_files_of_a_run(trained):
    from tgtc_style_amd import checkpoints, config as cfg, models
    sv = trained["sv"]
    assert sv == os.path.join(str(trained["basedir"]), SV)
    assert sorted(f for f in os.listdir(sv) if f.endswith(".tar")) == ["000040.tar"]
    ck = torch.load(os.path.join(sv, "000040.tar"), map_location="cpu")
    assert sorted(ck) == KEYS and ck["global_step"] == 40
    assert len(ck["optimizer"]["state"]) == 48 and len(ck["style_optimizer"]["param_groups"][0]["params"]) == 26
    assert all(int(s["step"]) == 41 for s in ck["optimizer"]["state"].values())
    args = cfg.parse_args(["--config", FERN])
    model, fine = models.StyleNerf(args, mode="coarse"), models.StyleNerf(args, mode="fine")
    assert checkpoints.load_nerf(sv, model, fine) == 40
    for name, m in (("model", model), ("model_fine", fine)):
        assert list(m.state_dict()) == list(ck[name])
        for k, v in m.state_dict().items():
            assert torch.equal(v.view(torch.int32), ck[name][k].view(torch.int32)), (name, k)
    # trained weights, not the students' initial ones; the control's did not move
    from tgtc_style_amd import synth
    assert not np.array_equal(ck["model"]["net.base_layers.0.weight"].numpy(), synth.nerf_state(10)["net.base_layers.0.weight"])
    ck0 = torch.load(os.path.join(trained["sv0"], "000040.tar"), map_location="cpu")
    assert np.array_equal(ck0["model_fine"]["net.rgb_layers.1.weight"].numpy(), synth.nerf_state(11)["net.rgb_layers.1.weight"])


def test_the_trained_checkpoint_renders(trained):
    from tgtc_style_amd import train_tgtcs
    out = train_tgtcs.main(["--config", FERN, "--basedir", str(trained["basedir"]), "--synthetic", "--synthetic_hw", "16",
                            "--batch_size", "256", "--render_valid", "--synthetic_frames", "2"])
    assert out == os.path.join(trained["sv"], "nerf_gen_data2")
    assert {"rgb_00000.png", "rgb_00001.png"} <= set(os.listdir(out))


def test_resume_continues_the_run(tmp_path, capsys):
    sv, log = _run(tmp_path, "--origin_step", "20")
    assert [e["step"] for e in log] == [0, 10, 20] and os.path.exists(os.path.join(sv, "000020.tar"))
    capsys.readouterr()
    sv2, log2 = _run(tmp_path, "--origin_step", "30")
    said = capsys.readouterr().out
    assert sv2 == sv and "Resuming" in said and "step 20" in said
    assert [e["step"] for e in log2] == [30] and log2[0]["window"] == 10          # steps 21 ... 30
    assert sorted(f for f in os.listdir(sv) if f.endswith(".tar")) == ["000020.tar", "000030.tar"]
    ck = torch.load(os.path.join(sv, "000030.tar"), map_location="cpu")
    assert sorted(ck) == KEYS and ck["global_step"] == 30
    assert all(int(s["step"]) == 31 for s in ck["optimizer"]["state"].values())
    stamp = os.path.getmtime(os.path.join(sv, "000030.tar"))
    sv3, log3 = _run(tmp_path, "--origin_step", "30")
    assert sv3 == sv and log3 == log2 and "nothing to train" in capsys.readouterr().out     # the log of the last loop that ran
    assert os.path.getmtime(os.path.join(sv, "000030.tar")) == stamp


def test_train_unfused_agrees_at_step_zero(tmp_path, trained):
    sv, log = _run(tmp_path, "--origin_step", "4", "--i_print", "1", "--train_unfused")
    assert [e["step"] for e in log] == [0, 1, 2, 3, 4]
    assert all(np.isfinite(e["loss"]) and np.isfinite(e["loss_rgb_fine"]) and e["overflows"] == 0 for e in log)
    fused0 = trained["log"][0]["loss"]
    print("step-0 loss: fused %.9g, per-layer %.9g" % (fused0, log[0]["loss"]))
    assert abs(log[0]["loss"] - fused0) <= 2e-5 * abs(fused0)
    assert os.path.exists(os.path.join(sv, "000004.tar"))


def test_origin_train_from_a_real_llff_directory(tmp_path):
    from tgtc_style_amd import train_loop, train_tgtcs
    base, _ = llff_scene(str(tmp_path / "scene"))
    sv = train_tgtcs.main(["--config", FERN, "--basedir", str(tmp_path / "logs"), "--datadir", base, "--origin_train",
                           "--origin_step", "2", "--batch_size", "32", "--i_print", "1"])
    assert sorted(f for f in os.listdir(sv) if f.endswith(".tar")) == ["000002.tar"]
    ck = torch.load(os.path.join(sv, "000002.tar"), map_location="cpu")
    assert sorted(ck) == KEYS and ck["global_step"] == 2
    assert [e["step"] for e in train_loop.last_log] == [0, 1, 2] and all(np.isfinite(e["loss"]) for e in train_loop.last_log)
    with pytest.raises(SystemExit) as e:
        train_tgtcs.main(["--config", FERN, "--basedir", str(tmp_path / "logs2"), "--datadir", str(tmp_path / "nowhere"),
                          "--origin_train", "--origin_step", "2"])
    assert "poses_bounds.npy" in str(e.value) and "images" in str(e.value)
