"""CPU: the host side of `train_tgtcs --origin_train` -- flags and refusals, the learning-rate and checkpoint schedules,
the epoch sampler, the overflow policy, the optimiser layout of a reference-written checkpoint, and the image / camera
tables of a real LLFF scene directory.  The kernel and the loop itself run in tests/test_origin_train_gpu.py."""
import itertools
import os

import numpy as np
import pytest
import torch

from tgtc_style_amd import config as cfg

from origin_train_cases import FERN, ROOT, llff_scene

FILES = os.path.join(ROOT, "tests", "golden", "files")


def test_flags_parse_and_refusals_name_the_flag(monkeypatch):
    from tgtc_style_amd import train_tgtcs
    a = cfg.parse_args(["--config", FERN])
    assert a.origin_train is False and a.train_seed == 0 and a.train_unfused is False
    a = cfg.parse_args(["--config", FERN, "--origin_train", "--train_seed", "-1", "--train_unfused"])
    assert a.origin_train is True and a.train_seed == -1 and a.train_unfused is True
    for flag in ("--render_valid", "--render_train", "--render_valid_style", "--render_train_style"):
        with pytest.raises(SystemExit) as e:
            train_tgtcs.main(["--config", FERN, "--synthetic", "--origin_train", flag])
        assert "--origin_train" in str(e.value) and flag in str(e.value)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        train_tgtcs.main(["--config", FERN, "--synthetic", "--origin_train"])
    assert "--origin_train" in str(e.value) and "WORLD_SIZE" in str(e.value)


def test_learning_rate_schedule():
    from tgtc_style_amd import train_loop
    a = cfg.parse_args(["--config", FERN, "--lrate", "5e-4", "--lrate_decay", "250000"])
    for s in (0, 1, 250000):
        assert train_loop.lrate_at(a, s) == a.lrate * 0.1 ** (s / a.lrate_decay)
    assert train_loop.lrate_at(a, 0) == 5e-4 and abs(train_loop.lrate_at(a, 250000) - 5e-5) <= 1e-18


def test_save_cadence():
    from tgtc_style_amd import train_loop
    got = {s for s in range(0, 1101) if train_loop.saves_at(s, 1050)}
    assert got == {500, 1000} | set(range(1050, 1101))


def test_epoch_sampler_is_a_seeded_shuffle_per_epoch():
    from tgtc_style_amd.train_data import EpochSampler
    s = EpochSampler(105, 32, seed=3, device="cpu")
    assert s.batches_per_epoch == 4
    seq = list(itertools.islice(iter(s), 12))
    assert [len(b) for b in seq] == [32, 32, 32, 9] * 3 and all(b.dtype == torch.int64 for b in seq)
    epochs = [torch.cat(seq[4 * e:4 * e + 4]) for e in range(3)]
    for e in epochs:
        assert sorted(e.tolist()) == list(range(105))
    assert not torch.equal(epochs[0], epochs[1]) and not torch.equal(epochs[1], epochs[2]) and not torch.equal(epochs[0], epochs[2])
    again = list(itertools.islice(iter(EpochSampler(105, 32, seed=3, device="cpu")), 12))
    assert all(torch.equal(a, b) for a, b in zip(seq, again))
    other = list(itertools.islice(iter(EpochSampler(105, 32, seed=4, device="cpu")), 12))
    assert not all(torch.equal(a, b) for a, b in zip(seq, other))
    # resume: the batch of step s from a sampler that never saw the steps before it, in any order
    fresh = EpochSampler(105, 32, seed=3, device="cpu")
    for step in (11, 5, 0, 4, 7, 1, 2, 3, 6, 8, 9, 10):
        assert torch.equal(fresh.batch_indices(step), seq[step]), step


def test_overflow_policy():
    from tgtc_style_amd import train_loop
    assert train_loop.overflow_policy(0, 0, 20) == (None, False)
    assert train_loop.overflow_policy(7, 7, 20) == (None, False)
    msg, abort = train_loop.overflow_policy(7, 10, 20)
    assert not abort and "3 of 20" in msg
    msg, abort = train_loop.overflow_policy(7, 27, 20)
    assert abort and "20" in msg and "momentum" in msg
    assert train_loop.overflow_policy(0, 0, 0) == (None, False)          # the per-layer path has no guard and no count
    assert "not a" in train_loop.overflow_policy.__doc__.lower() and "adam" in train_loop.overflow_policy.__doc__.lower()


def test_reference_checkpoint_optimizer_loads_into_the_loops_adam(tmp_path):
    """tests/golden/files/000500.tar was written by the reference (gen_golden.py g13_files): ONE Adam over the coarse then
    the fine parameters.  Its state must load into the loop's optimiser, moment for parameter."""
    import shutil
    from tgtc_style_amd import checkpoints as ck, models, train_loop

    class A:
        use_viewdir, act_type, embed_freq_coor, embed_freq_dir = True, "relu", 10, 4
        netdepth = netdepth_fine = 8
        netwidth = netwidth_fine = 8
        style_D, vae_latent, precision = 8, 32, "fp16x3"
        lrate = 5e-4

    shutil.copy(os.path.join(FILES, "000500.tar"), tmp_path / "000500.tar")
    model, fine = models.StyleNerf(A, mode="coarse"), models.StyleNerf(A, mode="fine")
    assert ck.load_nerf(str(tmp_path), model, fine) == 500
    state = ck.load_nerf_optimizer(str(tmp_path))
    assert sorted(state) == ["param_groups", "state"] and len(state["state"]) == 48
    opt = train_loop.make_optimizer(A, model, fine)
    opt.load_state_dict(state)
    params = list(model.parameters()) + list(fine.parameters())
    assert len(params) == 48 and [id(p) for p in opt.param_groups[0]["params"]] == [id(p) for p in params]
    for i, p in enumerate(params):
        assert opt.state[p]["exp_avg"].shape == p.shape and opt.state[p]["exp_avg_sq"].shape == p.shape, i
        assert torch.equal(opt.state[p]["exp_avg"], state["state"][i]["exp_avg"])
    assert ck.load_nerf_optimizer(str(tmp_path / "nowhere")) is None


def test_train_rays_of_a_real_llff_directory(tmp_path):
    from tgtc_style_amd import llff_poses, train_data
    base, imgs = llff_scene(str(tmp_path / "scene"))
    assert train_data.missing_scene_parts(base, 4.0) == []
    data = train_data.TrainRays.from_llff(base, 4.0, "cpu")
    table = data.images.numpy()
    assert table.shape == (3, 6, 8, 3) and table.dtype == np.float32
    for i, a in enumerate(imgs):
        assert np.array_equal(table[i], (a / 255.).astype(np.float32))              # sorted file order
    assert (data.h, data.w) == (6, 8) and data.rays_num == 3 * 6 * 8 and data.frame_num == 3
    assert (data.near, data.far) == (0., 1.)
    sc = llff_poses.scene_poses(np.load(os.path.join(base, "poses_bounds.npy")), (6, 8), factor=4)
    assert data.f == float(sc["hwf"][2]) == np.float32(0.9 * 8)
    assert data.c2w.shape == (3, 12) and data.c2w.dtype == torch.float32
    assert np.array_equal(data.c2w.numpy().reshape(3, 3, 4), sc["poses"][:, :3, :4])
    # what --origin_train says about an incomplete scene
    empty = tmp_path / "empty"
    empty.mkdir()
    assert train_data.missing_scene_parts(str(empty), 4.0) == ["poses_bounds.npy", "images/ or images_4/"]


def test_library_exports_the_batch_kernel():
    import ctypes
    from tgtc_style_amd import hip
    assert "tgtc_train_batch" in open(os.path.join(ROOT, "include", "tgtc_train.h")).read()
    assert "tgtc_train_batch" in hip.header_symbols()
    assert hasattr(ctypes.CDLL(hip.LIB_PATH), "tgtc_train_batch")
