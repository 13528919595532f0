"""CPU: the host side of `train_tgtcs --style_train` -- the frame-ordered walk against the reference's loader (g15), the
checkpoint / coherence / -log p schedules, the full-batch sampler, the tables of a fabricated directory in the reference's
layout, flags and refusals.  The kernel, the iteration and the loop run in tests/test_style_train_gpu.py."""
import itertools
import os

import numpy as np
import pytest
import torch

from tgtc_style_amd import config as cfg

from origin_train_cases import FERN, ROOT, llff_scene
from style_train_cases import style_inputs, write_stylized_data

G15 = os.path.join(ROOT, "tests", "golden", "g15_style_loader.npz")


def test_cursor_follows_the_reference_loader_call_by_call():
    from tgtc_style_amd.train_data import CoherenceCursor
    g = np.load(G15)
    assert g["cases"][:, :5].tolist() == [[2, 3, 4, 5, 8], [1, 3, 4, 5, 8], [3, 2, 3, 3, 4]]
    assert g["cases"][:, 5].tolist() == [40, 20, 40]
    for k, (S, F, h, w, B, calls) in enumerate(g["cases"].tolist()):
        want = g["case%d" % k]
        assert want.shape == (calls, 2 + B)
        c = CoherenceCursor(S, F, h * w, B)
        for n in range(calls):
            s, f, a = c.next()
            assert (s, f) == (want[n, 0], want[n, 1]), (k, n)
            assert [(a + i) % (h * w) for i in range(B)] == want[n, 2:].tolist(), (k, n)     # the kernel's pixel rule
    assert len({tuple(r[:2]) for r in g["case0"]}) == 6 and g["case0"][:, 0].max() == 1      # the walk reaches style 1


def test_cursor_at_n_is_n_steps_and_the_reset_starts_over():
    from tgtc_style_amd.train_data import CoherenceCursor
    for S, F, hw, B in ((2, 3, 20, 8), (1, 3, 20, 8), (3, 2, 9, 4), (1, 2, 6, 5)):
        c = CoherenceCursor(S, F, hw, B)
        for n in range(60):
            assert c.at(n).state() == c.state(), (S, F, hw, B, n)
            assert c.at(n).next() == CoherenceCursor(S, F, hw, B).at(n).next()
            s, f, a = c.next()
            assert 0 <= s < S and 0 <= f < F and 0 <= a and a + B < S * F * hw
    # (1, 2, 6, 5): 12 rows; a = 0, 0, 5, 5, then 10 + 5 >= 12 resets the walk
    c = CoherenceCursor(1, 2, 6, 5)
    assert [c.next() for _ in range(6)] == [(0, 0, 0), (0, 1, 0), (0, 0, 5), (0, 1, 5), (0, 0, 0), (0, 1, 0)]
    assert "reshuffle" in CoherenceCursor.__doc__ and "not reproduced" in CoherenceCursor.__doc__


def test_cursor_refuses_a_batch_as_large_as_the_data():
    from tgtc_style_amd.train_data import CoherenceCursor
    for B in (24, 25, 1000):
        with pytest.raises(ValueError) as e:
            CoherenceCursor(1, 2, 12, B)
        assert "replacement" in str(e.value)
    CoherenceCursor(1, 2, 12, 23)


def test_style_save_cadence():
    from tgtc_style_amd.train_loop import style_saves_at
    i_w, total = 5000, 128001
    want = {0: 3, 500: 0, 120500: 1, 121000: 1, 122000: 1, 122500: 0, 123000: 2, 128000: 2, 128001: 3, total: 3}
    for step, branch in want.items():
        assert style_saves_at(step, i_w, total) == branch, step
    assert style_saves_at(120000, i_w, total) == 3 and style_saves_at(125000, i_w, total) == 2    # branch 2 wins inside its range
    assert style_saves_at(120001, i_w, total) == 0 and style_saves_at(121500, i_w, total) == 1
    assert style_saves_at(130000, i_w, total) == 3 and style_saves_at(129000, i_w, total) == 0
    assert style_saves_at(40, i_w, 40) == 3 and style_saves_at(39, i_w, 40) == 0
    assert [s for s in range(1, 31) if style_saves_at(s, 10, 25)] == [10, 20, 25, 30]


def test_coherence_term_and_logp_weight_schedules():
    from tgtc_style_amd import train_loop
    a = cfg.parse_args(["--config", FERN])
    assert a.coh_until == 122000 and a.latent_lrate == 1e-3 and a.style_train is False
    assert train_loop.coh_in_loss(122000, a.coh_until) and not train_loop.coh_in_loss(122001, a.coh_until)
    assert train_loop.coh_in_loss(0, a.coh_until) and not train_loop.coh_in_loss(5, 4) and train_loop.coh_in_loss(4, 4)
    a = cfg.parse_args(["--config", FERN, "--logp_loss_lambda", "0.1", "--logp_loss_decay", "0.5", "--origin_step", "120001"])
    for step, power in ((120001, 0), (121000, 0), (121001, 1), (123456, 3), (128001, 8)):
        assert train_loop.logp_weight(a, step) == 0.1 * 0.5 ** power, step
    assert train_loop.logp_weight(a, 119002) == 0.1 * 0.5 ** 0           # int() truncates towards zero, as in the reference
    assert train_loop.logp_weight(a, 119001) == 0.1 * 0.5 ** -1
    # the ordered walk's position is a function of the step
    assert [train_loop.coh_calls_before(s, 120001) for s in (0, 7, 120001, 120002, 120010)] == [0, 7, 120001, 0, 8]


def test_full_batch_epoch_sampler():
    from tgtc_style_amd.train_data import EpochSampler
    s = EpochSampler(105, 32, seed=3, device="cpu", full_batches=True)
    assert s.batches_per_epoch == 3
    seq = list(itertools.islice(iter(s), 9))
    assert [len(b) for b in seq] == [32] * 9                               # no short batch
    for e in range(3):
        got = torch.cat(seq[3 * e:3 * e + 3]).tolist()
        assert len(set(got)) == 96 and min(got) >= 0 and max(got) < 105     # distinct indices within an epoch
    assert not torch.equal(seq[0], seq[3])
    # the same permutations as the default sampler: the option only drops the short batch
    d = EpochSampler(105, 32, seed=3, device="cpu")
    assert d.batches_per_epoch == 4 and torch.equal(d.batch_indices(0), seq[0]) and torch.equal(d.batch_indices(4), seq[3])
    fresh = EpochSampler(105, 32, seed=3, device="cpu", full_batches=True)
    for step in (8, 2, 5, 0):
        assert torch.equal(fresh.batch_indices(step), seq[step])
    with pytest.raises(ValueError):
        EpochSampler(10, 32, seed=3, device="cpu", full_batches=True)
    assert EpochSampler(32, 32, seed=0, device="cpu", full_batches=True).batches_per_epoch == 1


def test_tables_of_a_directory_in_the_reference_layout(tmp_path):
    import shutil
    from tgtc_style_amd import llff_poses, train_data
    base, _ = llff_scene(str(tmp_path / "scene"))
    gen = str(tmp_path / "logs" / "nerf_gen_data2")
    origin, stylised = style_inputs(base, gen)
    data = train_data.StyleTrainRays.from_directories(base, 4.0, gen, "cpu")
    assert (data.style_num, data.frame_num, data.h, data.w) == (1, 3, 6, 8) and data.data_num == 3 * 6 * 8
    assert data.images.dtype == torch.float32 and data.images.shape == (3, 6, 8, 3)
    assert data.stylized.dtype == torch.uint8 and data.stylized.shape == (1, 3, 6, 8, 3)
    for i in range(3):
        assert np.array_equal(data.images[i].numpy(), origin[i].astype(np.float32) / 255.)
        assert np.array_equal(data.stylized[0, i].numpy(), stylised[i])
    sc = llff_poses.scene_poses(np.load(os.path.join(base, "poses_bounds.npy")), (6, 8), factor=4)
    assert np.array_equal(data.c2w.numpy().reshape(3, 3, 4), sc["poses"][:, :3, :4]) and data.f == float(sc["hwf"][2])
    assert (data.near, data.far, data.ndc) == (0., 1., True)

    style_dir = os.path.join(base, "stylized_gen_4.0")

    def refused(*names):
        with pytest.raises(SystemExit) as e:
            train_data.StyleTrainRays.from_directories(base, 4.0, gen, "cpu")
        for n in names:
            assert n in str(e.value), (n, str(e.value))

    # more than one style in stylized_data.npz
    write_stylized_data(style_dir, 2)
    refused("one style per directory", "2 styles", "stylized_data.npz")
    write_stylized_data(style_dir, 1)
    # each missing part is named
    os.rename(os.path.join(style_dir, "002.jpg"), os.path.join(style_dir, "keep.jpg"))
    refused("002.jpg")
    os.rename(os.path.join(style_dir, "keep.jpg"), os.path.join(style_dir, "002.jpg"))
    os.rename(os.path.join(style_dir, "stylized_data.npz"), os.path.join(style_dir, "keep.npz"))
    refused("stylized_data.npz")
    os.rename(os.path.join(style_dir, "keep.npz"), os.path.join(style_dir, "stylized_data.npz"))
    os.rename(os.path.join(gen, "rgb_00002.png"), os.path.join(gen, "keep"))
    refused("2 rgb_*.png", "3 cameras")                                    # a frame-count mismatch
    os.rename(os.path.join(gen, "keep"), os.path.join(gen, "rgb_00002.png"))
    from PIL import Image
    Image.fromarray(np.zeros((5, 8, 3), np.uint8)).save(os.path.join(style_dir, "003.jpg"))
    refused("003.jpg", "6 x 8", "5 x 8")                                   # an image of the wrong size
    shutil.move(gen, gen + "_away")
    refused("rgb_*.png", "--render_train")
    shutil.move(gen + "_away", gen)
    os.remove(os.path.join(base, "poses_bounds.npy"))
    refused("poses_bounds.npy")


def test_synthetic_styles_are_seeded_and_not_the_identity():
    from tgtc_style_amd import train_data
    rng = np.random.default_rng(0)
    images = rng.random((2, 4, 5, 3), dtype=np.float32)
    plain = np.round(images * 255.).astype(np.uint8)
    for s in range(3):
        a, b = train_data._stylise(images, s), train_data._stylise(images, s)
        assert a.dtype == np.uint8 and a.shape == images.shape and np.array_equal(a, b)
        assert np.abs(a.astype(int) - plain.astype(int)).mean() > 20
    assert not np.array_equal(train_data._stylise(images, 0), train_data._stylise(images, 1))
    with pytest.raises(ValueError):
        train_data.StyleTrainRays(images, plain[None, :1], np.zeros((2, 3, 4), np.float32), [4, 5, 4.5], "cpu")


def test_flags_and_refusals(monkeypatch):
    from tgtc_style_amd import train_tgtcs
    a = cfg.parse_args(["--config", FERN, "--style_train", "--coh_until", "7", "--latent_lrate", "0.01"])
    assert a.style_train is True and a.coh_until == 7 and a.latent_lrate == 0.01
    assert all(k in cfg.HELP for k in ("style_train", "coh_until", "latent_lrate"))
    for flag in ("--render_valid", "--render_train", "--render_valid_style", "--render_train_style"):
        with pytest.raises(SystemExit) as e:
            train_tgtcs.main(["--config", FERN, "--synthetic", "--style_train", flag])
        assert "--style_train" in str(e.value) and flag in str(e.value)
    with pytest.raises(SystemExit) as e:
        train_tgtcs.main(["--config", FERN, "--synthetic", "--style_train", "--origin_train"])
    assert "--style_train" in str(e.value) and "--origin_train" in str(e.value)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        train_tgtcs.main(["--config", FERN, "--synthetic", "--style_train"])
    assert "--style_train" in str(e.value) and "WORLD_SIZE" in str(e.value)


def test_library_exports_the_style_batch_kernel():
    import ctypes
    from tgtc_style_amd import hip
    assert "tgtc_style_train_batch" in open(os.path.join(ROOT, "include", "tgtc_train.h")).read()
    assert "tgtc_style_train_batch" in hip.header_symbols()
    assert hasattr(ctypes.CDLL(hip.LIB_PATH), "tgtc_style_train_batch")
