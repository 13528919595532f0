"""CPU: the host side of frame-constant latents folded into per-latent biases (tgtc_style_folded_bytes, tgtc_style_fold_latents,
tgtc_styled_forward_list_folded, tgtc_render_rays_styled_sparse_folded, tgtc_restyle_rays_folded and their size functions):
exported symbols, the size functions against their unfolded siblings, argument errors that are returned before a device is
touched, the --fold_latents option, the 2-D zs rule of RayRenderer.render_latents."""
import ctypes
import itertools
import os

import pytest
import torch

from tgtc_style_amd import config as cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tgtc_style_folded_bytes", "tgtc_style_fold_latents", "tgtc_styled_forward_list_folded",
         "tgtc_render_styled_sparse_folded_workspace_bytes", "tgtc_render_rays_styled_sparse_folded",
         "tgtc_restyle_folded_workspace_bytes", "tgtc_restyle_rays_folded")
SIZE_NAMES = ("tgtc_style_folded_bytes", "tgtc_render_styled_sparse_folded_workspace_bytes", "tgtc_restyle_folded_workspace_bytes")
ERR_ARG, ERR_UNSUPPORTED = -1, -2
TABLE = 16384        # kStylePairBiasBytes: one pair bias table


def up(nbytes):
    return (nbytes + 255) // 256 * 256


def test_fold_symbols_exported_declared_and_bound():
    from tgtc_style_amd import hip
    lib = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "tgtc_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in hip.header_symbols(), name
        assert name + "(" in header, name
        assert getattr(hip.load(), name).argtypes is not None, name
    for name in SIZE_NAMES:
        assert getattr(hip.load(), name).restype is ctypes.c_size_t, name
    assert hip.missing_symbols() == []


def test_folded_bytes_is_one_table_per_latent():
    from tgtc_style_amd import hip
    lib = hip.load()
    for K in (-3, -1, 0):
        assert lib.tgtc_style_folded_bytes(K) == 0, K
    for K in (1, 2, 3, 4, 120, 1 << 16):
        assert lib.tgtc_style_folded_bytes(K) == TABLE * K, K


def test_workspaces_are_the_siblings_plus_the_tables():
    """Each folded workspace is its unfolded sibling's followed by one more plane: 16384 K bytes rounded up to 256.  Where the
    sibling returns 0 (negative arguments, K < 1) so does the folded one.  The grids are those of tests/test_restyle_cpu.py."""
    from tgtc_style_amd import hip
    lib = hip.load()
    Ks = (-1, 0, 1, 2, 3, 4)
    for count, K in itertools.product((-1, 0, 1, 21, 22, 5703, 3041280, (1 << 29)), Ks):
        sib = lib.tgtc_restyle_workspace_bytes(count, K)
        want = 0 if count < 0 or K < 1 else sib + up(TABLE * K)
        assert lib.tgtc_restyle_folded_workspace_bytes(count, K) == want, (count, K)
    for R, K, (nc, nf) in itertools.product((-1, 0, 1, 63, 64, 300, 160000, 1 << 24), Ks, ((128, 64), (64, 64), (100, 28), (-1, 64))):
        sib = lib.tgtc_render_styled_sparse_workspace_bytes(R, nc, nf, K)
        want = 0 if R < 0 or nc < 0 or K < 1 else sib + up(TABLE * K)
        assert (sib == 0) == (want == 0)
        assert lib.tgtc_render_styled_sparse_folded_workspace_bytes(R, nc, nf, K) == want, (R, nc, nf, K)


def test_calls_reject_bad_arguments_before_touching_a_device():
    """Null handles stand for handles here (no device): the calls must return before they read through any pointer.  Handle
    kinds, precisions and buffer sizes are checked on the device in tests/test_fold_latents_gpu.py."""
    from tgtc_style_amd import hip
    lib = hip.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    err = lambda: lib.tgtc_last_error()

    def fold(K=2):
        return lib.tgtc_style_fold_latents(None, p, K, p, 1 << 40, None)
    assert fold() == ERR_ARG and b"style_fold_latents" in err()                      # null handle
    for K in (0, -3):
        assert fold(K=K) == ERR_ARG and b"K >= 1" in err()

    def flist(K=2, R=4, N=128):
        return lib.tgtc_styled_forward_list_folded(None, None, p, p, p, p, K, R, N, p, p, p, None)
    assert flist() == ERR_ARG and b"styled_forward_list_folded" in err()             # null handles
    for K in (0, -3):
        assert flist(K=K) == ERR_ARG and b"K >= 1" in err()
    assert flist(R=-1) == ERR_ARG and flist(N=0) == ERR_ARG
    assert flist(R=1 << 24) == ERR_UNSUPPORTED and b"2^31" in err()                  # R x N >= 2^31
    assert flist(K=1 << 20, R=1 << 4) == ERR_UNSUPPORTED and b"2^31" in err()        # K x R x N >= 2^31

    def render(K=2, R=4, nc=64, nf=64, min_weight=0.):
        return lib.tgtc_render_rays_styled_sparse_folded(None, None, None, p, p, p, K, R, nc, nf, 0., 1., None, min_weight, p,
                                                         1 << 40, p, p, None, None)
    assert render() == ERR_ARG and b"render_rays_styled_sparse_folded" in err()      # null handles
    for K in (0, -3):
        assert render(K=K) == ERR_ARG and b"K >= 1" in err()
    assert render(R=-1) == ERR_ARG
    assert render(min_weight=-1e-6) == ERR_ARG and b"min_weight" in err()
    assert render(min_weight=float("nan")) == ERR_ARG and b"min_weight" in err()
    assert render(nc=2) == ERR_ARG and render(nf=0) == ERR_ARG and b"n_fine >= 1" in err()
    assert render(R=1 << 24) == ERR_UNSUPPORTED and b"2^31" in err()                 # R x N >= 2^31
    assert render(K=1 << 20, R=1 << 4) == ERR_UNSUPPORTED and b"2^31" in err()       # K x R x N >= 2^31

    def restyle(K=2, R=4, count=10, nc=64, nf=64):
        return lib.tgtc_restyle_rays_folded(None, None, p, p, p, K, R, nc, nf, p, 1 << 40, count, p, 1 << 40, p, p, None)
    assert restyle() == ERR_ARG and b"restyle_rays_folded" in err()                  # null handles
    for K in (0, -3):
        assert restyle(K=K) == ERR_ARG and b"K >= 1" in err()
    assert restyle(R=-1) == ERR_ARG and restyle(count=-1) == ERR_ARG
    assert restyle(nc=2) == ERR_ARG and restyle(nf=0) == ERR_ARG
    assert restyle(count=4 * 128 + 1) == ERR_ARG and b"exceeds" in err()             # count > R x N
    assert restyle(R=1 << 24) == ERR_UNSUPPORTED and b"2^31" in err()                # R x N >= 2^31
    assert restyle(K=1 << 20, R=1 << 10, count=1 << 11) == ERR_UNSUPPORTED and b"2^31" in err()     # K x count >= 2^31


def test_cli_fold_latents_is_refused_without_its_companions(tmp_path):
    from tgtc_style_amd import train_tgtcs
    base = ["--config", os.path.join(ROOT, "configs", "fern.txt")]
    assert cfg.parse_args(base).fold_latents is False
    assert cfg.parse_args(base + ["--fold_latents"]).fold_latents is True
    assert "fold_latents" in cfg.EXTRA and "fold_latents" in cfg.HELP
    run = base + ["--synthetic", "--render_valid_style", "--basedir", str(tmp_path), "--fold_latents"]
    with pytest.raises(SystemExit) as e:
        train_tgtcs.main(run + ["--cull_weight", "0"])                               # no --share_geometry
    assert "--fold_latents needs --render_valid_style --share_geometry" in str(e.value)
    with pytest.raises(SystemExit) as e:
        train_tgtcs.main(run + ["--share_geometry"])                                 # neither a cull weight nor a cache
    assert "--fold_latents needs --cull_weight >= 0 or --geometry_cache" in str(e.value)
    with pytest.raises(SystemExit) as e:
        train_tgtcs.main(run + ["--share_geometry", "--cull_weight", "-1"])
    assert "--fold_latents needs --cull_weight >= 0 or --geometry_cache" in str(e.value)
    with pytest.raises(SystemExit) as e:                                             # not a stylised validation render
        train_tgtcs.main(base + ["--synthetic", "--render_valid", "--basedir", str(tmp_path), "--fold_latents", "--share_geometry",
                                 "--cull_weight", "0"])
    assert "--fold_latents needs --render_valid_style" in str(e.value)
    assert os.listdir(str(tmp_path)) == []
    text = " ".join(cfg.config_parser().format_help().lower().split())
    assert "--fold_latents" in text and "one latent per (style, frame)" in text


def test_drivers_refuse_fold_latents_without_share_geometry_or_threshold():
    from tgtc_style_amd import rendering

    class Latents:
        sigma_scale = 0.

    class DS:
        mode = None

        def frame_batches(self, n):
            return iter(())

    class Loader:
        dataset = DS()
        batch_size = 1

    class A:
        N_samples, N_samples_fine = 64, 64
    with pytest.raises(ValueError, match="share_geometry"):
        rendering.render_style(None, None, None, None, Latents(), Loader(), A(), "cpu", fold_latents=True)
    with pytest.raises(ValueError, match="min_weight or a geometry_cache"):
        rendering._render_style_shared(Latents(), Loader(), A(), "cpu", None, object(), fold_latents=True)


def test_two_dimensional_zs_needs_a_min_weight():
    """zs [K,32] with min_weight=None would be the dense multi-latent kernel, which has no folded form: a ValueError, raised
    before anything else is looked at (no GPU here)."""
    from tgtc_style_amd import rendering
    r = rendering.RayRenderer(None, None, object())
    ro = torch.zeros(4, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="min_weight"):
        r.render_latents(ro, ro, 64, 64, zs=torch.zeros(2, 32))
    with pytest.raises(ValueError, match="min_weight"):
        r.render_latents(ro, ro, 64, 64, zs=torch.zeros(2, 32), min_weight=None)
