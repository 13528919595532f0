"""CPU: the host side of the multi-latent stylised render (K latent sets per ray, shared geometry): exported symbols,
the workspace layout the header documents, argument errors that are returned before a device is touched, CLI options."""
import ctypes
import itertools
import os

from tgtc_style_amd import config as cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tgtc_styled_forward_rays_multi", "tgtc_render_styled_multi_workspace_bytes", "tgtc_render_rays_styled_multi")
ERR_ARG = -1


def test_multi_symbols_exported_and_declared():
    from tgtc_style_amd import hip
    lib = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "tgtc_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in hip.header_symbols(), name
        assert name + "(" in header, name
    assert hip.load().tgtc_render_styled_multi_workspace_bytes.restype is ctypes.c_size_t


def test_multi_workspace_bytes_is_the_documented_layout():
    """Six planes, each rounded up to 256 bytes: ts_c, sigma_c, w_c [R,nc]; ts_f, sigma_f [R,nc+nf]; rgb_f [K,R,nc+nf,3]
    (RenderWorkspace's planes without the coarse colours, the fine colours K times)."""
    from tgtc_style_amd import hip
    f = hip.load().tgtc_render_styled_multi_workspace_bytes

    def up(n_floats):
        return (4 * n_floats + 255) // 256 * 256

    def expected(R, nc, nf, K):
        if R < 0 or nc < 0 or nf < 0 or K < 1:
            return 0
        nt = nc + nf
        return 3 * up(R * nc) + 2 * up(R * nt) + up(K * R * nt * 3)

    Rs, ncs, nfs, Ks = (-1, 0, 1, 7, 64, 2000, 160000), (-1, 0, 3, 64, 100, 128), (-1, 0, 1, 28, 64), (-1, 0, 1, 2, 3, 4, 8)
    for R, nc, nf, K in itertools.product(Rs, ncs, nfs, Ks):
        assert f(R, nc, nf, K) == expected(R, nc, nf, K), (R, nc, nf, K)
    # non-decreasing in each argument
    for R, nc, nf, K in itertools.product(Rs[1:], ncs[1:], nfs[1:], Ks[2:]):
        here = f(R, nc, nf, K)
        assert f(R + 1, nc, nf, K) >= here and f(R, nc + 1, nf, K) >= here and f(R, nc, nf + 1, K) >= here
        assert f(R, nc, nf, K + 1) >= here
    # K = 1 against the single-latent workspace: the same planes minus the coarse colours
    assert f(160000, 128, 64, 1) == hip.load().tgtc_render_workspace_bytes(160000, 128, 64) - up(160000 * 128 * 3)
    # the figure the header quotes: 369 MB of per-sample colour per latent for a 400 x 400 frame at 128 + 64
    assert f(160000, 128, 64, 4) - f(160000, 128, 64, 3) == 160000 * 192 * 3 * 4


def test_multi_calls_reject_bad_arguments_before_touching_a_device():
    from tgtc_style_amd import hip
    lib = hip.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)        # stands for any non-null pointer: the calls must return before they read through it
    # null handles
    assert lib.tgtc_styled_forward_rays_multi(None, None, p, p, p, p, 2, 4, 8, p, p, None) == ERR_ARG
    assert lib.tgtc_render_rays_styled_multi(None, None, None, p, p, p, 2, 4, 64, 64, 0., 1., None, p, 4096, p, p, None) == ERR_ARG
    assert b"render_rays_styled_multi" in lib.tgtc_last_error()
    # K = 0 / negative, also with null handles: still an argument error, never a launch
    for K in (0, -3):
        assert lib.tgtc_styled_forward_rays_multi(None, None, p, p, p, p, K, 4, 8, p, p, None) == ERR_ARG
        assert lib.tgtc_render_rays_styled_multi(None, None, None, p, p, p, K, 4, 64, 64, 0., 1., None, p, 4096, p, p, None) == ERR_ARG


def test_cli_options_of_the_shared_geometry_render():
    base = ["--config", os.path.join(ROOT, "configs", "fern.txt")]
    a = cfg.parse_args(base)
    assert a.share_geometry is False and a.synthetic_styles == 1
    a = cfg.parse_args(base + ["--share_geometry", "--synthetic_styles", "3"])
    assert a.share_geometry is True and a.synthetic_styles == 3
    # the consequence for the jitter is stated in the option's help
    assert "style 0 is rendered with the jitter it has without the flag" in " ".join(cfg.config_parser().format_help().lower().split())
