"""CPU: the host side of the stylised list entry points of the fp16x3+fp16mx pair without a plane
(tgtc_styled_forward_list_folded_mx, tgtc_render_rays_styled_sparse_folded_mx, tgtc_restyle_rays_folded_mx; csrc/mlp_list_mx.hip)
and of --style_precision: exported symbols, the argument errors that are returned before a device is touched -- on null handles
and on fake handles (zeroed memory behind the handle's kind and precision, what the checks in front of the first device call
read) --, the flag in the tables of config.py and every incomplete flag combination."""
import ctypes
import os

import pytest

from test_restyle_mx_cpu import fake_handle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tgtc_styled_forward_list_folded_mx", "tgtc_render_rays_styled_sparse_folded_mx", "tgtc_restyle_rays_folded_mx")
SIBLING = {"tgtc_styled_forward_list_folded_mx": "tgtc_styled_forward_list_folded",
           "tgtc_render_rays_styled_sparse_folded_mx": "tgtc_render_rays_styled_sparse_folded",
           "tgtc_restyle_rays_folded_mx": "tgtc_restyle_rays_folded"}
ERR_ARG, ERR_UNSUPPORTED = -1, -2
KIND_NERF, KIND_STYLE = 0, 1
PREC_FP16X3, PREC_FP16, PREC_FP16_FP6 = 0, 1, 2


def test_list_mx_symbols_exported_declared_and_registered():
    from tgtc_style_amd import hip
    lib = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "tgtc_hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    bound = hip.load()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in hip.header_symbols(), name
        assert "int " + name + "(" in header, name
        assert name in integration, name
        assert getattr(bound, name).argtypes == getattr(bound, SIBLING[name]).argtypes      # the sibling's arguments, one for one
    assert hip.missing_symbols() == []


def _handles():
    """(fp16mx NeRF, fp16x3 NeRF, fp16 NeRF, fp16x3 style without mx streams, fp16 style) as addresses, and what keeps them alive."""
    keep = [fake_handle(KIND_NERF, PREC_FP16_FP6), fake_handle(KIND_NERF, PREC_FP16X3), fake_handle(KIND_NERF, PREC_FP16),
            fake_handle(KIND_STYLE, PREC_FP16X3), fake_handle(KIND_STYLE, PREC_FP16)]
    return [ctypes.addressof(h) for h in keep], keep


def test_list_kernel_entry_rejects_bad_arguments_before_touching_a_device():
    from tgtc_style_amd import hip
    lib = hip.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)        # stands for any non-null pointer: the calls must return before they read through it
    err = lambda: lib.tgtc_last_error()
    (mx, x3, fast, style, style16), keep = _handles()

    def fwd(nerf=None, style_=None, K=2, R=4, N=128, ts=p):
        return lib.tgtc_styled_forward_list_folded_mx(nerf, style_, p, p, ts, p, K, R, N, p, p, p, None)
    assert fwd(K=0) == ERR_ARG and b"styled_forward_list_folded_mx: need K >= 1" in err()
    assert fwd(R=-1) == ERR_ARG and fwd(N=0) == ERR_ARG and b"bad argument" in err()
    assert fwd(R=1 << 31) == ERR_UNSUPPORTED and fwd(R=1 << 24) == ERR_UNSUPPORTED and b"2^31" in err()
    assert fwd(R=1 << 23, K=2) == ERR_UNSUPPORTED                                      # only K x R x N passes 2^31
    assert fwd() == ERR_ARG and b"null handle" in err()
    # the range checks come before the handles are looked at; then their kinds, then the precisions
    assert fwd(nerf=x3, style_=style, R=1 << 24) == ERR_UNSUPPORTED and b"2^31" in err()
    assert fwd(nerf=style, style_=style) == ERR_ARG and fwd(nerf=mx, style_=mx) == ERR_ARG and b"style a style handle" in err()
    for nerf in (x3, fast):
        assert fwd(nerf=nerf, style_=style) == ERR_UNSUPPORTED and b"must be in fp16mx" in err()
    assert fwd(nerf=mx, style_=style16) == ERR_UNSUPPORTED and b"no lo halves" in err()
    assert fwd(nerf=mx, style_=style) == ERR_UNSUPPORTED and b"no fp16mx streams" in err()
    assert fwd(nerf=mx, style_=style, R=0) == ERR_UNSUPPORTED                          # a pair without streams is never this entry's
    del keep


def test_render_entry_rejects_bad_arguments_before_touching_a_device():
    from tgtc_style_amd import hip
    lib = hip.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    err = lambda: lib.tgtc_last_error()
    (mx, x3, fast, style, style16), keep = _handles()

    def render(coarse=None, fine=None, style_=None, K=2, R=4, nc=64, nf=64, tau=0.0):
        return lib.tgtc_render_rays_styled_sparse_folded_mx(coarse, fine, style_, p, p, p, K, R, nc, nf, 0.0, 1.0, None, tau, p,
                                                            1 << 40, p, p, p, None)
    assert render(K=0) == ERR_ARG and b"render_rays_styled_sparse_folded_mx: need K >= 1" in err()
    assert render(tau=-1.0) == ERR_ARG and render(tau=float("nan")) == ERR_ARG and b"min_weight" in err()
    assert render(R=-1) == ERR_ARG and b"bad argument" in err()
    assert render(nc=2) == ERR_ARG and render(nf=0) == ERR_ARG and b"n_coarse >= 3" in err()
    assert render(R=1 << 31) == ERR_UNSUPPORTED and render(R=1 << 24) == ERR_UNSUPPORTED and b"2^31" in err()
    assert render(R=1 << 23, K=2) == ERR_UNSUPPORTED and b"2^31" in err()
    assert render() == ERR_ARG and b"null handle" in err()
    assert render(coarse=x3, fine=x3, style_=style, R=1 << 24) == ERR_UNSUPPORTED and b"2^31" in err()
    assert render(coarse=x3, fine=style, style_=style) == ERR_ARG and render(coarse=x3, fine=mx, style_=mx) == ERR_ARG
    for fine in (x3, fast):
        assert render(coarse=x3, fine=fine, style_=style) == ERR_UNSUPPORTED and b"must be in fp16mx" in err()
    assert render(coarse=x3, fine=mx, style_=style16) == ERR_UNSUPPORTED and b"no lo halves" in err()
    assert render(coarse=x3, fine=mx, style_=style) == ERR_UNSUPPORTED and b"no fp16mx streams" in err()
    del keep


def test_restyle_entry_rejects_bad_arguments_before_touching_a_device():
    from tgtc_style_amd import hip
    lib = hip.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    err = lambda: lib.tgtc_last_error()
    (mx, x3, fast, style, style16), keep = _handles()

    def restyle(fine=None, style_=None, K=2, R=4, nc=64, nf=64, count=10):
        return lib.tgtc_restyle_rays_folded_mx(fine, style_, p, p, p, K, R, nc, nf, p, 1 << 40, count, p, 1 << 40, p, p, None)
    assert restyle(K=0) == ERR_ARG and b"restyle_rays_folded_mx: need K >= 1" in err()
    assert restyle(R=-1) == ERR_ARG and restyle(count=-1) == ERR_ARG and b"bad argument" in err()
    assert restyle(nc=2) == ERR_ARG and restyle(nf=0) == ERR_ARG and b"n_fine >= 1" in err()
    assert restyle(R=1 << 24) == ERR_UNSUPPORTED and b"2^31" in err()                  # R x N >= 2^31
    assert restyle(count=4 * 128 + 1) == ERR_ARG and b"exceeds" in err()               # count > R x N
    assert restyle(R=1 << 22, count=1 << 28, K=8) == ERR_UNSUPPORTED and b"K x count" in err()
    assert restyle(R=1 << 22, count=1, K=512) == ERR_UNSUPPORTED and b"K x count" in err()    # K x R
    assert restyle() == ERR_ARG and b"null handle" in err()
    assert restyle(fine=x3, style_=style, R=1 << 24) == ERR_UNSUPPORTED and b"2^31" in err()
    assert restyle(fine=style, style_=style) == ERR_ARG and restyle(fine=mx, style_=mx) == ERR_ARG and b"style a style handle" in err()
    for fine in (x3, fast):
        assert restyle(fine=fine, style_=style) == ERR_UNSUPPORTED and b"must be in fp16mx" in err()
    assert restyle(fine=mx, style_=style16) == ERR_UNSUPPORTED and b"no lo halves" in err()
    assert restyle(fine=mx, style_=style) == ERR_UNSUPPORTED and b"no fp16mx streams" in err()
    # the siblings keep refusing the mixed pair as they did
    assert lib.tgtc_restyle_rays_folded(mx, style, p, p, p, 2, 4, 64, 64, p, 1 << 40, 10, p, 1 << 40, p, p, None) == ERR_ARG
    assert b"different precisions" in err()
    assert lib.tgtc_styled_forward_list_folded(mx, style, p, p, p, p, 2, 4, 128, p, p, p, None) == ERR_ARG
    assert lib.tgtc_render_rays_styled_sparse_folded(x3, mx, style, p, p, p, 2, 4, 64, 64, 0.0, 1.0, None, 0.0, p, 1 << 40, p, p, p,
                                                     None) == ERR_ARG
    del keep


def test_style_precision_flag_is_in_the_tables():
    from tgtc_style_amd import config
    assert config.EXTRA["style_precision"] == (str, "") and "fp16mx" in config.HELP["style_precision"]
    assert config.parse_args(["--expname", "x"]).style_precision == ""
    assert config.parse_args(["--expname", "x", "--style_precision", "fp16mx"]).style_precision == "fp16mx"


FULL = ["--expname", "x", "--synthetic", "--render_valid_style", "--share_geometry", "--fold_latents", "--cull_weight", "0",
        "--precision", "fp16x3+fp16mx", "--style_precision", "fp16mx"]


def _without(argv, flag, values=0):
    i = argv.index(flag)
    return argv[:i] + argv[i + 1 + values:]


@pytest.mark.parametrize("argv,words", [
    (_without(FULL, "--render_valid_style"), "--fold_latents needs"),           # the older check of --fold_latents comes first
    (_without(FULL, "--share_geometry"), "--fold_latents needs"),
    (_without(FULL, "--fold_latents"), "--style_precision needs --render_valid_style --share_geometry --fold_latents"),
    (_without(_without(FULL, "--fold_latents"), "--share_geometry"), "--style_precision needs"),
    (_without(FULL, "--cull_weight", 1), "--cull_weight >= 0 or --geometry_cache"),
    (_without(FULL, "--cull_weight", 1) + ["--cull_weight", "-1"], "--cull_weight >= 0 or --geometry_cache"),
    (_without(FULL, "--precision", 1), "fine half is fp16mx"),
    (_without(FULL, "--precision", 1) + ["--precision", "fp16x3"], "fine half is fp16mx"),
    (_without(FULL, "--precision", 1) + ["--precision", "fp16mx+fp16x3"], "fine half is fp16mx"),
    (_without(FULL, "--precision", 1) + ["--precision", "fp16"], "fine half is fp16mx"),
    (FULL[:-1] + ["fp16x3"], "--style_precision takes fp16mx"),
])
def test_incomplete_flag_combinations_exit(argv, words):
    from tgtc_style_amd import train_tgtcs
    with pytest.raises(SystemExit) as e:
        train_tgtcs.main(argv)
    assert words in str(e.value), e.value
