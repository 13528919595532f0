"""CPU: the host side of the chain geometry (tgtc_nerf_sigma_list_mx, tgtc_geometry_build_chain,
tgtc_render_rays_styled_sparse_chain; RayRenderer(..., geometry="chain"); --chain_geometry): the declarations, exports and
bindings, the argument errors that are returned before a device is touched, AUTO's rule for pass 2, the ValueErrors of the
renderer, the refusals of the command line, and the workspace sizes, which do not change."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED = -1, -2

_LIST = ("const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts, int64_t R, int N, "
         "const uint32_t* live, const uint32_t* n_live, ")
_BUILD = ("const tgtc_net* coarse, const tgtc_net* fine, const double* rays_o, const double* rays_d, int64_t R, int n_coarse, "
          "int n_fine, float near_, float far_, const float* jitter, float min_weight, void* workspace, size_t workspace_bytes, "
          "float* t_fine, uint32_t* live_count, void* stream")
_RENDER = ("const tgtc_net* coarse, const tgtc_net* fine, const tgtc_net* style, const double* rays_o, const double* rays_d, "
           "const float* z, int K, int64_t R, int n_coarse, int n_fine, float near_, float far_, const float* jitter, "
           "float min_weight, void* workspace, size_t workspace_bytes, float* rgb_fine, float* t_fine, uint32_t* live_count, "
           "void* stream")
DECLARATIONS = {
    "tgtc_nerf_sigma_list_mx": _LIST + "float* sigma, void* stream",
    "tgtc_geometry_build_chain": _BUILD,
    "tgtc_render_rays_styled_sparse_chain": "int form, " + _RENDER,
}
SIBLING = {"tgtc_nerf_sigma_list_mx": ("tgtc_nerf_sigma_list", 0), "tgtc_geometry_build_chain": ("tgtc_geometry_build", 0),
           "tgtc_render_rays_styled_sparse_chain": ("tgtc_render_rays_styled_sparse", 1)}


def _declared(text, name):
    m = re.search(r"^int\s+%s\(([^)]*)\);" % name, text, re.M)
    assert m, name
    return " ".join(m.group(1).split())


def test_header_declares_the_new_calls_and_the_library_exports_and_binds_them():
    from tgtc_style_amd import hip
    text = open(os.path.join(ROOT, "include", "tgtc_hip.h")).read()
    lib = ctypes.CDLL(hip.LIB_PATH)
    bound = hip.load()
    for name, args in DECLARATIONS.items():
        assert _declared(text, name) == args, name
        assert hasattr(lib, name) and name in hip._SIGNATURES and name in hip.header_symbols(), name
        arity = len(args.split(","))
        assert len(getattr(bound, name).argtypes) == arity, name
        sibling, extra = SIBLING[name]
        assert _declared(text, sibling) == (args.split(", ", 1)[1] if extra else args), name       # `form` in front, nothing else
        assert list(getattr(bound, name).argtypes)[extra:] == list(getattr(bound, sibling).argtypes), name
    assert bound.tgtc_render_rays_styled_sparse_chain.argtypes[0] is ctypes.c_int
    assert hip.missing_symbols() == []


def test_null_handles_and_a_bad_form_return_before_a_device_is_touched():
    from tgtc_style_amd import hip
    lib = hip.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)        # stands for any non-null pointer: the calls must return before they read through it
    err = lambda: lib.tgtc_last_error()
    assert lib.tgtc_nerf_sigma_list_mx(None, p, p, p, 4, 16, p, p, p, None) == ERR_ARG and b"nerf_sigma_list_mx" in err()
    assert lib.tgtc_geometry_build_chain(None, None, p, p, 4, 64, 64, 0.0, 1.0, None, 0.0, p, 1 << 40, p, p, None) == ERR_ARG
    assert b"geometry_build_chain: bad argument" in err()
    assert lib.tgtc_geometry_build_chain(None, None, p, p, 4, 64, 64, 0.0, 1.0, None, -1.0, p, 1 << 40, p, p, None) == ERR_ARG
    assert b"geometry_build_chain: min_weight" in err()
    assert lib.tgtc_geometry_build(None, None, p, p, 4, 64, 64, 0.0, 1.0, None, 0.0, p, 1 << 40, p, p, None) == ERR_ARG
    assert b"geometry_build: bad argument" in err()                      # the sibling's messages keep its name

    def render(form, K=2, R=4, nc=64, nf=64, tau=0.0):
        return lib.tgtc_render_rays_styled_sparse_chain(form, None, None, None, p, p, p, K, R, nc, nf, 0.0, 1.0, None, tau, p, 1 << 40,
                                                        p, p, p, None)
    for form in (0, 1, 2):
        assert render(form) == ERR_ARG and b"render_rays_styled_sparse_chain: null handle" in err()
        assert render(form, K=0) == ERR_ARG and b"need K >= 1" in err()
        assert render(form, tau=-1.0) == ERR_ARG and b"min_weight" in err()
        assert render(form, nc=2) == ERR_ARG and b"n_coarse >= 3" in err()
        assert render(form, R=1 << 24) == ERR_UNSUPPORTED and b"2^31" in err()
    for form in (3, -1, 8):
        assert render(form) == ERR_ARG and b"form is 0" in err()


def test_auto_decision_of_the_sigma_only_fine_pass():
    """pass 2 has ONE threshold -- it screens below it and never above --, and passes 0 and 1 decide what they decided"""
    from tgtc_style_amd import hip
    decide = hip.load().tgtc_screen_auto_decision
    total = 1 << 20
    assert decide(2, 0, 0) == 0 and decide(2, 5, 0) == 0                # nothing landed
    assert decide(2, total + 1, total) == 0                            # not a pair
    assert decide(2, total, total) == 0                                # every sample a candidate
    cands = [int(i / 200 * total) for i in range(201)]
    grids = {p: [decide(p, c, total) for c in cands] for p in (0, 1, 2)}
    for p, grid in grids.items():
        assert grid == sorted(grid, reverse=True), p
    # the thresholds of passes 0 and 1 on this grid: the float32 constants 0.56 and 0.45 of csrc/render.hip, as before this pass existed
    for p, thr in ((0, 0.56), (1, 0.45)):
        assert grids[p] == [int(c < float(np.float32(thr)) * total) for c in cands], p
    assert (sum(grids[2]) > 0) == AUTO_SCREENS_PASS_2


# whether AUTO ever screens pass 2: the measured threshold of csrc/render.hip (kScreenFineSigmaThreshold) is above 0
AUTO_SCREENS_PASS_2 = True


def test_renderer_rejects_a_bad_geometry_before_any_gpu_call():
    from tgtc_style_amd import rendering
    r = rendering.RayRenderer(None, None, None)
    ro = rd = torch.zeros(4, 3, dtype=torch.float64)
    z = torch.zeros(2, 32)
    with pytest.raises(ValueError, match="geometry is None or 'chain'"):
        r.build_geometry(ro, rd, 64, 64, geometry="x")
    with pytest.raises(ValueError, match="geometry is None or 'chain'"):
        r.render_latents(ro, rd, 64, 64, zs=z, min_weight=0., geometry="x")
    with pytest.raises(ValueError, match="geometry is None or 'chain'"):
        r.render(ro, rd, 64, 64, z=z[0], min_weight=0., geometry="ray")
    with pytest.raises(ValueError, match="needs a min_weight"):
        r.render_latents(ro, rd, 64, 64, zs=z, geometry="chain")
    with pytest.raises(ValueError, match="needs a min_weight"):
        r.render(ro, rd, 64, 64, z=z[0], geometry="chain")


def test_chain_geometry_flag_is_in_the_tables():
    from tgtc_style_amd import config
    assert config.EXTRA["chain_geometry"] == (None, False) and "geometry=chain" in config.HELP["chain_geometry"]
    assert config.parse_args(["--expname", "x"]).chain_geometry is False
    assert config.parse_args(["--expname", "x", "--chain_geometry"]).chain_geometry is True


FULL = ["--expname", "x", "--synthetic", "--render_valid_style", "--share_geometry", "--cull_weight", "0", "--chain_geometry"]


def _without(argv, flag, values=0):
    i = argv.index(flag)
    return argv[:i] + argv[i + 1 + values:]


@pytest.mark.parametrize("argv,words", [
    (_without(FULL, "--render_valid_style"), "--chain_geometry needs --render_valid_style --share_geometry"),
    (_without(FULL, "--render_valid_style") + ["--render_train_style"], "--chain_geometry needs --render_valid_style --share_geometry"),
    (_without(FULL, "--share_geometry"), "--chain_geometry needs --render_valid_style --share_geometry"),
    (_without(FULL, "--cull_weight", 1), "--chain_geometry needs --cull_weight >= 0 or --geometry_cache"),
    (_without(FULL, "--cull_weight", 1) + ["--cull_weight", "-1"], "--chain_geometry needs --cull_weight >= 0 or --geometry_cache"),
    (_without(FULL, "--share_geometry") + ["--geometry_cache", "d"], "--geometry_cache needs --share_geometry"),     # the older check first
])
def test_chain_geometry_refusals(argv, words):
    from tgtc_style_amd import train_tgtcs
    with pytest.raises(SystemExit) as e:
        train_tgtcs.main(argv)
    assert words in str(e.value), e.value


def test_render_style_rejects_a_chain_geometry_it_cannot_have():
    from tgtc_style_amd import rendering

    class A:
        N_samples, N_samples_fine = 64, 64

    class L:
        sigma_scale = 0.
    with pytest.raises(ValueError, match="geometry needs share_geometry"):
        rendering.render_style(None, None, None, None, L(), None, A, "cpu", geometry="chain")


def _up(n):
    return (n + 255) // 256 * 256


def _sparse_bytes(R, nc, nf, K):
    """the sparse workspace by the layout include/tgtc_hip.h documents: what the size function returned before this geometry"""
    nt = nc + nf
    return 3 * _up(4 * R * nc) + 2 * _up(4 * R * nt) + _up(12 * K * R * nt) + 2 * _up(4 * R * nt) + 8192


@pytest.mark.parametrize("R,nc,nf,K", [(1, 128, 64, 1), (5, 16, 8, 2), (130, 64, 32, 2), (4097, 128, 64, 4), (160000, 128, 64, 1)])
def test_workspace_sizes_are_what_they_were(R, nc, nf, K):
    from tgtc_style_amd import hip
    lib = hip.load()
    assert lib.tgtc_render_styled_sparse_workspace_bytes(R, nc, nf, K) == _sparse_bytes(R, nc, nf, K)
    folded = lib.tgtc_render_styled_sparse_folded_workspace_bytes(R, nc, nf, K)
    assert folded == _sparse_bytes(R, nc, nf, K) + _up(lib.tgtc_style_folded_bytes(K))
