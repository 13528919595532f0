"""CPU: the host side of the density screen of the plain render ("The screen") -- the new entry points are declared
with the stated signatures, exported and bound; null handles get the answers that touch no device; the workspace-fit rule and
AUTO's decision are what the header says, as pure host functions."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_LIST = ("const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts, int64_t R, int N, "
         "const uint32_t* live, const uint32_t* n_live, ")
DECLARATIONS = {
    "tgtc_net_enable_screen": ("int", "tgtc_net* net, void* stream"),
    "tgtc_net_screen_margin": ("float", "const tgtc_net* net"),
    "tgtc_net_set_screen": ("int", "tgtc_net* net, int mode"),
    "tgtc_net_screen_fraction": ("float", "const tgtc_net* net"),
    "tgtc_net_screened_renders": ("long long", "const tgtc_net* net"),
    "tgtc_screen_list_fits": ("int", "size_t bytes, int64_t M"),
    "tgtc_screen_auto_decision": ("int", "int pass, uint32_t candidates, uint32_t total"),
    "tgtc_nerf_screen_rays": ("int", "const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts, int64_t R, "
                                     "int N, float* sigma, void* stream"),
    "tgtc_nerf_sigma_list": ("int", _LIST + "float* sigma, void* stream"),
    "tgtc_nerf_forward_list_sigma": ("int", _LIST + "float* rgb, float* sigma, void* stream"),
}


def test_header_declares_the_new_calls_and_the_library_exports_them():
    from tgtc_style_amd import hip
    text = open(os.path.join(ROOT, "include", "tgtc_hip.h")).read()
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name, (ret, args) in DECLARATIONS.items():
        m = re.search(r"^([a-z ]+?)\s+%s\(([^)]*)\);" % name, text, re.M)
        assert m, name
        assert m.group(1) == ret and " ".join(m.group(2).split()) == args, (name, m.groups())
        assert hasattr(lib, name), name
        assert len(hip._SIGNATURES[name]) == len(args.split(",")), name
    for macro, value in (("TGTC_SCREEN_AUTO", 0), ("TGTC_SCREEN_OFF", 1), ("TGTC_SCREEN_ON", 2)):
        assert re.search(r"^#define %s %d$" % (macro, value), text, re.M), macro
    assert (hip.SCREEN_AUTO, hip.SCREEN_OFF, hip.SCREEN_ON) == (0, 1, 2)
    bound = hip.load()
    assert bound.tgtc_net_screen_margin.restype is ctypes.c_float and bound.tgtc_net_screen_fraction.restype is ctypes.c_float
    assert bound.tgtc_net_screened_renders.restype is ctypes.c_longlong
    # no handle: pure host answers, no device touched
    assert bound.tgtc_net_screen_margin(None) == -1.0 and bound.tgtc_net_screen_fraction(None) == -1.0
    assert bound.tgtc_net_screened_renders(None) == -1
    assert bound.tgtc_net_enable_screen(None, None) == -1 and bound.tgtc_net_set_screen(None, hip.SCREEN_ON) == -1
    assert bound.tgtc_nerf_screen_rays(None, None, None, None, 1, 1, None, None) == -1
    assert bound.tgtc_nerf_sigma_list(None, None, None, None, 1, 1, None, None, None, None) == -1
    assert bound.tgtc_nerf_forward_list_sigma(None, None, None, None, 1, 1, None, None, None, None, None) == -1
    # the earlier list entry keeps its arguments: the density is one more entry, not one more argument
    assert len(hip._SIGNATURES["tgtc_nerf_forward_list"]) == 10


@pytest.mark.parametrize("R,nc,nf", [(160000, 128, 64), (4097, 64, 32), (130, 128, 64), (5, 16, 8), (1, 128, 64), (40, 3, 32)])
def test_the_lists_fit_where_the_header_says(R, nc, nf):
    """coarse: list + 8192 bytes of scratch in the fine colour plane; fine: in the four dead coarse planes, the rule of the
    two-phase pass; the workspace is the seven planes it always was"""
    from tgtc_style_amd import hip
    lib = hip.load()
    up = lambda b: (b + 255) // 256 * 256
    nt = nc + nf
    assert lib.tgtc_render_workspace_bytes(R, nc, nf) == sum(up(4 * p) for p in (R * nc, R * nc, R * nc * 3, R * nc, R * nt, R * nt, R * nt * 3))
    rgb_f = R * nt * 12
    dead = 3 * up(R * nc * 4) + up(R * nc * 12)
    assert bool(lib.tgtc_screen_list_fits(rgb_f, R * nc)) == (rgb_f >= R * nc * 4 + 8192)
    assert bool(lib.tgtc_screen_list_fits(dead, R * nt)) == (dead >= R * nt * 4 + 8192)
    if (R, nc, nf) == (160000, 128, 64):
        assert lib.tgtc_screen_list_fits(rgb_f, R * nc) and lib.tgtc_screen_list_fits(dead, R * nt)
    if R <= 5:
        assert not lib.tgtc_screen_list_fits(rgb_f, R * nc) and not lib.tgtc_screen_list_fits(dead, R * nt)


def test_list_fit_edges():
    from tgtc_style_amd import hip
    fits = hip.load().tgtc_screen_list_fits
    assert fits(8192, 0) and not fits(8191, 0)
    assert fits(4 * 1000 + 8192, 1000) and not fits(4 * 1000 + 8191, 1000)
    assert not fits(1 << 40, -1) and not fits(1 << 40, 1 << 31) and fits(1 << 40, (1 << 31) - 1)     # 32-bit sample indices


def test_auto_decision():
    """nothing landed, or a word that is no (count, total) pair: dense; otherwise screen iff the share is below the
    threshold of the pass -- a threshold of 0 means that pass's AUTO never screens"""
    from tgtc_style_amd import hip
    decide = hip.load().tgtc_screen_auto_decision
    total = 1 << 20
    for p in (0, 1):
        assert decide(p, 0, 0) == 0 and decide(p, 5, 0) == 0          # nothing landed
        assert decide(p, total + 1, total) == 0                      # not a pair
        assert decide(p, total, total) == 0                          # every sample a candidate
        grid = [decide(p, int(s * total), total) for s in [i / 200 for i in range(201)]]
        assert grid == sorted(grid, reverse=True)                    # one threshold: screens below it, never above
        assert decide(p, 0, total) == grid[0]
    # the orbit of the benchmark (candidate shares 0.26 .. 0.34 coarse, 0.11 .. 0.14 fine) against the measured thresholds
    assert (decide(0, int(0.34 * total), total), decide(1, int(0.145 * total), total)) == AUTO_SCREENS_THE_ORBIT


AUTO_SCREENS_THE_ORBIT = (1, 1)


def test_renderer_takes_screen_and_rejects_anything_else():
    from tgtc_style_amd import rendering
    for screen in (None, True, False, (True, False), (None, True)):
        assert rendering.RayRenderer(None, None, screen=screen).screen == screen
    for bad in ("auto", 1.5, (True,), (True, False, None), (True, "x")):
        with pytest.raises(ValueError):
            rendering.RayRenderer(None, None, screen=bad)
