"""CPU: the host side of the two-phase fine pass of the plain render -- the new entry points are declared with the stated
signatures, exported and bound, and the workspace of the plain render is the seven planes it always was."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLARATIONS = {
    "tgtc_nerf_forward_list": ("int", "const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts, int64_t R, int N, "
                                      "const uint32_t* live, const uint32_t* n_live, float* rgb, void* stream"),
    "tgtc_net_set_cull": ("int", "tgtc_net* net, int mode"),
    "tgtc_net_live_fraction": ("float", "const tgtc_net* net"),
    "tgtc_net_culled_renders": ("long long", "const tgtc_net* net"),
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
    for macro, value in (("TGTC_CULL_AUTO", 0), ("TGTC_CULL_OFF", 1), ("TGTC_CULL_ON", 2)):
        assert re.search(r"^#define %s %d$" % (macro, value), text, re.M), macro
    assert (hip.CULL_AUTO, hip.CULL_OFF, hip.CULL_ON) == (0, 1, 2)
    bound = hip.load()
    assert bound.tgtc_net_live_fraction.restype is ctypes.c_float and bound.tgtc_net_culled_renders.restype is ctypes.c_longlong
    # no handle: pure host answers, no device touched
    assert bound.tgtc_net_live_fraction(None) == -1.0 and bound.tgtc_net_culled_renders(None) == -1
    assert bound.tgtc_net_set_cull(None, hip.CULL_ON) == -1
    assert bound.tgtc_nerf_forward_list(None, None, None, None, 1, 1, None, None, None, None) == -1
    # the paths are what they were: the two-phase pass is no path of its own
    assert (hip.PATH_AUTO, hip.PATH_RAY_KERNEL, hip.PATH_CHAIN) == (0, 1, 2)
    assert bound.tgtc_render_path(3, 0, 2, -1, 128, 64, 0) == -1


@pytest.mark.parametrize("R,nc,nf", [(160000, 128, 64), (37, 64, 64), (40, 3, 32)])
def test_plain_workspace_is_the_seven_planes(R, nc, nf):
    from tgtc_style_amd import hip
    up = lambda floats: (4 * floats + 255) // 256 * 256
    nt = nc + nf
    planes = [R * nc, R * nc, R * nc * 3, R * nc, R * nt, R * nt, R * nt * 3]    # ts_c sigma_c rgb_c w_c ts_f sigma_f rgb_f
    assert hip.load().tgtc_render_workspace_bytes(R, nc, nf) == sum(up(p) for p in planes)


def test_renderer_takes_cull_and_rejects_anything_else():
    from tgtc_style_amd import rendering
    for cull in (None, True, False):
        assert rendering.RayRenderer(None, None, cull=cull).cull is cull
    with pytest.raises(ValueError):
        rendering.RayRenderer(None, None, cull="auto")
