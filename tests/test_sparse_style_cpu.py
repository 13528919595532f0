"""CPU: the host side of the culled stylised render (style networks only on samples whose compositing weight exceeds a
threshold, tgtc_render_rays_styled_sparse): exported symbols, the workspace layout the header documents, argument errors
that are returned before a device is touched, the --cull_weight option."""
import ctypes
import itertools
import os

from tgtc_style_amd import config as cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tgtc_render_styled_sparse_workspace_bytes", "tgtc_render_rays_styled_sparse")
ERR_ARG = -1
SCRATCH = 8192      # the fixed scratch of the compaction (include/tgtc_hip.h)


def test_sparse_symbols_exported_and_declared():
    from tgtc_style_amd import hip
    lib = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "tgtc_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in hip.header_symbols(), name
        assert name + "(" in header, name
    assert hip.load().tgtc_render_styled_sparse_workspace_bytes.restype is ctypes.c_size_t
    assert hip.missing_symbols() == []


def test_sparse_workspace_bytes_is_the_documented_layout():
    """The six planes of the multi workspace, then w_f float [R,nc+nf], live uint32 [R*(nc+nf)] (each rounded up to 256
    bytes), then 8192 bytes of scratch."""
    from tgtc_style_amd import hip
    f = hip.load().tgtc_render_styled_sparse_workspace_bytes
    multi = hip.load().tgtc_render_styled_multi_workspace_bytes

    def up(n_words):
        return (4 * n_words + 255) // 256 * 256

    def expected(R, nc, nf, K):
        if R < 0 or nc < 0 or nf < 0 or K < 1:
            return 0
        nt = nc + nf
        return 3 * up(R * nc) + 2 * up(R * nt) + up(K * R * nt * 3) + 2 * up(R * nt) + SCRATCH

    Rs, ncs, nfs, Ks = (-1, 0, 1, 7, 64, 2000, 160000), (-1, 0, 3, 64, 100, 128), (-1, 0, 1, 28, 64), (-1, 0, 1, 2, 3, 4, 8)
    for R, nc, nf, K in itertools.product(Rs, ncs, nfs, Ks):
        got = f(R, nc, nf, K)
        assert got == expected(R, nc, nf, K), (R, nc, nf, K)
        if got:     # exactly the two documented planes and the fixed scratch above the multi workspace
            assert got - multi(R, nc, nf, K) == 2 * up(R * (nc + nf)) + SCRATCH, (R, nc, nf, K)
    for R, nc, nf, K in itertools.product(Rs[1:], ncs[1:], nfs[1:], Ks[2:]):
        here = f(R, nc, nf, K)
        assert f(R + 1, nc, nf, K) >= here and f(R, nc + 1, nf, K) >= here and f(R, nc, nf + 1, K) >= here
        assert f(R, nc, nf, K + 1) >= here


def test_sparse_call_rejects_bad_arguments_before_touching_a_device():
    from tgtc_style_amd import hip
    lib = hip.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)        # stands for any non-null pointer: the call must return before it reads through it

    def call(K=2, min_weight=0.):
        return lib.tgtc_render_rays_styled_sparse(None, None, None, p, p, p, K, 4, 64, 64, 0., 1., None, min_weight, p, 4096, p, p,
                                                  p, None)
    assert call() == ERR_ARG and b"render_rays_styled_sparse" in lib.tgtc_last_error()       # null handles
    for K in (0, -3):
        assert call(K=K) == ERR_ARG and b"K >= 1" in lib.tgtc_last_error()
    assert call(min_weight=-1.) == ERR_ARG and b"min_weight" in lib.tgtc_last_error()
    assert call(min_weight=float("nan")) == ERR_ARG and b"min_weight" in lib.tgtc_last_error()


def test_cli_cull_weight():
    base = ["--config", os.path.join(ROOT, "configs", "fern.txt")]
    a = cfg.parse_args(base)
    assert a.cull_weight == -1 and isinstance(a.cull_weight, float)
    a = cfg.parse_args(base + ["--cull_weight", "0"])
    assert a.cull_weight == 0 and isinstance(a.cull_weight, float)
    assert cfg.parse_args(base + ["--cull_weight", "1e-4"]).cull_weight == 1e-4
    text = " ".join(cfg.config_parser().format_help().lower().split())
    assert "0 reproduces the image" in text and "bit for bit" in text
    assert "a positive value bounds the change of each ray by the sum of its dropped weights" in text
