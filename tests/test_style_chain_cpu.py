"""CPU: the host side of the style trainer (include/tgtc_train.h "Style trainer") -- the five entry
points are exported, declared and bound, the workspace holds the twelve activation planes, bad arguments are refused
before the GPU is looked at, `--style_chain` parses and its refused combinations say which flag they refuse.  The kernels
run in tests/test_style_chain_gpu.py."""
import ctypes
import os
import re

import pytest

from tgtc_style_amd import config as cfg

from origin_train_cases import FERN, ROOT

SYMBOLS = ["tgtc_style_trainer_create", "tgtc_style_trainer_destroy", "tgtc_style_trainer_workspace_bytes",
           "tgtc_style_trainer_forward", "tgtc_style_trainer_backward"]


def test_the_entry_points_are_exported_and_declared():
    from tgtc_style_amd import fused_train, hip
    lib = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "tgtc_train.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in fused_train.SIGNATURES and name in hip.header_symbols()
    assert hip.missing_symbols() == []


def test_the_workspace_holds_the_twelve_planes():
    from tgtc_style_amd import hip, style_chain   # noqa: F401  (fused_train, through style_chain, registers the signatures)
    lib = hip.load()
    for R, n in ((1, 1), (5, 7), (100, 7), (9, 128), (256, 128)):
        need = int(lib.tgtc_style_trainer_workspace_bytes(R, n))
        M = R * n
        assert need >= 12 * M * 256 * 4 + M * 3 * 4, (R, n, need)
        assert need <= 19 * 1024 * M + (12 << 20), (R, n, need)           # the header's figure: 19 KB per sample + 12 MB
    # R * n <= 65 535 x 32 (the header says why); a refused shape has no workspace
    for R, n in ((0, 7), (-1, 7), (5, 0), (5, -3), (2 ** 31, 1), (2 ** 20, 2 ** 11), (65536, 32), (65535 * 32 + 1, 1), (16384, 128)):
        assert int(lib.tgtc_style_trainer_workspace_bytes(R, n)) == 0
    assert int(lib.tgtc_style_trainer_workspace_bytes(65535, 32)) > 0 and int(lib.tgtc_style_trainer_workspace_bytes(16383, 128)) > 0


def test_bad_arguments_are_refused_before_any_launch():
    """No GPU here: every one of these returns before the first HIP call."""
    from tgtc_style_amd import hip, style_chain   # noqa: F401
    lib = hip.load()
    h = ctypes.c_void_p()
    assert lib.tgtc_style_trainer_create(ctypes.byref(h)) == 0 and h.value
    assert lib.tgtc_style_trainer_create(None) == -1
    table = (ctypes.c_void_p * 26)(*([8] * 26))
    one = 8                                                   # a non-NULL pointer that is never dereferenced
    fwd = lambda tr, R, n, prec, ws, nbytes, params=table, x=one: lib.tgtc_style_trainer_forward(
        tr, params, x, one, one, one, R, n, prec, ws, nbytes, one, None)
    big = 1 << 40
    assert fwd(None, 5, 7, 0, one, big) == -1                 # NULL trainer
    assert fwd(h, 0, 7, 0, None, 0) == 0                      # R == 0: TGTC_OK
    assert fwd(h, -1, 7, 0, one, big) == -1 and fwd(h, 65536, 32, 0, one, big) == -1
    assert fwd(h, 5, 0, 0, one, big) == -1 and fwd(h, 5, -2, 0, one, big) == -1
    assert fwd(h, 5, 7, 2, one, big) == -1 and fwd(h, 5, 7, 3, one, big) == -1      # fp16mx, unknown
    assert "precision" in lib.tgtc_last_error().decode()
    assert fwd(h, 5, 7, 0, None, big) == -1 and fwd(h, 5, 7, 0, one, big, x=None) == -1 and fwd(h, 5, 7, 0, one, big, params=None) == -1
    holed = (ctypes.c_void_p * 26)(*([8] * 25 + [None]))
    assert fwd(h, 5, 7, 0, one, big, params=holed) == -1
    need = int(lib.tgtc_style_trainer_workspace_bytes(5, 7))
    assert fwd(h, 5, 7, 0, one, need - 1) == -1 and "workspace" in lib.tgtc_last_error().decode()
    bwd = lambda tr, R, n, ws, nbytes, grads=table: lib.tgtc_style_trainer_backward(tr, table, one, R, n, ws, nbytes, grads, None, None, None)
    assert bwd(None, 5, 7, one, big) == -1 and bwd(h, 5, 0, one, big) == -1 and bwd(h, 5, 7, one, big, grads=None) == -1
    assert bwd(h, 5, 7, one, need - 1) == -1 and "workspace" in lib.tgtc_last_error().decode()
    assert bwd(h, 5, 7, one, big) == -1 and "forward" in lib.tgtc_last_error().decode()      # a backward without its forward
    assert lib.tgtc_style_trainer_destroy(h) == 0 and lib.tgtc_style_trainer_destroy(None) == 0


def test_the_flag_parses():
    a = cfg.parse_args(["--config", FERN])
    assert a.style_chain is False
    a = cfg.parse_args(["--config", FERN, "--style_chain", "--style_train"])
    assert a.style_chain is True and a.style_train is True
    assert "style_chain" in cfg.EXTRA and "style_chain" in cfg.HELP


@pytest.mark.parametrize("others", [["--origin_train"], ["--style_train", "--render_valid"], ["--style_train", "--render_train"],
                                    ["--style_train", "--render_valid_style"], ["--style_train", "--render_train_style"],
                                    ["--render_valid_style"], ["--origin_train", "--style_train"], []])
def test_refused_combinations_name_the_flag(others):
    from tgtc_style_amd import train_tgtcs
    with pytest.raises(SystemExit) as e:
        train_tgtcs.main(["--config", FERN, "--synthetic", "--style_chain"] + others)
    said = str(e.value)
    assert "--style_chain" in said
    other = [f for f in others if f != "--style_train"]
    if other:
        assert other[0] in said
    else:
        assert "--style_train" in said


def test_the_default_is_the_per_layer_path():
    import inspect
    from tgtc_style_amd import training
    for fn in (training.style_train_iteration, training.style_train_step):
        assert inspect.signature(fn).parameters["chain"].default is None
