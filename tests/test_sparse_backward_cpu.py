"""CPU: the host side of the fused trainer's sparse backward (include/tgtc_train.h "Sparse backward", DESIGN.md section
3.4) -- the three entry points are exported and declared, the sparse workspace holds the dense one plus the live list,
`--train_sparse` parses and its refused combinations say which flag they refuse.  The kernels run in
tests/test_sparse_backward_gpu.py."""
import ctypes
import os
import re

import pytest

from tgtc_style_amd import config as cfg

from origin_train_cases import FERN, ROOT

SYMBOLS = ["tgtc_trainer_set_sparse", "tgtc_trainer_workspace_bytes_sparse", "tgtc_trainer_live_counts"]


def test_the_entry_points_are_exported_and_declared():
    from tgtc_style_amd import fused_train, hip
    lib = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "tgtc_train.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in fused_train.SIGNATURES and name in hip.header_symbols()
    assert re.search(r"#define\s+TGTC_TRAIN_DENSE\s+0\b", header) and re.search(r"#define\s+TGTC_TRAIN_SPARSE\s+1\b", header)
    assert (fused_train.TRAIN_DENSE, fused_train.TRAIN_SPARSE) == (0, 1)


def test_the_sparse_workspace_holds_the_dense_one_and_the_list():
    from tgtc_style_amd import fused_train, hip   # noqa: F401  (fused_train registers the signatures)
    lib = hip.load()
    for M in (1, 127, 128, 129, 385):
        dense, sparse = int(lib.tgtc_trainer_workspace_bytes(M)), int(lib.tgtc_trainer_workspace_bytes_sparse(M))
        assert dense > 0 and sparse >= dense + 4 * M, (M, dense, sparse)
    for M in (0, -1, -385):
        assert int(lib.tgtc_trainer_workspace_bytes_sparse(M)) == 0
    # a NULL trainer is refused before anything is looked at: TGTC_ERR_ARG
    assert lib.tgtc_trainer_set_sparse(None, 1) == -1
    n = ctypes.c_ulonglong(0)
    assert lib.tgtc_trainer_live_counts(None, None, ctypes.byref(n), ctypes.byref(n)) == -1


def test_the_flag_parses():
    a = cfg.parse_args(["--config", FERN])
    assert a.train_sparse is False
    a = cfg.parse_args(["--config", FERN, "--origin_train", "--train_sparse"])
    assert a.train_sparse is True and a.origin_train is True
    assert "train_sparse" in cfg.EXTRA and "train_sparse" in cfg.HELP


@pytest.mark.parametrize("others", [["--origin_train", "--train_unfused"], ["--style_train"], ["--origin_train", "--render_valid"],
                                    ["--origin_train", "--render_train"], ["--origin_train", "--render_valid_style"],
                                    ["--origin_train", "--render_train_style"], ["--render_valid"], []])
def test_refused_combinations_name_the_flag(others):
    from tgtc_style_amd import train_tgtcs
    with pytest.raises(SystemExit) as e:
        train_tgtcs.main(["--config", FERN, "--synthetic", "--train_sparse"] + others)
    said = str(e.value)
    assert "--train_sparse" in said
    other = [f for f in others if f != "--origin_train"]
    if other:
        assert other[0] in said
    else:
        assert "--origin_train" in said


def test_sparse_is_a_mode_of_the_fused_path_only():
    from tgtc_style_amd import models
    a = cfg.parse_args(["--config", FERN])
    m = models.StyleNerf(a, mode="fine")
    with pytest.raises(ValueError):
        m.trainable(fused=False, sparse=True)
    assert m.training_live_counts() == (0, 0)
