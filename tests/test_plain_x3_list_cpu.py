"""CPU: the host side of the two-phase fine pass for a fine handle in fp16x3 -- tgtc_nerf_forward_list_x3 is
declared with the stated signature, exported and bound; pass 3 of tgtc_screen_auto_decision obeys the edge rules of the other
passes, whose thresholds stay; --two_phase parses and is refused where it has no meaning, before any GPU work; RayRenderer's
argument validation is what it was."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIGNATURE = ("const tgtc_net* net, const double* rays_o, const double* rays_d, const float* ts, int64_t R, int N, "
             "const uint32_t* live, const uint32_t* n_live, float* rgb, float* sigma, void* stream")


def test_header_declares_the_list_entry_and_the_library_exports_it():
    from tgtc_style_amd import hip
    name = "tgtc_nerf_forward_list_x3"
    text = open(os.path.join(ROOT, "include", "tgtc_hip.h")).read()
    m = re.search(r"^([a-z ]+?)\s+%s\(([^)]*)\);" % name, text, re.M)
    assert m, name
    assert m.group(1) == "int" and " ".join(m.group(2).split()) == SIGNATURE, m.groups()
    assert hasattr(ctypes.CDLL(hip.LIB_PATH), name)
    assert len(hip._SIGNATURES[name]) == len(SIGNATURE.split(",")) == 11
    assert name in hip.header_symbols() and not hip.missing_symbols()
    bound = hip.load()
    # no handle: a pure host answer, no device touched
    assert getattr(bound, name)(None, None, None, None, 1, 1, None, None, None, None, None) == -1
    assert callable(hip.nerf_forward_list_x3)
    # the siblings keep their argument lists
    assert len(hip._SIGNATURES["tgtc_nerf_forward_list"]) == 10 and len(hip._SIGNATURES["tgtc_nerf_forward_list_sigma"]) == 11


THRESHOLDS = {0: 0.56, 1: 0.45, 2: 0.51, 3: 0.68}     # 3: measured with tools/time_plain_x3.py --step0 (csrc/render.hip)


def test_auto_decision_keeps_its_passes_and_gains_pass_3():
    from tgtc_style_amd import hip
    decide = hip.load().tgtc_screen_auto_decision
    total = 1 << 20
    for p, thr in THRESHOLDS.items():
        for share in [i / 400 for i in range(401)]:
            c = int(share * total)
            if abs(c / total - thr) < 1e-6:
                continue                                             # (the float comparison at the threshold itself)
            assert decide(p, c, total) == int(c / total < thr), (p, share)
    for p in (0, 1, 2, 3):
        assert decide(p, 0, 0) == 0 and decide(p, 5, 0) == 0          # nothing landed
        assert decide(p, total + 1, total) == 0                      # not a pair
        assert decide(p, total, total) == 0                          # every sample a candidate
    grid = [decide(3, int(s * total), total) for s in [i / 200 for i in range(201)]]
    assert grid == sorted(grid, reverse=True)                        # one threshold: screens below it, never above


def test_two_phase_parses():
    from tgtc_style_amd import config
    assert config.parse_args(["--render_valid"]).two_phase is False
    args = config.parse_args(["--render_valid", "--two_phase", "--precision", "fp16x3"])
    assert args.two_phase is True and args.precision == "fp16x3"
    assert "two_phase" in config.EXTRA and "byte-identical" in config.HELP["two_phase"] and "ray kernel" in config.HELP["two_phase"]


@pytest.mark.parametrize("flags,named", [
    (["--render_valid_style"], "render_valid_style"), (["--render_train_style"], "render_train_style"),
    (["--origin_train"], "origin_train"), (["--style_train"], "style_train"),
    (["--render_valid", "--render_valid_style"], "render_valid_style"), ([], "render_valid")])
def test_two_phase_is_refused_where_it_has_no_meaning(flags, named, monkeypatch):
    """SystemExit that names what the flag needs, before train() -- and with it any GPU work -- is reached"""
    from tgtc_style_amd import train_tgtcs

    def no_train(args):
        raise AssertionError("train() was reached")
    monkeypatch.setattr(train_tgtcs, "train", no_train)
    with pytest.raises(SystemExit) as e:
        train_tgtcs.main(["--synthetic", "--expname", "x", "--two_phase"] + flags)
    assert "--two_phase" in str(e.value) and "--render_valid" in str(e.value) and named in str(e.value)


def test_renderer_argument_validation_is_unchanged():
    from tgtc_style_amd import rendering
    for cull in (None, True, False):
        for screen in (None, True, False, (None, False), (True, True)):
            for fused in (True, False, "single"):
                r = rendering.RayRenderer(None, None, fused=fused, cull=cull, screen=screen)
                assert (r.fused, r.cull, r.screen) == (fused, cull, screen)
    for bad in (dict(cull="on"), dict(cull=1.5), dict(screen="auto"), dict(screen=(True,)), dict(screen=(True, "x")),
                dict(fused="chain"), dict(fused=None), dict(stash="big")):
        with pytest.raises(ValueError):
            rendering.RayRenderer(None, None, **bad)
