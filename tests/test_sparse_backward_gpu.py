"""GPU: the sparse backward of the fused trainer (include/tgtc_train.h "Sparse backward", csrc/mlp_train.hip,
train_dgrad_kernel.inc) against float64 autograd on the oracle's network, over the edges of its live
list: counts on both sides of the 16-slot chain tile, the 32-slot weight-gradient step and the 128-slot workgroup, a lone
live sample at either end of the batch and on both sides of a workgroup boundary, nothing live at all.

Inputs and references are those of the training-kernel sweep (tests/train_kernel_cases.py, family D): `train_samples` (737
samples away from every ReLU kink), `train_upstream`, `train_reference`; the upstream w_rgb / w_sig are multiplied by a 0/1
mask and the float64 and float32 references are computed with the same masked upstream.  The rule is the sweep's
(`_check_24` of tests/test_train_kernel_shapes_gpu.py, restated here): per tensor, error relative to the float64 tensor
maximum <= max(2e-5, 3 x float32 autograd)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import train_kernel_cases as tc
from origin_train_cases import FERN

pytestmark = pytest.mark.gpu

ERR_ARG = -1                     # TGTC_ERR_ARG
SV = "fern_style_style_nerf_relu_UseViewDir_ImgFactor4"
LAYERS = ["base_layers.%d" % i for i in range(8)] + ["sigma_layer", "base_remap_layer", "rgb_layers.0", "rgb_layers.1"]
KEYS = ["net.%s.%s" % (l, p) for l in LAYERS for p in ("weight", "bias")]      # fused_train.mlp_parameters order


def _every(k):
    return lambda m: m % k == 0


# name -> (M, predicate on the sample index); 385 = three workgroup tiles and one sample
MASKS = {
    "all": (385, lambda m: m >= 0),
    "every7": (385, _every(7)),                               # 55 live: three list tiles and seven
    "100to148": (385, lambda m: (m >= 100) & (m < 148)),      # 48: one and a half weight-gradient steps
    "first16": (385, lambda m: m < 16),
    "first32": (385, lambda m: m < 32),
    "first33": (385, lambda m: m < 33),
    "only0": (385, lambda m: m == 0),
    "only384": (385, lambda m: m == 384),
    "only127": (385, lambda m: m == 127),
    "127and128": (385, lambda m: (m == 127) | (m == 128)),
    "not3of737": (737, lambda m: m % 3 != 0),
}
SEQUENCE = list(MASKS)
# The mask of the tests whose mask is this file's choice.  d sigma_layer.bias is ONE number, the sum of d_sigma over the live
# samples, and its own "tensor maximum": under the rule it must be right to 2e-5 of ITSELF.  With train_upstream(385) the
# m % 7 mask leaves a sum of -9.4e-8 out of sum |d_sigma| = 3.9e-4 (a 4 148-fold cancellation): 2e-5 of it is 1.9e-12, below
# the half-ulp of a single summand's partial sums in float32, and whether ANY float32 accumulation -- either mode's column
# sums with their atomics, or float32 autograd -- lands inside is a matter of the order of the additions.  Where the choice is
# ours the mask is one whose sum does not cancel (100 <= m < 148: 11-fold; m % 3 != 0 of 737: 13-fold).
OWN = "100to148"


def mask_of(name):
    M, pred = MASKS[name]
    return pred(torch.arange(M)).float()


_refs = {}


def references(name):
    """(pts, dirs, masked w_rgb, masked w_sig, float64 gradients, float32 gradients) of a mask, computed once"""
    if name not in _refs:
        M = MASKS[name][0]
        pts, dirs = (t[:M] for t in tc.train_samples())
        w_rgb, w_sig = tc.train_upstream(M)
        k = mask_of(name)
        w_rgb, w_sig = w_rgb * k[:, None], w_sig * k
        g64, _, _ = tc.train_reference(pts, dirs, w_rgb, w_sig, torch.float64)
        g32, _, _ = tc.train_reference(pts, dirs, w_rgb, w_sig, torch.float32)
        _refs[name] = (pts, dirs, w_rgb, w_sig, g64, g32)
    return _refs[name]


def bounds(g64, g32):
    """the rule: per tensor (bound relative to the float64 tensor maximum, that maximum)"""
    out = {}
    for k, ref in g64.items():
        scale = float(ref.abs().max()) + 1e-300
        out[k] = (max(2e-5, 3 * float((g32[k] - ref).abs().max()) / scale), scale)
    return out


def check_24(grads, g64, g32, tag):
    bad, worst = [], 0.0
    for k, (bound, scale) in bounds(g64, g32).items():
        err = float((grads[k].double() - g64[k]).abs().max()) / scale
        worst = max(worst, err)
        if not err <= bound:
            bad.append((k, err, bound))
    print("%s: worst of the 24 gradients %.2e of the tensor maximum" % (tag, worst))
    assert not bad, (tag, bad)


def params():
    from tgtc_style_amd import synth
    sd = tc.T(synth.nerf_state(1))
    return [sd[k].float().contiguous().cuda() for k in KEYS]


class Trainer:
    """fused_train.NerfTrainer with the workspace in the test's hands"""

    def __init__(self, sparse):
        from tgtc_style_amd import fused_train, hip
        self.hip, self.t = hip, fused_train.NerfTrainer(sparse=sparse)
        self.lib, self.ps = self.t.lib, params()

    def workspace(self, M, sparse_size, fill=None):
        n = int(self.lib.tgtc_trainer_workspace_bytes_sparse(M) if sparse_size else self.lib.tgtc_trainer_workspace_bytes(M))
        ws = torch.empty(n, dtype=torch.uint8, device="cuda")
        if fill is not None:
            ws.fill_(fill)
        return ws

    def forward(self, pts, dirs, ws):
        self.rgb, self.sigma = self.t.forward(self.ps, pts.cuda().contiguous(), dirs.cuda().contiguous(), ws)
        return self.rgb, self.sigma

    def backward(self, w_rgb, w_sig, ws):
        """-> gradients by state-dict key, on the host"""
        grads = self.t.backward(self.ps, self.rgb, w_rgb.cuda().contiguous(), w_sig.cuda().contiguous(), ws)
        return {k: g.cpu() for k, g in zip(KEYS, grads)}

    def run(self, name, fill=None, sparse_size=None, upstream=None):
        pts, dirs, w_rgb, w_sig, _, _ = references(name)
        ws = self.workspace(pts.shape[0], self.t.sparse if sparse_size is None else sparse_size, fill)
        self.forward(pts, dirs, ws)
        return self.backward(*(upstream or (w_rgb, w_sig)), ws)


@pytest.fixture(scope="module")
def sparse():
    return Trainer(True)


@pytest.fixture(scope="module")
def dense():
    return Trainer(False)


_dense_forward = {}


def dense_forward(dense, M):
    if M not in _dense_forward:
        pts, dirs = (t[:M] for t in tc.train_samples())
        rgb, sigma = dense.forward(pts, dirs, dense.workspace(M, False))
        _dense_forward[M] = (rgb.clone(), sigma.clone())
    return _dense_forward[M]


# ---------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", SEQUENCE)
def test_float64_parity_over_the_edges_of_the_list(sparse, dense, name):
    """All 24 gradients under the rule; the forward is the dense-mode trainer's bit for bit; the guard does not fire.

    [every7]: 23 of the 24 tensors are as far inside the rule as in every other case; d sigma_layer.bias sits on the
    cancellation described at OWN above, and its error follows the order in which the atomics of the column sums land:
    2.43e-6 of itself when this file runs alone (both modes, also in test_dense_against_sparse), 7.29e-5 -- outside the rule --
    when it runs behind the other training tests; the dense mode, the code path as it was, gave 7.05e-5 in that same run.
    The case and the rule stay as they were set: this case FAILS on that one number whenever the order is not the lucky
    one, and no float32 accumulation can promise 1.9e-12 on 55 summands of 1e-5."""
    _, _, _, _, g64, g32 = references(name)
    before = sparse.t.overflows()
    grads = sparse.run(name)
    sparse.t.status()
    assert sparse.t.overflows() == before
    rgb, sigma = dense_forward(dense, MASKS[name][0])
    assert torch.equal(sparse.rgb.view(torch.int32), rgb.view(torch.int32))
    assert torch.equal(sparse.sigma.view(torch.int32), sigma.view(torch.int32))
    check_24(grads, g64, g32, name)


# ---------------------------------------------------------------------------------------------------- 2
def test_nothing_live():
    t = Trainer(True)
    _, _, w_rgb, w_sig, _, _ = references("all")
    grads = t.run("all", upstream=(torch.zeros_like(w_rgb), torch.zeros_like(w_sig)))
    t.t.status()
    assert t.t.overflows() == 0
    assert all(bool((g == 0).all()) for g in grads.values())
    assert t.t.live_counts() == (0, 385)


# ---------------------------------------------------------------------------------------------------- 3
def test_negative_zero_is_dead():
    t = Trainer(True)
    _, _, w_rgb, w_sig, g64, g32 = references(OWN)
    k = mask_of(OWN)
    neg = torch.tensor(-0.0)
    w_rgb_n, w_sig_n = torch.where(k[:, None] > 0, w_rgb, neg), torch.where(k > 0, w_sig, neg)
    assert bool(torch.signbit(w_sig_n[1])) and float(w_sig_n[1]) == 0.0
    grads = t.run(OWN, upstream=(w_rgb_n, w_sig_n))
    assert t.t.live_counts() == (48, 385)
    check_24(grads, g64, g32, "-0.0 on the dead samples")


def test_a_nan_on_a_dead_sample_is_live_and_ends_as_the_dense_backward_does(sparse, dense):
    _, _, w_rgb, w_sig, g64, g32 = references(OWN)
    bad = w_sig.clone()
    assert float(bad[1]) == 0.0
    bad[1] = float("nan")
    for t in (dense, sparse):
        before = t.t.overflows()
        grads = t.run(OWN, upstream=(w_rgb, bad))
        assert t.t.overflows() == before + 1
        assert all(bool((g == 0).all()) for g in grads.values())
        with pytest.raises(RuntimeError):
            t.t.status()
    grads = sparse.run(OWN)
    sparse.t.status()
    check_24(grads, g64, g32, "after the NaN")


# ---------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("name", ["first33", "only384"])
def test_unwritten_memory_is_not_read_as_data(sparse, name):
    """The workspace holds 0xFF bytes (NaN as fp32 and fp16, 2^32 - 1 as an index) wherever the forward, the compaction and
    the chain do not write: the dZ rows and the list entries past the count among them."""
    _, _, _, _, g64, g32 = references(name)
    grads = sparse.run(name, fill=0xFF)
    sparse.t.status()
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    check_24(grads, g64, g32, name + " in 0xFF")


# ---------------------------------------------------------------------------------------------------- 5
def test_dense_against_sparse(sparse, dense):
    """The m % 7 mask, as the sparse backward's specification sets it.  d sigma_layer.bias (see OWN above) is the one tensor
    of the 24 whose outcome follows the order of the float32 additions, in the dense mode -- the code path as it was -- as
    much as in the sparse one: 2.43e-6 in both modes when this file runs alone, dense 7.05e-5 (outside: this test then
    FAILS at its first check, on the dense mode) behind the other training tests."""
    _, _, _, _, g64, g32 = references("every7")
    gd, gs = dense.run("every7"), sparse.run("every7")
    check_24(gd, g64, g32, "dense")
    check_24(gs, g64, g32, "sparse")
    for k, (bound, scale) in bounds(g64, g32).items():
        assert float((gd[k].double() - gs[k].double()).abs().max()) / scale <= 2 * bound, k


# ---------------------------------------------------------------------------------------------------- 6
def test_mode_and_buffers():
    t = Trainer(False)
    lib, hip = t.lib, t.hip
    pts, dirs, w_rgb, w_sig, g64, g32 = references(OWN)
    # the default mode is dense: a backward adds nothing to the sums
    check_24(t.run(OWN), g64, g32, "default mode")
    assert t.t.live_counts() == (0, 0)
    # dense mode takes a workspace of the sparse size
    check_24(t.run(OWN, sparse_size=True), g64, g32, "dense mode, sparse-size workspace")
    assert t.t.live_counts() == (0, 0)
    # a bad mode is refused and changes nothing
    assert lib.tgtc_trainer_set_sparse(t.t.handle, 7) == ERR_ARG and lib.tgtc_trainer_set_sparse(t.t.handle, -1) == ERR_ARG
    t.run(OWN)
    assert t.t.live_counts() == (0, 0)
    # sparse mode with a dense-size workspace: TGTC_ERR_ARG, nothing launched, and no dense backward in its place
    assert lib.tgtc_trainer_set_sparse(t.t.handle, 1) == 0
    ws = t.workspace(385, False)
    t.forward(pts, dirs, ws)                                    # the forward accepts either size
    sentinel = [torch.full_like(p, -7.0) for p in t.ps]
    table = (ctypes.c_void_p * 24)(*[p.data_ptr() for p in t.ps])
    out = (ctypes.c_void_p * 24)(*[g.data_ptr() for g in sentinel])
    d_rgb, d_sig = w_rgb.cuda().contiguous(), w_sig.cuda().contiguous()
    rc = lib.tgtc_trainer_backward(t.t.handle, table, hip.ptr(t.rgb), hip.ptr(d_rgb), hip.ptr(d_sig), 385, hip.ptr(ws), ws.numel(),
                                   out, hip.stream())
    torch.cuda.synchronize()
    assert rc == ERR_ARG and b"sparse" in lib.tgtc_last_error()
    assert all(bool((g == -7.0).all()) for g in sentinel)
    assert t.t.live_counts() == (0, 0)
    # ... and with the sparse size the same handle runs sparse
    ws = t.workspace(385, True)
    t.forward(pts, dirs, ws)
    check_24(t.backward(w_rgb, w_sig, ws), g64, g32, "after set_sparse(1)")
    assert t.t.live_counts() == (48, 385)


class Args:
    use_viewdir, act_type, embed_freq_coor, embed_freq_dir = True, "relu", 10, 4
    netdepth = netdepth_fine = 8
    netwidth = netwidth_fine = 256
    style_D, vae_latent, precision = 8, 32, "fp16x3"


def _net(seed, mode, sparse):
    from tgtc_style_amd import models, synth
    m = models.StyleNerf(Args, mode=mode)
    m.load_state_dict(tc.T(synth.nerf_state(seed)))
    return m.cuda().trainable(sparse=sparse)


def test_two_forwards_before_one_backward_each_with_its_own_lease():
    pts, dirs, w_rgb, w_sig, g64, g32 = references("not3of737")
    m = _net(1, "fine", True)
    loss = 0
    for lo, hi in ((0, 300), (300, 737)):
        out = m(pts=pts[lo:hi].cuda(), dirs=dirs[lo:hi].cuda())
        loss = loss + (out["rgb"] * w_rgb[lo:hi].cuda()).sum() + (out["sigma"].reshape(hi - lo) * w_sig[lo:hi].cuda()).sum()
    loss.backward()
    m._trainer.status()
    assert m.training_overflows() == 0 and m.training_live_counts() == (491, 737)
    check_24({k: p.grad.detach().cpu() for k, p in m.state_dict(keep_vars=True).items()}, g64, g32, "two forwards")


# ---------------------------------------------------------------------------------------------------- 7
def test_counters_are_the_exact_sums():
    t = Trainer(True)
    live = total = 0
    for name in SEQUENCE:
        t.run(name)
        live, total = live + int(mask_of(name).sum()), total + MASKS[name][0]
    assert t.t.live_counts() == (live, total)
    assert t.t.overflows() == 0


# ---------------------------------------------------------------------------------------------------- 8
def test_one_iteration_of_origin_train():
    """training.origin_train_step on 64 rays, 16 + 16 samples, noise of std 1, teacher weights, learning rate 0: sparse
    against dense trainers.  Same forward, so the same losses bit for bit; the 48 gradients within the sum of the two
    bounds of test_dense_against_sparse -- taken at the rule's floor, 2e-5 + 2e-5 of the tensor maximum, which is the
    stricter reading where no float32 yardstick exists."""
    from tgtc_style_amd import synth, training, utils
    o, d = utils.gen_rays(8, 8, synth.fern_intrinsics(8, 8), synth.spiral_pose(2))
    gt = torch.from_numpy(np.random.default_rng(5).uniform(0.2, 0.8, (64, 3)).astype(np.float32)).cuda()
    got = {}
    for sp in (False, True):
        model, fine = _net(0, "coarse", sp), _net(1, "fine", sp)
        opt = torch.optim.SGD(list(model.parameters()) + list(fine.parameters()), lr=0.0)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(17)
        r = training.origin_train_step(model, fine, opt, o, d, gt, 16, 16, 0., 1., sigma_noise_std=1.0, as_float=False, generator=gen)
        for net in (model, fine):
            net._trainer.status()
        grads = [p.grad.detach().cpu() for p in list(model.parameters()) + list(fine.parameters())]
        got[sp] = (r, grads, model.training_live_counts(), fine.training_live_counts())
    (rd, gd, cd, fd), (rs, gs, cs, fs) = got[False], got[True]
    for k in ("loss", "loss_rgb", "loss_rgb_fine"):
        assert torch.equal(rd[k].view(torch.int32), rs[k].view(torch.int32)), k
    assert len(gd) == len(gs) == 48
    worst = 0.0
    for i, (a, b) in enumerate(zip(gd, gs)):
        scale = float(a.abs().max())
        assert scale > 0 and bool(torch.isfinite(b).all()), i
        e = float((a.double() - b.double()).abs().max()) / scale
        worst = max(worst, e)
        assert e <= 4e-5, (i, e)
    print("worst of the 48 gradients, sparse against dense: %.2e of the tensor maximum" % worst)
    assert cd == fd == (0, 0)
    assert cs[1] == 64 * 16 and fs[1] == 64 * 32
    print("live shares: coarse %.3f fine %.3f" % (cs[0] / cs[1], fs[0] / fs[1]))
    assert 0 < cs[0] < cs[1] and 0 < fs[0] < fs[1]


# ---------------------------------------------------------------------------------------------------- 9
def test_the_command_line(tmp_path):
    from tgtc_style_amd import train_loop, train_tgtcs
    logs = {}
    for sp in (False, True):
        base = tmp_path / ("sparse" if sp else "dense")
        sv = train_tgtcs.main(["--config", FERN, "--basedir", str(base), "--origin_train", "--synthetic", "--synthetic_hw", "16",
                               "--batch_size", "256", "--origin_step", "4", "--i_print", "1", "--train_seed", "0"]
                              + (["--train_sparse"] if sp else []))
        logs[sp] = list(train_loop.last_log)
        assert sv == os.path.join(str(base), SV) and os.path.exists(os.path.join(sv, "000004.tar"))
    assert [e["step"] for e in logs[False]] == [0, 1, 2, 3, 4] == [e["step"] for e in logs[True]]
    assert np.float64(logs[False][0]["loss"]).tobytes() == np.float64(logs[True][0]["loss"]).tobytes()
    for sp in (False, True):
        for e in logs[sp]:
            print(e)
            assert all(np.isfinite(v) for v in e.values()) and e["overflows"] == 0
            if sp:
                assert 0 < e["live_coarse"] <= 1 and 0 < e["live_fine"] <= 1
            else:
                assert "live_coarse" not in e and "live_fine" not in e
