"""GPU: the training-side kernels over the shapes, input families and pointer combinations of tests/train_kernel_cases.py,
each against float64 on the CPU ("The training-kernel sweep").  The C entry points are called through
hip.load() / hip.ptr / hip.check, as utils._Composite and autograd_ops._Linear call them: the NULL-pointer combinations
cannot be reached through autograd, which materialises a missing gradient as zeros.

Every output buffer is pre-filled with NaN and every workspace with fp16 NaN halves, so an element a kernel leaves unwritten,
or a pad column it reads without clearing, shows."""
import numpy as np
import pytest
import torch

import train_kernel_cases as tc

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _hip():
    from tgtc_style_amd import hip
    from tgtc_style_amd import style2d  # noqa: F401  (registers the ctypes signatures of the tgtc_s2d_* entries)
    return hip, hip.load()


def _dev(t):
    return None if t is None else t.cuda().contiguous()


def _nan(*shape):
    return torch.full(shape, NAN, device="cuda", dtype=torch.float32)


# =============================================================================================== A. compositing
def composite_train(rgb, sigma, ts, noise, white, want_weights=True):
    hip, lib = _hip()
    R, N = sigma.shape
    a = [_dev(t) for t in (rgb, sigma, ts, noise)]
    rgb_exp, t_exp, w = _nan(R, 3), _nan(R), (_nan(R, N) if want_weights else None)
    hip.check(lib.tgtc_composite_train(hip.ptr(a[0]), hip.ptr(a[1]), hip.ptr(a[2]), hip.ptr(a[3]), int(white), R, N, hip.ptr(rgb_exp),
                                       hip.ptr(t_exp), hip.ptr(w), hip.stream()))
    return {"rgb_exp": rgb_exp.cpu(), "t_exp": t_exp.cpu(), "weights": None if w is None else w.cpu()}


def composite_backward(rgb, sigma, ts, noise, white, g_rgb, g_t, g_w, want=("d_rgb", "d_sigma")):
    hip, lib = _hip()
    R, N = sigma.shape
    a = [_dev(t) for t in (rgb, sigma, ts, noise, g_rgb, g_t, g_w)]
    d_rgb = _nan(R, N, 3) if "d_rgb" in want else None
    d_sigma = _nan(R, N) if "d_sigma" in want else None
    hip.check(lib.tgtc_composite_backward(hip.ptr(a[0]), hip.ptr(a[1]), hip.ptr(a[2]), hip.ptr(a[3]), int(white), R, N, hip.ptr(a[4]),
                                          hip.ptr(a[5]), hip.ptr(a[6]), hip.ptr(d_rgb), hip.ptr(d_sigma), hip.stream()))
    return {"d_rgb": None if d_rgb is None else d_rgb.cpu(), "d_sigma": None if d_sigma is None else d_sigma.cpu()}


def _check_rays(got, ref64, ref32, worst, tag, keys=None):
    """per ray: max |got - ref| / max |ref| <= max(the existing bound, 3 x the same figure of float32 autograd).  The existing
    bound of the gradients is relative (1e-5, 1e-4), that of the forward outputs 2e-6 ABSOLUTE: there it is divided by the
    ray's max |ref|."""
    for k in keys or tc.COMPOSITE_BOUNDS:
        R = ref64[k].shape[0]
        err = tc.rows_error(got[k].reshape(R, -1), ref64[k].reshape(R, -1))
        yard = tc.rows_error(ref32[k].reshape(R, -1), ref64[k].reshape(R, -1))
        yard = torch.where(torch.isinf(yard), torch.zeros_like(yard), yard)
        floor = torch.full_like(yard, tc.COMPOSITE_BOUNDS[k])
        if not k.startswith("d_"):
            floor = floor / ref64[k].reshape(R, -1).abs().amax(1).clamp_min(1e-300)
        bound = torch.maximum(3 * yard, floor)
        w = worst.setdefault(k, [0.0, 0.0, ""])
        if R and float(err.max()) >= w[0]:
            w[0], w[2] = float(err.max()), tag
        w[1] = max(w[1], float(yard.max()) if R else 0.0)
        assert bool((err <= bound).all()), (tag, k, err.tolist(), bound.tolist())


def _print_worst(title, worst):
    for k, (e, y, tag) in worst.items():
        print("%s %-8s worst per-ray error %.2e (at %s); float32 autograd up to %.2e" % (title, k, e, tag, y))


@pytest.mark.parametrize("family", tc.FAMILIES)
def test_composite_matches_float64_on_every_ray(family):
    """tgtc_composite_train and tgtc_composite_backward on every N of the family (base: the whole N grid, i.e. every template
    instance on both sides of its boundary), white background on and off, noise given and NULL: every output of every RAY
    against float64 autograd on the oracle, relative to that ray's own maximum."""
    worst = {}
    for fam, N, white, nz in [c for c in tc.composite_cases() if c[0] == family]:
        inp, up, ref64, ref32 = tc.composite_references(fam, N, white, nz)
        got = composite_train(*inp, white)
        got.update(composite_backward(*inp, white, *up))
        _check_rays(got, ref64, ref32, worst, "N=%d white=%d noise=%s" % (N, white, "given" if nz else "NULL"))
        if fam == "dead":         # nothing lives: exactly zero, exactly the background
            assert all(float(got[k].abs().max()) == 0 for k in ("t_exp", "weights", "d_rgb", "d_sigma"))
            assert bool((got["rgb_exp"] == float(white)).all())
        if fam == "ties":
            assert float(got["d_sigma"][:, 0:N - 1:2].abs().max()) == 0 and float(got["weights"][:, 0:N - 1:2].abs().max()) == 0
        if fam == "opaque":
            k = tc.opaque_index(N)
            assert float(got["weights"][:, k + 1:].max()) < 1e-9 and bool((got["d_sigma"][:, k] == 0).all())
    _print_worst(family, worst)


@pytest.mark.parametrize("R", tc.COMPOSITE_R_EDGES[1])
def test_composite_ray_counts_around_one_workgroup(R):
    N = tc.COMPOSITE_R_EDGES[0]
    inp, up, ref64, ref32 = tc.composite_references("base", N, 1, True, R=R)
    got = composite_train(*inp, 1)
    got.update(composite_backward(*inp, 1, *up))          # R = 0: both return without a launch
    assert got["weights"].shape == (R, N) and got["d_rgb"].shape == (R, N, 3)
    if R:
        _check_rays(got, ref64, ref32, {}, "R=%d" % R)


def test_composite_refuses_more_than_512_samples():
    N = tc.COMPOSITE_MAX_N + 1
    inp, up = tc.composite_inputs("base", 1, N), tc.composite_upstream(1, N)
    with pytest.raises(RuntimeError, match="exceeds 512"):
        composite_train(*inp, 0)
    with pytest.raises(RuntimeError, match="exceeds 512"):
        composite_backward(*inp, 0, *up)
    with pytest.raises(RuntimeError):                     # and neither output asked for
        composite_backward(*tc.composite_inputs("base", 2, 65), 0, *tc.composite_upstream(2, 65), want=())


def test_composite_of_one_sample_is_the_closed_form():
    """N = 1: delta = 1e10, so w = 1 if sigma + noise > 0 else 0 (the oracle's delta[..., :1] of an empty tensor is empty: it
    does not define this shape).  rgb_exp = w rgb (+ 1 - w on white), t_exp = w t, d sigma = 0, d rgb = w g_rgb -- exactly."""
    R = 9
    rgb, sigma, ts, noise = tc.base_inputs(R, 1, 3)
    noise = noise * 8
    raw = sigma + noise
    assert bool((raw > 0).any()) and bool((raw < 0).any()) and bool(((sigma > 0) != (raw > 0)).any())
    g_rgb, g_t, g_w = tc.composite_upstream(R, 1)
    for white in (0, 1):
        for nz in (noise, None):
            w = ((sigma if nz is None else raw) > 0).float()
            fwd = composite_train(rgb, sigma, ts, nz, white)
            bwd = composite_backward(rgb, sigma, ts, nz, white, g_rgb, g_t, g_w)
            assert torch.equal(fwd["weights"], w) and torch.equal(fwd["t_exp"], w[:, 0] * ts[:, 0])
            assert torch.equal(fwd["rgb_exp"], w * rgb[:, 0] + (1 - w) * white)
            assert float(bwd["d_sigma"].abs().max()) == 0 and torch.equal(bwd["d_rgb"], w[:, :, None] * g_rgb[:, None, :])


@pytest.mark.parametrize("N", tc.POINTER_N)
def test_composite_null_pointer_combinations(N):
    R = tc.COMPOSITE_R
    worst = {}
    for white in (0, 1):
        inp, up, _, _ = tc.composite_references("base", N, white, True)
        names = ("g_rgb", "g_t", "g_w")
        # each upstream gradient alone: the missing ones are zeros in the reference
        for i, name in enumerate(names):
            only = [u if j == i else None for j, u in enumerate(up)]
            got = composite_backward(*inp, white, *only)
            ref64, ref32 = tc.composite_reference(*inp, white, *only), tc.composite_reference(*inp, white, *only, dtype=torch.float32)
            assert float(ref64["d_sigma"].abs().max()) > 0
            _check_rays(got, ref64, ref32, worst, "N=%d white=%d only %s" % (N, white, name), keys=("d_rgb", "d_sigma"))
        # each output alone: bit for bit the output of the call that asks for both
        both = composite_backward(*inp, white, *up)
        for k in ("d_rgb", "d_sigma"):
            one = composite_backward(*inp, white, *up, want=(k,))
            assert torch.equal(one[k], both[k]) and all(v is None for kk, v in one.items() if kk != k)
        # no weights asked for: the other two outputs do not change
        a, b = composite_train(*inp, white), composite_train(*inp, white, want_weights=False)
        assert b["weights"] is None and torch.equal(a["rgb_exp"], b["rgb_exp"]) and torch.equal(a["t_exp"], b["t_exp"])
    _print_worst("single upstream gradient N=%d" % N, worst)


# =============================================================================================== B. dense layers
def linear_forward(x, W, b, relu, precision, pre=False):
    """tgtc_s2d_linear, or tgtc_s2d_linear_pre with the weight's halves from tgtc_s2d_split when K is a multiple of 4"""
    hip, lib = _hip()
    (M, K), N = x.shape, W.shape[0]
    xd, Wd, bd = _dev(x), _dev(W), _dev(b)
    y = _nan(M, N)
    if not pre:
        hip.check(lib.tgtc_s2d_linear(hip.ptr(xd), M, K, hip.ptr(Wd), hip.ptr(bd), N, int(relu), hip.PRECISIONS[precision], hip.ptr(y), hip.stream()))
        return y
    hi = lo = None
    if K % 4 == 0:
        hi = torch.empty(N * K, dtype=torch.float16, device="cuda")
        lo = torch.empty_like(hi)
        hip.check(lib.tgtc_s2d_split(hip.ptr(Wd), N * K, hip.ptr(hi), hip.ptr(lo), hip.stream()))
    hip.check(lib.tgtc_s2d_linear_pre(hip.ptr(xd), M, K, hip.ptr(Wd), hip.ptr(hi), hip.ptr(lo), hip.ptr(bd), N, int(relu),
                                      hip.PRECISIONS[precision], hip.ptr(y), hip.stream()))
    return y


def linear_backward(x, dy, relu_y, W, precision, want=("dx", "dW", "db")):
    """tgtc_s2d_linear_backward -> dict of the outputs asked for (device tensors); relu_y a device tensor or None"""
    hip, lib = _hip()
    (M, K), N = x.shape, W.shape[0]
    xd, dyd, Wd = _dev(x), _dev(dy), _dev(W)
    nbytes = lib.tgtc_s2d_linear_backward_workspace_bytes(M, K, N)
    ws = torch.full(((nbytes + 3) // 4,), 0x7e007e00, dtype=torch.int32, device="cuda")      # every half an fp16 NaN
    out = {"dx": _nan(M, K) if "dx" in want else None, "dW": _nan(N, K) if "dW" in want else None, "db": _nan(N) if "db" in want else None}
    hip.check(lib.tgtc_s2d_linear_backward(hip.ptr(xd), hip.ptr(dyd), hip.ptr(relu_y), hip.ptr(Wd), M, K, N, hip.PRECISIONS[precision],
                                           hip.ptr(ws), ws.numel() * 4, hip.ptr(out["dx"]), hip.ptr(out["dW"]), hip.ptr(out["db"]), hip.stream()))
    return {k: v for k, v in out.items() if v is not None}


def _tensor_error(got, ref):
    e = float((got.double().cpu() - ref).abs().max()) / (float(ref.abs().max()) + 1e-300)
    return e if e == e else float("inf")


def _check_backward_x3(got, ref64, ref32, tag, worst):
    """the existing test's bounds of the tensor maximum, and the same per output row of dx and of dW relative to the row's own
    maximum, there with max(bound, 3 x the float32 yardstick of that row)"""
    for k in ("dx", "dW", "db"):
        e = _tensor_error(got[k], ref64[k])
        worst["tensor " + k] = max(worst.get("tensor " + k, 0.0), e)
        assert e <= tc.LINEAR_BOUNDS[k], (tag, k, e)
    for k in ("dx", "dW"):
        err = tc.rows_error(got[k].cpu(), ref64[k])
        yard = tc.rows_error(ref32[k], ref64[k])
        yard = torch.where(torch.isinf(yard), torch.zeros_like(yard), yard)
        bound = torch.clamp_min(3 * yard, tc.LINEAR_BOUNDS[k])
        worst["row " + k] = max(worst.get("row " + k, 0.0), float(err.max()))
        worst["row " + k + " float32"] = max(worst.get("row " + k + " float32", 0.0), float(yard.max()))
        bad = torch.nonzero(err > bound).reshape(-1)
        assert bad.numel() == 0 and bool((err == err).all()), (tag, k, "%d rows" % bad.numel(), bad[:5].tolist(), err[bad[:5]].tolist(), bound[bad[:5]].tolist())


@pytest.mark.parametrize("M,K,N", tc.LINEAR_CASES)
def test_linear_and_its_backward_on_every_branch(M, K, N):
    """fp16x3, with the ReLU gate (taken from the kernel's own forward output) and without: y of both forward entries, dx, dW
    and db against float64, whole tensors and row by row."""
    x, W, b, dy = tc.linear_inputs(M, K, N)
    worst = {}
    for relu in (True, False):
        y = linear_forward(x, W, b, relu, "fp16x3")
        y_pre = linear_forward(x, W, b, relu, "fp16x3", pre=True)
        assert torch.equal(y, y_pre)          # the same halves, whoever split them
        gate = (y > 0).cpu() if relu else None
        ref64, ref32 = tc.linear_reference(x, W, b, dy, gate), tc.linear_reference(x, W, b, dy, gate, torch.float32)
        e = _tensor_error(y, torch.relu(ref64["y"]) if relu else ref64["y"])
        worst["tensor y"] = max(worst.get("tensor y", 0.0), e)
        assert e <= tc.LINEAR_BOUNDS["y"], ("y", relu, e)
        got = linear_backward(x, dy, y if relu else None, W, "fp16x3")
        _check_backward_x3(got, ref64, ref32, "relu=%s" % relu, worst)
    print("(%d, %d, %d) nsplit %d mc %d: " % ((M, K, N) + tc.backward_split(M, K, N)) + "  ".join("%s %.2e" % kv for kv in sorted(worst.items())))


@pytest.mark.parametrize("M,K,N", tc.SUBSET_CASES)
def test_linear_backward_output_subsets_are_bit_identical(M, K, N):
    x, W, b, dy = tc.linear_inputs(M, K, N)
    y = linear_forward(x, W, b, True, "fp16x3")
    full = linear_backward(x, dy, y, W, "fp16x3")
    assert all(bool(torch.isfinite(v).all()) for v in full.values())
    for want in tc.SUBSETS:
        got = linear_backward(x, dy, y, W, "fp16x3", want=want)
        assert set(got) == set(want)
        for k in want:
            assert torch.equal(got[k], full[k]), (want, k, float((got[k] - full[k]).abs().max()))


def test_linear_backward_rescales_the_upstream_gradient_exactly():
    """dy x 2^-100 and x 2^100 (the two ends of the exponent range grad_scale_kernel clamps to, tests/train_kernel_cases.py
    scale_case_dy): the gradients are the scale-1 gradients times the power of two, bit for bit.  dy = 0: exactly zero."""
    M, K, N = tc.SCALE_CASE
    x, W, b, dy = tc.linear_inputs(M, K, N)
    dy = tc.scale_case_dy(dy)
    base = linear_backward(x, dy, None, W, "fp16x3")
    ref64, ref32 = tc.linear_reference(x, W, b, dy, None), tc.linear_reference(x, W, b, dy, None, torch.float32)
    _check_backward_x3(base, ref64, ref32, "scale 1", {})
    for p in tc.SCALES:
        got = linear_backward(x, dy * 2.0 ** p, None, W, "fp16x3")
        for k in ("dx", "dW", "db"):
            assert bool(torch.isfinite(got[k]).all()) and torch.equal(got[k], base[k] * 2.0 ** p), (p, k)
    zero = linear_backward(x, torch.zeros_like(dy), None, W, "fp16x3")
    assert all(float(zero[k].abs().max()) == 0 for k in ("dx", "dW", "db"))


def test_linear_backward_with_rows_of_very_different_size():
    """Every third row of dy at 2^-30 of the others -- a batch in which samples behind a surface carry almost no gradient."""
    M, K, N = tc.UNEVEN_CASE
    x, W, b, dy = tc.linear_inputs(M, K, N)
    dy = tc.uneven_rows(dy)
    worst = {}
    for relu in (True, False):
        y = linear_forward(x, W, b, relu, "fp16x3")
        gate = (y > 0).cpu() if relu else None
        got = linear_backward(x, dy, y if relu else None, W, "fp16x3")
        ref64, ref32 = tc.linear_reference(x, W, b, dy, gate), tc.linear_reference(x, W, b, dy, gate, torch.float32)
        small = tc.rows_error(got["dx"].cpu()[1::3], ref64["dx"][1::3])
        print("relu=%s: dx rows at 2^-30: worst per-row error %.2e; the other rows %.2e" % (
            relu, float(small.max()), float(tc.rows_error(got["dx"].cpu()[0::3], ref64["dx"][0::3]).max())))
        _check_backward_x3(got, ref64, ref32, "relu=%s" % relu, worst)
    print("  ".join("%s %.2e" % kv for kv in sorted(worst.items())))


@pytest.mark.parametrize("M,K,N", tc.FP16_CASES)
def test_linear_fp16_is_the_product_of_once_rounded_operands(M, K, N):
    """precision = fp16 against tests/train_kernel_cases.py fp16_model: the float64 product of the operands rounded once to
    fp16 where the kernels round them.  max(2e-6, 3 x the float32 product of the same operands) of the tensor maximum: a lost
    lo half would not show at the 1e-3 an unrounded reference needs, a wrong row or a dropped term does here."""
    x, W, b, dy = tc.linear_inputs(M, K, N)
    worst = {}
    for relu in (True, False):
        y = linear_forward(x, W, b, relu, "fp16")
        y_pre = linear_forward(x, W, b, relu, "fp16", pre=True)
        assert torch.equal(y, y_pre)
        gate = (y > 0).cpu() if relu else None
        m64, m32 = tc.fp16_model(x, W, b, dy, gate), tc.fp16_model(x, W, b, dy, gate, torch.float32)
        got = linear_backward(x, dy, y if relu else None, W, "fp16")
        got["y"] = y
        for k in ("y", "dx", "dW", "db"):
            ref = torch.relu(m64[k]) if (k == "y" and relu) else m64[k]
            ref32 = torch.relu(m32[k]) if (k == "y" and relu) else m32[k]
            e, yard = _tensor_error(got[k], ref), _tensor_error(ref32, ref)
            worst[k] = max(worst.get(k, (0, 0)), (e, yard))
            assert e <= max(tc.FP16_BOUND, 3 * yard), (relu, k, e, yard)
    print("(%d, %d, %d) fp16: " % (M, K, N) + "  ".join("%s %.2e (float32 %.2e)" % (k, e, yd) for k, (e, yd) in sorted(worst.items())))


@pytest.mark.parametrize("n", tc.ACTIVATION_N)
def test_activation_modes(n):
    hip, lib = _hip()
    for mode in (0, 1, 2):
        dy, y = tc.activation_inputs(mode, n)
        out, dyd, yd = _nan(n), _dev(dy), _dev(y)
        hip.check(lib.tgtc_s2d_activation(hip.ptr(dyd), hip.ptr(yd), n, mode, hip.ptr(out), hip.stream()))
        ref = tc.activation_reference(mode, dy, y)
        got = out.cpu().double()
        if mode == 0:         # a selection: exact, and y == 0 is closed
            assert torch.equal(got, ref)
        else:                 # mode 1: three float32 roundings; mode 2: expf (two ulp), an add and a divide -- at most eight half
                              # ulps, 2^-21; a result below the float32 normal range (sigmoid(-100) = 4e-44) may be zero
            assert bool(((got - ref).abs() <= 2.0 ** -21 * ref.abs() + 1.2e-38).all()), (mode, float((got - ref).abs().max()))
            assert mode == 1 or bool(((got >= 0) & (got <= 1)).all())


# =============================================================================================== C. latent gather
def latents_forward(lat, mu, sid, fid, scale, llff):
    hip, lib = _hip()
    S, F, D = lat.shape
    R = sid.shape[0]
    a = [_dev(t) for t in (lat, mu, sid, fid)]
    out = _nan(R, D)
    hip.check(lib.tgtc_latents_forward(hip.ptr(a[0]), hip.ptr(a[1]), S, F, D, hip.ptr(a[2]), hip.ptr(a[3]), R, float(scale), int(llff),
                                       hip.ptr(out), hip.stream()))
    return out.cpu()


def latents_backward(g, shape, sid, fid, scale, llff, want=("d_latents", "d_mu")):
    hip, lib = _hip()
    S, F, D = shape
    R = sid.shape[0]
    a = [_dev(t) for t in (g, sid, fid)]
    d_lat = torch.zeros(S, F, D, device="cuda") if "d_latents" in want else None
    d_mu = torch.zeros(S, D, device="cuda") if "d_mu" in want else None
    hip.check(lib.tgtc_latents_backward(hip.ptr(a[0]), S, F, D, hip.ptr(a[1]), hip.ptr(a[2]), R, float(scale), int(llff), hip.ptr(d_lat),
                                        hip.ptr(d_mu), hip.stream()))
    return {"d_latents": None if d_lat is None else d_lat.cpu(), "d_mu": None if d_mu is None else d_mu.cpu()}


@pytest.mark.parametrize("llff", [True, False])
@pytest.mark.parametrize("R", tc.LATENT_R)
def test_latent_gather_and_its_gradient(R, llff):
    lat, mu = tc.latent_tables()
    sid, fid = tc.latent_ids(R, llff)
    g = torch.from_numpy(np.random.default_rng(5 + R).standard_normal((R, tc.LATENT_D)).astype(np.float32))
    worst = [0.0, 0.0, 0.0]
    for scale in tc.LATENT_SCALES:
        out64, dl64, dm64 = tc.latent_reference(lat, mu, sid, fid, scale, llff, g)
        _, dl32, dm32 = tc.latent_reference(lat, mu, sid, fid, scale, llff, g, torch.float32)
        out = latents_forward(lat, mu, sid, fid, scale, llff)
        assert out.shape == (R, tc.LATENT_D)
        if R:
            worst[0] = max(worst[0], float((out.double() - out64).abs().max()))
            assert float((out.double() - out64).abs().max()) <= 1e-7
        both = latents_backward(g, lat.shape, sid, fid, scale, llff)
        for want in (("d_latents",), ("d_mu",)):
            one = latents_backward(g, lat.shape, sid, fid, scale, llff, want=want)
            assert one[want[0]] is not None and all(v is None for k, v in one.items() if k != want[0])
            both_k, one_k = both[want[0]], one[want[0]]
            # the atomics' order is free: the two calls agree to rounding, each is held to the reference below
            for got in (both_k, one_k):
                ref, ref32 = (dl64, dl32) if want[0] == "d_latents" else (dm64, dm32)
                assert bool((got[ref == 0] == 0).all())                  # a row no ray gathers receives nothing
                scale_ = float(ref.abs().max())
                if scale_ > 0:
                    e, yard = float((got.double() - ref).abs().max()) / scale_, float((ref32 - ref).abs().max()) / scale_
                    i = 1 if want[0] == "d_latents" else 2
                    worst[i] = max(worst[i], e)
                    assert e <= max(1e-6, 3 * yard), (want, scale, e, yard)
    print("R=%d llff=%s: forward %.2e absolute; d latents %.2e, d mu %.2e of the tensor maximum" % (R, llff, *worst))


def test_latent_ids_outside_the_tables_raise_before_any_launch():
    """models.check_latent_ids runs on the host before tgtc_latents_forward: nothing is launched with these ids."""
    from tgtc_style_amd import models
    F, D = tc.LATENT_F, tc.LATENT_D
    for S in (1, tc.LATENT_S):
        lat = models.StyleLatents_variational(style_num=S, frame_num=F, latent_dim=D).cuda()
        for trainable in (False, True):
            lat.trainable(trainable)
            for sid, fid, kind in tc.bad_latent_ids(S, F):
                with pytest.raises(IndexError):
                    lat(style_ids=torch.tensor([0, sid]), frame_ids=torch.tensor([0, fid]), type=kind)
        ok = lat(style_ids=torch.tensor([S - 1]), frame_ids=torch.tensor([7 * S * F - 1 - (S - 1) * F]), type="llff")
        assert ok.shape == (1, D) and bool(torch.isfinite(ok).all())


# =============================================================================================== D. fused trainer
class Args:
    use_viewdir, act_type, embed_freq_coor, embed_freq_dir = True, "relu", 10, 4
    netdepth = netdepth_fine = 8
    netwidth = netwidth_fine = 256
    style_D, vae_latent, precision = 8, 32, "fp16x3"


def _fused(pts, dirs, w_rgb, w_sig):
    """fused forward + backward of the fine network (synth seed 1) -> (gradients by state-dict key, rgb, sigma); the guard
    must not fire"""
    from tgtc_style_amd import models, synth
    M = pts.shape[0]
    m = models.StyleNerf(Args, mode="fine")
    m.load_state_dict(tc.T(synth.nerf_state(1)))
    m = m.cuda().trainable()
    before = m.training_overflows()
    out = m(pts=pts.cuda(), dirs=dirs.cuda())
    ((out["rgb"] * w_rgb.cuda()).sum() + (out["sigma"].reshape(M) * w_sig.cuda()).sum()).backward()
    m._trainer.status()
    assert m.training_overflows() == before
    grads = {k: p.grad.detach().cpu() for k, p in m.state_dict(keep_vars=True).items()}
    assert len(grads) == 24 and all(g is not None for g in grads.values())
    return grads, out["rgb"].detach().cpu(), out["sigma"].detach().reshape(M).cpu()


def _check_24(grads, g64, g32, tag):
    bad, worst = [], 0.0
    for k, ref in g64.items():
        scale = float(ref.abs().max()) + 1e-300
        err = float((grads[k].double() - ref).abs().max()) / scale
        yard = float((g32[k] - ref).abs().max()) / scale
        worst = max(worst, err)
        if not err <= max(2e-5, 3 * yard):
            bad.append((k, err, yard))
    print("%s: worst of the 24 gradients %.2e of the tensor maximum" % (tag, worst))
    assert not bad, (tag, bad)


@pytest.mark.parametrize("M", tc.TRAIN_M)
def test_fused_trainer_at_the_edges_of_its_tile(M):
    """M samples away from every ReLU kink, so that the float64 oracle and the fp16x3 forward agree on every gate: the fused
    forward and all 24 gradients against float64 autograd, max(2e-5, 3 x float32 autograd) of the tensor maximum."""
    pts, dirs, w_rgb, w_sig, g64, g32, rgb64, sig64 = tc.train_references(M)
    grads, rgb, sig = _fused(pts, dirs, w_rgb, w_sig)
    assert float((rgb.double() - rgb64).abs().max()) <= 2e-5
    assert float((sig.double() - sig64).abs().max()) <= 2e-5 * float(sig64.abs().max())
    _check_24(grads, g64, g32, "M=%d" % M)


@pytest.mark.parametrize("case", [1, 2, 3])
def test_fused_trainer_with_uneven_upstream_gradients(case):
    """M = 385 = three full tiles and one sample, the tiles' upstream gradients of very different size (uneven_scales): what
    a training batch looks like, and what scale_exp's `b == 0 ? keep : clamp(..)` is for.  Cases 1 and 2 against float64 under
    the rule of the test above; case 3 sits below the clamp, where precision is lost by design: finite, and no guard."""
    pts, dirs, w_rgb, w_sig, g64, g32, _, _ = tc.train_references(385, case)
    grads, _, _ = _fused(pts, dirs, w_rgb, w_sig)
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    if case != 3:
        assert all(float(g.abs().max()) > 0 for g in g64.values())
        _check_24(grads, g64, g32, "case %d" % case)
