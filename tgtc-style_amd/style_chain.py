"""Style trainer (include/tgtc_train.h, csrc/style2d.hip): the forward and the backward of both style MLPs of `Style_train`
-- StyleMLP_before_concat feeding StyleMLP_Wild_multilayers -- as two library calls in place of 26 differentiable layer
calls with their concatenations (autograd_ops.py, the per-layer path).

    trainer = StyleTrainer()
    rgb = trainer.apply(concat_model, style_model, x, base_remap, z, zbar_rows, n)

`apply` is one torch.autograd.Function, differentiable w.r.t. the 26 parameters and the two latent inputs; x and base_remap
(outputs of the frozen NeRF pass) carry no gradient.  Same GEMM kernel, same per-layer arithmetic: the forward's bits are
those of the per-layer path.  Opt-in: nothing selects it for the caller (`training.style_train_iteration(chain=...)`,
`train_tgtcs --style_train --style_chain`)."""
import ctypes

import torch

from . import hip
from .fused_train import MAX_WORKSPACE_BYTES, _table

N_PLANES = 12      # hidden activations kept from forward to backward: 5 of the concat MLP, 7 of the style MLP
_PRECISIONS = ("fp16x3", "fp16")


def chain_parameters(concat_model, style_model):
    """The 26 tensors in the order of include/tgtc_train.h: the concat MLP's 5 linears, then the style MLP's 8, weight then
    bias for each."""
    out = []
    for layer in list(concat_model.layers) + list(style_model.layers):
        out += [layer.weight, layer.bias]
    if len(out) != 26:
        raise NotImplementedError("style trainer: built for style_D=8 (5 + 8 linears), got %d tensors" % len(out))
    return out


class StyleTrainer:
    """Workspaces (12 activation planes and the backward's scratch, about 19 KB per sample) belong to ONE forward /
    backward pair, as fused_train.NerfTrainer's do: `lease` hands one out per forward, the autograd node keeps it until its
    backward has run, `release` returns it to the pool.  An iteration of Style_train -- a coarse and a fine forward before
    one backward -- holds two.  A forward whose backward never runs (its result dropped, an exception in between) keeps
    its workspace out of the pool and its record in the library until this object goes (include/tgtc_train.h).

    trace_workspaces (tests): a list that receives (workspace, R, n) of every forward `apply` runs."""

    def __init__(self):
        self.lib = hip.load()
        h = ctypes.c_void_p()
        hip.check(self.lib.tgtc_style_trainer_create(ctypes.byref(h)))
        self.handle = h
        self._pool = []
        self.trace_workspaces = None

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.tgtc_style_trainer_destroy(self.handle)
        except Exception:
            pass

    def workspace_bytes(self, R, n):
        return int(self.lib.tgtc_style_trainer_workspace_bytes(R, n))

    def lease(self, R, n, device):
        """a workspace for one forward / backward pair of R rays x n samples"""
        need = self.workspace_bytes(R, n)
        if need > MAX_WORKSPACE_BYTES:
            raise ValueError("style trainer workspace for %d x %d samples = %.1f GiB (about 19 KB per sample): use smaller "
                             "batches or train on the per-layer path" % (R, n, need / 2.0 ** 30))
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        for i, ws in enumerate(self._pool):
            if ws.numel() >= need and ws.device == device:
                return self._pool.pop(i)
        return torch.empty(need, dtype=torch.uint8, device=device)

    def release(self, ws):
        if ws is not None and len(self._pool) < 4:
            self._pool.append(ws)

    def forward(self, params, x, base_remap, lat_c, lat_s, R, n, precision, ws):
        """x [R*n,63], base_remap [R*n,256], lat_c / lat_s [R,32], contiguous float32 -> rgb [R*n,3]; the inputs are read
        again by the backward of this call."""
        rgb = torch.empty(R * n, 3, device=x.device, dtype=torch.float32)
        hip.check(self.lib.tgtc_style_trainer_forward(self.handle, _table(params), hip.ptr(x), hip.ptr(base_remap), hip.ptr(lat_c),
                                                      hip.ptr(lat_s), R, n, hip.PRECISIONS[precision], hip.ptr(ws), ws.numel(),
                                                      hip.ptr(rgb), hip.stream()))
        return rgb

    def backward(self, params, d_rgb, R, n, ws, want_lat_c=True, want_lat_s=True):
        """-> (gradients of the 26 parameters, d_lat_c [R,32] or None, d_lat_s [R,32] or None)"""
        dev = d_rgb.device
        flat = torch.empty(sum(p.numel() for p in params), device=dev, dtype=torch.float32)
        grads, at = [], 0
        for p in params:
            grads.append(flat[at:at + p.numel()].view(p.shape))
            at += p.numel()
        d_c = torch.empty(R, 32, device=dev, dtype=torch.float32) if want_lat_c else None
        d_s = torch.empty(R, 32, device=dev, dtype=torch.float32) if want_lat_s else None
        hip.check(self.lib.tgtc_style_trainer_backward(self.handle, _table(params), hip.ptr(d_rgb), R, n, hip.ptr(ws), ws.numel(),
                                                       _table(grads), hip.ptr(d_c), hip.ptr(d_s), hip.stream()))
        return grads, d_c, d_s

    @staticmethod
    def activations(ws, R, n):
        """Test hook: the 12 hidden activations [R*n, 256] a forward left in `ws` (views; concat MLP's 5, then the style
        MLP's 7), valid until the workspace's next use."""
        M = R * n
        planes = ws[:N_PLANES * M * 1024].view(torch.float32).view(N_PLANES, M, 256)      # M * 1 KiB each: 256-byte aligned
        return [planes[i] for i in range(N_PLANES)]

    def apply(self, concat_model, style_model, x, base_remap, z, zbar_rows, n):
        """x [R, n, 63] (or [R*n, 63]), base_remap [R, n, 256]: the frozen NeRF pass's `pts` and `base_remap`; z [R, 32]: the
        latent row of each ray (the concat MLP's); zbar_rows [R, 32]: the style MLP's (the reference's mean of z, broadcast
        over the 32 columns); n samples per ray -> rgb [R, n, 3] (or [R*n, 3])."""
        concat_model._require_supported(), style_model._require_supported()
        if concat_model.precision != style_model.precision or concat_model.precision not in _PRECISIONS:
            raise ValueError("style trainer: both style MLPs in fp16x3 or both in fp16 (got %s, %s)"
                             % (concat_model.precision, style_model.precision))
        hip.require_gpu(x, base_remap, z, zbar_rows)
        lead = x.shape[:-1]
        R = z.shape[0]
        if x.numel() != R * n * 63 or base_remap.numel() != R * n * 256 or z.shape != (R, 32) or zbar_rows.shape != (R, 32):
            raise ValueError("style trainer: x %s, base_remap %s, z %s, zbar_rows %s do not make %d rays x %d samples"
                             % (tuple(x.shape), tuple(base_remap.shape), tuple(z.shape), tuple(zbar_rows.shape), R, n))
        xf = x.detach().reshape(-1, 63).to(torch.float32).contiguous()
        rf = base_remap.detach().reshape(-1, 256).to(torch.float32).contiguous()
        rgb = _StyleChainFn.apply(self, xf, rf, z, zbar_rows, n, concat_model.precision,
                                  *chain_parameters(concat_model, style_model))
        return rgb.reshape(*lead, 3)


class _StyleChainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, trainer, x, remap, z, zbar, n, precision, *params):
        hip.require_gpu(*params)
        ps = [p.detach().float().contiguous() for p in params]
        lat_c, lat_s = z.detach().float().contiguous(), zbar.detach().float().contiguous()
        R = lat_c.shape[0]
        ws = trainer.lease(R, n, x.device)
        rgb = trainer.forward(ps, x, remap, lat_c, lat_s, R, n, precision, ws)
        if trainer.trace_workspaces is not None:
            trainer.trace_workspaces.append((ws, R, n))
        # the stash of THIS call and the inputs its backward reads again, until that backward has run
        ctx.trainer, ctx.ps, ctx.ws, ctx.inputs, ctx.shape = trainer, ps, ws, (x, remap, lat_c, lat_s), (R, n)
        return rgb

    @staticmethod
    def backward(ctx, d_rgb):
        if ctx.ws is None:
            raise RuntimeError("style trainer: backward called twice on one forward (retain_graph): the activation stash was "
                               "returned to the pool after the first backward")
        R, n = ctx.shape
        grads, d_c, d_s = ctx.trainer.backward(ctx.ps, d_rgb.float().contiguous(), R, n, ctx.ws,
                                               ctx.needs_input_grad[3], ctx.needs_input_grad[4])
        ctx.trainer.release(ctx.ws)
        ctx.ws = ctx.inputs = None
        return (None, None, None, d_c, d_s, None, None) + tuple(grads)
