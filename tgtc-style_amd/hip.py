"""ctypes binding of libtgtc_hip.so (include/tgtc_hip.h).

PyTorch is used for device memory and streams only: every call passes raw `data_ptr()`s and the
current HIP stream.  There is NO CPU fallback: if the library is missing or a call fails, a
RuntimeError is raised.
"""
import ctypes
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TGTC_LIB") or os.path.join(_HERE, "csrc", "libtgtc_hip.so")   # TGTC_LIB: development builds

PREC_FP16X3 = 0   # split-fp16, fp32-equivalent (parity mode)
PREC_FP16 = 1     # single fp16 MFMA product (fast mode)
PREC_FP16_FP6 = 2  # fp16 product + two block-scaled fp6 correction products (NeRF nets only)
PRECISIONS = {"fp16x3": PREC_FP16X3, "fp16": PREC_FP16, "fp16mx": PREC_FP16_FP6}

PATH_AUTO = 0         # tgtc_render_path: the library's fastest path for the render
PATH_RAY_KERNEL = 1   # one launch of the persistent ray kernel, no workspace
PATH_CHAIN = 2        # per-sample kernels through the workspace (the split path for coarse fp16x3 + fine fp16mx)

CULL_AUTO = 0         # tgtc_net_set_cull: two-phase fine pass iff the last landed live share is below the library's threshold
CULL_OFF = 1          # always the dense fine pass
CULL_ON = 2           # always densities first, the colour head on the live samples only

SCREEN_AUTO = 0       # tgtc_net_set_screen: screened pass iff the last landed candidate share is below the pass's threshold
SCREEN_OFF = 1        # never
SCREEN_ON = 2         # wherever the list fits

_lib = None

c_void_p, c_int, c_int64, c_float, c_double, c_size_t = (ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
                                                         ctypes.c_float, ctypes.c_double, ctypes.c_size_t)


class Linear(ctypes.Structure):
    """tgtc_linear: host pointers to an nn.Linear's weight [out,in] and bias [out]."""
    _fields_ = [("weight", c_void_p), ("bias", c_void_p), ("out_features", ctypes.c_int32),
                ("in_features", ctypes.c_int32)]


# name -> argtypes (restype is int unless listed in _RESTYPES)
_SIGNATURES = {
    "tgtc_version": [],
    "tgtc_last_error": [],
    "tgtc_gen_rays": [c_int, c_int, c_double, c_double, c_double, c_double, c_void_p, c_int, c_int, c_double,
                      c_int64, c_int64, c_void_p, c_void_p, c_void_p],
    "tgtc_train_batch": [c_int, c_int, c_double, c_double, c_double, c_double, c_void_p, c_int, c_void_p, c_void_p, c_int64,
                         c_int, c_int, c_double, c_void_p, c_void_p, c_void_p, c_void_p],      # include/tgtc_train.h
    "tgtc_style_train_batch": [c_int, c_int, c_double, c_double, c_double, c_double, c_void_p, c_int, c_int, c_void_p,
                               c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_int64, c_int, c_int, c_double,
                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "tgtc_sample_coarse": [c_void_p, c_void_p, c_int64, c_int, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p],
    "tgtc_posenc": [c_void_p, c_int, c_int64, c_int, c_void_p, c_void_p],
    "tgtc_nerf_create": [ctypes.POINTER(Linear), c_int, c_int, ctypes.POINTER(c_void_p)],
    "tgtc_net_destroy": [c_void_p],
    "tgtc_net_precision": [c_void_p],
    "tgtc_nerf_forward": [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "tgtc_nerf_mlp_forward": [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p],
    "tgtc_nerf_forward_rays": [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p],
    "tgtc_nerf_forward_list": [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "tgtc_nerf_forward_list_x3": [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p],
    "tgtc_net_set_cull": [c_void_p, c_int],
    "tgtc_net_live_fraction": [c_void_p],
    "tgtc_net_culled_renders": [c_void_p],
    "tgtc_net_stash_bytes": [c_int64, c_int, c_float],
    "tgtc_net_set_stash": [c_void_p, c_void_p, c_size_t],
    "tgtc_nerf_stash_fill": [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "tgtc_nerf_stash_heads": [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p],
    "tgtc_net_enable_screen": [c_void_p, c_void_p],
    "tgtc_net_screen_margin": [c_void_p],
    "tgtc_net_set_screen": [c_void_p, c_int],
    "tgtc_net_screen_fraction": [c_void_p],
    "tgtc_net_screened_renders": [c_void_p],
    "tgtc_screen_list_fits": [c_size_t, c_int64],
    "tgtc_screen_auto_decision": [c_int, ctypes.c_uint32, ctypes.c_uint32],
    "tgtc_nerf_screen_rays": [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p],
    "tgtc_nerf_sigma_list": [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "tgtc_nerf_forward_list_sigma": [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p],
    # the chain geometry (include/tgtc_hip.h, last section): the siblings' argument lists, `form` in front of the render's
    "tgtc_nerf_sigma_list_mx": [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "tgtc_geometry_build_chain": [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_float, c_float, c_void_p, c_float,
                                  c_void_p, c_size_t, c_void_p, c_void_p, c_void_p],
    "tgtc_render_rays_styled_sparse_chain": [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int,
                                             c_int, c_float, c_float, c_void_p, c_float, c_void_p, c_size_t, c_void_p, c_void_p,
                                             c_void_p, c_void_p],
    "tgtc_composite": [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "tgtc_composite_train": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "tgtc_composite_backward": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p],
    "tgtc_sample_fine": [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p],
    "tgtc_coarse_to_fine": [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p],
    "tgtc_coarse_to_fine_traced": [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "tgtc_composite_live_colours": [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "tgtc_render_workspace_bytes": [c_int64, c_int, c_int],
    "tgtc_render_path": [c_int, c_int, c_int, c_int, c_int, c_int, c_int],
    "tgtc_render_depths": [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_float, c_float, c_void_p, c_void_p, c_void_p],
    "tgtc_render_rays_plain": [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_float, c_float,
                               c_void_p, c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "tgtc_image_epilogue": [c_void_p, c_void_p, c_int64, c_int64, c_float, c_void_p, c_void_p, c_void_p],
    "tgtc_latents_forward": [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int64, c_float, c_int,
                             c_void_p, c_void_p],
    "tgtc_latents_backward": [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int64, c_float, c_int, c_void_p, c_void_p, c_void_p],
}
_RESTYPES = {"tgtc_last_error": ctypes.c_char_p, "tgtc_net_screen_margin": c_float, "tgtc_net_screen_fraction": c_float,
             "tgtc_net_screened_renders": ctypes.c_longlong, "tgtc_net_live_fraction": c_float, "tgtc_net_stash_bytes": c_size_t, "tgtc_net_culled_renders": ctypes.c_longlong, "tgtc_render_workspace_bytes": c_size_t,
             "tgtc_render_styled_multi_workspace_bytes": c_size_t,
             "tgtc_render_styled_sparse_workspace_bytes": c_size_t,
             "tgtc_geometry_cache_bytes": c_size_t, "tgtc_restyle_workspace_bytes": c_size_t,
             "tgtc_style_folded_bytes": c_size_t, "tgtc_render_styled_sparse_folded_workspace_bytes": c_size_t,
             "tgtc_restyle_folded_workspace_bytes": c_size_t, "tgtc_geometry_trunk_bytes": c_size_t}
# the argument lists that whole families of entry points share (include/tgtc_hip.h: "the sibling's arguments, one for one")
_CULLED_RENDER = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_float, c_float,
                  c_void_p, c_float, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]
_LIST_RESTYLE = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_void_p, c_size_t, c_int64,
                 c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]
_PLANE_RESTYLE = [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_void_p, c_size_t, c_int64, c_void_p,
                  c_size_t, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]
_TRUNK_BUILD = [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_size_t, c_int64, c_void_p, c_size_t, c_void_p]
_FOLDED_LIST = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p, c_void_p, c_void_p,
                c_void_p]

_OPTIONAL = {
    "tgtc_style_create": [ctypes.POINTER(Linear), c_int, ctypes.POINTER(Linear), c_int, c_int, ctypes.POINTER(c_void_p)],
    "tgtc_concat_mlp_forward": [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p],
    "tgtc_style_mlp_forward": [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p],
    "tgtc_styled_forward_rays": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int,
                                 c_void_p, c_void_p, c_void_p],
    "tgtc_render_rays_styled": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int,
                                c_float, c_float, c_void_p, c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p],
    "tgtc_styled_forward_rays_multi": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int,
                                       c_void_p, c_void_p, c_void_p],
    "tgtc_render_styled_multi_workspace_bytes": [c_int64, c_int, c_int, c_int],
    "tgtc_render_rays_styled_multi": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int,
                                      c_int, c_float, c_float, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p],
    "tgtc_render_styled_sparse_workspace_bytes": [c_int64, c_int, c_int, c_int],
    "tgtc_render_rays_styled_sparse": _CULLED_RENDER,
    "tgtc_geometry_build": [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_float, c_float, c_void_p, c_float,
                            c_void_p, c_size_t, c_void_p, c_void_p, c_void_p],
    "tgtc_geometry_cache_bytes": [c_int64, c_int64],
    "tgtc_geometry_pack": [c_void_p, c_int64, c_int, c_int, c_float, c_int64, c_void_p, c_size_t, c_void_p],
    "tgtc_restyle_workspace_bytes": [c_int64, c_int],
    "tgtc_restyle_rays": _LIST_RESTYLE,
    "tgtc_style_folded_bytes": [c_int],
    "tgtc_style_fold_latents": [c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_void_p],
    "tgtc_styled_forward_list_folded": _FOLDED_LIST,
    "tgtc_render_styled_sparse_folded_workspace_bytes": [c_int64, c_int, c_int, c_int],
    "tgtc_render_rays_styled_sparse_folded": _CULLED_RENDER,
    "tgtc_restyle_folded_workspace_bytes": [c_int64, c_int],
    "tgtc_restyle_rays_folded": _LIST_RESTYLE,
    "tgtc_geometry_trunk_bytes": [c_int, c_int64],
    "tgtc_geometry_trunk": _TRUNK_BUILD,
    "tgtc_restyle_rays_trunk": _PLANE_RESTYLE,
    "tgtc_restyle_rays_trunk_folded": _PLANE_RESTYLE,
    "tgtc_style_enable_mx": [c_void_p, c_void_p],
    "tgtc_style_has_mx": [c_void_p],
    "tgtc_style_mx_read": [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_size_t],
    "tgtc_restyle_rays_trunk_folded_mx": _PLANE_RESTYLE,
    "tgtc_geometry_trunk_mx": _TRUNK_BUILD,
    "tgtc_geometry_trunk_read": [c_int, c_void_p, c_size_t, c_int64, c_void_p, c_void_p, c_void_p],
    "tgtc_styled_forward_list_folded_mx": _FOLDED_LIST,
    "tgtc_render_rays_styled_sparse_folded_mx": _CULLED_RENDER,
    "tgtc_restyle_rays_folded_mx": _LIST_RESTYLE,
}


def register(signatures, restypes=None):
    """Add the entry points of another header (include/tgtc_style2d.h) to the binding table."""
    _SIGNATURES.update(signatures)
    _RESTYPES.update(restypes or {})
    if _lib is not None:
        for name, argtypes in signatures.items():
            fn = getattr(_lib, name)
            fn.argtypes = argtypes
            fn.restype = _RESTYPES.get(name, c_int)


def header_symbols():
    """Every entry point include/tgtc_hip.h declares (used by the CPU export test)."""
    return sorted(list(_SIGNATURES) + list(_OPTIONAL))


def load():
    """Load the shared library (no GPU needed for loading / symbol checks)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libtgtc_hip.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "or `make -C tgtc-style_amd/csrc` (expected at %s)" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for table in (_SIGNATURES, _OPTIONAL):
        for name, argtypes in table.items():
            fn = getattr(lib, name)   # AttributeError if a declared symbol is not exported
            fn.argtypes = argtypes
            fn.restype = _RESTYPES.get(name, c_int)
    _lib = lib
    return lib


def missing_symbols():
    """Header symbols the built library does not export (must be empty)."""
    lib = ctypes.CDLL(LIB_PATH)
    return [n for n in header_symbols() if not hasattr(lib, n)]


def check(rc):
    if rc != 0:
        raise RuntimeError("libtgtc_hip: error %d: %s" % (rc, load().tgtc_last_error().decode()))


def ptr(t):
    """Device (or host) pointer of a tensor; None -> NULL."""
    if t is None:
        return None
    assert t.is_contiguous(), "tgtc ops need contiguous tensors"
    return t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def require_gpu(*tensors):
    if not torch.cuda.is_available():
        raise RuntimeError("tgtc_style_amd: no GPU visible; the HIP path has no CPU fallback")
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("tgtc_style_amd: expected a CUDA/HIP tensor, got device %s" % t.device)


def make_linears(pairs):
    """[(weight, bias), ...] (tensors or arrays) -> (ctypes array of tgtc_linear, keepalive list)."""
    arr = (Linear * len(pairs))()
    keep = []
    for i, (w, b) in enumerate(pairs):
        w = np.ascontiguousarray(w.detach().cpu().numpy() if isinstance(w, torch.Tensor) else w, dtype=np.float32)
        b = np.ascontiguousarray(b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else b, dtype=np.float32)
        keep += [w, b]
        arr[i].weight = w.ctypes.data
        arr[i].bias = b.ctypes.data
        arr[i].out_features, arr[i].in_features = w.shape
    return arr, keep


class Net:
    """Owns a tgtc_net handle (packed weights resident in HBM)."""

    def __init__(self, handle, precision):
        self.handle = handle
        self.precision = precision
        self.stash = None
        self.screen_tried = False   # enable_screen has run (whether or not the calibration left a screen)

    def set_cull(self, mode):
        """The policy of the two-phase fine pass for chain renders with this net as the fine network (CULL_*)."""
        check(load().tgtc_net_set_cull(self.handle, mode))

    def live_fraction(self):
        """Share of fine samples with sigma > 0 in the last such render whose statistic has landed; -1.0 while unknown."""
        return float(load().tgtc_net_live_fraction(self.handle))

    def culled_renders(self):
        """How many of those renders took the two-phase fine pass."""
        return int(load().tgtc_net_culled_renders(self.handle))

    def set_stash(self, buf):
        """Attach a uint8 device tensor as the stash of the two-phase fine pass (tgtc_net_set_stash); None detaches.  The
        handle keeps the tensor alive."""
        if buf is None:
            check(load().tgtc_net_set_stash(self.handle, None, 0))
        else:
            require_gpu(buf)
            check(load().tgtc_net_set_stash(self.handle, ptr(buf), buf.numel() * buf.element_size()))
        self.stash = buf

    def enable_screen(self):
        """Pack the fp16 form of an fp16x3 / fp16mx NeRF handle and calibrate its margin (tgtc_net_enable_screen: once, one
        host synchronisation; RuntimeError for a style or fp16 handle).  The margin stays -1 where the calibration finds no
        error to scale (a constant density): the handle then renders as before."""
        check(load().tgtc_net_enable_screen(self.handle, stream()))
        self.screen_tried = True

    def set_screen(self, mode):
        """The policy of the screened passes of chain renders with this net (SCREEN_*)."""
        check(load().tgtc_net_set_screen(self.handle, mode))

    def screen_margin(self):
        """The calibrated margin of the density screen; -1.0 when no screen is enabled."""
        return float(load().tgtc_net_screen_margin(self.handle))

    def screen_fraction(self):
        """Share of candidates (screen density not <= -margin) in the last such pass whose statistic has landed; -1.0 while unknown."""
        return float(load().tgtc_net_screen_fraction(self.handle))

    def screened_renders(self):
        """How many chain renders screened their pass with this net."""
        return int(load().tgtc_net_screened_renders(self.handle))

    def has_mx(self):
        """Whether this style pair carries its fp16mx streams (tgtc_style_enable_mx)."""
        return bool(load().tgtc_style_has_mx(self.handle))

    def enable_mx(self):
        """Pack the fp16mx streams of an fp16x3 style pair beside its other streams (once; RuntimeError for another handle)."""
        check(load().tgtc_style_enable_mx(self.handle, stream()))

    def __del__(self):
        try:
            if self.handle and _lib is not None:
                _lib.tgtc_net_destroy(self.handle)
        except Exception:
            pass
        self.handle = None


NERF_LAYER_KEYS = (["base_layers.%d" % i for i in range(8)] +
                   ["sigma_layer", "base_remap_layer", "rgb_layers.0", "rgb_layers.1"])


def nerf_create(state, precision="fp16x3", prefix="net."):
    """Pack a StyleNerf / MLP_style state dict (reference key names) into a device-resident net."""
    require_gpu()
    lib = load()
    pairs = [(state[prefix + k + ".weight"], state[prefix + k + ".bias"]) for k in NERF_LAYER_KEYS]
    arr, keep = make_linears(pairs)
    h = c_void_p()
    check(lib.tgtc_nerf_create(arr, len(pairs), PRECISIONS[precision], ctypes.byref(h)))
    del keep
    return Net(h, precision)


def nerf_forward_list_x3(net, rays_o, rays_d, ts, live, n_live, rgb, sigma=None):
    """tgtc_nerf_forward_list_x3: the full fp16x3 network of `net` (a Net) over the device-side list live[: *n_live] of the
    [R, N] grid ts -- rgb [R*N,3] (and sigma [R*N] where given) are written at the listed samples only.  n_live is a device
    tensor of one int32; nothing is synchronised.  RuntimeError for a handle in another precision."""
    require_gpu(rays_o, rays_d, ts, live, n_live, rgb, sigma)
    R, N = ts.shape
    check(load().tgtc_nerf_forward_list_x3(net.handle, ptr(rays_o), ptr(rays_d), ptr(ts), R, N, ptr(live), ptr(n_live), ptr(rgb),
                                           ptr(sigma), stream()))


def style_create(concat_state=None, style_state=None, precision="fp16x3"):
    """Pack StyleMLP_before_concat (5 linears `layers.0..4`) and / or StyleMLP_Wild_multilayers (8 linears
    `layers.0..7`) state dicts into one device-resident handle.  A missing net is packed as zeros."""
    require_gpu()
    lib = load()
    keep = []
    if concat_state is not None:
        ca, k = make_linears([(concat_state["layers.%d.weight" % i], concat_state["layers.%d.bias" % i]) for i in range(5)])
        keep.append(k)
        nc = 5
    else:
        ca, nc = None, 0
    if style_state is not None:
        sa, k = make_linears([(style_state["layers.%d.weight" % i], style_state["layers.%d.bias" % i]) for i in range(8)])
        keep.append(k)
        ns = 8
    else:
        sa, ns = None, 0
    h = c_void_p()
    check(lib.tgtc_style_create(ca, nc, sa, ns, PRECISIONS[precision], ctypes.byref(h)))
    del keep
    return Net(h, precision)
