"""Render drivers.

`RayRenderer` is the MI355X-native fast path: one C-ABI call per batch of rays enqueues the whole
coarse -> fine chain (reference rendering.py:27-51 for plain, :118-178 for stylised) on the current
stream, with every intermediate kept in a preallocated device workspace.

`cal_geometry`, `render_style` and `render_train_style` keep the reference's signatures
(rendering.py:5, :93-94, :242-243) for drop-in use from `train_tgtcs.py`-style drivers.
"""
import os

import numpy as np
import torch

from . import hip


class GeometryCache:
    """The ray-only half of a culled stylised render (tgtc_geometry_build + tgtc_geometry_pack): one flat uint8 buffer in the
    layout include/tgtc_hip.h documents -- a 256-byte header, t [R], ray_start [R+1], live / ts_live / w_live [count], every
    plane rounded up to 256 bytes -- plus the metadata a restyle is checked against.  `key` is any string the caller uses
    to tell caches apart (None: unchecked).

    `trunk` (None unless asked for: RayRenderer.build_trunk) is the trunk plane of tgtc_geometry_trunk, a uint8 device tensor
    of trunk_nbytes(trunk_precision, count) bytes -- base_remap of every list entry as the style kernels' operand fragments,
    1 KiB per live sample in fp16x3, 512 B in fp16 -- from which `restyle` runs without any NeRF network.  It is valid only
    for this list and for style pairs packed in `trunk_precision` (a name of hip.PRECISIONS): the plane's LAYOUT.
    `trunk_source` is the precision of the NeRF handle that produced it (None without a plane): `trunk_precision`, or "fp16mx"
    for the fp16x3 plane of tgtc_geometry_trunk_mx."""
    MAGIC, VERSION = 0x43475447, 1
    TRUNK_TILE_BYTES = 131072

    def __init__(self, buffer, R, N, count, min_weight, key=None, n_coarse=None, n_fine=None):
        self.buffer, self.R, self.N, self.count = buffer, int(R), int(N), int(count)
        self.min_weight, self.key = float(min_weight), key
        self.n_coarse, self.n_fine = n_coarse, n_fine
        self.trunk = self.trunk_precision = self.trunk_source = None
        if buffer.dtype != torch.uint8 or buffer.dim() != 1 or buffer.numel() < self.nbytes(self.R, self.count):
            raise ValueError("GeometryCache: the buffer must be uint8 [>= %d] for R = %d, count = %d"
                             % (self.nbytes(self.R, self.count), self.R, self.count))

    @staticmethod
    def _planes(R, count):
        """name -> (byte offset, words); the total size in bytes."""
        up = lambda words: (4 * words + 255) // 256 * 256
        out, off = {}, 256
        for name, words in (("t", R), ("ray_start", R + 1), ("live", count), ("ts_live", count), ("w_live", count)):
            out[name] = (off, words)
            off += up(words)
        return out, off

    @classmethod
    def nbytes(cls, R, count):
        return cls._planes(R, count)[1]

    @classmethod
    def trunk_nbytes(cls, precision, count):
        """tgtc_geometry_trunk_bytes: one 128 KiB tile per 128 (fp16x3) / 256 (fp16) list entries; 0 for an empty list or a
        precision the style kernels are not built for.  `precision`: a name of hip.PRECISIONS or the library's enum."""
        per_tile = {hip.PREC_FP16X3: 128, hip.PREC_FP16: 256}.get(hip.PRECISIONS.get(precision, precision))
        if per_tile is None or count <= 0:
            return 0
        return (count + per_tile - 1) // per_tile * cls.TRUNK_TILE_BYTES

    def attach_trunk(self, trunk, precision, source=None):
        """Take `trunk` as this cache's plane.  ValueError unless it is uint8 [trunk_nbytes(precision, count)].
        source: the precision of the NeRF handle that produced it; None means `precision`, "fp16mx" goes with an fp16x3 plane
        only (tgtc_geometry_trunk_mx), anything else is a ValueError."""
        if precision not in ("fp16x3", "fp16"):
            raise ValueError("GeometryCache: a trunk plane exists in fp16x3 and fp16 only (got %r)" % (precision,))
        source = precision if source is None else source
        if source != precision and (source, precision) != ("fp16mx", "fp16x3"):
            raise ValueError("GeometryCache: a %s trunk plane comes from a %s NeRF handle, or an fp16x3 plane from an fp16mx one "
                             "(got source %r)" % (precision, precision, source))
        need = self.trunk_nbytes(precision, self.count)
        if trunk.dtype != torch.uint8 or trunk.dim() != 1 or trunk.numel() != need:
            raise ValueError("GeometryCache: the %s trunk plane of %d list entries is uint8 [%d], got %s %s"
                             % (precision, self.count, need, trunk.dtype, list(trunk.shape)))
        self.trunk, self.trunk_precision, self.trunk_source = trunk, precision, source

    def drop_trunk(self):
        """Release the plane; the cache restyles through the fine NeRF handle again."""
        self.trunk = self.trunk_precision = self.trunk_source = None

    def _view(self, name, dtype):
        off, words = self._planes(self.R, self.count)[0][name]
        return self.buffer[off:off + 4 * words].view(dtype)

    header = property(lambda self: self.buffer[:256].view(torch.int32))
    t = property(lambda self: self._view("t", torch.float32))
    ray_start = property(lambda self: self._view("ray_start", torch.int32))      # the library's uint32, < 2^31
    live = property(lambda self: self._view("live", torch.int32))
    ts_live = property(lambda self: self._view("ts_live", torch.float32))
    w_live = property(lambda self: self._view("w_live", torch.float32))

    def save(self, path, with_trunk=False):
        """One file: the buffer (moved to the host) and the metadata.  The trunk plane is left out unless with_trunk (it is
        some 80 times the buffer, and build_trunk makes it again from a loaded cache in about one trunk pass); a file saved
        without it is the file of a cache that never had one.  "trunk_source" is written where it differs from
        "trunk_precision": a file without the key holds a plane from a handle of the plane's own precision."""
        d = {"buffer": self.buffer.detach().cpu(), "R": self.R, "N": self.N, "count": self.count,
             "min_weight": self.min_weight, "key": self.key, "n_coarse": self.n_coarse, "n_fine": self.n_fine}
        if with_trunk:
            if self.trunk is None:
                raise ValueError("GeometryCache.save: with_trunk, but the cache carries no trunk plane")
            d["trunk"], d["trunk_precision"] = self.trunk.detach().cpu(), self.trunk_precision
            if self.trunk_source != self.trunk_precision:
                d["trunk_source"] = self.trunk_source
        torch.save(d, path)

    @classmethod
    def load(cls, path, device):
        """The cache of `save` on `device`, with its trunk plane if the file has one.  ValueError if the header in the buffer
        contradicts the metadata, the list leaves the sample range or the plane's size contradicts trunk_nbytes (a damaged
        file must not reach the kernels)."""
        d = torch.load(path, map_location="cpu")
        c = cls(d["buffer"].contiguous(), d["R"], d["N"], d["count"], d["min_weight"], d["key"], d["n_coarse"], d["n_fine"])
        want = [cls.MAGIC, cls.VERSION, c.R & 0xffffffff, c.R >> 32, c.N, c.count,
                int(np.float32(c.min_weight).view(np.uint32))]
        want = [w - (1 << 32) if w >= 1 << 31 else w for w in want]
        if c.header[:7].tolist() != want:
            raise ValueError("GeometryCache.load: %s: the buffer's header does not match R, N, count, min_weight" % path)
        if c.count and not (0 <= int(c.live.min()) and int(c.live.max()) < c.R * c.N and int(c.ray_start[-1]) == c.count
                            and int(c.ray_start.min()) >= 0 and int(c.ray_start.max()) <= c.count):
            raise ValueError("GeometryCache.load: %s: the list leaves the sample range" % path)
        if d.get("trunk") is not None:
            c.attach_trunk(d["trunk"].contiguous(), d.get("trunk_precision"), d.get("trunk_source"))
            c.trunk = c.trunk.to(device)
        c.buffer = c.buffer.to(device)
        return c


class RayRenderer:
    """Fused renderer over packed networks.

    coarse / fine: `models.StyleNerf` modules (or anything with `.packed()` returning a hip.Net).
    style: optional `models.StylePair` for the stylised chain.
    """

    _CULL = {None: hip.CULL_AUTO, False: hip.CULL_OFF, True: hip.CULL_ON}

    _SCREEN = {None: hip.SCREEN_AUTO, False: hip.SCREEN_OFF, True: hip.SCREEN_ON}

    def __init__(self, coarse, fine, style=None, fused=True, cull=None, stash=None, screen=None):
        """fused=True: the library's fastest path (TGTC_PATH_AUTO) -- a single persistent ray kernel where one is built, except
        for coarse fp16x3 + fine fp16mx, whose fine pass runs faster on the two-tile per-sample kernel (the split path).
        fused="single" asks for the single ray kernel and nothing else (TGTC_PATH_RAY_KERNEL).  fused=False forces the chain
        of per-sample kernels (TGTC_PATH_CHAIN).  All three agree to rounding, the network arithmetic bit for bit
        (tests/test_fused_gpu.py).  include/tgtc_hip.h, tgtc_render_path, holds the rule.
        cull (plain render on the chain, fine fp16mx): None leaves the two-phase fine pass to the library (TGTC_CULL_AUTO:
        densities first and the colour head on the live samples only once the fine handle has seen a low enough live
        share), True / False force it on / off.  The mode lives on the FINE HANDLE and is set by every plain render of
        this renderer; the images are the same bits either way (include/tgtc_hip.h).
        A fine handle in fp16x3 takes the two-phase pass with cull=True only, and on the chain only (fused=False: fused=True
        resolves fp16x3+fp16x3 to the ray kernel, which has no such pass): the density-only launch, then the full fp16x3
        network over the list of live samples (tgtc_nerf_forward_list_x3).  None and False leave its pass dense, as it was.
        stash (fine fp16mx only): None attaches the stash of the two-phase pass as STASH_DEFAULT says, True / False force it,
        a uint8 device tensor is attached as it is (any size from one slot per region up is correct);
        it is allocated at the first such render, STASH_SHARE x 932 bytes per fine sample (about 4 GB for 400 x 400 rays at
        128 + 64), and never with cull=False.  The same bits again.
        screen (plain render on the chain; coarse fp16x3, fine fp16mx): the density screen of the two passes (include/tgtc_hip.h)
        -- fp16 densities of all samples first, the exact kernels on the candidates only.  None enables the screen on both
        handles at the first such render (one host synchronisation per handle) and leaves the decision to the library
        (TGTC_SCREEN_AUTO), True forces it wherever it fits, False switches it off; one value for both passes, or a pair
        (coarse, fine).  cull=False switches the fine screen off as well.  With cull=True the fine screen covers a fine handle
        in fp16x3 too (enabled at the first such render; under cull=None / False that handle's plain render has no screen).
        The same bits again: measured for samples inside the
        screen's box |x|, |y|, |z| <= 2, where its margin is calibrated; a sample outside it is always handed to the exact
        kernel, so near / far beyond NDC cost time, not bits (DESIGN 3.1 "The screen's domain").
        The culled stylised calls and build_geometry use `screen` only under geometry="chain" (DESIGN 3.1i): there the fine
        screen covers a fine handle in fp16x3 as well and does not depend on `cull`."""
        if isinstance(screen, tuple):
            if len(screen) != 2 or any(v not in self._SCREEN for v in screen):
                raise ValueError("screen must be None, True, False or a pair of those (coarse, fine)")
        elif screen not in self._SCREEN:
            raise ValueError("screen must be None, True, False or a pair of those (coarse, fine)")
        if not (stash is None or stash is True or stash is False or isinstance(stash, torch.Tensor)):
            raise ValueError("stash must be None, True, False or a uint8 device tensor")
        if fused not in (True, False, "single"):
            raise ValueError("fused must be True, False or 'single'")
        if cull not in self._CULL:
            raise ValueError("cull must be None, True or False")
        self.coarse, self.fine, self.style, self.fused, self.cull = coarse, fine, style, fused, cull
        self.stash = stash
        self.screen = screen
        self._stash = None
        self._ws = None
        self._ws_multi = None
        self._ws_restyle = None

    def apply_cull(self):
        """Put this renderer's `cull` on the fine handle (a host call; handles are repacked when weights change)."""
        self.fine.packed().set_cull(self._CULL[self.cull])

    def apply_screen(self, chain=False):
        """Put this renderer's `screen` on the two handles, enabling the screen where a pass may be screened (host calls;
        handles are repacked when weights change).  Handles in fp16 have no screen.
        chain: the call is a chain geometry (geometry="chain"), whose sigma-only fine pass is screened for a fine handle in
        fp16x3 as well; plain renders screen a fine handle in fp16mx, and one in fp16x3 where cull is True (its two-phase
        pass exists under TGTC_CULL_ON only)."""
        pair = self.screen if isinstance(self.screen, tuple) else (self.screen, self.screen)
        fine_precs = ("fp16mx", "fp16x3") if chain or self.cull is True else ("fp16mx",)
        for net, want, precs in ((self.coarse.packed(), pair[0], ("fp16x3",)), (self.fine.packed(), pair[1], fine_precs)):
            if net.precision not in precs:
                continue
            if want is not False and not net.screen_tried:
                net.enable_screen()
            net.set_screen(self._SCREEN[want])

    # The live share the lazily attached stash is sized for: the library's kCullLiveThreshold (csrc/render.hip).  AUTO never
    # culls above it, so a frame AUTO culls overflows only where single waves see more live samples than the frame's share.
    STASH_SHARE = 0.14
    # Whether plain chain renders attach a stash by default (stash=None); DESIGN 3.1 holds the measurement behind it.
    STASH_DEFAULT = True

    def _apply_stash(self, R, nt, device):
        """Attach (lazily allocated, kept while large enough) or detach the stash of the two-phase fine pass on the fine
        handle: fine handles in fp16mx only, never with cull=False (include/tgtc_hip.h, tgtc_net_set_stash)."""
        net = self.fine.packed()
        want = self.STASH_DEFAULT if self.stash is None else self.stash
        if want is False or self.cull is False or net.precision != "fp16mx":
            if net.stash is not None:
                net.set_stash(None)
            return
        if isinstance(want, torch.Tensor):            # the caller's own buffer, whatever it holds
            if net.stash is not want:
                net.set_stash(want)
            return
        need = hip.load().tgtc_net_stash_bytes(R, nt, self.STASH_SHARE)
        if self._stash is None or self._stash.numel() < need or self._stash.device != device:
            if net.stash is not None:
                net.set_stash(None)
            self._stash = None   # (freed before its successor is allocated)
            self._stash = torch.empty(need, dtype=torch.uint8, device=device)
        if net.stash is not self._stash:
            net.set_stash(self._stash)

    _REQUEST = {True: hip.PATH_AUTO, "single": hip.PATH_RAY_KERNEL, False: hip.PATH_CHAIN}

    def _path(self, nc, nf, request=None, styled=False, want_coarse=False):
        """The path the library resolves `request` (default: this renderer's `fused`) to, or its error code (< 0)."""
        request = self._REQUEST[self.fused] if request is None else request
        pc, pf = (hip.PRECISIONS[n.packed().precision] for n in (self.coarse, self.fine))
        ps = hip.PRECISIONS[self.style.packed().precision] if styled else -1
        return hip.load().tgtc_render_path(request, pc, pf, ps, nc, nf, int(want_coarse))

    def _split_is_faster(self):
        """Does the library's fastest path take the per-sample kernels although a ray kernel is built?  (The rule does not
        depend on the sample counts then; 64 + 64 is a shape every ray kernel takes.)"""
        return self._fused_shape(64, 64) and self._path(64, 64, hip.PATH_AUTO) == hip.PATH_CHAIN

    def _fused_shape(self, nc, nf):
        """Is the single ray kernel of the plain render built for these sample counts and precisions?"""
        return self._path(nc, nf, hip.PATH_RAY_KERNEL) == hip.PATH_RAY_KERNEL

    def _fused_styled_shape(self, nc, nf):
        """The same for the stylised render (its ray kernel takes the three handles' precisions)."""
        return self._path(nc, nf, hip.PATH_RAY_KERNEL, styled=True) == hip.PATH_RAY_KERNEL

    def _workspace(self, R, nc, nf, device):
        need = hip.load().tgtc_render_workspace_bytes(R, nc, nf)
        if self._ws is None or self._ws.numel() < need or self._ws.device != device:
            self._ws = torch.empty(need, dtype=torch.uint8, device=device)
        return self._ws

    @staticmethod
    def _rays(rays_o, rays_d):
        """rays_o, rays_d as contiguous float64, then the ray count and the device."""
        rays_o = rays_o.to(torch.float64).contiguous()
        rays_d = rays_d.to(torch.float64).contiguous()
        return rays_o, rays_d, rays_o.shape[0], rays_o.device

    @staticmethod
    def _jitter(jitter):
        return None if jitter is None else jitter.to(torch.float32).contiguous()

    def _scratch(self, attr, need, device):
        """The uint8 scratch tensor this renderer keeps under `attr`, grown to `need` bytes on `device`."""
        ws = getattr(self, attr)
        if ws is None or ws.numel() < need or ws.device != device:
            ws = None
            setattr(self, attr, None)       # release the old one first: the two together may not fit
            ws = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
            setattr(self, attr, ws)
        return ws

    @staticmethod
    def _check_geometry(who, geometry, min_weight):
        """geometry: None (the ray kernel's first half and a dense sigma pass, today's call) or "chain" (the plain chain's
        passes, screened as `screen` says; the culled calls only).  ValueError otherwise; True for "chain"."""
        if geometry not in (None, "chain"):
            raise ValueError("%s: geometry is None or 'chain', got %r" % (who, geometry))
        if geometry is not None and min_weight is None:
            raise ValueError("%s: geometry='chain' needs a min_weight (the culled render)" % who)
        return geometry == "chain"

    @staticmethod
    def _check_zs(zs, R):
        """zs [K,R,32] (per ray) or [K,32] (frame-constant: folded) as contiguous float32, then K and whether it is folded."""
        zs = zs.to(torch.float32).contiguous()
        folded = zs.dim() == 2
        if folded:
            if zs.shape[0] < 1 or zs.shape[1] != 32:
                raise ValueError("zs must be [K,32] with K >= 1, got %s" % list(zs.shape))
        elif zs.dim() != 3 or zs.shape[0] < 1 or zs.shape[1] != R or zs.shape[2] != 32:
            raise ValueError("zs must be [K,%d,32] with K >= 1, got %s" % (R, list(zs.shape)))
        return zs, zs.shape[0], folded

    def render(self, rays_o, rays_d, n_coarse, n_fine, near=0., far=1., jitter=None, z=None, want_coarse=False,
               min_weight=None, geometry=None):
        """rays_o, rays_d float64 [R,3] on the GPU -> dict rgb [R,3], t [R] (+ rgb_coarse, t_coarse).

        min_weight (stylised render only, a float >= 0): the style networks run only on the fine samples whose compositing
        weight exceeds it -- `render_latents(..., min_weight=...)` with K = 1, returning rgb [R,3], t [R] and "live".
        geometry (with a min_weight only): handed to render_latents."""
        self._check_geometry("render", geometry, min_weight)
        if min_weight is not None:
            if want_coarse:
                raise ValueError("min_weight and want_coarse exclude each other (the culled render has no coarse image)")
            if self.style is None or z is None:
                raise ValueError("min_weight belongs to the stylised render: it needs a style pair and z")
            out = self.render_latents(rays_o, rays_d, n_coarse, n_fine, near=near, far=far, jitter=jitter,
                                      zs=z.unsqueeze(0), min_weight=min_weight, geometry=geometry)
            out["rgb"] = out["rgb"][0]
            return out
        hip.require_gpu(rays_o, rays_d)
        lib = hip.load()
        if n_fine <= 0:
            raise ValueError("N_samples_fine must be > 0 (the reference render paths dereference None otherwise)")
        rays_o, rays_d, R, dev = self._rays(rays_o, rays_d)
        plain = self.style is None or z is None
        path = self._path(n_coarse, n_fine, styled=not plain, want_coarse=want_coarse)
        if path < 0:
            if self.fused == "single":
                raise ValueError("fused='single': no single-kernel build for this render (precisions, sample counts or coarse image)")
            hip.check(path)
        ws = self._workspace(R, n_coarse, n_fine, dev) if path == hip.PATH_CHAIN else None
        rgb = torch.empty(R, 3, device=dev, dtype=torch.float32)
        t = torch.empty(R, device=dev, dtype=torch.float32)
        rgb_c = torch.empty(R, 3, device=dev, dtype=torch.float32) if want_coarse else None
        t_c = torch.empty(R, device=dev, dtype=torch.float32) if want_coarse else None
        jitter = self._jitter(jitter)
        rest = (path, hip.ptr(ws), 0 if ws is None else ws.numel(), hip.ptr(rgb), hip.ptr(t), hip.ptr(rgb_c), hip.ptr(t_c),
                   hip.stream())
        if plain:
            self.apply_cull()
            if path == hip.PATH_CHAIN:
                self._apply_stash(R, n_coarse + n_fine, dev)
                self.apply_screen()
            hip.check(lib.tgtc_render_rays_plain(self.coarse.packed().handle, self.fine.packed().handle, hip.ptr(rays_o),
                                                 hip.ptr(rays_d), R, n_coarse, n_fine, float(near), float(far), hip.ptr(jitter),
                                                 *rest))
        else:
            z = z.to(torch.float32).contiguous()
            hip.check(lib.tgtc_render_rays_styled(self.coarse.packed().handle, self.fine.packed().handle,
                                                  self.style.packed().handle, hip.ptr(rays_o), hip.ptr(rays_d), hip.ptr(z), R,
                                                  n_coarse, n_fine, float(near), float(far), hip.ptr(jitter), *rest))
        out = {"rgb": rgb, "t": t}
        if want_coarse:
            out["rgb_coarse"], out["t_coarse"] = rgb_c, t_c
        return out

    def ray_kernel_depths(self, rays_o, rays_d, n_coarse, n_fine, near=0., far=1., jitter=None):
        """The merged fine-pass depths float [R, n_coarse + n_fine] (ascending) a ray kernel built for this renderer's coarse
        handle evaluates its fine pass at: the depths-only instance of the plain ray kernel (tgtc_render_depths), one launch,
        no workspace.  ValueError where no such kernel is built (sample counts, or a coarse handle in fp16mx)."""
        hip.require_gpu(rays_o, rays_d)
        rays_o, rays_d, R, dev = self._rays(rays_o, rays_d)
        ts = torch.empty(R, n_coarse + n_fine, device=dev, dtype=torch.float32)
        jitter = self._jitter(jitter)
        rc = hip.load().tgtc_render_depths(self.coarse.packed().handle, hip.ptr(rays_o), hip.ptr(rays_d), R, n_coarse, n_fine,
                                           float(near), float(far), hip.ptr(jitter), hip.ptr(ts), hip.stream())
        if rc == -2:       # TGTC_ERR_UNSUPPORTED
            raise ValueError("ray_kernel_depths: no depths-only ray kernel for this coarse precision and these sample counts")
        hip.check(rc)
        return ts

    def render_latents(self, rays_o, rays_d, n_coarse, n_fine, near=0., far=1., jitter=None, zs=None, min_weight=None,
                       style_precision=None, geometry=None):
        """The same rays under K latent sets in one call: zs float [K,R,32] -> dict rgb [K,R,3], t [R].

        The coarse pass, the fine depths and the fine NeRF trunk run once and are shared by the K images (one launch of
        the multi-latent kernel, csrc/mlp_style_multi.hip); rgb[k] and t are the bits of
        `RayRenderer(..., fused=False).render(..., z=zs[k])`.  Always the chain of per-sample kernels: `fused` has no say.
        The workspace holds K per-sample colour planes (369 MB per latent for a 400 x 400 frame at 128 + 64).

        min_weight=None is that call.  A float >= 0 takes tgtc_render_rays_styled_sparse instead: sigma of every fine sample
        first, then the NeRF trunk and the style networks only on the samples whose compositing weight exceeds min_weight
        (csrc/mlp_style_sparse.hip).  0 reproduces the images bit for bit; a positive value changes each ray by at most the
        sum of its dropped weights and leaves t alone.  The result then carries "live": the number of samples the style
        networks ran on, a device scalar (int32 view of the library's uint32) that is NOT synchronised.

        zs float [K,32] (with a min_weight): K latents that are the same for every ray.  Takes
        tgtc_render_rays_styled_sparse_folded: the latent columns of the style networks become K bias tables and the kernels
        run without the latent k-steps; no [K,R,32] plane exists.  Results differ from the [K,R,32] call with the rows
        repeated within the precision's error (zs = 0: bit for bit).  The dense multi-latent kernel has no such form: a
        2-D zs with min_weight=None is a ValueError.

        style_precision: None is the calls above.  "fp16mx" is the culled frame of the fp16x3+fp16mx pair in one call
        (tgtc_render_rays_styled_sparse_folded_mx): the geometry half as above, then trunk (fp16mx, the fine handle's own stream)
        and the K latents (the pair's fp16mx streams, packed at the first such call) of every tile of the list in one kernel.
        It needs zs [K,32], a min_weight, a fine handle in fp16mx and an fp16x3 style pair: anything else is a ValueError
        before any launch.  rgb, t are the bits of build_geometry(min_weight, keep_trunk=True, trunk_precision="fp16x3") +
        restyle(style_precision="fp16mx"), without the plane.  No default selects it.

        geometry: None is the calls above.  "chain" (with a min_weight; anything else is a ValueError before any launch) takes
        the ray-only half from the plain chain's passes instead of the ray kernel's first half and a dense sigma pass
        (tgtc_render_rays_styled_sparse_chain, in the form the other arguments select): coarse pass and sigma-only fine pass are
        screened as this renderer's `screen` says (apply_screen is called first; a fine handle in fp16x3 gets its screen too).
        Screened or not the results are the same bits, and t is the bits of `RayRenderer(..., fused=False).render(...)` without
        a style; against geometry=None the depths differ by the rounding between two coarse kernels.  No default selects it."""
        chain = self._check_geometry("render_latents", geometry, min_weight)
        if style_precision not in (None, "fp16mx"):
            raise ValueError("render_latents: style_precision is None or 'fp16mx', got %r" % (style_precision,))
        mx = style_precision == "fp16mx"
        if mx:
            if self.style is None or zs is None or zs.dim() != 2:
                raise ValueError("render_latents: style_precision='fp16mx' takes a style pair and frame-constant latents zs [K,32]")
            if min_weight is None:
                raise ValueError("render_latents: style_precision='fp16mx' needs a min_weight (the culled render)")
            if self.fine.packed().precision != "fp16mx" or self.style.packed().precision != "fp16x3":
                raise ValueError("render_latents: style_precision='fp16mx' needs a fine handle in fp16mx and an fp16x3 style pair "
                                 "(fine %s, pair %s)" % (self.fine.packed().precision, self.style.packed().precision))
        if zs is not None and zs.dim() == 2 and min_weight is None:
            raise ValueError("zs [K,32] (latents constant over the rays) needs a min_weight: the dense multi-latent kernel has "
                             "no folded form")
        hip.require_gpu(rays_o, rays_d, zs)
        lib = hip.load()
        if self.style is None or zs is None:
            raise ValueError("render_latents needs a style pair and zs [K,R,32] or [K,32]")
        if n_fine <= 0:
            raise ValueError("N_samples_fine must be > 0 (the reference render paths dereference None otherwise)")
        rays_o, rays_d, R, dev = self._rays(rays_o, rays_d)
        zs, K, folded = self._check_zs(zs, R)
        if min_weight is not None:
            min_weight = float(min_weight)
            if not min_weight >= 0:
                raise ValueError("min_weight must be >= 0 (got %r)" % min_weight)
            need = (lib.tgtc_render_styled_sparse_folded_workspace_bytes if folded else
                    lib.tgtc_render_styled_sparse_workspace_bytes)(R, n_coarse, n_fine, K)
        else:
            need = lib.tgtc_render_styled_multi_workspace_bytes(R, n_coarse, n_fine, K)
        ws = self._scratch("_ws_multi", need, dev)
        rgb = torch.empty(K, R, 3, device=dev, dtype=torch.float32)
        t = torch.empty(R, device=dev, dtype=torch.float32)
        jitter = self._jitter(jitter)
        if min_weight is not None:
            live = torch.zeros((), device=dev, dtype=torch.int32)
            call = lib.tgtc_render_rays_styled_sparse_folded if folded else lib.tgtc_render_rays_styled_sparse
            if mx:
                self.style.packed().enable_mx()                     # a no-op from the second call on
                call = lib.tgtc_render_rays_styled_sparse_folded_mx
            if chain:
                self.apply_screen(chain=True)
                form = 2 if mx else 1 if folded else 0
                call = lambda *a: lib.tgtc_render_rays_styled_sparse_chain(form, *a)
            hip.check(call(self.coarse.packed().handle, self.fine.packed().handle, self.style.packed().handle, hip.ptr(rays_o),
                           hip.ptr(rays_d), hip.ptr(zs), K, R, n_coarse, n_fine, float(near), float(far), hip.ptr(jitter),
                           min_weight, hip.ptr(ws), ws.numel(), hip.ptr(rgb), hip.ptr(t), hip.ptr(live), hip.stream()))
            return {"rgb": rgb, "t": t, "live": live}
        hip.check(lib.tgtc_render_rays_styled_multi(self.coarse.packed().handle, self.fine.packed().handle,
                                                    self.style.packed().handle, hip.ptr(rays_o), hip.ptr(rays_d), hip.ptr(zs), K,
                                                    R, n_coarse, n_fine, float(near), float(far), hip.ptr(jitter), hip.ptr(ws),
                                                    ws.numel(), hip.ptr(rgb), hip.ptr(t), hip.stream()))
        return {"rgb": rgb, "t": t}

    def build_geometry(self, rays_o, rays_d, n_coarse, n_fine, near=0., far=1., jitter=None, min_weight=0., key=None,
                       keep_trunk=False, trunk_precision=None, geometry=None):
        """Everything of `render_latents(..., min_weight=min_weight)` that depends on the rays alone -- coarse pass, fine
        depths, sigma pass, weights, compaction -- as a GeometryCache (about 12 bytes per live sample + 8 per ray).  The
        host reads the live count once here (one synchronisation per build); `restyle` has none.
        keep_trunk: also `build_trunk` the cache (1 KiB per live sample in fp16x3, 512 B in fp16); trunk_precision goes to
        `build_trunk`.
        geometry: None, or "chain" for the chain geometry of render_latents (tgtc_geometry_build_chain; anything else is a
        ValueError before any launch).  The cache is the one `render_latents(..., geometry="chain")` would use; `restyle`
        does not know which geometry built a cache."""
        chain = self._check_geometry("build_geometry", geometry, min_weight)
        hip.require_gpu(rays_o, rays_d)
        lib = hip.load()
        if n_fine <= 0:
            raise ValueError("N_samples_fine must be > 0 (the reference render paths dereference None otherwise)")
        min_weight = float(min_weight)
        if not min_weight >= 0:
            raise ValueError("min_weight must be >= 0 (got %r)" % min_weight)
        rays_o, rays_d, R, dev = self._rays(rays_o, rays_d)
        ws = self._scratch("_ws_multi", lib.tgtc_render_styled_sparse_workspace_bytes(R, n_coarse, n_fine, 1), dev)
        jitter = self._jitter(jitter)
        live = torch.zeros((), device=dev, dtype=torch.int32)
        if chain:
            self.apply_screen(chain=True)
        build = lib.tgtc_geometry_build_chain if chain else lib.tgtc_geometry_build
        hip.check(build(self.coarse.packed().handle, self.fine.packed().handle, hip.ptr(rays_o), hip.ptr(rays_d),
                        R, n_coarse, n_fine, float(near), float(far), hip.ptr(jitter), min_weight, hip.ptr(ws),
                        ws.numel(), None, hip.ptr(live), hip.stream()))
        count = int(live)
        buf = torch.zeros(lib.tgtc_geometry_cache_bytes(R, count), dtype=torch.uint8, device=dev)   # padding bytes: 0 in the file
        hip.check(lib.tgtc_geometry_pack(hip.ptr(ws), R, n_coarse, n_fine, min_weight, count, hip.ptr(buf), buf.numel(),
                                         hip.stream()))
        cache = GeometryCache(buf, R, n_coarse + n_fine, count, min_weight, key, n_coarse, n_fine)
        return self.build_trunk(cache, rays_o, rays_d, trunk_precision=trunk_precision) if keep_trunk else cache

    def build_trunk(self, cache, rays_o, rays_d, trunk_precision=None):
        """Give `cache` its trunk plane: the fine NeRF trunk once over the cached list (tgtc_geometry_trunk; no coarse pass,
        no sigma pass, no synchronisation), base_remap kept as the style kernels' operand fragments in the fine handle's
        precision.  `restyle` then needs no NeRF network for this cache.  rays_o / rays_d must be the rays of the build.
        Returns the cache.
        trunk_precision: None is that call.  "fp16x3" asks for an fp16x3 plane: from an fp16x3 fine handle the same call, from
        an fp16mx fine handle tgtc_geometry_trunk_mx -- the trunk in fp16mx, base_remap split into the fp16x3 plane's hi / lo
        fragments (`cache.trunk_source` is then "fp16mx"), which an fp16x3 style pair restyles from in fp16x3 or with
        style_precision="fp16mx".  Every other combination is a ValueError before any launch.  No default selects it."""
        from_mx = False
        if trunk_precision is not None:
            have = self.fine.packed().precision
            if trunk_precision != "fp16x3" or have not in ("fp16x3", "fp16mx"):
                raise ValueError("build_trunk: trunk_precision is None (the fine handle's own plane: fp16x3 or fp16) or 'fp16x3' "
                                 "with a fine handle in fp16x3 or fp16mx (got %r, fine handle in %s)" % (trunk_precision, have))
            from_mx = have == "fp16mx"
        hip.require_gpu(rays_o, rays_d, cache.buffer)
        lib = hip.load()
        if rays_o.shape[0] != cache.R:
            raise ValueError("build_trunk: %d rays, the cache holds %d" % (rays_o.shape[0], cache.R))
        rays_o, rays_d, _, dev = self._rays(rays_o, rays_d)
        fine = self.fine.packed()
        layout = "fp16x3" if from_mx else fine.precision
        plane = torch.empty(cache.trunk_nbytes(layout, cache.count), dtype=torch.uint8, device=dev)
        call = lib.tgtc_geometry_trunk_mx if from_mx else lib.tgtc_geometry_trunk
        hip.check(call(fine.handle, hip.ptr(rays_o), hip.ptr(rays_d), cache.R, cache.n_coarse, cache.n_fine,
                       hip.ptr(cache.buffer), cache.buffer.numel(), cache.count, hip.ptr(plane), plane.numel(), hip.stream()))
        cache.attach_trunk(plane, layout, fine.precision)
        return cache

    # (use_trunk, folded, mx) -> the library's restyle.  From the plane the plane consumers, which take no NeRF handle;
    # otherwise the list kernels behind the fine handle.  The fp16mx forms exist for frame-constant latents only.
    _RESTYLE = {(False, False, False): "tgtc_restyle_rays",
                (False, True, False): "tgtc_restyle_rays_folded",
                (False, True, True): "tgtc_restyle_rays_folded_mx",
                (True, False, False): "tgtc_restyle_rays_trunk",
                (True, True, False): "tgtc_restyle_rays_trunk_folded",
                (True, True, True): "tgtc_restyle_rays_trunk_folded_mx"}

    def restyle(self, cache, rays_o, rays_d, zs, key=None, n_coarse=None, n_fine=None, use_trunk=None, style_precision=None):
        """The rays of `cache` under K latent sets: zs float [K,R,32] -> dict rgb [K,R,3], t [R], live (the cache's count, a
        host int).  One launch of the compact indexed style kernel over the cached list and one compositing launch; the
        bits of `render_latents(..., min_weight=cache.min_weight)`.  rays_o / rays_d must be the rays the cache was built
        from (it stores depths, not positions).  ValueError before any launch if R, a given n_coarse + n_fine or a given
        `key` does not match the cache.
        zs float [K,32]: K latents that are the same for every ray, through tgtc_restyle_rays_folded (see render_latents);
        the same cache serves both forms.
        use_trunk: None takes the cache's trunk plane iff it carries one (`build_trunk`), False ignores it, True insists
        (ValueError without one).  From the plane the call is tgtc_restyle_rays_trunk[_folded]: the style networks alone, the
        same bits, and no NeRF network -- a renderer built with coarse=None, fine=None can make it.  ValueError before any
        launch if the plane was built in another precision than the style pair's.
        style_precision: None runs the style networks in the pair's own precision.  "fp16mx" runs them in fp16mx
        (tgtc_restyle_rays_trunk_folded_mx: one fp16 product and two block-scaled fp6 corrections instead of three fp16
        products; 1e-3 of float64 per sample instead of 5e-5) on a second pair of streams the fp16x3 pair packs at the first
        such call.  That form exists for zs [K,32] and an fp16x3 style pair only, from a cache with an fp16x3 trunk plane or --
        when the cache carries no plane, or use_trunk=False -- behind THIS RENDERER'S FINE HANDLE IN fp16mx
        (tgtc_restyle_rays_folded_mx: trunk and latents of a tile in one kernel, base_remap parked in the style handle's
        slab; no plane is allocated and `cache.trunk` is left alone; the bits of the plane path on a plane of
        build_trunk(trunk_precision="fp16x3")).  Anything else is a ValueError before any launch.  No default selects it."""
        if self.style is None:
            raise ValueError("restyle needs a style pair")
        if style_precision not in (None, "fp16mx"):
            raise ValueError("restyle: style_precision is None or 'fp16mx', got %r" % (style_precision,))
        mx = style_precision == "fp16mx"
        if mx:
            if zs.dim() != 2:
                raise ValueError("restyle: style_precision='fp16mx' takes frame-constant latents zs [K,32], got %s" % list(zs.shape))
            no_plane = use_trunk is False or cache.trunk is None
            if no_plane and (self.fine is None or self.fine.packed().precision != "fp16mx"):
                raise ValueError("restyle: style_precision='fp16mx' restyles from a trunk plane (build_trunk), or without one "
                                 "behind a fine handle in fp16mx")
            if no_plane and use_trunk:
                raise ValueError("restyle: use_trunk=True, but the cache carries no trunk plane (build_trunk)")
            if self.style.packed().precision != "fp16x3" or (not no_plane and cache.trunk_precision != "fp16x3"):
                raise ValueError("restyle: style_precision='fp16mx' needs an fp16x3 style pair and, with a plane, an fp16x3 trunk "
                                 "plane (plane %s, pair %s)" % (cache.trunk_precision, self.style.packed().precision))
        if use_trunk is None:
            use_trunk = cache.trunk is not None
        elif use_trunk and cache.trunk is None:
            raise ValueError("restyle: use_trunk=True, but the cache carries no trunk plane (build_trunk)")
        if use_trunk and cache.trunk_precision != self.style.packed().precision:
            raise ValueError("restyle: the trunk plane was built in %s, the style pair is packed in %s"
                             % (cache.trunk_precision, self.style.packed().precision))
        hip.require_gpu(rays_o, rays_d, zs, cache.buffer, cache.trunk if use_trunk else None)
        lib = hip.load()
        R = rays_o.shape[0]
        if R != cache.R:
            raise ValueError("restyle: %d rays, the cache holds %d" % (R, cache.R))
        if (n_coarse is not None or n_fine is not None) and (n_coarse, n_fine) != (cache.n_coarse, cache.n_fine):
            raise ValueError("restyle: %s + %s samples per ray, the cache was built with %s + %s"
                             % (n_coarse, n_fine, cache.n_coarse, cache.n_fine))
        if key is not None and key != cache.key:
            raise ValueError("restyle: the cache was built under another key")
        rays_o, rays_d, _, dev = self._rays(rays_o, rays_d)
        zs, K, folded = self._check_zs(zs, R)
        need = (lib.tgtc_restyle_folded_workspace_bytes if folded else lib.tgtc_restyle_workspace_bytes)(cache.count, K)
        ws = self._scratch("_ws_restyle", need, dev)
        rgb = torch.empty(K, R, 3, device=dev, dtype=torch.float32)
        t = torch.empty(R, device=dev, dtype=torch.float32)
        if mx:
            self.style.packed().enable_mx()                         # a no-op from the second call on
        call = getattr(lib, self._RESTYLE[bool(use_trunk), folded, mx])
        if use_trunk:
            hip.check(call(self.style.packed().handle, hip.ptr(rays_o), hip.ptr(rays_d), hip.ptr(zs), K, R, cache.n_coarse,
                           cache.n_fine, hip.ptr(cache.buffer), cache.buffer.numel(), cache.count, hip.ptr(cache.trunk),
                           cache.trunk.numel(), hip.ptr(ws), ws.numel(), hip.ptr(rgb), hip.ptr(t), hip.stream()))
        else:
            hip.check(call(self.fine.packed().handle, self.style.packed().handle, hip.ptr(rays_o), hip.ptr(rays_d), hip.ptr(zs), K,
                           R, cache.n_coarse, cache.n_fine, hip.ptr(cache.buffer), cache.buffer.numel(), cache.count, hip.ptr(ws),
                           ws.numel(), hip.ptr(rgb), hip.ptr(t), hip.stream()))
        return {"rgb": rgb, "t": t, "live": cache.count}


# =====================================================================================================
# Drop-in drivers with the reference's signatures (rendering.py:5, :93-94, :242-243).
#
# They accept the same injected callables and the same dataloader / dataset duck types as the reference
# (a dataloader yields dicts of tensors; `dataloader.dataset` carries cps / cps_valid / hwf / near / far /
# frame_num / h / w / mode).  With HIP-backed callables from this package every stage runs on the GPU; pass
# `renderer=RayRenderer(...)` to replace the per-stage chain by the fused single-call path.
# Unlike the reference they return cleanly and require N_samples_fine > 0 (Q2).
# =====================================================================================================
def _save_png(path, arr):
    """utils.py:463 to8b = uint8 cast.  The file is encoded and written by the background writer (image_writer.py);
    the drivers drain it before they return."""
    from .image_writer import writer
    writer().save(path, arr if isinstance(arr, torch.Tensor) else np.asarray(arr).astype(np.uint8))


def _drain_images():
    from .image_writer import writer
    writer().drain()


def _to_device(batch, device):
    return {k: torch.as_tensor(np.asarray(v) if not isinstance(v, torch.Tensor) else v).to(device) for k, v in batch.items()}


def _require_fine(args):
    if not args.N_samples_fine > 0:
        raise ValueError("N_samples_fine must be > 0: the reference's render paths dereference None otherwise "
                         "(rendering.py:186; train_tgtcs.py:184)")


# ---- multi-GPU hooks of the dataset duck type (train_tgtcs.ShardedScene; absent on reference-style datasets) --------
# A rank either owns whole images (frames sharding: it renders image k iff k % world == rank and writes its files
# itself) or a contiguous pixel range of EVERY image (rays sharding: the ranks' rows are all-gathered and rank 0
# writes).  The drivers only need: the global number of the i-th image this rank completes, how many rays of an
# image it renders, and how to assemble a finished image.
def _image_id(ds, local_no):
    return ds.global_image(local_no) if hasattr(ds, 'global_image') else local_no


def _local_res(ds, res):
    return ds.rays_per_image() if hasattr(ds, 'rays_per_image') else res


def _assemble(ds, rgb, t):
    """-> (rgb [h*w,3], t [h*w], this rank writes the files)"""
    return ds.assemble(rgb, t) if hasattr(ds, 'assemble') else (rgb, t, True)


def _write_depth_rgb(sv_path, rgb, t, h, w, rgb_name, depth_name, eps=1e-7, depth_channels=1):
    """rendering.py:202-217 (:358-361 for eps = 0, three depth channels): per-image min-max depth normalisation, x255,
    int32, uint8 cast.  CUDA tensors take the device epilogue (only the 8-bit images cross PCIe); numpy arrays the
    reference's own host arithmetic."""
    if isinstance(rgb, torch.Tensor) and rgb.is_cuda:
        from . import utils
        rgb8, depth8 = utils.frames_to_uint8(rgb, t, 1, eps)       # stay on the device: the writer copies them out
        rgb8, depth8 = rgb8.reshape(h, w, 3), depth8.reshape(h, w)
        if depth_channels == 3:
            depth8 = depth8.unsqueeze(-1).expand(h, w, 3).contiguous()
    else:
        rgb, t = np.asarray(rgb, np.float32), np.asarray(t, np.float32)
        with np.errstate(invalid="ignore", divide="ignore"):
            sv_t = (t - t.min()) / ((t.max() - t.min() + eps) if eps else (t.max() - t.min()))
            rgb8 = np.array(rgb.reshape(h, w, 3) * 255, np.int32).astype(np.uint8)
            depth8 = np.array(sv_t.reshape(h, w) * 255, np.int32).astype(np.uint8)
        if depth_channels == 3:
            depth8 = np.ascontiguousarray(np.broadcast_to(depth8[..., None], [h, w, 3]))
    _save_png(os.path.join(sv_path, rgb_name), rgb8)
    _save_png(os.path.join(sv_path, depth_name), depth8)


def cal_geometry(model_forward, samp_func, dataloader, args, device, sv_path=None, model_forward_fine=None,
                 samp_func_fine=None, renderer=None):
    """reference rendering.py:5-90: plain NeRF render of every ray the loader yields; writes rgb_%05d.png,
    depth_%05d.png, geometry_%05d.npz per image and geometry.npz; returns (rgb_map [F,h,w,3], t_map [F,h,w,1])."""
    from . import utils
    _require_fine(args)
    if sv_path is not None:
        os.makedirs(sv_path, exist_ok=True)
    ds = dataloader.dataset
    train = 'train' in ds.mode
    cps = ds.cps if train else ds.cps_valid
    frame_num, h, w = (ds.frame_num if train else ds.cps_valid.shape[0]), ds.h, ds.w
    res = h * w
    # frames sharding (train_tgtcs.ShardedScene): this rank renders the images k with k % world == rank, in that order
    world, rank = getattr(ds, 'world', 1), getattr(ds, 'rank', 0)
    if world > 1 and getattr(ds, 'shard', 'frames') != 'frames':
        raise ValueError("cal_geometry shards by whole frames (--shard frames): geometry_%05d.npz is a per-frame file")
    local_frames = len(range(rank, frame_num, world)) if world > 1 else frame_num
    rgb_map = np.zeros([local_frames * res, 3], np.float32)
    t_map = np.zeros([local_frames * res], np.float32)
    coor_map = np.zeros([local_frames * res, 3], np.float32)
    img_id = pixel_id = 0
    for batch in dataloader:
        b = _to_device(batch, device)
        rays_o, rays_d = b['rays_o'], b['rays_d']
        if renderer is not None:
            out = renderer.render(rays_o, rays_d, args.N_samples, args.N_samples_fine, near=ds.near, far=ds.far)
            rgb_f, t_f = out["rgb"], out["t"]
        else:
            pts, ts = samp_func(rays_o=rays_o, rays_d=rays_d, N_samples=args.N_samples, near=ds.near, far=ds.far)
            R = rays_o.shape[0]
            ret = model_forward(pts=pts, dirs=rays_d.unsqueeze(1).expand([R, args.N_samples, 3]))
            _, _, weights = utils.alpha_composition(ret['rgb'], ret['sigma'], ts, 0)
            pts_f, ts_f = samp_func_fine(rays_o, rays_d, ts, weights, args.N_samples_fine)
            n = args.N_samples + args.N_samples_fine
            ret = model_forward_fine(pts=pts_f, dirs=rays_d.unsqueeze(1).expand([R, n, 3]))
            rgb_f, t_f, _ = utils.alpha_composition(ret['rgb'], ret['sigma'], ts_f, 0)
        rgb_np, t_np = rgb_f.detach().cpu().numpy(), t_f.detach().cpu().numpy()
        coor = t_np[..., None] * rays_d.detach().cpu().numpy() + rays_o.detach().cpu().numpy()   # rendering.py:54
        n = coor.shape[0]
        rgb_map[pixel_id:pixel_id + n], t_map[pixel_id:pixel_id + n], coor_map[pixel_id:pixel_id + n] = rgb_np, t_np, coor
        pixel_id += n
        done = pixel_id // res - img_id
        if done > 0 and sv_path is not None:
            for i in range(img_id, img_id + done):
                sl = slice(i * res, (i + 1) * res)
                gid = _image_id(ds, i)
                _write_depth_rgb(sv_path, rgb_map[sl], t_map[sl], h, w, 'rgb_%05d.png' % gid, 'depth_%05d.png' % gid)
                np.savez(os.path.join(sv_path, 'geometry_%05d' % gid), coor_map=coor_map[sl].reshape(h, w, 3),
                         cps=cps[gid], hwf=ds.hwf, near=ds.near, far=ds.far)
        img_id += max(done, 0)
    rgb_map, t_map = rgb_map.reshape(-1, h, w, 3), t_map.reshape(-1, h, w, 1)
    _drain_images()
    if sv_path is not None:
        if world > 1:
            # the scene-wide file: rank 0 puts the per-frame files of all ranks together (one node, one file system)
            ds.dist.barrier()
            if rank == 0:
                whole = np.stack([np.load(os.path.join(sv_path, 'geometry_%05d.npz' % k))['coor_map'] for k in range(frame_num)])
                np.savez(os.path.join(sv_path, 'geometry'), coor_map=whole, cps=cps, hwf=ds.hwf, near=ds.near, far=ds.far)
            ds.dist.barrier()
        else:
            np.savez(os.path.join(sv_path, 'geometry'), coor_map=coor_map.reshape(-1, h, w, 3), cps=cps, hwf=ds.hwf,
                     near=ds.near, far=ds.far)
    return rgb_map, t_map


def _styled_batch(b, args, ds, samp_func, model_forward, style_forward, concat_style_forward, latents_model_1,
                  model_forward_fine, samp_func_fine, renderer, min_weight=None):
    """One batch of the stylised chain (rendering.py:118-178 == :280-327).  min_weight: RayRenderer.render's."""
    from . import utils
    rays_o, rays_d = b['rays_o'], b['rays_d']
    z = latents_model_1(style_ids=b['style_id'].long(), frame_ids=b['frame_id'].long(), type=args.dataset_type)
    if renderer is not None:
        # stratified jitter (utils.py:518-524, perturb=True at rendering.py:118,280): the reference draws it per batch;
        # a dataset may deliver it per ray instead, so that the image does not depend on batching or sharding
        jitter = b['jitter'] if 'jitter' in b else torch.rand(rays_o.shape[0], args.N_samples, device=rays_o.device)
        out = renderer.render(rays_o, rays_d, args.N_samples, args.N_samples_fine, near=ds.near, far=ds.far,
                              jitter=jitter, z=z, min_weight=min_weight)
        return out["rgb"], out["t"]
    if min_weight is not None:
        raise ValueError("min_weight needs renderer=RayRenderer(...): the per-stage chain has no culled form")
    R, L = rays_o.shape[0], z.shape[-1]
    zbar = torch.mean(z, dim=1, keepdim=True)                      # rendering.py:126

    def one_pass(fwd, pts, n):
        ret = fwd(pts=pts, dirs=rays_d.unsqueeze(1).expand([R, n, 3]))
        cf = concat_style_forward(x=ret['pts'], latent=z.unsqueeze(1).expand([R, n, L]))['concat_features']
        both = torch.cat((ret['base_remap'], cf), dim=-1)           # rendering.py:132
        rgb = style_forward(x=ret['pts'], concated=both, latent=zbar.unsqueeze(2).expand([R, n, L]))['rgb']
        return rgb, ret['sigma']

    pts, ts = samp_func(rays_o=rays_o, rays_d=rays_d, N_samples=args.N_samples, near=ds.near, far=ds.far, perturb=True)
    rgb, sig = one_pass(model_forward, pts, args.N_samples)
    _, _, weights = utils.alpha_composition(rgb, sig, ts, 0)
    pts_f, ts_f = samp_func_fine(rays_o, rays_d, ts, weights, args.N_samples_fine)
    rgb, sig = one_pass(model_forward_fine, pts_f, args.N_samples + args.N_samples_fine)
    rgb_f, t_f, _ = utils.alpha_composition(rgb, sig, ts_f, 0)
    return rgb_f, t_f


def _geometry_key(ds, args, renderer, fid, p0, p1, min_weight, tag):
    """What the geometry of pixels [p0, p1) of validation frame `fid` depends on, as one hex digest: pose, intrinsics, frame
    size, pixel range, sample counts, near / far, the frame's jitter seed, the NeRF precisions, min_weight and the caller's
    tag (train_tgtcs passes the NeRF checkpoint step)."""
    import hashlib
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(ds.cps_valid[fid], np.float64).tobytes())
    h.update(np.ascontiguousarray(np.asarray(ds.hwf, np.float64)).tobytes())
    h.update(repr((int(ds.h), int(ds.w), int(p0), int(p1), int(args.N_samples), int(args.N_samples_fine), float(ds.near),
                   float(ds.far), int(getattr(ds, 'jitter_seed', 0)), int(getattr(ds, 'jitter_samples', 0)), int(fid),
                   renderer.coarse.packed().precision, renderer.fine.packed().precision, float(min_weight), tag)).encode())
    return h.hexdigest()


def _cached_geometry(renderer, directory, name, key, build):
    """The GeometryCache in `directory`/`name` if it is there and carries `key`, else `build()` saved under that name."""
    path = os.path.join(directory, name)
    if os.path.exists(path):
        try:
            cache = GeometryCache.load(path, torch.device("cuda", torch.cuda.current_device()))
            if cache.key == key:
                return cache
        except (ValueError, KeyError, RuntimeError, EOFError):
            pass                        # unreadable or stale: rebuilt below
    cache = build()
    tmp = path + ".tmp%d" % os.getpid()
    cache.save(tmp)
    os.replace(tmp, path)
    return cache


def _render_style_shared(latents_model_1, dataloader, args, device, sv_path, renderer, min_weight=None, geometry_cache=None,
                         geometry_tag=None, fold_latents=False, style_precision=None, geometry=None):
    """render_style with share_geometry: walk the FRAMES of the validation path and render all styles of a frame in one
    `RayRenderer.render_latents` call (shared coarse pass, fine depths and fine NeRF trunk), under the jitter of the frame's
    style-0 image.  Same file names as the per-image walk.  The dataset supplies the frames through its `frame_batches`
    hook (train_tgtcs.SyntheticScene): the rays this rank renders of each frame it takes part in -- its pixel range of
    every frame under rays sharding, whole frames dealt round-robin under frames sharding.
    min_weight: RayRenderer.render_latents' (None: the style networks run on every sample).
    geometry_cache: a directory of GeometryCache files, one per (frame, pixel range of a call).  A file with a matching key is
    loaded and the call becomes `RayRenderer.restyle`; otherwise the geometry is built, saved there and restyled.  The
    images are those of min_weight (None counts as 0) without the cache, bit for bit.
    fold_latents: the latent model is evaluated on ONE row per style and the calls take zs [K,32] (RayRenderer.render_latents /
    restyle: the folded kernels); needs a min_weight or a geometry_cache, and every ray of a call in the same frame.
    style_precision: None, or "fp16mx" for a renderer whose fine handle is in fp16mx (fold_latents only): handed to
    RayRenderer.render_latents, or with a geometry_cache to RayRenderer.restyle on a cache without a plane.  The geometry key
    does not change: it describes the NeRF half only.
    geometry: None, or "chain" (needs a min_weight or a geometry_cache): RayRenderer.render_latents' / build_geometry's.  The
    tag of the cache keys gains "geometry=chain", so a directory never serves a cache of one geometry to a run of the other."""
    ds = dataloader.dataset
    if geometry not in (None, "chain"):
        raise ValueError("geometry is None or 'chain', got %r" % (geometry,))
    if geometry is not None and min_weight is None and geometry_cache is None:
        raise ValueError("geometry='chain' needs a min_weight or a geometry_cache (it is the geometry of the culled render)")
    if geometry is not None:
        geometry_tag = "%s geometry=%s" % (geometry_tag, geometry)
    if style_precision is not None and not fold_latents:
        raise ValueError("style_precision needs fold_latents (the fp16mx style kernels take zs [K,32])")
    if renderer is None or not hasattr(ds, 'frame_batches'):
        raise ValueError("share_geometry needs renderer=RayRenderer(...) and a dataset with the frame_batches hook")
    if fold_latents and min_weight is None and geometry_cache is None:
        raise ValueError("fold_latents needs a min_weight or a geometry_cache (the dense multi-latent kernel has no folded form)")
    frame_num, h, w, styles = ds.cps_valid.shape[0], ds.h, ds.w, ds.style_num
    res = _local_res(ds, h * w)
    nt = args.N_samples + args.N_samples_fine
    # rays per call: K x R x nt samples stay below 2^31 and the per-sample colour of a call below 2 GiB
    per_call = max(1, min(((1 << 31) - 1) // (styles * nt), (2 << 30) // (styles * nt * 12)))
    rgbs, ts, have = [], [], 0
    mode = {} if style_precision is None else {"style_precision": style_precision}
    chain = {} if geometry is None else {"geometry": geometry}
    if geometry_cache is not None:
        os.makedirs(geometry_cache, exist_ok=True)
        min_weight = 0. if min_weight is None else float(min_weight)
        first_pixel = ds._pixels()[0] if hasattr(ds, '_pixels') else 0
    for batch in ds.frame_batches(dataloader.batch_size):
        b = _to_device(batch, device)
        fid = int(b['frame_id'][0])
        R = b['rays_o'].shape[0]
        for lo in range(0, R, per_call):
            sl = slice(lo, min(lo + per_call, R))
            frame_ids = b['frame_id'][sl].long()
            if fold_latents:
                if not bool((frame_ids == frame_ids[0]).all()):
                    raise ValueError("fold_latents: the rays of a call belong to more than one frame")
                one = frame_ids[:1]
                zs = torch.cat([latents_model_1(style_ids=torch.full_like(one, sid), frame_ids=one, type=args.dataset_type)
                                for sid in range(styles)])       # [K,32]
            else:
                zs = torch.stack([latents_model_1(style_ids=torch.full_like(frame_ids, sid), frame_ids=frame_ids,
                                                  type=args.dataset_type) for sid in range(styles)])
            jitter = b['jitter'][sl] if 'jitter' in b else torch.rand(frame_ids.shape[0], args.N_samples, device=device)
            if geometry_cache is not None:
                if 'jitter' not in b:
                    raise ValueError("geometry_cache needs a dataset that delivers its jitter per ray (a cached geometry "
                                     "fixes the sample positions; a fresh draw per call would not be reproduced)")
                p0, p1 = first_pixel + have + sl.start, first_pixel + have + sl.stop
                key = _geometry_key(ds, args, renderer, fid, p0, p1, min_weight, geometry_tag)
                ro, rd = b['rays_o'][sl], b['rays_d'][sl]
                cache = _cached_geometry(renderer, geometry_cache, 'geometry_%05d_%09d_%09d.pt' % (fid, p0, p1), key,
                                         lambda: renderer.build_geometry(ro, rd, args.N_samples, args.N_samples_fine, near=ds.near,
                                                                         far=ds.far, jitter=jitter, min_weight=min_weight, key=key,
                                                                         **chain))
                out = renderer.restyle(cache, ro, rd, zs, key=key, n_coarse=args.N_samples, n_fine=args.N_samples_fine,
                                       **mode)
            else:
                out = renderer.render_latents(b['rays_o'][sl], b['rays_d'][sl], args.N_samples, args.N_samples_fine,
                                              near=ds.near, far=ds.far, jitter=jitter, zs=zs, min_weight=min_weight, **mode,
                                              **chain)
            rgbs.append(out["rgb"].detach()), ts.append(out["t"].detach())
        have += R
        if have == res:           # a frame (this rank's part of it) is complete
            rgb_all, t_all = torch.cat(rgbs, 1), torch.cat(ts, 0)
            for sid in range(styles):
                rgb_img, t_img, writer = _assemble(ds, rgb_all[sid].contiguous(), t_all)
                if sv_path is not None and writer:
                    _write_depth_rgb(sv_path, rgb_img, t_img, h, w, 'style_%05d_fine_%05d.png' % (sid, fid),
                                     'style_%05d_fine_depth_%05d.png' % (sid, fid))
            rgbs, ts, have = [], [], 0
    _drain_images()
    return np.zeros([0, 3], np.float32), np.zeros([0], np.float32)


def render_style(model_forward, samp_func, style_forward, concat_style_forward, latents_model_1, dataloader, args,
                 device, sv_path=None, model_forward_fine=None, samp_func_fine=None, sigma_scale=0., renderer=None,
                 share_geometry=False, min_weight=None, geometry_cache=None, geometry_tag=None, fold_latents=False,
                 style_precision=None, geometry=None):
    """reference rendering.py:93-239: stylised render of the `valid_style` rays; one
    style_%05d_fine_%05d.png + style_%05d_fine_depth_%05d.png pair per completed frame.
    Returns (rgb_map_fine, t_map_fine) = the rays left over after the last whole image, like the reference.
    share_geometry=True (not in the reference): all styles of a frame in one multi-latent call, see _render_style_shared.
    min_weight (not in the reference; needs `renderer`): the style networks only on the fine samples whose compositing
    weight exceeds it, see RayRenderer.render_latents; None runs them on every sample.
    geometry_cache (share_geometry only): a directory in which the ray-only half of every call is kept and reused, see
    _render_style_shared; geometry_tag: a string that goes into the cache keys (what the driver cannot see, e.g. the NeRF
    checkpoint step); fold_latents (share_geometry only): one latent per (style, frame), see _render_style_shared;
    style_precision (share_geometry with fold_latents only): "fp16mx", see _render_style_shared;
    geometry (share_geometry with a min_weight or a geometry_cache only): "chain", see _render_style_shared."""
    _require_fine(args)
    if geometry is not None and not share_geometry:
        raise ValueError("geometry needs share_geometry=True")
    if style_precision is not None and not (share_geometry and fold_latents):
        raise ValueError("style_precision needs share_geometry=True and fold_latents=True")
    if geometry_cache is not None and not share_geometry:
        raise ValueError("geometry_cache needs share_geometry=True (the cache belongs to the walk by frames)")
    if fold_latents and not share_geometry:
        raise ValueError("fold_latents needs share_geometry=True (one latent per style and frame belongs to the walk by frames)")
    latents_model_1.sigma_scale = sigma_scale
    if sv_path is not None:
        os.makedirs(sv_path, exist_ok=True)
    ds = dataloader.dataset
    ds.mode = 'valid_style'
    if share_geometry:
        return _render_style_shared(latents_model_1, dataloader, args, device, sv_path, renderer, min_weight=min_weight,
                                    geometry_cache=geometry_cache, geometry_tag=geometry_tag, fold_latents=fold_latents,
                                    style_precision=style_precision, geometry=geometry)
    frame_num, h, w = ds.cps_valid.shape[0], ds.h, ds.w
    res = _local_res(ds, h * w)
    pend_rgb, pend_t, image_no = torch.zeros([0, 3], device=device), torch.zeros([0], device=device), 0
    for batch in dataloader:
        b = _to_device(batch, device)
        rgb_f, t_f = _styled_batch(b, args, ds, samp_func, model_forward, style_forward, concat_style_forward,
                                   latents_model_1, model_forward_fine, samp_func_fine, renderer, min_weight=min_weight)
        pend_rgb = torch.cat([pend_rgb, rgb_f.detach().float()], 0)      # stays on the device until a frame is complete
        pend_t = torch.cat([pend_t, t_f.detach().float()], 0)
        while pend_rgb.shape[0] >= res:
            rgb_img, t_img, writer = _assemble(ds, pend_rgb[:res], pend_t[:res])
            if sv_path is not None and writer:
                # file numbering: images are consecutive (style, frame) pairs (rendering.py:209-218)
                gid = _image_id(ds, image_no)
                _write_depth_rgb(sv_path, rgb_img, t_img, h, w,
                                 'style_%05d_fine_%05d.png' % (gid // frame_num, gid % frame_num),
                                 'style_%05d_fine_depth_%05d.png' % (gid // frame_num, gid % frame_num))
            image_no += 1
            pend_rgb, pend_t = pend_rgb[res:], pend_t[res:]
    _drain_images()
    return pend_rgb.cpu().numpy(), pend_t.cpu().numpy()


def render_train_style(samp_func, model_forward, style_forward, concat_style_forward, latents_model_1, dataset, args,
                       device, sv_path=None, model_forward_fine=None, samp_func_fine=None, sigma_scale=0.,
                       renderer=None, min_weight=None):
    """reference rendering.py:242-375: stylised render of the training views in `train_style` order; the batch is the
    largest divisor of h*w not above --chunk (:251-253); images already on disk are skipped (:267-270); RGB is clamped
    to [0,1] (:328); depth is min-max normalised without epsilon and written as 3 channels (:358-361).
    min_weight: as in render_style."""
    _require_fine(args)
    os.makedirs(sv_path, exist_ok=True)
    latents_model_1.sigma_scale = sigma_scale
    frame_num, h, w = dataset.frame_num, dataset.h, dataset.w
    dataset.mode = 'train_style'
    batch_size = args.chunk
    local = _local_res(dataset, h * w)
    while local % batch_size != 0:
        batch_size -= 1
    iters_per_image = local // batch_size
    loader = dataset.batches(batch_size) if hasattr(dataset, 'batches') else torch.utils.data.DataLoader(
        dataset, shuffle=False, batch_size=batch_size, num_workers=getattr(args, 'num_workers', 0))
    it = img_count = 0
    rgbs, ts = [], []
    for batch in loader:
        gid = _image_id(dataset, img_count)
        path = os.path.join(sv_path, 'style_%05d_fine_%05d.png' % (gid // frame_num, gid % frame_num))
        # (rays sharding: every rank must take the same decision, or the all-gather of a frame would hang)
        exists = os.path.exists(path) and not (getattr(dataset, 'world', 1) > 1 and getattr(dataset, 'shard', '') == 'rays')
        if not exists:
            b = _to_device(batch, device)
            rgb_f, t_f = _styled_batch(b, args, dataset, samp_func, model_forward, style_forward, concat_style_forward,
                                       latents_model_1, model_forward_fine, samp_func_fine, renderer, min_weight=min_weight)
            rgbs.append(torch.clamp(rgb_f, 0., 1.).detach())
            ts.append(t_f.detach())
        it += 1
        if it == iters_per_image:
            if not exists:
                rgb_img, t_img, writer = _assemble(dataset, torch.cat(rgbs, 0), torch.cat(ts, 0))
                if writer:
                    _write_depth_rgb(sv_path, rgb_img, t_img, h, w, os.path.basename(path),
                                     os.path.basename(path).replace('_fine_', '_fine_depth_'), eps=0., depth_channels=3)
            img_count += 1
            it, rgbs, ts = 0, [], []
    _drain_images()
    return img_count
