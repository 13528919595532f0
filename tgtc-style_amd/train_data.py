"""Data side of `Origin_train` (train_loop.py): the reference's `RaySampler` + `DataLoader(shuffle=True)`
(dataset.py:63-144, train_tgtcs.py:110-113,160) without the host ray tables.

The reference stores float64 `rays_o` / `rays_d` of every pixel of every training frame (0.6 GB for fern at factor 4) and
its loader gathers `batch_size` shuffled rows of them, and of the images, on the host per iteration.  Here the device
holds the images (float32 [F,H,W,3], what llff_images.load_images returns) and the cameras ([F,12]); a batch is the
shuffled indices (`EpochSampler`, drawn on the device) through ONE launch of `tgtc_train_batch` (csrc/train_batch.hip),
which computes each row's ray from its frame's camera with the bits of `utils.gen_rays` and copies its colour.

Data side of `Style_train` (train_loop.style_train): the reference's `StyleRaySampler_gen` and its two `LightDataLoader`s
(dataset.py:398-539, :641-779).  `StyleTrainRays` adds the stylised frames as a uint8 table; `CoherenceCursor` is the
frame-ordered loader's integer state; both batches of an iteration are ONE launch of `tgtc_style_train_batch`
(csrc/style_train_batch.hip).
"""
import os

import numpy as np
import torch

from . import hip

_MASK63 = (1 << 63) - 1


def images_dir_factor(datadir, factor):
    """How `factor` is spelt in the scene's `images_<factor>/`: an integral factor as an integer (`images_4`, the LLFF
    convention), unless only the directory of the float spelling exists (`images_4.0`, which the reference's
    `'_{}'.format(args.factor)` makes of its float flag, load_llff.py:70)."""
    if float(factor).is_integer():
        as_int = int(factor)
        if not os.path.isdir(os.path.join(datadir, "images_{}".format(as_int))) and \
                os.path.isdir(os.path.join(datadir, "images_{}".format(float(factor)))):
            return float(factor)
        return as_int
    return factor


def missing_scene_parts(datadir, factor):
    """What a real `--datadir` lacks for training, as a list of names (empty: complete)."""
    missing = []
    if not os.path.exists(os.path.join(datadir, "poses_bounds.npy")):
        missing.append("poses_bounds.npy")
    f = images_dir_factor(datadir, factor)
    if not (os.path.isdir(os.path.join(datadir, "images")) or os.path.isdir(os.path.join(datadir, "images_{}".format(f)))):
        missing.append("images/ or images_{}/".format(f))
    return missing


class TrainRays:
    """The training views of one scene on `device`: `images` float32 [F,H,W,3], `c2w` float32 [F,12] (3x4 row-major per
    frame), `hwf`, `near` / `far` (0 / 1 under NDC).  `batch(index)` -> rays_o, rays_d float64 [R,3], rgb_gt float32 [R,3]
    of the flat indices frame * H * W + row * W + col (dataset.py:137-144)."""

    def __init__(self, images, cps, hwf, device, near=0., far=1., ndc=True, pixel_alignment=False):
        images = np.ascontiguousarray(images, dtype=np.float32)
        cps = np.asarray(cps, dtype=np.float32)
        self.h, self.w, self.f = int(hwf[0]), int(hwf[1]), float(hwf[2])
        self.hwf = [self.h, self.w, self.f]
        if images.ndim != 4 or images.shape[1:] != (self.h, self.w, 3) or cps.shape[0] != images.shape[0]:
            raise ValueError("TrainRays: images %s do not match %d cameras of %d x %d" % (images.shape, cps.shape[0], self.h, self.w))
        self.frame_num = images.shape[0]
        self.cps = cps
        self.device = torch.device(device)
        self.images = torch.from_numpy(images).to(self.device)
        self.c2w = torch.from_numpy(np.ascontiguousarray(cps[:, :3, :4]).reshape(self.frame_num, 12)).to(self.device)
        self.near, self.far, self.ndc, self.pixel_alignment = float(near), float(far), bool(ndc), bool(pixel_alignment)
        self.rays_num = self.frame_num * self.h * self.w

    @classmethod
    def from_llff(cls, datadir, factor, device, no_ndc=False, pixel_alignment=False):
        """A real LLFF scene (dataset.py:69-134): every frame trains.  Images and the (H, W, focal) patched into the pose
        table from llff_images.load_data, the recentred cameras from llff_poses.scene_poses."""
        from . import llff_images, llff_poses
        f = images_dir_factor(datadir, factor)
        poses, _, imgs = llff_images.load_data(datadir, f)
        images = np.moveaxis(imgs, -1, 0).astype(np.float32)                       # llff_images.load_images
        h, w = int(poses[0, 4, 0]), int(poses[1, 4, 0])
        sc = llff_poses.scene_poses(np.load(os.path.join(datadir, "poses_bounds.npy")), (h, w), factor=f)
        if no_ndc:
            near, far = float(sc["bds"].min() * .9), float(sc["bds"].max() * 1.)   # dataset.py:76-78
        else:
            near, far = 0., 1.
        return cls(images, sc["poses"][:, :3, :4], sc["hwf"], device, near=near, far=far, ndc=not no_ndc,
                   pixel_alignment=pixel_alignment)

    @classmethod
    def from_synthetic(cls, args, device, frames=20):
        """The teacher scene of `--synthetic`: the `frames` training cameras of train_tgtcs.SyntheticScene at
        --synthetic_hw, each rendered once by the plain RayRenderer from synth.nerf_state(0) / (1), jitter off."""
        from . import models, rendering, synth, utils
        hw = args.synthetic_hw
        focal = synth.fern_intrinsics(hw, hw)
        cps = np.stack([synth.spiral_pose(7 * i) for i in range(frames)])          # SyntheticScene.cps
        to_t = lambda sd: {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}
        teacher = []
        for seed, mode in ((0, 'coarse'), (1, 'fine')):
            m = models.StyleNerf(args, mode=mode)
            m.load_state_dict(to_t(synth.nerf_state(seed)))
            teacher.append(m.to(device))
        renderer = rendering.RayRenderer(*teacher)
        images = np.empty((frames, hw, hw, 3), np.float32)
        with torch.no_grad():
            for i in range(frames):
                o, d = utils.gen_rays(hw, hw, focal, cps[i], pixel_alignment=args.pixel_alignment, device=device)
                images[i] = renderer.render(o, d, args.N_samples, args.N_samples_fine, near=0., far=1.)["rgb"] \
                    .reshape(hw, hw, 3).cpu().numpy()
        return cls(images, cps, [hw, hw, focal], device, pixel_alignment=args.pixel_alignment)

    def batch(self, index):
        """index int64 [R] on the device -> (rays_o, rays_d, rgb_gt) through tgtc_train_batch.  An index outside
        [0, F*H*W) gives NaN rays and zero colour (the kernel reads nothing for it)."""
        hip.require_gpu(self.images, self.c2w, index)
        if index.dtype != torch.int64:
            raise TypeError("TrainRays.batch: int64 indices, got %s" % index.dtype)
        index = index.contiguous()
        R = index.shape[0]
        o = torch.empty(R, 3, device=self.device, dtype=torch.float64)
        d = torch.empty(R, 3, device=self.device, dtype=torch.float64)
        rgb = torch.empty(R, 3, device=self.device, dtype=torch.float32)
        hip.check(hip.load().tgtc_train_batch(self.h, self.w, self.f, self.f, 0.5 * self.w, 0.5 * self.h, hip.ptr(self.c2w),
                                              self.frame_num, hip.ptr(self.images), hip.ptr(index), R,
                                              int(self.pixel_alignment), int(self.ndc), 1.0, hip.ptr(o), hip.ptr(d),
                                              hip.ptr(rgb), hip.stream()))
        return o, d, rgb


def _stylise(images, style):
    """The stylised copy `style` of the synthetic teacher frames: a fixed colour transform per style (seeded by the style
    number alone) -- the channels rotated by style + 1 places, mixed by a random row-stochastic matrix, shifted and
    inverted in one channel -- quantised to uint8 like the JPEGs of the 2-D pass.  Never the identity."""
    rng = np.random.default_rng(7001 + style)
    mix = 0.55 * np.roll(np.eye(3), style + 1, axis=1) + 0.45 * rng.dirichlet(np.ones(3), 3)
    shift = rng.uniform(-0.08, 0.08, 3)
    out = images.astype(np.float64) @ mix.T + shift
    k = style % 3
    out[..., k] = 1.0 - out[..., k]
    return np.round(np.clip(out, 0., 1.) * 255.).astype(np.uint8)


class StyleTrainRays(TrainRays):
    """The data of `Style_train` on `device` (the reference's StyleRaySampler_gen, dataset.py:398-539): what TrainRays
    holds -- `images` are the un-stylised colours (rgb_origin), the frames `--render_train` wrote -- plus `stylized`, the
    uint8 [S,F,H,W,3] table of collect_all_stylized_images (11 MB per style for fern at factor 4), and `style_num`.
    `batch(index, coh)` is ONE launch of tgtc_style_train_batch (csrc/style_train_batch.hip) for both batches of an
    iteration."""

    def __init__(self, images, stylized, cps, hwf, device, **kw):
        super().__init__(images, cps, hwf, device, **kw)
        stylized = np.ascontiguousarray(stylized)
        if stylized.dtype != np.uint8 or stylized.ndim != 5 or stylized.shape[1:] != (self.frame_num, self.h, self.w, 3):
            raise ValueError("StyleTrainRays: stylised table %s %s is not uint8 [S,%d,%d,%d,3]" % (
                stylized.dtype, stylized.shape, self.frame_num, self.h, self.w))
        self.style_num = stylized.shape[0]
        self.stylized = torch.from_numpy(stylized).to(self.device)
        self.data_num = self.style_num * self.rays_num               # dataset.py:636-637

    @classmethod
    def from_synthetic(cls, args, device, frames=20):
        """The teacher frames of TrainRays.from_synthetic as rgb_origin and --synthetic_styles stylised copies of them
        (`_stylise`)."""
        base = TrainRays.from_synthetic(args, device, frames=frames)
        images = base.images.cpu().numpy()
        stylized = np.stack([_stylise(images, s) for s in range(max(1, args.synthetic_styles))])
        return cls(images, stylized, base.cps, base.hwf, device, pixel_alignment=args.pixel_alignment)

    @classmethod
    def from_directories(cls, datadir, factor, gen_path, device, no_ndc=False, pixel_alignment=False):
        """The reference's layout (dataset.py:398-481): cameras from <datadir>/poses_bounds.npy (llff_poses.scene_poses, as
        from_llff), rgb_origin from <gen_path>/rgb_*.png sorted (what --render_train writes), the style from
        <datadir>/stylized_gen_<factor>/stylized_data.npz and its stylised frames NNN.jpg counted from 001 beside it.  The
        layout holds ONE style per directory (the reference's `style_paths` has one entry, dataset.py:458): a
        stylized_data.npz that declares more is refused.  SystemExit names whatever is missing or does not fit."""
        import glob
        from PIL import Image
        from . import llff_poses, trans_test
        no = lambda what: SystemExit("train_tgtcs: --style_train needs %s" % what)
        pb = os.path.join(datadir, "poses_bounds.npy")
        if not os.path.exists(pb):
            raise no("the cameras of the scene: no poses_bounds.npy in --datadir %s" % datadir)
        files = sorted(glob.glob(os.path.join(gen_path, "rgb_*.png")))
        if not files:
            raise no("the rendered training views: no rgb_*.png in %s (run --render_train first)" % gen_path)
        style_dir = os.path.join(datadir, "stylized_gen_" + str(factor))
        sd = trans_test.read_stylized_data(datadir, factor)
        if sd is None:
            raise no("the 2-D pass's style data: no %s" % os.path.join(style_dir, "stylized_data.npz"))
        if sd["style_num"] != 1 or len(np.atleast_1d(sd["style_paths"])) > 1:
            raise no("one style per directory, the reference's layout (its style_paths has one entry): %s declares %d "
                     "styles" % (os.path.join(style_dir, "stylized_data.npz"), max(sd["style_num"], len(np.atleast_1d(sd["style_paths"])))))
        arr = np.load(pb)
        h0, w0 = arr[0, :15].reshape(3, 5)[:2, 4]
        sc = llff_poses.scene_poses(arr, (int(h0 // factor), int(w0 // factor)), factor=factor)   # as the scene --render_train rendered
        h, w = int(sc["hwf"][0]), int(sc["hwf"][1])
        frames = sc["poses"].shape[0]
        if len(files) != frames:
            raise no("one rendered view per camera: %d rgb_*.png in %s, %d cameras in poses_bounds.npy" % (len(files), gen_path, frames))

        def read(path):
            a = np.array(Image.open(path).convert("RGB"), np.uint8)
            if a.shape != (h, w, 3):
                raise no("images of %d x %d: %s is %d x %d" % (h, w, path, a.shape[0], a.shape[1]))
            return a

        images = np.stack([read(f).astype(np.float32) / 255. for f in files])                # dataset.py:407
        stylized = np.empty((1, frames, h, w, 3), np.uint8)
        for j in range(frames):
            path = os.path.join(style_dir, "%03d.jpg" % (j + 1))                              # dataset.py:480
            if not os.path.exists(path):
                raise no("a stylised frame per camera: no %s" % path)
            stylized[0, j] = read(path)
        if no_ndc:
            near, far = float(sc["bds"].min() * .9), float(sc["bds"].max() * 1.)
        else:
            near, far = 0., 1.
        return cls(images, stylized, sc["poses"][:, :3, :4], sc["hwf"], device, near=near, far=far, ndc=not no_ndc,
                   pixel_alignment=pixel_alignment)

    def batch(self, index, coh=None):
        """index int64 [R] on the device: shuffled rows s*F*H*W + f*H*W + p (dataset.py:498-502); coh = (style, frame,
        start, n): the frame-ordered rows appended after them (CoherenceCursor).  -> dict rays_o, rays_d float64 [R+n,3],
        rgb_gt, rgb_origin float32 [R+n,3], style_id, frame_id int64 [R+n].  An index outside [0, S*F*H*W) gives NaN rays,
        zero colours and ids -1."""
        hip.require_gpu(self.images, self.stylized, self.c2w, index)
        if index.dtype != torch.int64:
            raise TypeError("StyleTrainRays.batch: int64 indices, got %s" % index.dtype)
        index = index.contiguous()
        R = index.shape[0]
        cs, cf, ca, n = (0, 0, 0, 0) if coh is None else (int(v) for v in coh)
        T = R + n
        f64 = lambda: torch.empty(T, 3, device=self.device, dtype=torch.float64)
        f32 = lambda: torch.empty(T, 3, device=self.device, dtype=torch.float32)
        i64 = lambda: torch.empty(T, device=self.device, dtype=torch.int64)
        out = {'rays_o': f64(), 'rays_d': f64(), 'rgb_gt': f32(), 'rgb_origin': f32(), 'style_id': i64(), 'frame_id': i64()}
        hip.check(hip.load().tgtc_style_train_batch(
            self.h, self.w, self.f, self.f, 0.5 * self.w, 0.5 * self.h, hip.ptr(self.c2w), self.frame_num, self.style_num,
            hip.ptr(self.images), hip.ptr(self.stylized), hip.ptr(index) if R else None, R, n, cs, cf, ca,
            int(self.pixel_alignment), int(self.ndc), 1.0, hip.ptr(out['rays_o']), hip.ptr(out['rays_d']),
            hip.ptr(out['rgb_gt']), hip.ptr(out['rgb_origin']), hip.ptr(out['style_id']), hip.ptr(out['frame_id']), hip.stream()))
        return out


class CoherenceCursor:
    """The integer state of the reference's frame-ordered loader, LightDataLoader(shuffle=False).loss_coh_get_batch
    (dataset.py:752-775): (style s, frame f, start a), all 0 at first.  `next()` -> the (s, f, a) of a call: its batch is
    pixels (a + i) mod hw, i < B, of frame f of style s.  The walk visits every frame of a style with one pixel window,
    then moves the window by B; once the window has passed the frame it moves on to the next style, starting over.

    Where a + B reaches S*F*hw the reference resets a to 0 AND reshuffles its (until then ordered) index array, after
    which its "ordered" batches are random pixels.  That point is never reached in a configured run (fern: about 297 000
    calls) and the reshuffle is deliberately not reproduced: here the walk just starts over.  B >= S*F*hw, where the
    reference samples with replacement instead, is refused."""

    def __init__(self, S, F, hw, B):
        self.S, self.F, self.hw, self.B = int(S), int(F), int(hw), int(B)
        self.data_num = self.S * self.F * self.hw
        if min(self.S, self.F, self.hw, self.B) <= 0:
            raise ValueError("CoherenceCursor: S, F, hw and B must be positive")
        if self.B >= self.data_num:
            raise ValueError("CoherenceCursor: a batch of %d rows needs more than %d rows of data (the reference samples "
                             "with replacement there; not built)" % (self.B, self.data_num))
        self.s = self.f = self.a = 0

    def next(self):
        if self.a + self.B >= self.data_num:
            self.a = 0                                   # the reference also reshuffles here: see the class docstring
        out = (self.s, self.f, self.a)
        if self.f == self.F - 1 and self.s != self.S - 1 and self.a >= self.hw:
            self.s, self.f, self.a = self.s + 1, 0, 0
        elif self.f != self.F - 1:
            self.f += 1
        else:
            self.f, self.a = 0, self.a + self.B
        return out

    def state(self):
        return (self.s, self.f, self.a)

    def at(self, n):
        """A new cursor in the state after `n` calls from the start: integers only, so the cursor of a resumed run is a
        function of its step count."""
        c = CoherenceCursor(self.S, self.F, self.hw, self.B)
        for _ in range(int(n)):
            c.next()
        return c


class EpochSampler:
    """The reference's DataLoader(shuffle=True) over `n_rays` indices: a fresh permutation per epoch, drawn on `device`,
    cut into ceil(n_rays / batch_size) batches, the last one partial.  The permutation of epoch e depends on (seed, e)
    alone, so the batch of global step s is a pure function of (seed, s): a resumed run continues the sequence of the
    uninterrupted one.  seed None: a base seed from the OS, like the reference's unseeded loader (no such continuity).
    full_batches=True: floor(n_rays / batch_size) batches per epoch, all full -- the LightDataLoader of `Style_train`
    reshuffles instead of delivering a short batch (dataset.py:676-679), and its coherence term compares equal shapes."""

    def __init__(self, n_rays, batch_size, seed, device="cuda", full_batches=False):
        if n_rays <= 0 or batch_size <= 0:
            raise ValueError("EpochSampler: n_rays and batch_size must be positive")
        self.n, self.batch_size, self.device = int(n_rays), int(batch_size), torch.device(device)
        self.seed = int.from_bytes(os.urandom(7), "little") if seed is None else int(seed)
        self.batches_per_epoch = -(-self.n // self.batch_size)
        if full_batches:
            if self.batch_size > self.n:
                raise ValueError("EpochSampler: no full batch of %d in %d indices" % (self.batch_size, self.n))
            self.batches_per_epoch = self.n // self.batch_size
        self._epoch, self._perm = None, None

    def permutation(self, epoch):
        if epoch != self._epoch:
            g = torch.Generator(device=self.device)
            g.manual_seed((((self.seed + 1) * 0x9E3779B97F4A7C15) ^ ((epoch + 1) * 0xBF58476D1CE4E5B9)) & _MASK63)
            self._perm, self._epoch = torch.randperm(self.n, generator=g, device=self.device), epoch
        return self._perm

    def batch_indices(self, step):
        """int64 [<= batch_size]: the indices of global step `step`"""
        epoch, b = divmod(int(step), self.batches_per_epoch)
        return self.permutation(epoch)[b * self.batch_size:(b + 1) * self.batch_size]

    def __iter__(self):
        step = 0
        while True:
            yield self.batch_indices(step)
            step += 1
