"""Data side of `Origin_train` (train_loop.py): the reference's `RaySampler` + `DataLoader(shuffle=True)`
(dataset.py:63-144, train_tgtcs.py:110-113,160) without the host ray tables.

The reference stores float64 `rays_o` / `rays_d` of every pixel of every training frame (0.6 GB for fern at factor 4) and
its loader gathers `batch_size` shuffled rows of them, and of the images, on the host per iteration.  Here the device
holds the images (float32 [F,H,W,3], what llff_images.load_images returns) and the cameras ([F,12]); a batch is the
shuffled indices (`EpochSampler`, drawn on the device) through ONE launch of `tgtc_train_batch` (csrc/train_batch.hip),
which computes each row's ray from its frame's camera with the bits of `utils.gen_rays` and copies its colour.
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


class EpochSampler:
    """The reference's DataLoader(shuffle=True) over `n_rays` indices: a fresh permutation per epoch, drawn on `device`,
    cut into ceil(n_rays / batch_size) batches, the last one partial.  The permutation of epoch e depends on (seed, e)
    alone, so the batch of global step s is a pure function of (seed, s): a resumed run continues the sequence of the
    uninterrupted one.  seed None: a base seed from the OS, like the reference's unseeded loader (no such continuity)."""

    def __init__(self, n_rays, batch_size, seed, device="cuda"):
        if n_rays <= 0 or batch_size <= 0:
            raise ValueError("EpochSampler: n_rays and batch_size must be positive")
        self.n, self.batch_size, self.device = int(n_rays), int(batch_size), torch.device(device)
        self.seed = int.from_bytes(os.urandom(7), "little") if seed is None else int(seed)
        self.batches_per_epoch = -(-self.n // self.batch_size)
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
