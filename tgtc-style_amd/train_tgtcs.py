"""`python -m tgtc_style_amd.train_tgtcs --config configs/fern.txt --render_valid_style [--synthetic]`
`python -m tgtc_style_amd.train_tgtcs --config configs/fern.txt --origin_train [--synthetic]`
`python -m tgtc_style_amd.train_tgtcs --config configs/fern.txt --style_train [--synthetic]`

The render half of the reference entry point (train_tgtcs.py:13-215): build the four networks and the latent
table, reload the newest checkpoints, and dispatch to render_style / render_train_style (or cal_geometry with
--render_valid).  Output directory and file names are the reference's (train_tgtcs.py:20,164,196;
rendering.py:216-217,363-364).

Of the training half, `--origin_train` runs the reference's first stage, `Origin_train` (train_tgtcs.py:218-309), on the
HIP training kernels: the NeRF pair is trained from the scene's images up to --origin_step, resuming from the newest
NNNNNN.tar or starting fresh, and leaves the reference's checkpoint files (train_loop.py, train_data.py).  A mode the
caller asks for: without the flag nothing trains.  `--style_train` runs `Style_train` (train_tgtcs.py:312-571): the two style
MLPs and the latent table are trained on the frozen NeRF pair from the frames of `--render_train` and their stylised copies
(train_loop.style_train), and leave style_NNNNNN.tar / latent_NNNNNN.tar for `--render_valid_style`.  The 2-D module's
training and the VGG content / style losses are the reference's and stay out of this build.

No dataset or checkpoint ships with this repository, so `--synthetic` provides a seeded scene: synth.nerf_state/...
weights and a closed-form camera path (for --origin_train: a teacher scene rendered from those weights, and seeded
student weights).  Without it the reference layout is expected: <sv_path>/NNNNNN.tar, style_NNNNNN.tar,
latent_NNNNNN.tar to render from, <datadir>/poses_bounds.npy and images/ or images_<factor>/ to train from.
"""
import os
import sys

import numpy as np
import torch

from . import config as cfg
from . import checkpoints, models, rendering, synth, utils


class ShardedScene:
    """Multi-GPU side of the dataset duck type (one process per GPU, torch.distributed).

    shard = 'frames' (BASELINE config 5): rank r owns the images k with k % world == r, renders them whole and writes
    their files itself -- no collective at all.  shard = 'rays' (config 4): every rank renders the contiguous pixel
    range parallel.shard_range(h*w, rank, world) of EVERY image; a finished image is reassembled by one all-gather
    of [rays, 4] rows (RCCL over xGMI with the nccl backend) and written by rank 0."""
    rank, world, shard, dist = 0, 1, 'frames', None
    jitter_samples, jitter_seed = 0, 0     # > 0: batches carry per-ray stratified jitter drawn from a per-IMAGE generator

    def image_jitter(self, k):
        """[h*w, N_samples] uniforms of image k: the same rows whatever the batch size, rank or sharding."""
        g = torch.Generator(device=self.device)
        g.manual_seed(self.jitter_seed + 1000003 * k)
        return torch.rand(self.h * self.w, self.jitter_samples, generator=g, device=self.device)

    def set_sharding(self, rank, world, shard, dist=None):
        self.rank, self.world, self.shard, self.dist = rank, world, shard, dist

    def _images(self, n_img):
        return [k for k in range(n_img) if self.shard == 'rays' or k % self.world == self.rank]

    def _pixels(self):
        from . import parallel
        return parallel.shard_range(self.h * self.w, self.rank, self.world) if self.shard == 'rays' else (0, self.h * self.w)

    # hooks read by rendering.py
    def global_image(self, local_no):
        return local_no if self.shard == 'rays' else local_no * self.world + self.rank

    def rays_per_image(self):
        lo, hi = self._pixels()
        return hi - lo

    def assemble(self, rgb, t):
        if self.world == 1 or self.shard != 'rays':
            return rgb, t, True
        from . import parallel
        rows = parallel.gather_rows(torch.cat([rgb, t[:, None]], 1).contiguous(), self.h * self.w, self.rank, self.world, self.dist)
        return rows[:, :3], rows[:, 3], self.rank == 0


class SyntheticScene(ShardedScene):
    """Duck type of the reference datasets for the render drivers (dataset.py:361-470 attributes), with rays
    generated on the device per frame instead of stored float64 tables (dataset.py:412-433)."""

    def __init__(self, h, w, frames, valid_frames, device="cuda", style_num=1):
        self.h, self.w, self.f = h, w, synth.fern_intrinsics(h, w)
        self.hwf = [h, w, self.f]
        self.near, self.far = 0., 1.
        to44 = lambda p: np.concatenate([p, np.array([[0, 0, 0, 1]], np.float32)], 0)
        self.cps = np.stack([to44(synth.spiral_pose(7 * i)) for i in range(frames)])
        self.cps_valid = np.stack([to44(synth.spiral_pose(i, n=valid_frames)) for i in range(valid_frames)])
        self.frame_num, self.style_num = frames, style_num
        self.mode, self.device = 'train', device

    def batches(self, batch_size):
        poses = self.cps if 'train' in self.mode else self.cps_valid
        n_img = len(poses) * (self.style_num if 'style' in self.mode else 1)
        first, last = self._pixels()
        for k in self._images(n_img):
            sid, fid = divmod(k, len(poses))
            o, d = utils.gen_rays(self.h, self.w, self.f, poses[fid][:3, :4], first_pixel=first, n=last - first,
                                  device=self.device)
            jit = self.image_jitter(k)[first:last] if self.jitter_samples and 'style' in self.mode else None
            for lo in range(0, last - first, batch_size):
                n = min(batch_size, last - first - lo)
                batch = {'rays_o': o[lo:lo + n], 'rays_d': d[lo:lo + n],
                         'style_id': torch.full((n,), sid, dtype=torch.long), 'frame_id': torch.full((n,), fid, dtype=torch.long)}
                if jit is not None:
                    batch['jitter'] = jit[lo:lo + n]
                yield batch

    def frame_batches(self, batch_size):
        """The validation path by FRAMES, for renders that take all styles of a frame in one call (--share_geometry): the
        rays this rank renders of each frame -- its pixel range of every frame under rays sharding, whole frames dealt
        round-robin under frames sharding -- with the jitter of the frame's style-0 image (image index 0 * frames + fid)."""
        poses = self.cps_valid
        first, last = self._pixels()
        for fid in range(len(poses)):
            if self.shard != 'rays' and fid % self.world != self.rank:
                continue
            o, d = utils.gen_rays(self.h, self.w, self.f, poses[fid][:3, :4], first_pixel=first, n=last - first,
                                  device=self.device)
            jit = self.image_jitter(fid)[first:last] if self.jitter_samples else None
            for lo in range(0, last - first, batch_size):
                n = min(batch_size, last - first - lo)
                batch = {'rays_o': o[lo:lo + n], 'rays_d': d[lo:lo + n], 'frame_id': torch.full((n,), fid, dtype=torch.long)}
                if jit is not None:
                    batch['jitter'] = jit[lo:lo + n]
                yield batch


class LlffPoseScene(SyntheticScene):
    """A real LLFF scene as far as rendering needs it: camera poses from `<datadir>/poses_bounds.npy`
    (llff_poses.scene_poses = load_llff.load_llff_data without the images; dataset.py:69-102), rays generated on the
    device.  Training views = the recentred poses, validation views = the 120-view spiral (`valid_frames` of it)."""

    def __init__(self, datadir, factor, device="cuda", valid_frames=None, style_num=1):
        from . import llff_poses
        arr = np.load(os.path.join(datadir, 'poses_bounds.npy'))
        h0, w0 = arr[0, :15].reshape(3, 5)[:2, 4]
        sc = llff_poses.scene_poses(arr, (int(h0 // factor), int(w0 // factor)), factor=factor)
        self.h, self.w, self.f = int(sc["hwf"][0]), int(sc["hwf"][1]), float(sc["hwf"][2])
        self.hwf = [self.h, self.w, self.f]
        self.near, self.far = 0., 1.                                  # NDC (dataset.py:379-380)
        self.cps = llff_poses.valid_camera_poses(sc["poses"])
        self.cps_valid = llff_poses.valid_camera_poses(sc["render_poses"])[:valid_frames]
        self.frame_num, self.style_num = self.cps.shape[0], style_num
        self.mode, self.device = 'train', device


class _Loader:
    def __init__(self, dataset, batch_size):
        self.dataset, self.batch_size = dataset, batch_size

    def __iter__(self):
        return self.dataset.batches(self.batch_size)


def _t(sd):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}


def _init_distributed():
    """One process per GPU under torchrun (RANK / WORLD_SIZE / LOCAL_RANK); the process group comes up BEFORE the first
    HIP call of the process.  TGTC_DIST_BACKEND=gloo lets several ranks share a GPU (functional rehearsals, tests)."""
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world == 1:
        return 0, 1, 0, None
    import torch.distributed as dist
    backend = os.environ.get("TGTC_DIST_BACKEND", "nccl")
    if dist.is_initialized():          # a batch of scenes in one process (render_batch.py): the group is already up
        return rank, world, (local if backend == "nccl" else local % max(torch.cuda.device_count(), 1)), dist
    if backend == "nccl":
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    else:
        dist.init_process_group(backend)
        local = local % max(torch.cuda.device_count(), 1)
    return rank, world, local, dist


def _broadcast_from_rank0(t, dist):
    """In-place broadcast of a parameter table; gloo (several test ranks on one GPU) moves it through host memory."""
    if dist.get_backend() == "nccl":
        dist.broadcast(t, 0)
    else:
        host = t.detach().cpu()
        dist.broadcast(host, 0)
        t.copy_(host)


def _make_latents(args, device, sv_path, style_num, frame_num, stylized, world=1, dist=None):
    """The latent table of a run: the newest latent checkpoint, else drawn around the VAE's encoding of the style
    features, else (--synthetic) the seeded table (train_tgtcs.py:128-155)."""
    latents = models.StyleLatents_variational(style_num=style_num, frame_num=frame_num,
                                              latent_dim=args.vae_latent).to(device)
    if not args.no_reload and checkpoints.load_latents(sv_path, latents):                  # train_tgtcs.py:139-146
        pass
    elif stylized is not None and style_num == stylized["style_num"] and os.path.exists(args.vae_pth_path):
        # train_tgtcs.py:128-155: no latent checkpoint -> the VAE encodes the style features into mu / logvar and every
        # frame's latent is drawn around them
        vae = models.VAE(data_dim=1024, latent_dim=args.vae_latent, W=args.vae_w, D=args.vae_d, kl_lambda=args.vae_kl_lambda)
        vae.load_state_dict(torch.load(args.vae_pth_path, map_location='cpu'))
        vae.eval().to(device)
        feats = torch.from_numpy(np.asarray(stylized["style_features"], np.float32)).to(device)
        _, mu, logvar = vae.encode(feats)
        latents.style_latents_mu = torch.nn.Parameter(mu.detach())
        latents.style_latents_logvar = torch.nn.Parameter(logvar.detach())
        latents.set_latents(generator=torch.Generator().manual_seed(args.latent_seed) if args.latent_seed >= 0 else None)
        if world > 1:
            # the draw comes from each process's own unseeded generator: rank 0's table is THE table, or the stripes / frames
            # of different ranks would be rendered with different style latents
            latents = latents.to(device)
            for p in (latents.latents, latents.style_latents_mu, latents.style_latents_logvar):
                _broadcast_from_rank0(p.data, dist)
        print('Initializing Latent Model from', args.vae_pth_path)
    elif args.synthetic:
        latents.load_state_dict(_t(synth.latents_state(4, style_num=style_num, frame_num=frame_num)))
    else:
        raise SystemExit("train_tgtcs: no latent checkpoint in %s and no stylized_data.npz + --vae_pth_path to initialise "
                         "the latents from (use --synthetic for the seeded scene)" % sv_path)
    return latents.to(device)


def _origin_train(args, device, sv_path, model, model_fine, concat_model, style_model):
    """--origin_train: the first stage of the reference's schedule (train_tgtcs.py:56-72,108-113,563-571) -> sv_path."""
    from . import train_data, train_loop
    if not args.synthetic:
        missing = train_data.missing_scene_parts(args.datadir, args.factor)
        if missing:
            raise SystemExit("train_tgtcs: --origin_train needs a scene to train from: --datadir %s has no %s (or run with "
                             "--synthetic for the seeded teacher scene)" % (args.datadir, " and no ".join(missing)))
    global_step, first_step, optimizer_state = 0, 0, None
    step = None if args.no_reload else checkpoints.load_nerf(sv_path, model, model_fine)           # train_tgtcs.py:60-72
    if step is not None:
        # The file holds the state AFTER iteration `step`.  The reference re-runs that iteration on reload (one extra Adam
        # step); here the run continues with the next one, as the uninterrupted run would.
        global_step, first_step = int(step), int(step) + 1
        optimizer_state = checkpoints.load_nerf_optimizer(sv_path)
    elif args.synthetic:
        model.load_state_dict(_t(synth.nerf_state(10)))             # seeded, well-conditioned students (teacher: 0 / 1)
        model_fine.load_state_dict(_t(synth.nerf_state(11)))
    if global_step + 1 >= args.origin_step:                          # train_tgtcs.py:109
        print('Origin_train: global step %d has reached --origin_step %d, nothing to train' % (global_step, args.origin_step))
        return sv_path
    if step is not None:
        print('Resuming Origin_train from the checkpoint of step %d in %s: continuing at step %d' % (global_step, sv_path, first_step))
    else:
        print('Origin_train: no NeRF checkpoint in %s, starting at step 0 from %s' % (
            sv_path, 'the seeded synthetic students' if args.synthetic else 'freshly initialised networks'))
    if args.synthetic:
        data = train_data.TrainRays.from_synthetic(args, device)
    else:
        data = train_data.TrainRays.from_llff(args.datadir, args.factor, device, no_ndc=args.no_ndc,
                                              pixel_alignment=args.pixel_alignment)
    print('Origin_train: %d frames of %d x %d, %d rays, %d per batch' % (data.frame_num, data.h, data.w, data.rays_num,
                                                                         args.batch_size))
    end = train_loop.origin_train(args, model, model_fine, data, sv_path, first_step, optimizer_state=optimizer_state,
                                  style_optimizer=train_loop.make_style_optimizer(args, style_model, concat_model))
    print('Origin_train done at step %d, checkpoints in %s.  Next: --render_train, the 2-D pass over its frames '
          "(trans_test), then --style_train; training the 2-D module itself stays the reference's" % (end - 1, sv_path))
    return sv_path


def _style_train(args, device, sv_path, model, model_fine, concat_model, style_model):
    """--style_train: the reference's Style_train stage (train_tgtcs.py:312-571) -> sv_path."""
    from . import train_data, train_loop, trans_test
    nerf_step = None if args.no_reload else checkpoints.load_nerf(sv_path, model, model_fine)      # train_tgtcs.py:60-72
    if nerf_step is None:
        if not args.synthetic:
            raise SystemExit("train_tgtcs: --style_train needs the trained NeRF pair: no NeRF checkpoint in %s (run "
                             "--origin_train first, or use --synthetic for the seeded scene)" % sv_path)
        model.load_state_dict(_t(synth.nerf_state(0)))
        model_fine.load_state_dict(_t(synth.nerf_state(1)))
    elif int(nerf_step) + 1 < args.origin_step:
        raise SystemExit("train_tgtcs: --style_train starts where Origin_train ends: the NeRF checkpoint in %s is of step "
                         "%d, short of --origin_step %d (finish --origin_train first, or lower --origin_step)" % (
                             sv_path, int(nerf_step), args.origin_step))
    style_step = None if args.no_reload else checkpoints.load_style(sv_path, style_model, concat_model)   # :74-82
    optimizer_state = None
    if style_step is not None:
        # as in _origin_train: the file holds the state AFTER iteration `style_step`, the run continues with the next one
        first_step = int(style_step) + 1
        optimizer_state = checkpoints.load_style_optimizer(sv_path)
    else:
        if args.synthetic:
            concat_model.load_state_dict(_t(synth.concat_state(2)))
            style_model.load_state_dict(_t(synth.style_state(3)))
        first_step = int(nerf_step) + 1 if nerf_step is not None else 0
    if first_step > args.total_step:
        print('Style_train: global step %d has reached --total_step %d, nothing to train' % (first_step - 1, args.total_step))
        return sv_path
    if style_step is not None:
        print('Resuming Style_train from the checkpoint of step %d in %s: continuing at step %d' % (int(style_step), sv_path, first_step))
    else:
        print('Style_train: no style checkpoint in %s, starting at step %d from %s' % (
            sv_path, first_step, 'the seeded synthetic style networks' if args.synthetic else 'freshly initialised style networks'))
    if args.synthetic:
        data = train_data.StyleTrainRays.from_synthetic(args, device)
        stylized = None
    else:
        data = train_data.StyleTrainRays.from_directories(args.datadir, args.factor, os.path.join(sv_path, 'nerf_gen_data2'),
                                                          device, no_ndc=args.no_ndc, pixel_alignment=args.pixel_alignment)
        stylized = trans_test.read_stylized_data(args.datadir, args.factor)
    latents = _make_latents(args, device, sv_path, data.style_num, data.frame_num, stylized)
    print('Style_train: %d style(s), %d frames of %d x %d, %d rows, %d per batch' % (
        data.style_num, data.frame_num, data.h, data.w, data.data_num, args.batch_size_style))
    end = train_loop.style_train(args, model, model_fine, concat_model, style_model, latents, data, sv_path, first_step,
                                 optimizer_state=optimizer_state)
    print('Style_train done at step %d, checkpoints in %s; --render_valid_style renders from them' % (end - 1, sv_path))
    return sv_path


def train(args):
    rank, world, local, dist = _init_distributed()
    if not torch.cuda.is_available():
        raise SystemExit("train_tgtcs: no GPU visible; the HIP render path has no CPU fallback")
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    use_viewdir_str = '_UseViewDir_' if args.use_viewdir else ''
    sv_path = os.path.join(args.basedir, args.expname + '_' + args.nerf_type + '_' + args.act_type + use_viewdir_str +
                           'ImgFactor' + str(int(args.factor)))        # train_tgtcs.py:19-20
    os.makedirs(sv_path, exist_ok=True)

    if (args.origin_train or args.style_train) and args.train_seed >= 0:
        torch.manual_seed(args.train_seed)      # a fresh start trains the default nn.Linear initialisation, as the reference
    model = models.StyleNerf(args, mode='coarse').to(device)
    model_fine = models.StyleNerf(args, mode='fine').to(device)
    concat_model = models.StyleMLP_before_concat(args).to(device)
    style_model = models.StyleMLP_Wild_multilayers(args).to(device)
    if args.origin_train:
        return _origin_train(args, device, sv_path, model, model_fine, concat_model, style_model)
    if args.style_train:
        return _style_train(args, device, sv_path, model, model_fine, concat_model, style_model)
    global_step = 0
    step = None if args.no_reload else checkpoints.load_nerf(sv_path, model, model_fine)           # train_tgtcs.py:60-72
    nerf_step = -1 if step is None else int(step)      # part of the --geometry_cache keys (-1: the seeded synthetic weights)
    if step is not None:
        global_step = step
    elif args.synthetic:
        model.load_state_dict(_t(synth.nerf_state(0)))
        model_fine.load_state_dict(_t(synth.nerf_state(1)))
    else:
        raise SystemExit("train_tgtcs: no NeRF checkpoint in %s (use --synthetic for the seeded scene)" % sv_path)
    step = None if args.no_reload else checkpoints.load_style(sv_path, style_model, concat_model)   # train_tgtcs.py:74-82
    if step is not None:
        global_step = step
    elif args.synthetic:
        concat_model.load_state_dict(_t(synth.concat_state(2)))
        style_model.load_state_dict(_t(synth.style_state(3)))

    # what the 2-D pass left next to the scene (dataset.py:437-440): style images, their 1024-d features, their number
    from . import trans_test
    stylized = trans_test.read_stylized_data(args.datadir, args.factor)
    if os.path.exists(os.path.join(args.datadir, 'poses_bounds.npy')):
        # rendering needs the cameras of the scene, not its images
        dataset = LlffPoseScene(args.datadir, args.factor, device=device,
                                valid_frames=args.synthetic_frames if args.synthetic else None,
                                style_num=stylized["style_num"] if stylized else 1)
    elif args.synthetic:
        hw = args.synthetic_hw
        dataset = SyntheticScene(hw, hw, frames=20, valid_frames=args.synthetic_frames, device=device,
                                 style_num=args.synthetic_styles)
    else:
        raise SystemExit("train_tgtcs: no poses_bounds.npy in --datadir %s (the image side of the LLFF loader is not part "
                         "of this build, SURVEY section 8f); run with --synthetic for the seeded scene" % args.datadir)
    dataset.jitter_samples = args.N_samples     # per-ray jitter: images independent of --batch_size / --chunk / sharding
    if world > 1:
        if (args.render_valid or args.render_train) and args.shard != 'frames':
            raise SystemExit("train_tgtcs: the geometry pass (--render_valid / --render_train) shards by whole frames "
                             "(--shard frames): geometry_%05d.npz is a per-frame file")
        dataset.set_sharding(rank, world, args.shard, dist)
    # rays per render call: the reference feeds --batch_size rays at a time from its host loader; with device-generated rays
    # a whole image (this rank's part of it) per call keeps the persistent kernels busy -- 78 calls of 2 048 rays cost a
    # 400x400 frame ~30 ms of launch gaps -- and gives the same pixels
    batch_size = args.batch_size if args.literal_batches else max(args.batch_size, dataset.rays_per_image())
    latents = _make_latents(args, device, sv_path, dataset.style_num, dataset.frame_num, stylized, world, dist)

    renderer = rendering.RayRenderer(model, model_fine, models.StylePair(concat_model, style_model))
    common = dict(samp_func=utils.sampling_pts_uniform, model_forward=utils.batchify(lambda **kw: model(**kw), args.chunk),
                  model_forward_fine=utils.batchify(lambda **kw: model_fine(**kw), args.chunk),
                  samp_func_fine=utils.sampling_pts_fine_torch, args=args, device=device)
    styled = dict(style_forward=utils.batchify(lambda **kw: style_model(**kw), args.chunk),
                  concat_style_forward=utils.batchify(lambda **kw: concat_model(**kw), args.chunk),
                  latents_model_1=latents, sigma_scale=args.sigma_scale, renderer=renderer,
                  min_weight=args.cull_weight if args.cull_weight >= 0 else None)   # --cull_weight, default -1 = off
    with torch.no_grad():
        if args.render_valid_style:
            out = os.path.join(sv_path, 'render_valid_' + str(global_step))
            model.set_enable_style(True), model_fine.set_enable_style(True)
            dataset.mode = 'valid_style'
            rendering.render_style(dataloader=_Loader(dataset, batch_size), sv_path=out, share_geometry=args.share_geometry,
                                   geometry_cache=args.geometry_cache or None, geometry_tag="nerf_step=%d" % nerf_step,
                                   fold_latents=args.fold_latents, style_precision=args.style_precision or None,
                                   geometry="chain" if args.chain_geometry else None, **common, **styled)
            print('Done, saving to', out)
            return out
        if args.render_train_style:
            out = os.path.join(sv_path, 'render_train_' + str(global_step))
            model.set_enable_style(True), model_fine.set_enable_style(True)
            rendering.render_train_style(dataset=dataset, sv_path=out, **common, **styled)
            print('Done, saving to', out)
            return out
        if args.render_valid or args.render_train:
            out = os.path.join(sv_path, 'nerf_gen_data2')
            dataset.mode = 'train' if args.render_train else 'valid'
            # --two_phase: the chain with the two-phase fine pass forced on (the dense chain's bytes); default: the fastest path
            plain = (rendering.RayRenderer(model, model_fine, fused=False, cull=True) if args.two_phase
                     else rendering.RayRenderer(model, model_fine))
            rendering.cal_geometry(dataloader=_Loader(dataset, batch_size), sv_path=out, renderer=plain, **common)
            print('Done, saving to', out)
            return out
    raise SystemExit("train_tgtcs: nothing to do -- pass --render_valid_style, --render_train_style, --render_valid, "
                     "--render_train, --origin_train or --style_train (of the reference's training stages Origin_train and "
                     "Style_train are part of this build, and only when asked for)")


def _finish_distributed():
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.barrier()
            dist.destroy_process_group()


def main(argv=None):
    args = cfg.parse_args(argv)
    if args.geometry_cache and not args.share_geometry:
        raise SystemExit("train_tgtcs: --geometry_cache needs --share_geometry (the cache is kept per frame, for all styles "
                         "of the frame; add --share_geometry or drop --geometry_cache)")
    if args.fold_latents and not (args.render_valid_style and args.share_geometry):
        raise SystemExit("train_tgtcs: --fold_latents needs --render_valid_style --share_geometry (one latent per style and "
                         "frame belongs to the walk by frames)")
    if args.fold_latents and not (args.cull_weight >= 0 or args.geometry_cache):
        raise SystemExit("train_tgtcs: --fold_latents needs --cull_weight >= 0 or --geometry_cache (the folded kernels are "
                         "those of the culled render and of the restyle; the dense multi-latent kernel has no folded form)")
    if args.style_precision:
        if args.style_precision != "fp16mx":
            raise SystemExit("train_tgtcs: --style_precision takes fp16mx (got %r)" % args.style_precision)
        if not (args.render_valid_style and args.share_geometry and args.fold_latents):
            raise SystemExit("train_tgtcs: --style_precision needs --render_valid_style --share_geometry --fold_latents (the "
                             "fp16mx style kernels take one latent per style and frame)")
        if not (args.cull_weight >= 0 or args.geometry_cache):
            raise SystemExit("train_tgtcs: --style_precision needs --cull_weight >= 0 or --geometry_cache (the fp16mx style "
                             "kernels are those of the culled render and of the restyle)")
        if args.precision.partition('+')[2] != "fp16mx" and args.precision != "fp16mx":
            raise SystemExit("train_tgtcs: --style_precision fp16mx needs a --precision whose fine half is fp16mx, e.g. "
                             "fp16x3+fp16mx (got %s; the kernel runs the fine trunk and the style networks of a tile together)"
                             % args.precision)
    if args.chain_geometry:
        if not (args.render_valid_style and args.share_geometry):
            raise SystemExit("train_tgtcs: --chain_geometry needs --render_valid_style --share_geometry (it is a geometry of the "
                             "culled multi-latent render and of the geometry cache)")
        if not (args.cull_weight >= 0 or args.geometry_cache):
            raise SystemExit("train_tgtcs: --chain_geometry needs --cull_weight >= 0 or --geometry_cache (the dense multi-latent "
                             "render has no chain geometry)")
    if args.two_phase:
        others = [f for f in ("render_valid_style", "render_train_style", "origin_train", "style_train") if getattr(args, f)]
        if others or not (args.render_valid or args.render_train):
            raise SystemExit("train_tgtcs: --two_phase needs --render_valid or --render_train and nothing else (it is the fine "
                             "pass of the plain render on the chain%s)"
                             % ("; it does not go with --" + " / --".join(others) if others else ""))
    if args.train_sparse:
        renders = [f for f in ("render_valid", "render_train", "render_valid_style", "render_train_style") if getattr(args, f)]
        if args.train_unfused:
            raise SystemExit("train_tgtcs: --train_sparse is a mode of the fused training kernels; it does not go with "
                             "--train_unfused (the per-layer path has no sparse backward)")
        if args.style_train:
            raise SystemExit("train_tgtcs: --train_sparse goes with --origin_train; it does not go with --style_train (the "
                             "NeRF pair is frozen there: no NeRF backward runs)")
        if renders:
            raise SystemExit("train_tgtcs: --train_sparse goes with --origin_train; it does not go with --%s (a render "
                             "runs no backward)" % " / --".join(renders))
        if not args.origin_train:
            raise SystemExit("train_tgtcs: --train_sparse needs --origin_train (it is the backward of that stage)")
    if args.style_chain:
        renders = [f for f in ("render_valid", "render_train", "render_valid_style", "render_train_style") if getattr(args, f)]
        if args.origin_train:
            raise SystemExit("train_tgtcs: --style_chain goes with --style_train; it does not go with --origin_train (the "
                             "style MLPs are not trained there)")
        if renders:
            raise SystemExit("train_tgtcs: --style_chain goes with --style_train; it does not go with --%s (a render "
                             "runs no backward)" % " / --".join(renders))
        if not args.style_train:
            raise SystemExit("train_tgtcs: --style_chain needs --style_train (it is the style MLPs' step of that stage)")
    if args.origin_train and args.style_train:
        raise SystemExit("train_tgtcs: --origin_train and --style_train are two stages: one call each, in that order")
    for stage in ("origin_train", "style_train"):
        if not getattr(args, stage):
            continue
        renders = [f for f in ("render_valid", "render_train", "render_valid_style", "render_train_style") if getattr(args, f)]
        if renders:
            raise SystemExit("train_tgtcs: --%s trains and returns; it does not go with --%s (render from the "
                             "checkpoints in a second call)" % (stage, " / --".join(renders)))
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise SystemExit("train_tgtcs: --%s runs on one GPU (WORLD_SIZE = %s): the reference has no "
                             "data-parallel training and neither has this build" % (stage, os.environ["WORLD_SIZE"]))
    if args.expname is None:
        raise SystemExit("train_tgtcs: --expname (or --config) is required")
    try:
        return train(args)      # the reference wraps this in `while True` (train_tgtcs.py:596-597); once is enough
    finally:
        _finish_distributed()


if __name__ == '__main__':
    main()
