"""Command-line / config-file surface of the reference (config.py:5-148) without configargparse.

Format (configs/*.txt): one `key = value` per line, `#` starts a comment (also trailing), a bare `key` sets a
store-true flag; command-line options override the file.  The flag table below reproduces the reference's names
and defaults; flags that only matter to training are accepted and carried, not interpreted.
"""
import argparse

# name -> (type, default); type None = store_true flag.  Defaults: reference config.py:6-145.
FLAGS = {
    "expname": (str, None), "basedir": (str, "./logs/"), "datadir": (str, "./data/"), "styledir": (str, "./style/"),
    "dataset_type": (str, "llff"), "no_ndc": (None, False), "white_bkgd": (None, False), "half_res": (None, False),
    "spherify": (None, False), "decoder_pth_path": (str, "./pretrained/decoder.pth"),
    "vgg_pth_path": (str, "./pretrained/vgg_normalised.pth"), "vae_pth_path": (str, "./pretrained/vae.pth"),
    "factor": (float, 1.0), "gen_factor": (float, 0.2), "valid_factor": (float, 0.05), "num_workers": (int, 0),
    "store_rays": (int, 1), "use_viewdir": (None, False), "sample_type": (str, "uniform"), "act_type": (str, "relu"),
    "nerf_type": (str, "nerf"), "style_type": (str, "mlp"), "latent_type": (str, "variational"),
    "nerf_type_fine": (str, "nerf"), "sigma_noise_std": (float, 1.0), "siren_sigma_mul": (float, 20.0),
    "rgb_loss_lambda": (float, 1.0), "rgb_loss_lambda_2d": (float, 10.0), "style_loss_lambda": (float, 1.0),
    "content_loss_lambda": (float, 1.0), "loss_coh_lambda": (float, 5e3), "logp_loss_lambda": (float, 0.1),
    "logp_loss_decay": (float, 1.0), "lambda_u": (float, 0.01), "netdepth": (int, 8), "netwidth": (int, 256),
    "netdepth_fine": (int, 8), "netwidth_fine": (int, 256), "style_D": (int, 8), "style_feature_dim": (int, 1024),
    "vae_d": (int, 4), "vae_w": (int, 512), "vae_latent": (int, 32), "vae_kl_lambda": (float, 0.1),
    "embed_freq_coor": (int, 10), "embed_freq_dir": (int, 4), "batch_size": (int, 2048),
    "batch_size_style": (int, 1024), "lrate": (float, 5e-4), "lrate_decay": (int, 100000), "chunk": (int, 1024 * 32),
    "no_reload": (None, False), "total_step": (int, 50000001), "origin_step": (int, 250000),
    "decoder_step": (int, 170000), "steps_per_opt": (int, 1), "steps_patch": (int, -1), "N_samples": (int, 64),
    "N_samples_fine": (int, 64), "i_print": (int, 100), "i_weights": (int, 5000), "i_video": (int, 5000000),
    "ckp_num": (int, 3), "render_valid": (None, False), "render_train": (None, False),
    "render_valid_style": (None, False), "render_train_style": (None, False), "sigma_scale": (float, 1.0),
    "pixel_alignment": (None, False), "TT_far": (float, 8.0),
}
# additions of this build (not in the reference)
EXTRA = {
    "precision": (str, "fp16x3"),      # fp16x3 (fp32-equivalent, default) | fp16mx | fp16, or "coarse+fine" e.g. fp16x3+fp16mx
    "shard": (str, "frames"),          # under torchrun: frames = whole images round-robin over the ranks, rank-local files;
                                       # rays = contiguous ray ranges of every image + one all-gather, rank 0 writes
    "literal_batches": (None, False),  # render --batch_size rays per call like the reference; default: whole images per call
                                       # (rays come from the device and the stratified jitter is seeded per ray, so an image
                                       # does not depend on how its rays are batched)
    "synthetic": (None, False),        # no dataset / checkpoints: seeded weights + closed-form camera path
    "synthetic_hw": (int, 400),        # frame size of the synthetic scene
    "synthetic_frames": (int, 2),      # frames of the synthetic validation path
    "synthetic_styles": (int, 1),      # styles of the synthetic scene's latent table (1: one style)
    "share_geometry": (None, False),   # --render_valid_style: all styles of a frame in ONE multi-latent call (HELP below)
    "cull_weight": (float, -1.0),      # stylised renders: style networks only where the compositing weight exceeds it (HELP below)
    "geometry_cache": (str, ""),       # --share_geometry: directory of cached ray geometry, reused across runs (HELP below)
    "fold_latents": (None, False),     # --share_geometry with --cull_weight or --geometry_cache: one latent per (style, frame) (HELP below)
    "style_precision": (str, ""),      # --fold_latents with a fine network in fp16mx: "fp16mx" runs the style networks in fp16mx (HELP below)
    "chain_geometry": (None, False),   # --share_geometry with --cull_weight or --geometry_cache: the plain chain's screened passes (HELP below)
    "two_phase": (None, False),        # --render_valid / --render_train: the chain with the two-phase fine pass (HELP below)
    "latent_seed": (int, -1),          # seed of the latent draw when the table is initialised from the VAE (-1: unseeded, like
                                       # the reference); under torchrun rank 0 draws and broadcasts either way
    "origin_train": (None, False),     # run the reference's Origin_train loop on the HIP training kernels (HELP below)
    "train_seed": (int, 0),            # --origin_train: seed of the initial weights, the batches and the draws (HELP below)
    "train_unfused": (None, False),    # --origin_train: train on the per-layer path, the cross-check of the fused kernels
    "train_sparse": (None, False),     # --origin_train: the sparse backward of the fused training kernels (HELP below)
    "style_train": (None, False),      # run the reference's Style_train loop: style MLPs and latent table (HELP below)
    "coh_until": (int, 122000),        # --style_train: last step with the coherence term in the style optimiser's loss
    "latent_lrate": (float, 1e-3),     # --style_train: learning rate of the latent table's own Adam
    "style_chain": (None, False),      # --style_train: both style MLPs through the library's style trainer (HELP below)
}


HELP = {
    "origin_train": "train the coarse / fine NeRF pair from the scene (the reference's Origin_train, steps up to "
                    "--origin_step inclusive): resumes from the newest NNNNNN.tar under the output directory or starts "
                    "fresh, writes the reference's checkpoint files (every 500 steps and at the end, --ckp_num kept), "
                    "prints a line every --i_print steps, and returns; the later stages (2-D module, Style_train) stay "
                    "the reference's.  The scene is --datadir (poses_bounds.npy and images/ or images_<factor>/) or, with "
                    "--synthetic, a teacher scene rendered from the seeded networks.  Refused together with a --render_* "
                    "flag and under torchrun (single GPU)",
    "train_seed": "with --origin_train / --style_train: seeds the fresh weights, the shuffled batches, the stratified jitter and the "
                  "density-noise draws; the batch and draws of a step depend on (seed, step) alone, so a resumed run "
                  "continues the interrupted one.  -1: unseeded, like the reference.  Default 0",
    "train_unfused": "with --origin_train: differentiable per-layer HIP dense layers in place of the fused training "
                     "kernels (same arithmetic, one launch per product); the cross-check",
    "train_sparse": "with --origin_train: run the backward of the fused training kernels over the samples whose upstream "
                    "gradient is not exactly zero (a sample with sigma + noise <= 0 has compositing weight 0 and adds "
                    "nothing to any gradient).  Same gradients up to fp32 / fp16x3 rounding; the [ORIGIN TRAIN] line also "
                    "carries the live share of each network since the previous line.  Never switched on by itself.  Refused "
                    "together with --train_unfused, --style_train (its NeRF pair is frozen) and any --render_* flag",
    "style_train": "train the two style MLPs and the latent table on the frozen NeRF pair (the reference's Style_train, "
                   "steps up to --total_step inclusive).  NeRF weights from the newest NNNNNN.tar, style MLPs from the "
                   "newest style_*.tar or freshly initialised, latents from the newest latent_*.tar, else the VAE, else "
                   "(--synthetic) the seeded table.  Starts after the newest style checkpoint, else after the NeRF "
                   "checkpoint (refused while that is short of --origin_step), else at 0.  Data: --datadir "
                   "(poses_bounds.npy, stylized_gen_<factor>/stylized_data.npz and NNN.jpg) and the rgb_*.png of "
                   "--render_train under the output directory, or with --synthetic the teacher frames and "
                   "--synthetic_styles recoloured copies.  --batch_size_style rows per batch, constant --lrate, writes "
                   "style_NNNNNN.tar / latent_NNNNNN.tar on the reference's cadence (--i_weights, --ckp_num), prints a "
                   "line every --i_print steps.  Refused together with --origin_train, a --render_* flag and under torchrun",
    "coh_until": "with --style_train: the coherence term is part of the style optimiser's loss while step <= this "
                 "(default 122000, the reference's literal)",
    "latent_lrate": "with --style_train: learning rate of the latent table's own Adam (default 1e-3, the reference's literal)",
    "style_chain": "with --style_train: run the forward and the backward of the two style MLPs as two calls of the library's "
                   "style trainer (tgtc_style_trainer_forward / _backward: the per-layer GEMMs chained inside the library, "
                   "layer inputs read in place, the latent gradient summed per ray) in place of 26 differentiable layer "
                   "calls per pass.  Same forward bits, gradients equal up to fp32 / fp16x3 rounding.  Never switched on by "
                   "itself.  Refused together with --origin_train and any --render_* flag",
    "synthetic_styles": "styles of the synthetic scene's latent table (default 1)",
    "share_geometry": "with --render_valid_style: render all styles of a frame in one multi-latent call that shares the "
                      "coarse pass, the fine depths and the fine NeRF trunk.  Style 0 is rendered with the jitter it has "
                      "without the flag (its images agree with such a run to the rounding between the chain and the "
                      "stylised ray kernel, 1.2e-7 on a pixel); the other styles use style 0's jitter instead of their own "
                      "draw, so all styles of a frame share sample positions and depth",
    "cull_weight": "with --render_valid_style (with or without --share_geometry) or --render_train_style: run the style "
                   "networks only on the fine samples whose compositing weight exceeds this value, after a sigma-only pass "
                   "over all samples.  0 reproduces the image of the chain of per-sample kernels bit for bit (samples of "
                   "weight exactly 0 add +0 to a pixel); a positive value bounds the change of each ray by the sum of its "
                   "dropped weights and leaves the depth image alone.  Default -1: off, every sample is styled",
    "geometry_cache": "with --render_valid_style --share_geometry (required; refused otherwise): a directory that keeps the "
                      "ray-only half of every frame (fine depths, the list of samples with compositing weight above "
                      "--cull_weight, their depths and weights; about 12 bytes per live sample).  A frame whose file is "
                      "there and was built for the same camera, pixel range, sample counts, jitter seed, NeRF checkpoint "
                      "step, precisions and --cull_weight is restyled from it without any NeRF density pass; otherwise it "
                      "is built and saved.  The images are those of the run without the cache, bit for bit.  An unset "
                      "--cull_weight means 0 here",
    "fold_latents": "with --render_valid_style --share_geometry and either --cull_weight >= 0 or --geometry_cache (refused "
                    "otherwise): hand the style networks ONE latent per (style, frame) instead of a copy per ray.  The "
                    "latent columns of the two style networks are folded into a bias table per style and the kernels run "
                    "without the latent k-steps, so no [styles, rays, 32] latent plane is built (20 MB per style for a "
                    "400 x 400 frame) and each style costs a tenth fewer matrix operations per live sample.  The colour "
                    "images agree with the run without the flag to the precision's rounding (at most one 8-bit level), the "
                    "depth images bit for bit, and a --geometry_cache directory serves both.  All rays of a call must "
                    "belong to one frame",
    "style_precision": "fp16mx: with --render_valid_style --share_geometry --fold_latents, either --cull_weight >= 0 or "
                       "--geometry_cache, and a --precision whose fine half is fp16mx (refused otherwise): the stylised frame "
                       "of such a pair, e.g. fp16x3+fp16mx, which has none without the flag.  The fine NeRF trunk and the "
                       "style networks of a 128-sample tile run in fp16mx in one kernel (the style pair stays packed in "
                       "fp16x3 and gets a second pair of streams); colours are within 1e-3 of float64 per sample.  With "
                       "--geometry_cache the frames are restyled from the cached geometry in the same kernel: no trunk "
                       "plane is built or saved, and the files and keys of the directory are those of the run without the "
                       "flag.  Default empty: off",
    "chain_geometry": "with --render_valid_style --share_geometry and either --cull_weight >= 0 or --geometry_cache (refused "
                      "otherwise): take the ray-only half of every call -- fine depths, densities, weights -- from the "
                      "passes of the plain chain render instead of the ray kernel's first half and a dense density pass.  "
                      "Each of the two density passes then runs the density screen where its network has one and the "
                      "library's rule says it pays: fp16 densities of every sample, the exact kernel on the candidates only; "
                      "screened or not, the images are the same bits.  Against a run without the flag the fine depths "
                      "differ by the rounding between two coarse kernels, so the cache keys carry geometry=chain and a "
                      "--geometry_cache directory never serves one run's files to the other.  Default: off",
    "two_phase": "with --render_valid or --render_train (refused with a --render_*_style flag, --origin_train or "
                 "--style_train): render on the chain of per-sample kernels with the two-phase fine pass forced on -- "
                 "densities of every fine sample first (behind the density screen where the library's rule says it pays), "
                 "then the full fine network on the samples that carry density only.  For a --precision whose fine half is "
                 "fp16x3 (the default) this is the only way to that pass; for fp16mx the library's own policy reaches it "
                 "too.  The image files are byte-identical to a run on the dense chain; against the default run (the ray "
                 "kernel) they differ by the rounding between the chain and the ray kernel.  Default: off",
}


def read_config_file(path):
    """`key = value` lines -> list of argv tokens."""
    argv = []
    with open(path) as f:
        for raw in f:
            line = raw.split("#", 1)[0].strip()
            if not line:
                continue
            if "=" in line:
                k, v = (s.strip() for s in line.split("=", 1))
                argv += ["--" + k, v]
            else:
                argv.append("--" + line)
    return argv


def config_parser():
    p = argparse.ArgumentParser(description="TGTC-Style render CLI on MI355X")
    p.add_argument("--config", type=str, default=None, help="config file path")
    for table in (FLAGS, EXTRA):
        for name, (typ, default) in table.items():
            if typ is None:
                p.add_argument("--" + name, action="store_true", default=default, help=HELP.get(name))
            else:
                p.add_argument("--" + name, type=typ, default=default, help=HELP.get(name))
    return p


def parse_args(argv=None):
    """File first, command line second (so the command line wins), like configargparse."""
    import sys
    argv = list(sys.argv[1:] if argv is None else argv)
    p = config_parser()
    pre, _ = p.parse_known_args(argv)
    merged = (read_config_file(pre.config) if pre.config else []) + argv
    return p.parse_args(merged)
