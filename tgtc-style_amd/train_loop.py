"""The reference's `Origin_train` loop (train_tgtcs.py:218-309) around `training.origin_train_step`: shuffled batches from
the device (train_data.py), one Adam over both NeRF networks, the exponential learning-rate decay, the checkpoint cadence
and file layout, the `[ORIGIN TRAIN]` line every `i_print` steps -- the only place where the host waits for the GPU.

What differs from the reference, on purpose:
  * randomness is seeded (`--train_seed`, -1 = unseeded like the reference): the batch, the stratified jitter and the
    density-noise draws of global step s are functions of (seed, s) alone, so two runs agree and a resumed run continues
    the interrupted one;
  * the time fields of the printed line are replaced by steps/s, and the line carries the mean loss of the steps since the
    previous line (one step's loss on a shuffled batch is noisy);
  * the overflow guard of the fused training kernels (include/tgtc_train.h) is read at the same cadence, see
    `overflow_policy`.
"""
import math
import time

import torch

from . import checkpoints, training
from .train_data import EpochSampler

_MASK63 = (1 << 63) - 1

last_log = []       # the entries of the most recent origin_train call (one dict per printed line)


def lrate_at(args, step):
    """The learning rate the reference sets AFTER the iteration of global step `step` (train_tgtcs.py:272-276)."""
    return args.lrate * (0.1 ** (step / args.lrate_decay))


def saves_at(step, origin_step):
    """Whether a checkpoint is written after the iteration of global step `step` (train_tgtcs.py:284)."""
    return (step % 500 == 0 and step > 0) or step >= origin_step


def overflow_policy(count_before, count_now, backwards):
    """What to do about the fused training path's overflow guard at an `i_print` line -> (message or None, abort).

    count_before / count_now: the sum of both networks' `training_overflows()` at the previous line and now; backwards:
    how many fused backwards ran in between.  A backward that overflowed had its 24 gradients ZERO-FILLED by the library.
    Under Adam that is NOT a skipped step: the first and second moments decay towards zero and the weights still move by
    lr * m_hat / (sqrt(v_hat) + eps), i.e. on momentum alone.  A few such steps are reported and tolerated; a window in
    which EVERY backward overflowed means the run no longer follows its gradients at all, and aborts."""
    new = count_now - count_before
    if new <= 0:
        return None, False
    if backwards > 0 and new >= backwards:
        return ("every one of the %d backwards since the previous line overflowed the fp16 range of the fused training "
                "kernels and had its gradients zero-filled: Adam is stepping on momentum alone.  Lower --lrate, or train "
                "on the per-layer path (--train_unfused)" % backwards), True
    return "%d of %d backwards overflowed (gradients zero-filled; Adam stepped on momentum)" % (new, backwards), False


def make_optimizer(args, model, model_fine):
    """train_tgtcs.py:29-39: ONE Adam, coarse parameters then fine, each in nn.Module.parameters() order -- the order the
    `optimizer` entry of a NNNNNN.tar file is written in."""
    params = list(model.parameters()) + (list(model_fine.parameters()) if model_fine is not None else [])
    return torch.optim.Adam(params=params, lr=args.lrate, betas=(0.9, 0.999))


def make_style_optimizer(args, style_model, concat_model):
    """train_tgtcs.py:54: the Adam whose (untouched) state the reference writes into every NNNNNN.tar."""
    return torch.optim.Adam(params=list(style_model.parameters()) + list(concat_model.parameters()), lr=args.lrate,
                            betas=(0.9, 0.999))


def step_seed(seed, step):
    return (((seed + 1) * 0xD1B54A32D192ED03) ^ ((step + 1) * 0x9E3779B97F4A7C15)) & _MASK63


def mse2psnr(x):
    return -10. * math.log10(x) if x > 0 else float("inf")          # utils.py mse2psnr


def origin_train(args, model, model_fine, data, sv_path, global_step, optimizer_state=None, style_optimizer=None, log=None):
    """Runs the iterations global_step ... args.origin_step INCLUSIVE and returns origin_step + 1 (the reference's
    condition, train_tgtcs.py:307-309).  data: train_data.TrainRays; optimizer_state: the `optimizer` dict of the
    checkpoint the networks were restored from; style_optimizer: written into the files as the reference does.
    One dict per printed line is appended to `log` (default: the module's `last_log`, emptied first)."""
    global last_log
    if log is None:
        last_log = log = []
    fused = not getattr(args, "train_unfused", False)
    model.trainable(fused=fused), model_fine.trainable(fused=fused)
    optimizer = make_optimizer(args, model, model_fine)
    if optimizer_state:
        optimizer.load_state_dict(optimizer_state)
    seed = getattr(args, "train_seed", 0)
    seeded = seed is not None and seed >= 0
    sampler = EpochSampler(data.rays_num, args.batch_size, seed if seeded else None, device=data.device)
    gen = torch.Generator(device=data.device) if seeded else None
    n_fine = args.N_samples_fine
    backwards_per_step = (2 if n_fine > 0 else 1) if fused else 0
    overflows = lambda: model.training_overflows() + model_fine.training_overflows()
    count_before = overflows()
    acc = torch.zeros((), device=data.device)          # sum of the losses since the previous line, on the device
    window, t0 = 0, time.perf_counter()
    while True:
        rays_o, rays_d, rgb_gt = data.batch(sampler.batch_indices(global_step))
        if gen is not None:
            gen.manual_seed(step_seed(seed, global_step))
        r = training.origin_train_step(model, model_fine, optimizer, rays_o, rays_d, rgb_gt, args.N_samples, n_fine,
                                       data.near, data.far, sigma_noise_std=args.sigma_noise_std, as_float=False,
                                       generator=gen)
        acc += r['loss']
        window += 1
        if global_step % args.i_print == 0:
            # train_tgtcs.py:257-270; the .tolist() is the loop's only wait for the GPU
            fine = r.get('loss_rgb_fine')
            vals = torch.stack([r['loss'], r['loss_rgb'], fine if fine is not None else r['loss_rgb'], acc]).tolist()
            count_now = overflows()
            dt = time.perf_counter() - t0
            entry = {'step': global_step, 'loss': vals[0], 'loss_rgb': vals[1], 'psnr': mse2psnr(vals[1]),
                     'mean_loss': vals[3] / window, 'window': window, 'steps_per_s': window / dt if dt > 0 else 0.,
                     'overflows': count_now}
            line = "[ORIGIN TRAIN] Iter: %d Loss: %s PSNR: %s" % (global_step, vals[0], entry['psnr'])
            if fine is not None:
                entry.update(loss_rgb_fine=vals[2], psnr_fine=mse2psnr(vals[2]))
                line += " PSNR Fine: %s RGB Loss: %s RGB Fine Loss: %s" % (entry['psnr_fine'], vals[1], vals[2])
            else:
                line += " RGB Loss: %s" % vals[1]
            line += " Mean loss of %d step(s): %s %.1f steps/s" % (window, entry['mean_loss'], entry['steps_per_s'])
            message, abort = overflow_policy(count_before, count_now, backwards_per_step * window)
            if message and not abort:
                line += " -- " + message
            print(line, flush=True)
            log.append(entry)
            if abort:
                raise SystemExit("train_tgtcs: Origin_train stopped at step %d: %s" % (global_step, message))
            count_before, window, t0 = count_now, 0, time.perf_counter()
            acc.zero_()
        new_lrate = lrate_at(args, global_step)
        for group in optimizer.param_groups:
            group['lr'] = new_lrate
        if saves_at(global_step, args.origin_step):
            path = checkpoints.save_nerf(sv_path, global_step, model, model_fine if n_fine > 0 else None, optimizer,
                                         style_optimizer, keep=args.ckp_num)
            print('Saved checkpoints at', path, flush=True)
        global_step += 1
        if global_step > args.origin_step:
            return global_step
