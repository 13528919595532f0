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

And the reference's `Style_train` loop (train_tgtcs.py:312-571) around `training.style_train_iteration`: `style_train`
(`train_tgtcs --style_train`).  Both batches of an iteration come from one launch (train_data.StyleTrainRays.batch), the
style optimiser keeps the constant --lrate, the latent table has its own Adam (--latent_lrate), the coherence term leaves
the style optimiser's loss after --coh_until, the files follow `style_saves_at`.  Two pieces of state are not in the
reference's files and therefore RESTART when a run is resumed, as they do there: the latent Adam's moments (the reference
makes a fresh optimiser at every entry of Style_train, models.py:541-542) and the coherence state, which restarts at
cnt = 0 -- the first resumed iteration has no coherence term.  Seeding as above; the position of the frame-ordered walk is
a function of the step count alone (`coh_calls_before`).
"""
import math
import os
import time

import torch

from . import checkpoints, training
from .train_data import CoherenceCursor, EpochSampler

_MASK63 = (1 << 63) - 1

last_log = []       # the entries of the most recent origin_train / style_train call (one dict per printed line)
record_trace = False    # True: style_train keeps (step, batch indices, cursor triple) of every step in `last_trace`; the
last_trace = []         # indices are read back from the device every step, so this is for tests, not for runs


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


def style_saves_at(step, i_weights, total_step):
    """Whether `Style_train` writes its two files after the iteration of global step `step`, and by which of the
    reference's three branches (train_tgtcs.py:503-560) -> 0 (no), 1 (every 500 steps in (120000, 122000]), 2 (every 1000
    steps in (120000, 128001)) or 3 (step % i_weights == 0 or step == total_step: the only branch that prunes)."""
    if 120000 < step <= 122000 and step % 500 == 0:
        return 1
    if 120000 < step < 128001 and step % 1000 == 0:
        return 2
    if step % i_weights == 0 or step == total_step:
        return 3
    return 0


def coh_in_loss(step, coh_until):
    """The coherence term is part of the style optimiser's loss while step <= --coh_until (train_tgtcs.py:486-493, where
    the bound is the literal 122000)."""
    return step <= coh_until


def logp_weight(args, step):
    """train_tgtcs.py:426: the weight of the -log p term at global step `step`."""
    return args.logp_loss_lambda * (args.logp_loss_decay ** int((step - args.origin_step) / 1000))


def coh_calls_before(step, origin_step):
    """How many frame-ordered batches were drawn before global step `step`: Style_train starts after Origin_train, at
    origin_step + 1 -- or at 0 in a run without NeRF training (--synthetic without files).  A function of the step
    alone, so the cursor of a resumed run (train_data.CoherenceCursor.at) is that of the uninterrupted one."""
    return step - (origin_step + 1) if step > origin_step else step


def _prune(ckpts_path, want, reject, keep):
    """train_tgtcs.py:545-548, :557-560: the first of the sorted family goes when it has more than `keep` files."""
    files = [f for f in sorted(os.listdir(ckpts_path)) if 'tar' in f and want in f and reject not in f]
    if len(files) > keep:
        os.remove(os.path.join(ckpts_path, files[0]))


def style_train(args, model, model_fine, concat_model, style_model, latents, data, sv_path, global_step,
                optimizer_state=None, log=None, trace=None):
    """The reference's `Style_train` loop (train_tgtcs.py:312-571) around training.style_train_iteration: runs the
    iterations global_step ... args.total_step INCLUSIVE and returns total_step + 1.  data: train_data.StyleTrainRays.

    Per iteration: the shuffled batch (EpochSampler over S*F*H*W rows, full batches only) and the frame-ordered one
    (CoherenceCursor) leave ONE launch of tgtc_style_train_batch; both run through the operators in one pass; one backward
    serves the style optimiser (Adam over the style MLP then the concat MLP at the constant --lrate -- the reference's
    Style_train has no decay) and the latent table's own Adam([latents], --latent_lrate).  The -log p weight follows
    `logp_weight`, the coherence term stays in the style optimiser's loss while step <= --coh_until, the files follow
    `style_saves_at`.  A `[STYLE TRAIN]` line is printed when step % i_print == 0 and at the first step of the run -- the
    loop's only wait for the GPU, one device-to-host transfer -- and a non-finite loss there stops the run.  The window
    mean on the line (`mean_loss`) is that of the reference's `loss` = loss_rgb + loss_logp (train_tgtcs.py:482), the
    objective both optimisers share and the one term that is comparable from window to window: the coherence term is
    absent every frame_num-th step and after --coh_until, and its size follows which frames the walk compares (on the
    synthetic scene its 10-step mean swings by a factor of two in a run whose learning rates are zero).  The log entry
    also keeps `mean_total`, the style optimiser's loss, and `mean_loss_rgb`.

    As in the reference, two pieces of state are NOT in its files and restart on resume: the latent Adam's moments
    (`set_optimizer` makes a fresh one at every entry of Style_train) and the coherence state, which restarts at cnt = 0,
    so the first resumed step has no coherence term.  The style optimiser's state is in style_NNNNNN.tar and is restored
    (`optimizer_state`).  Randomness is seeded as in origin_train: batch and draws of step s depend on (--train_seed, s),
    the ordered cursor on s alone.  trace (a list; default `last_trace` when the module's `record_trace` is set): (step,
    batch indices on the host, cursor triple) per step, for tests -- it reads the indices back every step."""
    global last_log, last_trace
    if log is None:
        last_log = log = []
    if trace is None and record_trace:
        last_trace = trace = []
    model.set_enable_style(True), model_fine.set_enable_style(True)         # train_tgtcs.py:338-342; frozen, fused forward
    concat_model.trainable(), style_model.trainable(), latents.trainable()
    latents.style_latents_mu.requires_grad_(False), latents.style_latents_logvar.requires_grad_(False)   # in neither optimiser
    style_optimizer = make_style_optimizer(args, style_model, concat_model)
    if optimizer_state:
        style_optimizer.load_state_dict(optimizer_state)
        for group in style_optimizer.param_groups:
            group['lr'] = args.lrate
    latent_optimizer = torch.optim.Adam([latents.latents], lr=args.latent_lrate)          # models.py:541-542
    chain = None
    if getattr(args, "style_chain", False):          # --style_chain: only ever the caller's choice
        from . import style_chain
        chain = style_chain.StyleTrainer()
    seed = getattr(args, "train_seed", 0)
    seeded = seed is not None and seed >= 0
    B = args.batch_size_style
    sampler = EpochSampler(data.data_num, B, seed if seeded else None, device=data.device, full_batches=True)
    cursor = CoherenceCursor(data.style_num, data.frame_num, data.h * data.w, B).at(coh_calls_before(global_step, args.origin_step))
    coherence = training.CoherenceState(data.frame_num)
    gen = torch.Generator(device=data.device) if seeded else None
    n_fine = args.N_samples_fine
    acc = torch.zeros(3, device=data.device)      # sums of loss, total and loss_rgb since the previous line, on the device
    window, t0, first = 0, time.perf_counter(), global_step
    while True:
        index = sampler.batch_indices(global_step)
        cs, cf, ca = cursor.next()
        if trace is not None:
            trace.append((global_step, index.cpu().numpy().copy(), (cs, cf, ca)))
        batch = data.batch(index, coh=(cs, cf, ca, B))
        if gen is not None:
            gen.manual_seed(step_seed(seed, global_step))
        with_coh = coh_in_loss(global_step, args.coh_until)
        r = training.style_train_iteration(
            model, model_fine, concat_model, style_model, latents, style_optimizer, latent_optimizer, batch, B,
            args.N_samples, n_fine, data.near, data.far, coherence, sigma_noise_std=args.sigma_noise_std,
            rgb_loss_lambda=args.rgb_loss_lambda, logp_loss_lambda=logp_weight(args, global_step),
            loss_coh_lambda=args.loss_coh_lambda, coh_in_loss=with_coh, data_type=args.dataset_type, generator=gen,
            check_ids=False, as_float=False, chain=chain)
        acc += torch.stack([r['loss'], r['total'], r['loss_rgb']])
        window += 1
        if global_step % args.i_print == 0 or global_step == first:
            # train_tgtcs.py:562-567; the .tolist() is the loop's only wait for the GPU
            vals = torch.cat([torch.stack([r['total'], r['loss_coh'], r['loss_rgb'], r['loss_logp']]), acc]).tolist()
            dt = time.perf_counter() - t0
            entry = {'step': global_step, 'loss': vals[0], 'loss_coh': vals[1], 'only_loss': args.loss_coh_lambda * vals[1],
                     'loss_rgb': vals[2], 'loss_logp': vals[3], 'mean_loss': vals[4] / window, 'mean_total': vals[5] / window,
                     'mean_loss_rgb': vals[6] / window, 'window': window, 'steps_per_s': window / dt if dt > 0 else 0.,
                     'coh_in_loss': with_coh}
            print("[STYLE TRAIN] Iter: %d Loss: %s only Loss: %s Pixel RGB Loss: %s -Log(p) Loss: %s Mean Pixel + -Log(p) "
                  "loss of %d step(s): %s %.1f steps/s" % (global_step, vals[0], entry['only_loss'], vals[2], vals[3], window, entry['mean_loss'],
                                       entry['steps_per_s']), flush=True)
            log.append(entry)
            if not all(math.isfinite(v) for v in vals):
                raise SystemExit("train_tgtcs: Style_train stopped at step %d: the loss is not finite (%s)" % (global_step, vals[:4]))
            window, t0 = 0, time.perf_counter()
            acc.zero_()
        branch = style_saves_at(global_step, args.i_weights, args.total_step)
        if branch:
            for path in (checkpoints.save_style(sv_path, global_step, style_model, concat_model, style_optimizer),
                         checkpoints.save_latents(sv_path, global_step, latents)):
                print('Saved checkpoints at', path, flush=True)
            if branch == 3:
                _prune(sv_path, 'style', 'latent', args.ckp_num)
                _prune(sv_path, 'latent', 'style', args.ckp_num)
        global_step += 1
        if global_step > args.total_step:
            return global_step


def origin_train(args, model, model_fine, data, sv_path, global_step, optimizer_state=None, style_optimizer=None, log=None):
    """Runs the iterations global_step ... args.origin_step INCLUSIVE and returns origin_step + 1 (the reference's
    condition, train_tgtcs.py:307-309).  data: train_data.TrainRays; optimizer_state: the `optimizer` dict of the
    checkpoint the networks were restored from; style_optimizer: written into the files as the reference does.
    One dict per printed line is appended to `log` (default: the module's `last_log`, emptied first)."""
    global last_log
    if log is None:
        last_log = log = []
    fused = not getattr(args, "train_unfused", False)
    sparse = bool(getattr(args, "train_sparse", False))          # --train_sparse: only ever the caller's choice
    model.trainable(fused=fused, sparse=sparse), model_fine.trainable(fused=fused, sparse=sparse)
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
    live_before = (model.training_live_counts(), model_fine.training_live_counts()) if sparse else None
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
            if sparse:
                # the window's live share of each network's sparse backwards, read where the overflow counters are read
                live_now = (model.training_live_counts(), model_fine.training_live_counts())
                shares = [(n[0] - b[0]) / (n[1] - b[1]) if n[1] > b[1] else 0. for b, n in zip(live_before, live_now)]
                entry.update(live_coarse=shares[0], live_fine=shares[1])
                line += " Live: %.3f coarse %.3f fine" % (shares[0], shares[1])
                live_before = live_now
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
