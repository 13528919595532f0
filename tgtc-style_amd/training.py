"""One iteration of the reference's `Origin_train` body (train_tgtcs.py:226-254) on the HIP operators: stratified coarse
sampling with jitter, coarse NeRF, compositing with the density-noise regulariser, inverse-CDF fine sampling on the
(detached) coarse weights, fine NeRF, compositing, the two MSE losses, backward, optimiser step.

The networks must be marked `.trainable()` (models.StyleNerf): their forward then runs layer by layer on the differentiable
HIP dense layers (autograd_ops.py) and `utils.alpha_composition` carries its own backward kernel.  The samplers carry no
gradient, as in the reference (utils.py:562-579 detach).  The loop around `origin_train_step` -- shuffled batches, learning-rate decay,
checkpoint cadence, logging -- is train_loop.origin_train (`train_tgtcs --origin_train`).

`style_train_step` is the body of the reference's `Style_train` (train_tgtcs.py:352-482) batch by batch, as the reference
runs it; `style_train_iteration` is the same iteration for the loop train_loop.style_train (`train_tgtcs --style_train`):
both batches in one pass over the operators and the reference's two optimisers from one backward.  Both run the two style
MLPs on the per-layer path (autograd_ops.py) unless the caller hands them a `chain` (style_chain.StyleTrainer): the two
module forwards of a pass are then one call of the library's style trainer (include/tgtc_train.h) -- the same per-layer
arithmetic, chained inside the library.  `chain=None`, the default, is the per-layer path; nothing selects the chain for the
caller.  The VGG content / style losses of the reference's later stages
and the training of the 2-D module stay outside this build."""
import torch

from . import utils


def img2mse(x, y):
    return torch.mean((x - y) ** 2)         # utils.py img2mse


def origin_train_step(model, model_fine, optimizer, rays_o, rays_d, rgb_gt, N_samples, N_samples_fine, near, far,
                      sigma_noise_std=1.0, jitter=None, as_float=True, generator=None):
    """-> dict(loss, loss_rgb, loss_rgb_fine); parameters of both networks updated in place.  as_float=False returns the
    losses as detached device scalars WITHOUT synchronising: the reference reads them only every i_print iterations
    (train_tgtcs.py:257-266), and a float() per iteration serialises the host with the GPU.  generator (a device
    torch.Generator): the stratified jitter (unless `jitter` is given) and the two density-noise planes are drawn from it,
    in that order, instead of from the global generator -- a seeded iteration."""
    val = (lambda t: float(t.detach())) if as_float else (lambda t: t.detach())
    R = rays_o.shape[0]
    noise = lambda n: None
    if generator is not None:
        if jitter is None:
            jitter = torch.rand(R, N_samples, device=rays_o.device, generator=generator)
        if sigma_noise_std > 0:
            noise = lambda n: torch.randn(R, n, device=rays_o.device, generator=generator) * sigma_noise_std
    pts, ts = utils.sampling_pts_uniform(rays_o=rays_o, rays_d=rays_d, N_samples=N_samples, near=near, far=far, perturb=True,
                                         jitter=jitter)
    ret = model(pts=pts, dirs=rays_d.unsqueeze(1).expand([R, N_samples, 3]))
    rgb_exp, _, weights = utils.alpha_composition(ret['rgb'], ret['sigma'], ts, sigma_noise_std, noise=noise(N_samples))
    loss_rgb = img2mse(rgb_gt, rgb_exp)
    loss, out = loss_rgb, {}
    if N_samples_fine > 0:
        pts_fine, ts_fine = utils.sampling_pts_fine_torch(rays_o, rays_d, ts, weights.detach(), N_samples_fine)
        n = N_samples + N_samples_fine
        ret = model_fine(pts=pts_fine, dirs=rays_d.unsqueeze(1).expand([R, n, 3]))
        rgb_exp_fine, _, _ = utils.alpha_composition(ret['rgb'], ret['sigma'], ts_fine, sigma_noise_std, noise=noise(n))
        loss_rgb_fine = img2mse(rgb_gt, rgb_exp_fine)
        loss = loss + loss_rgb_fine
        out['loss_rgb_fine'] = val(loss_rgb_fine)
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    out.update(loss=val(loss), loss_rgb=val(loss_rgb))
    return out


def L2_norm(x):
    return torch.sqrt(torch.sum(x ** 2) + 1e-8)          # utils.py:459


def cosine_similarity(a, b):
    """VGGNet.py:204-210: per-row cosine of two [R, C] tensors with the reference's +1e-8 on the norms."""
    a_n = a / (torch.norm(a, dim=1, keepdim=True) + 1e-8)
    b_n = b / (torch.norm(b, dim=1, keepdim=True) + 1e-8)
    return torch.sum(a_n * b_n, dim=1)


class CoherenceState:
    """What the coherence term of `Style_train` carries from one iteration to the next (train_tgtcs.py:346-349): the
    stylised coarse / fine colours of the previous frame-ordered batch (x, y), the un-stylised colours of the same rays
    (x_origin) and the batch counter `cnt` that restarts the comparison every `frame_num` batches (:396-403, :451-458).

    The reference leaves x and y attached to the previous iteration's graph and calls `backward(retain_graph=True)`; the
    optimiser has by then updated, in place, weights that graph saved, so autograd raises at the second iteration (current
    PyTorch: "one of the variables needed for gradient computation has been modified by an inplace operation").  Here the
    carried tensors are values (detached): the loss is the reference's number, its gradient flows through the current
    batch."""

    def __init__(self, frame_num):
        self.frame_num, self.cnt = frame_num, 0
        self.x = self.y = self.x_origin = None

    def coarse(self, rgb2, rgb_origin2):
        loss = rgb2.new_zeros(())
        if self.cnt != self.frame_num and self.cnt != 0:
            loss = L2_norm(cosine_similarity(rgb2, self.x) - cosine_similarity(rgb_origin2, self.x_origin))
        self.x, self.x_origin = rgb2.detach(), rgb_origin2.detach()
        return loss

    def fine(self, rgb_fine2, rgb_origin2):
        """x_origin has just been replaced by THIS batch's colours (:399-403 run first), so the second cosine compares
        rgb_origin2 with itself, as in the reference (:456)."""
        loss = rgb_fine2.new_zeros(())
        if self.cnt == self.frame_num:
            self.cnt = 1
        else:
            if self.cnt != 0:
                loss = L2_norm(cosine_similarity(rgb_fine2, self.y) - cosine_similarity(rgb_origin2, self.x_origin))
            self.cnt += 1
        self.y = rgb_fine2.detach()
        return loss


def style_train_step(model, model_fine, concat_model, style_model, latents, optimizer, rays_o, rays_d, rgb_gt, style_ids,
                     frame_ids, N_samples, N_samples_fine, near, far, sigma_noise_std=1.0, rgb_loss_lambda=1.0,
                     logp_loss_lambda=0.0, data_type='llff', jitter=None, coherence=None, coh_batch=None,
                     loss_coh_lambda=0.0, as_float=True, chain=None):
    """One `Style_train` iteration (train_tgtcs.py:352-482): the shuffled batch's rendering, pixel and -log p terms and,
    with `coherence` (a CoherenceState) and `coh_batch` (dict rays_o, rays_d, rgb_origin, style_id, frame_id [, jitter]: the
    frame-ordered batch of `loss_coh_get_batch`, :366-370), the cosine-coherence term between consecutive frame-ordered
    batches, weighted by `loss_coh_lambda` (args.loss_coh_lambda; the reference drops the term after step 122 000, :472-479).
    The NeRF networks are frozen feature extractors (their fused forward, no graph); the concat / style MLPs and the latent
    table -- marked `.trainable()` -- receive gradients through the HIP dense layers, the latent gather and compositing.
    The VGG content / style losses of the reference's later stages (:484-560) are not part of it."""
    def styled(ro, rd, sid, fid, jit):
        R = ro.shape[0]
        z = latents(style_ids=sid, frame_ids=fid, type=data_type)
        zbar = torch.mean(z, dim=1, keepdim=True)
        L = z.shape[-1]

        def one_pass(nerf, pts, n):
            with torch.no_grad():
                ret = nerf(pts=pts, dirs=rd.unsqueeze(1).expand([R, n, 3]))
            if chain is not None:
                return chain.apply(concat_model, style_model, ret['pts'], ret['base_remap'], z, zbar.expand(R, L), n), ret['sigma']
            cf = concat_model(x=ret['pts'], latent=z.unsqueeze(1).expand([R, n, L]))['concat_features']
            both = torch.cat((ret['base_remap'], cf), dim=-1)
            rgb = style_model(x=ret['pts'], concated=both, latent=zbar.unsqueeze(2).expand([R, n, L]))['rgb']
            return rgb, ret['sigma']

        pts, ts = utils.sampling_pts_uniform(rays_o=ro, rays_d=rd, N_samples=N_samples, near=near, far=far, perturb=True, jitter=jit)
        rgb, sigma = one_pass(model, pts, N_samples)
        rgb_exp, _, weights = utils.alpha_composition(rgb, sigma, ts, sigma_noise_std)
        rgb_exp_fine = None
        if N_samples_fine > 0:
            pts_f, ts_f = utils.sampling_pts_fine_torch(ro, rd, ts, weights.detach(), N_samples_fine)
            rgb, sigma = one_pass(model_fine, pts_f, N_samples + N_samples_fine)
            rgb_exp_fine, _, _ = utils.alpha_composition(rgb, sigma, ts_f, sigma_noise_std)
        return rgb_exp, rgb_exp_fine

    loss_coh = None
    if coherence is not None and coh_batch is not None:          # :366-403, :436-458
        rgb2, rgb_fine2 = styled(coh_batch['rays_o'], coh_batch['rays_d'], coh_batch['style_id'], coh_batch['frame_id'],
                                 coh_batch.get('jitter'))
        loss_coh = coherence.coarse(rgb2, coh_batch['rgb_origin'])
        if rgb_fine2 is not None:
            loss_coh = loss_coh + coherence.fine(rgb_fine2, coh_batch['rgb_origin'])
    rgb_exp, rgb_exp_fine = styled(rays_o, rays_d, style_ids, frame_ids, jitter)
    loss_rgb = rgb_loss_lambda * img2mse(rgb_exp, rgb_gt)
    loss_logp = logp_loss_lambda * latents.minus_logp(style_ids=style_ids, frame_ids=frame_ids, data_type=data_type)
    if rgb_exp_fine is not None:
        loss_rgb = loss_rgb + rgb_loss_lambda * img2mse(rgb_exp_fine, rgb_gt)
    loss = loss_rgb + loss_logp
    total = loss if loss_coh is None else loss + loss_coh_lambda * loss_coh     # loss_for_style (:470)
    optimizer.zero_grad()
    total.backward()
    optimizer.step()
    val = (lambda t: float(t.detach())) if as_float else (lambda t: t.detach())     # see origin_train_step
    out = {'loss': val(loss), 'loss_rgb': val(loss_rgb), 'loss_logp': val(loss_logp)}
    if loss_coh is not None:
        out['loss_coh'] = val(loss_coh)
    return out


def style_train_iteration(model, model_fine, concat_model, style_model, latents, style_optimizer, latent_optimizer, batch, R,
                          N_samples, N_samples_fine, near, far, coherence, sigma_noise_std=1.0, rgb_loss_lambda=1.0,
                          logp_loss_lambda=0.0, loss_coh_lambda=0.0, coh_in_loss=True, data_type='llff', jitter=None,
                          generator=None, check_ids=True, as_float=False, chain=None):
    """The same `Style_train` iteration as `style_train_step` with its coherence batch, for the loop
    (train_loop.style_train): BOTH batches in ONE pass, and the reference's two optimisers from ONE backward.

    batch: the dict of train_data.StyleTrainRays.batch -- rows [0, R) are the shuffled batch, rows [R, R + B) the
    frame-ordered one.  All R + B rows go through sampling, the frozen NeRF passes, the style networks and compositing
    together; every per-row quantity is independent of its neighbours, so the two batches are slices of the results.  The
    iteration is bound by the host's enqueue, and this halves its launches.

    The reference steps `style_optimizer` on loss_rgb + loss_logp + lambda_coh * loss_coh (on loss_rgb + loss_logp alone
    once global_step > 122 000: coh_in_loss=False) and then `latents_model_1.optimize(loss)`, its own Adam([latents]) on
    the gradient of loss_rgb + loss_logp alone (train_tgtcs.py:482-495, models.py:541-548).  Here the latents of the ordered
    rows are gathered DETACHED: the coherence term then reaches the style networks only, loss_rgb + loss_logp depends on
    the shuffled rows only, and one backward of the style optimiser's loss leaves exactly those two gradients -- the style
    networks' from everything, the latent table's from loss_rgb + loss_logp.  style_latents_mu / _logvar are in neither
    optimiser and do not move.

    generator (a device torch.Generator): the stratified jitter [R+B, N_samples] (unless `jitter` is given), then the
    density-noise plane of the coarse pass [R+B, N_samples], then that of the fine pass [R+B, N_samples+N_samples_fine],
    are drawn from it in that order.  check_ids=False skips the latent table's id check and its read-back (ids from the
    batch kernel and an in-range sampler).  -> dict loss, loss_rgb, loss_logp, loss_coh (unweighted), total (the style
    optimiser's loss), detached device scalars unless as_float."""
    ro, rd = batch['rays_o'], batch['rays_d']
    sid, fid = batch['style_id'], batch['frame_id']
    T = ro.shape[0]
    noise = lambda n: None
    if generator is not None:
        if jitter is None:
            jitter = torch.rand(T, N_samples, device=ro.device, generator=generator)
        if sigma_noise_std > 0:
            noise = lambda n: torch.randn(T, n, device=ro.device, generator=generator) * sigma_noise_std
    z = latents(style_ids=sid[:R], frame_ids=fid[:R], type=data_type, check_ids=check_ids)
    if T > R:
        with torch.no_grad():
            z2 = latents(style_ids=sid[R:], frame_ids=fid[R:], type=data_type, check_ids=check_ids)
        z = torch.cat((z, z2), dim=0)
    zbar = torch.mean(z, dim=1, keepdim=True)
    L = z.shape[-1]

    def one_pass(nerf, pts, n):
        with torch.no_grad():
            ret = nerf(pts=pts, dirs=rd.unsqueeze(1).expand([T, n, 3]))
        if chain is not None:
            return chain.apply(concat_model, style_model, ret['pts'], ret['base_remap'], z, zbar.expand(T, L), n), ret['sigma']
        cf = concat_model(x=ret['pts'], latent=z.unsqueeze(1).expand([T, n, L]))['concat_features']
        both = torch.cat((ret['base_remap'], cf), dim=-1)
        rgb = style_model(x=ret['pts'], concated=both, latent=zbar.unsqueeze(2).expand([T, n, L]))['rgb']
        return rgb, ret['sigma']

    pts, ts = utils.sampling_pts_uniform(rays_o=ro, rays_d=rd, N_samples=N_samples, near=near, far=far, perturb=True, jitter=jitter)
    rgb, sigma = one_pass(model, pts, N_samples)
    rgb_exp, _, weights = utils.alpha_composition(rgb, sigma, ts, sigma_noise_std, noise=noise(N_samples))
    rgb_gt, rgb_origin2 = batch['rgb_gt'][:R], batch['rgb_origin'][R:]
    loss_rgb = rgb_loss_lambda * img2mse(rgb_exp[:R], rgb_gt)
    loss_coh = coherence.coarse(rgb_exp[R:], rgb_origin2) if T > R else rgb_exp.new_zeros(())
    if N_samples_fine > 0:
        n = N_samples + N_samples_fine
        pts_f, ts_f = utils.sampling_pts_fine_torch(ro, rd, ts, weights.detach(), N_samples_fine)
        rgb, sigma = one_pass(model_fine, pts_f, n)
        rgb_exp_fine, _, _ = utils.alpha_composition(rgb, sigma, ts_f, sigma_noise_std, noise=noise(n))
        loss_rgb = loss_rgb + rgb_loss_lambda * img2mse(rgb_exp_fine[:R], rgb_gt)
        if T > R:
            loss_coh = loss_coh + coherence.fine(rgb_exp_fine[R:], rgb_origin2)
    loss_logp = logp_loss_lambda * latents.minus_logp(style_ids=sid[:R], frame_ids=fid[:R], data_type=data_type, check_ids=check_ids)
    loss = loss_rgb + loss_logp
    total = loss + loss_coh_lambda * loss_coh if coh_in_loss else loss
    style_optimizer.zero_grad()
    if latent_optimizer is not None:
        latent_optimizer.zero_grad()
    total.backward()
    style_optimizer.step()
    if latent_optimizer is not None:
        latent_optimizer.step()
    val = (lambda t: float(t.detach())) if as_float else (lambda t: t.detach())
    return {'loss': val(loss), 'loss_rgb': val(loss_rgb), 'loss_logp': val(loss_logp), 'loss_coh': val(loss_coh),
            'total': val(total)}
