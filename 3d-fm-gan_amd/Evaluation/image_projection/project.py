"""Reconstruction criterion and optimisation loop of the image projection (reference
Evaluation/image_projection/project/__init__.py:125-129, 147-221, 228-333).

    ImageReconstructionLoss  :147-221   mse (or the mask-weighted mse) * mse_weight, plus, once that value has fallen
                                        below the loss type's threshold mse_T, LPIPS of the clamped images at 256^2,
                                        summed over the batch
    _adjust_learning_rate    :228-234   cosine ramp-down over the last quarter, linear ramp-up over the first 5 %
    optimize                 :245-333   iterations + 1 steps of a torch optimiser, or of LBFGS.FullBatchLBFGS (:274-285),
                                        on the Generator's inputs

What is different, on purpose:
  * the image stage of the criterion (difference, square, mask, sum; clamp, reduction to 256^2, ScalingLayer, NHWC) is
    one HIP launch forward and one backward (op/projection_loss.py) wherever the kernels serve the tensors, the
    perceptual module has forward_cached and PROJECT_FUSE is on; otherwise op.projection_loss.projection_stage_composite,
    the same mathematics from aten ops in the reference's order;
  * with pre_cache the VGG trunk runs over the target once per projection and its five taps are kept (the reference keeps
    the resized target and runs the trunk over it again in every iteration);
  * the comparison of the mse term with mse_T is the only host synchronisation of an iteration, and it is no longer made
    once LPIPS has joined (the reference compares in every iteration);
  * `percept=` takes a perceptual module with loaded weights.  Without it lpips.PerceptualLoss is built with its own
    initialisation: the pretrained blobs are not shipped, so a loss (and a projection) obtained that way is a load
    figure, not a published one;
  * `device` may be a torch.device or any device string (the reference reads a GPU index from the string's last
    character).
Reference behaviour kept on purpose:
  * the weighted mse divides by the mask's sum only (not by the channel count);
  * the threshold is tested on mse * mse_weight, LPIPS stays on once it has joined, and perceptual_weight is accepted
    and unused;
  * with pre_cache the target and the mask's sum of the first call are kept for the criterion's lifetime: one criterion
    per target;
  * the mask is handed to the perceptual module as its `normalize` argument, which fails for a mask of more than one
    element: LPIPS together with a mask raises here too, with a message that says why;
  * optimize runs iterations + 1 steps, and the learning rate is 0 at the first and the last of them.
Not provided: the scipy branch of optimize, the alex / squeeze nets, VGGPerceptualLoss (its weights are a download).
"""
import math
import os

import torch

from lpips import scaling_layer_of
from . import LBFGS
from op.projection_loss import TARGET, projection_stage, projection_stage_serves, projection_trunk_input

# Image stage of the criterion on the HIP kernels where they serve; False keeps the aten composite.
PROJECT_FUSE = os.environ.get('FMGAN_NO_PROJECT_FUSE', '0') != '1'

MSE_T = {'mse': 0.0, 'mse+lpips+mix': 0.01, 'mse+lpips': 100}


class ImageReconstructionLoss(torch.nn.Module):
    """The reference's criterion.  loss: 'mse' (LPIPS never joins), 'mse+lpips+mix' (joins once the mse term is below
    0.01) or 'mse+lpips' (below 100: from the first call for images in [-1, 1]).  percept: see the module docstring."""

    def __init__(self, model='net-lin', net='vgg', device='cuda', loss='mse+lpips', pre_cache=True, percept=None):
        super().__init__()
        if loss not in MSE_T:
            raise NotImplementedError('The loss type %s is not implemented' % loss)
        self.loss_type = loss
        self.mse_T = MSE_T[loss]
        self.pre_cache = pre_cache
        self.target_cache = None            # the clamped target at perceptual_size (composite form)
        self.target_features = None         # the trunk's taps of the scaled target (forward_cached form)
        self.mask_sum_cache = None
        self.lpips_model = model
        self.lpips_net = net
        self.perceptual = None
        if self.mse_T > 0.0:
            if percept is None:
                import lpips
                percept = lpips.PerceptualLoss(model=model, net=net).to(device).to(memory_format=torch.channels_last)
            self.perceptual = percept
        self.use_lpips = False

    def _lpips(self, y, output, target, mask, perceptual_size, scaling):
        """The LPIPS term.  y: the trunk input of `output` when the stage has produced it, else None."""
        if mask is not None:
            raise RuntimeError('ImageReconstructionLoss: LPIPS with a mask is not defined: the reference hands the mask to '
                               'lpips.PerceptualLoss as `normalize`, which fails for a mask of more than one element; use '
                               "loss='mse' with a mask")
        if y is None:               # LPIPS joined in this very call of the composite form
            y = projection_trunk_input(output, scaling, perceptual_size)
        if scaling is not None:
            if self.target_features is None or not self.pre_cache:
                with torch.no_grad():
                    target_s = projection_trunk_input(target.detach(), scaling, perceptual_size)
                self.target_features = self.perceptual.target_features(target_s)
            return self.perceptual.forward_cached(y, self.target_features).sum()
        # a perceptual term without forward_cached scales its inputs itself and sees the target in every call
        if self.target_cache is None or not self.pre_cache:
            self.target_cache = projection_trunk_input(target.detach(), None, perceptual_size)
        return self.perceptual(y, self.target_cache).sum()

    def forward(self, output, targets_kwargs, mse_weight=1, perceptual_weight=1, perceptual_size=TARGET):
        target = targets_kwargs['target']
        mask = targets_kwargs['mask']
        assert output.shape == target.shape, 'output {} and target {} do not match'.format(output.shape, target.shape)
        if mask is not None:
            assert output.shape[2:] == mask.shape, 'output {} and mask {} do not match'.format(output.shape, mask.shape)
            if self.mask_sum_cache is None or not self.pre_cache:
                self.mask_sum_cache = mask.sum()
            denom = self.mask_sum_cache
        else:
            denom = output.numel()
        may_join = self.mse_T > 0.0
        # the perceptual module's ScalingLayer when it can take cached target features
        scaling = scaling_layer_of(self.perceptual, 'forward_cached') if may_join else None
        fuse = PROJECT_FUSE and (scaling is not None or not may_join)
        served = fuse and perceptual_size == TARGET and projection_stage_serves(output, target, mask, scaling)
        # the trunk input comes with the stage when LPIPS is on; the kernel also writes it in a call in which LPIPS may
        # join (the same launch), the composite computes it only once it has
        want_y = mask is None and (self.use_lpips or (may_join and served))
        sq_sum, y = projection_stage(output, target, mask, scaling, want_y, fuse=fuse, size=perceptual_size)
        loss = sq_sum / denom * mse_weight
        if may_join and not self.use_lpips and bool(loss < self.mse_T):
            self.use_lpips = True
        if self.use_lpips:
            loss = loss + self._lpips(y, output, target, mask, perceptual_size, scaling)
        return loss


def learning_rate(i, iterations, initial_lr, rampdown=0.25, rampup=0.05):
    """The rate of step i of iterations + 1: initial_lr times a cosine ramp-down over the last `rampdown` of the run and
    a linear ramp-up over its first `rampup`; 0 at i = 0 and at i = iterations.  The factors are multiplied in the
    reference's order, so the rates are its rates bit for bit."""
    t = i / iterations
    down = 0.5 - 0.5 * math.cos(min(1, (1 - t) / rampdown) * math.pi)
    return initial_lr * (down * min(1, t / rampup))


def _adjust_learning_rate(i, iterations, initial_lr, optimizer, rampdown=0.25, rampup=0.05):
    optimizer.param_groups[0]['lr'] = learning_rate(i, iterations, initial_lr, rampdown, rampup)


def _print_loss(loss, iteration, iterations, print_iterations):
    if iteration and print_iterations and iteration % print_iterations == 0:
        width = int(math.log10(iterations)) + 1
        print('[' + str(iteration).rjust(width, ' ') + ']' + '{:.4f}'.format(float(loss.detach())))


def optimize(model, input_kwargs, targets, criterion, optimizer, iterations, print_iterations=10, device=None,
             history=None):
    """iterations + 1 steps of `optimizer` on the tensors of input_kwargs, which model(**input_kwargs) turns into the
    image that criterion(image, targets) scores; returns the last loss as a numpy scalar.  LBFGS.FullBatchLBFGS runs its
    line search with a closure that returns the loss without its gradients and max_ls 10; torch.optim.LBFGS runs with a
    closure; every other torch optimiser (Adam, SGD, ...) with _adjust_learning_rate from its initial rate.  history: a
    list that receives (learning rate, or FullBatchLBFGS's step length, and the detached loss) per step (not in the
    reference; the losses stay on the device).
    print_iterations 0 prints nothing; printing a loss synchronises with the host."""
    for key in input_kwargs:
        value = input_kwargs[key]
        if torch.is_tensor(value):
            value.requires_grad = True
        elif isinstance(value, (list, tuple)):
            for v in value:
                if torch.is_tensor(v):
                    v.requires_grad = True
    if not isinstance(optimizer, torch.optim.Optimizer):
        raise ValueError('Unsupported optimizer: a torch.optim.Optimizer or LBFGS.FullBatchLBFGS is expected (the scipy '
                         'objective of the reference is not provided). Documentation of supported optimizers '
                         'can be found here:\n\nhttps://pytorch.org/docs/stable/optim.html\n')
    if isinstance(optimizer, LBFGS.FullBatchLBFGS):
        def closure():
            optimizer.zero_grad()
            return criterion(model(**input_kwargs), targets)
        loss = closure()
        loss.backward()
        for i in range(iterations + 1):
            options = {'closure': closure, 'current_loss': loss, 'max_ls': 10}
            loss, _, t, _, _, _, _, _ = optimizer.step(options)
            _print_loss(loss, i, iterations, print_iterations)
            if history is not None:
                history.append((t, loss.detach()))
    elif isinstance(optimizer, torch.optim.LBFGS):
        for i in range(iterations + 1):
            def closure():
                optimizer.zero_grad()
                outputs = model(**input_kwargs)
                loss = criterion(outputs, targets)
                loss.backward()
                _print_loss(loss, i, iterations, print_iterations)
                return loss
            loss = optimizer.step(closure)
            if history is not None:
                history.append((optimizer.param_groups[0]['lr'], loss.detach()))
    else:
        initial_lr = optimizer.param_groups[0]['lr']
        for i in range(iterations + 1):
            optimizer.zero_grad()
            _adjust_learning_rate(i, iterations, initial_lr, optimizer)
            outputs = model(**input_kwargs)
            loss = criterion(outputs, targets)
            loss.backward()
            _print_loss(loss, i, iterations, print_iterations)
            optimizer.step()
            if history is not None:
                history.append((optimizer.param_groups[0]['lr'], loss.detach()))
    return loss.detach().cpu().numpy()
