"""Restatement in float64 torch of the two clipping formulas that csrc/gradclip.hip implements, for its parity tests:
adaptive gradient clipping (the reference's AGC.step / unitwise_norm, learning/lr_scheduler.py:114-215) and global-norm
clipping (torch.nn.utils.clip_grad_norm_, norm_type 2).  Plain tensor expressions per tensor, nothing shared with the kernels.
Inputs are cast to float64 and stay there; the caller rounds the result to float32 once.

tests/test_gradclip_cpu.py pins both functions to tests/golden/agc.npz (the reference's own class and torch's own function, in
float32).  Tensors may live on any device."""
import torch


def unitwise_norm(x):
    """learning/lr_scheduler.py:114-130."""
    if x.ndim <= 1:
        dim, keepdim = 0, False
    elif x.ndim in (2, 3):
        dim, keepdim = 0, True
    elif x.ndim in (4, 5):
        dim, keepdim = list(range(1, x.ndim)), True
    else:
        raise ValueError('Wrong input dimensions')
    return torch.sum(x ** 2, dim=dim, keepdim=keepdim) ** 0.5


def agc(p, g, clipping, eps):
    """One tensor of AGC.step (learning/lr_scheduler.py:203-213) -> (clipped gradient, trigger per unit, grad_norm / max_norm
    per unit), all float64 (trigger: bool)."""
    p, g = p.detach().double(), g.detach().double()
    param_norm = torch.clamp(unitwise_norm(p), min=eps)
    grad_norm = unitwise_norm(g)
    max_norm = param_norm * clipping
    trigger = grad_norm > max_norm
    clipped = g * (max_norm / torch.clamp(grad_norm, min=1e-6))
    return torch.where(trigger, clipped, g), trigger, grad_norm / max_norm


def global_clip(grads, max_norm):
    """torch.nn.utils.clip_grad_norm_ -> (clipped gradients, total_norm, clip_coef), float64."""
    grads = [g.detach().double() for g in grads]
    total = torch.sqrt(sum((g ** 2).sum() for g in grads))
    coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
    return [g * coef for g in grads], total, coef


def clip_then_agc(params, grads, max_norm=None, clipping=None, eps=1e-3):
    """The step's order (learning/engine.py:442-452, then AGC.step): global clip, then AGC on the clipped gradients.  Either
    may be None (off).  -> (gradients float64, total_norm or None, clip_coef or None, [trigger per unit of every tensor],
    [grad_norm / max_norm per unit of every tensor])."""
    total = coef = None
    grads = [g.detach().double() for g in grads]
    if max_norm is not None:
        grads, total, coef = global_clip(grads, max_norm)
    triggers, ratios = [], []
    if clipping is not None:
        out = [agc(p, g, clipping, eps) for p, g in zip(params, grads)]
        grads, triggers, ratios = [o[0] for o in out], [o[1].reshape(-1) for o in out], [o[2].reshape(-1) for o in out]
    return grads, total, coef, triggers, ratios
