"""What the published MobileNetV3 / MixNet / EfficientNet / FBNet retrain recipes need beside plain SGD: the two parameter groups
("no weight decay on BatchNorm gamma / beta and on biases") and RMSprop in TensorFlow's form.  Pure torch, imports without the HIP
library; on a GPU model ``model_eval.train_step`` runs optimizers built from these on the fused tail (``RetrainState.plan`` ->
'groups': ``tfnas_opt_groups_step``), and ``RMSpropTF.step()`` below is the torch route and the CPU route."""
import torch
from torch import nn

_NORMS = (nn.modules.batchnorm._NormBase, nn.GroupNorm, nn.LayerNorm)


def param_groups(model, weight_decay, no_decay=('bn', 'bias')):
    """The param-group dicts ``[{'params': decayed, 'weight_decay': weight_decay}, {'params': the rest, 'weight_decay': 0.0}]``
    for any torch optimizer.  ``no_decay`` names what goes into the second group: 'bn' -- every parameter that belongs directly to
    a normalisation module (BatchNorm gamma / beta); 'bias' -- every parameter named ``bias`` (the squeeze-excite convolutions'
    and the classifier's).  The decision reads the owning module's type and the parameter's name, never the number of dimensions:
    ``MixDepthwiseConv2d.weight`` is one packed 1-D tensor and is a convolution weight like any other.  Every parameter lands in
    exactly one group (a shared one where it is met first); a group that would be empty is left out."""
    unknown = set(no_decay) - {'bn', 'bias'}
    if unknown:
        raise ValueError("param_groups: no_decay takes 'bn' and 'bias', got %r" % sorted(unknown))
    decay, rest, seen = [], [], set()
    for mod in model.modules():
        for name, p in mod.named_parameters(recurse=False):
            if id(p) in seen:
                continue
            seen.add(id(p))
            plain = not (('bn' in no_decay and isinstance(mod, _NORMS)) or ('bias' in no_decay and name == 'bias'))
            (decay if plain else rest).append(p)
    groups = [{'params': decay, 'weight_decay': weight_decay}, {'params': rest, 'weight_decay': 0.0}]
    return [g for g in groups if g['params']]


class RMSpropTF(torch.optim.Optimizer):
    """RMSprop as TensorFlow evaluates it (what the EfficientNet / MixNet / MobileNetV3 recipes ran: decay 0.9, momentum 0.9,
    eps 1e-3): eps INSIDE the square root, the learning rate INSIDE the momentum buffer, the squared-gradient average starting at
    ones::

        d = grad + weight_decay * p
        square_avg <- square_avg + (1 - alpha) * (d * d - square_avg)
        momentum_buffer <- momentum * momentum_buffer + lr * d / sqrt(square_avg + eps)
        p <- p - momentum_buffer

    State per parameter: 'step' (int), 'square_avg', 'momentum_buffer' (kept with momentum 0 too); ``state_dict`` is the ordinary one.
    ``step()`` is a plain per-tensor torch implementation."""

    def __init__(self, params, lr=1e-2, alpha=0.9, eps=1e-3, weight_decay=0.0, momentum=0.9):
        if not lr >= 0.0:
            raise ValueError('RMSpropTF: invalid learning rate %r' % (lr,))
        if not eps > 0.0:
            raise ValueError('RMSpropTF: eps must be positive, got %r' % (eps,))
        if not 0.0 <= alpha <= 1.0:
            raise ValueError('RMSpropTF: alpha must lie in [0, 1], got %r' % (alpha,))
        if not momentum >= 0.0:
            raise ValueError('RMSpropTF: invalid momentum %r' % (momentum,))
        if not weight_decay >= 0.0:
            raise ValueError('RMSpropTF: invalid weight_decay %r' % (weight_decay,))
        super().__init__(params, dict(lr=lr, alpha=alpha, eps=eps, weight_decay=weight_decay, momentum=momentum))

    @staticmethod
    def init_state(state, p):
        """The state of a parameter that has not been stepped yet (the fused route starts from the same)."""
        state['step'] = 0
        state['square_avg'] = torch.ones_like(p, memory_format=torch.preserve_format)
        state['momentum_buffer'] = torch.zeros_like(p, memory_format=torch.preserve_format)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            lr, alpha, eps, wd, mom = (group[k] for k in ('lr', 'alpha', 'eps', 'weight_decay', 'momentum'))
            for p in group['params']:
                if p.grad is None:
                    continue
                state = self.state[p]
                if 'square_avg' not in state:
                    self.init_state(state, p)
                state['step'] += 1
                d = p.grad if wd == 0 else p.grad.add(p, alpha=wd)
                sq, buf = state['square_avg'], state['momentum_buffer']
                sq.add_(d * d - sq, alpha=1.0 - alpha)
                buf.mul_(mom).addcdiv_(d, (sq + eps).sqrt_(), value=lr)
                p.sub_(buf)
        return loss
