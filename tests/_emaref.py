"""Float64 restatement of the weight EMA of the retrain path (csrc/opt_kernels.hip: k_opt_sgd_ema / k_ema_lerp;
tfnas_amd/model_eval.py: WeightEma), shared by tests/test_ema_refs.py (which proves it against torch.lerp and against the textbook
``decay * ema + (1 - decay) * w`` in float64) and by the GPU tests (tests/test_gpu_ema_kernels.py, tests/test_gpu_ema_retrain.py).
The SGD part of "SGD step, then EMA" is _smallref.sgd_clip_ref.  Inputs are widened to float64 as they come in."""
import numpy as np

import _smallref as sr

U = sr.U


def lerp_ref(ema, w, alpha):
    """ema' = ema + alpha (w - ema): the formula the kernels evaluate as fma(alpha, w - ema, ema)."""
    ema, w = sr.d64(ema), sr.d64(w)
    return ema + alpha * (w - ema)


def alpha_ref(t, decay, warmup=True):
    """Step weight of update number ``t`` (0-based): 1 - min(decay, (1 + t) / (10 + t)) with warm-up, else 1 - decay."""
    return 1.0 - (min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay)


def lerp_bound(ema_new, w, ema_old, alpha):
    """Element-wise bound of the fp32 evaluation: 2 * 2^-24 * (|ema'| + alpha |w - ema|) -- one rounding of the difference
    (which the multiplication scales by alpha) and one of the fma, doubled so that a multiply followed by an add also passes."""
    return 2 * U * (np.abs(sr.d64(ema_new)) + alpha * np.abs(sr.d64(w) - sr.d64(ema_old)))


def sgd_ema_ref(w, g, m, ema, ranges, goff, max_norm, lr, mom, wd, grad_scale, alpha):
    """One tfnas_sgd_clip_ema_step: _smallref.sgd_clip_ref, then the lerp of ``ema`` towards the NEW weights inside the ranges.
    Returns (w', g', m', total_norm, ema')."""
    w2, g2, m2, tot = sr.sgd_clip_ref(w, g, m, ranges, goff, max_norm, lr, mom, wd, grad_scale)
    e2 = sr.d64(ema)
    for o, n in ranges:
        e2[o:o + n] = lerp_ref(e2[o:o + n], w2[o:o + n], alpha)
    return w2, g2, m2, tot, e2
