"""Float64 NumPy oracle of Keras 2.1.2 Adam (keras.optimizers.Adam as the reference compiles it: model.py:153, 251, 306, 403,
464), beside oracle.layers.rmsprop_step / sgd_momentum_step."""
import numpy as np


# ------------------------------------------------------------------------------------------------------------------------------
# Adam (keras/optimizers.py, Keras 2.1.2): NOT torch's rule - epsilon is added to the un-corrected sqrt(v')
# ------------------------------------------------------------------------------------------------------------------------------
def adam_lr_t(lr, t, beta1=0.9, beta2=0.999):
    """step size of update number t = iterations + 1 (t >= 1)"""
    return lr * np.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)


def adam_step(p, g, m, v, lr, t, beta1=0.9, beta2=0.999, eps=1e-8):
    """m' = b1 m + (1 - b1) g ; v' = b2 v + (1 - b2) g^2 ; p' = p - lr_t m' / (sqrt(v') + eps).  Returns (p', m', v')."""
    dt = p.dtype.type
    m2 = dt(beta1) * m + dt(1.0 - beta1) * g
    v2 = dt(beta2) * v + dt(1.0 - beta2) * g * g
    p2 = p - dt(adam_lr_t(lr, t, beta1, beta2)) * m2 / (np.sqrt(np.maximum(v2, 0)) + dt(eps))
    return p2, m2, v2
