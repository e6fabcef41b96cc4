"""Plain numpy restatement of what the tail of a training step does to one flat parameter vector (csrc/tail_dev.hpp): the two
regulariser terms and the update rules of torch.optim.Adam / torch.optim.RMSprop (centered=False, weight_decay=0).  It pins what
the kernels implement -- RMSprop's eps OUTSIDE the square root, lr applied to the momentum buffer -- and is itself checked against
the torch optimisers on the CPU (tests/test_host_optimizer_options.py).  No fused multiply-adds here: results agree with the kernels
and with torch to a few units in the last place, not bit for bit."""
import numpy as np


def regularised_grad(w, g, l1=0.0, l2=0.0):
    """g + l1 sign(w) + 2 l2 w, both terms from the weight BEFORE the update; a lambda of 0 (or None) switches its term off."""
    out = np.array(g, dtype=np.float64, copy=True)
    if l2:
        out = out + 2.0 * l2 * w
    if l1:
        out = out + l1 * np.sign(w)
    return out


def loss_total(data, w, l1=0.0, l2=0.0):
    """data + l1 sum|w| + l2 sum w^2 (utils/train.py:484-492), the norms of the weights before the update."""
    return data + (l1 or 0.0) * np.abs(w).sum() + (l2 or 0.0) * np.square(w).sum()


def rmsprop_step(w, g, square_avg, buf, lr, alpha=0.99, eps=1e-16, momentum=0.9):
    """One torch.optim.RMSprop step on the (already regularised) gradient g.  Returns (w, square_avg, buf); with momentum == 0 the
    buffer is returned untouched."""
    v = alpha * square_avg + (1.0 - alpha) * g * g
    avg = np.sqrt(v) + eps
    if momentum > 0:
        buf = momentum * buf + g / avg
        return w - lr * buf, v, buf
    return w - lr * (g / avg), v, buf


def adam_step(w, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """One torch.optim.Adam step (step number t, counted from 1) on the (already regularised) gradient g.  Returns (w, m, v)."""
    m = m + (g - m) * (1.0 - beta1)
    v = beta2 * v + (1.0 - beta2) * g * g
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    denom = np.sqrt(v) / np.sqrt(bc2) + eps
    return w - (lr / bc1) * (m / denom), m, v
