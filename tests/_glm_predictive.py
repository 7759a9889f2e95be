"""The float64 linear predictor of a tests/_glm_pointwise.case, for
tests/test_gpu_glm_predictive.py."""
import numpy as np

import _glm_pointwise as GP


def eta64(c, q, icpt="none", sliced=False, **_):
    """(eta [C, S, N], third [C, S, N], scale [C, S, 1] or a scalar), float64:
    third = 2 (P + 4) 2^-24 A is _glm_pointwise's dot-product share at |r| = 1
    (A = |a| + |off_i| + sum_k |X_ik beta_k|): the bound of the f32 eta."""
    q = np.asarray(q, np.float64)
    boff = GP.LEAD if sliced else 0
    beta = q[..., boff:boff + c.P]
    exp_scale = "log_sigma" in c.shapes
    a = (q[..., -2 if exp_scale else -1, None] if icpt == "param"
         else np.float64(GP.A_CONST if icpt == "const" else 0.0))
    off = c.d.off.astype(np.float64) if c.d.off is not None else np.zeros(c.N)
    X = c.d.X.astype(np.float64)
    eta = beta @ X.T + a + off
    A = np.abs(beta) @ np.abs(X).T + np.abs(a) + np.abs(off)
    with np.errstate(all="ignore"):
        s = np.exp(q[..., -1:]) if exp_scale else np.float64(GP.SIGMA_CONST)
    return eta, 2.0 * (c.P + 4) * 2.0 ** -24 * A, s
