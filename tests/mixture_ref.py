"""Float64 numpy statement of the mixture predictive (DESIGN "Mixture predictive";
include/mgp_hip.h, mgp_mixture_predict / mgp_mixture_density_grid).  The reference
project has no counterpart, so this file is the specification the tests hold the
kernels to.  Latents are point-major [N, K] here (the oracle's layout).

    S >= 1: logits_s = mu_a + z_s sqrt(max(var_a + jitter, 0)),  w = mean_s softmax_k(logits_s)
    S == 0: w = softmax_k(mu_a)            (predict_assign's plug-in weights)
    log_density[n] = logsumexp_{s,k}(log_softmax_k(logits_s) + log N(Y | mu_f, s2)) - log S
    density[n, g]  = sum_k w N(y_grid[g] | mu_f, s2),    s2 = var_f + lik_var
    mix_mean = sum_k w mu_f,   mix_var = sum_k w (s2 + (mu_f - mix_mean)^2)
"""
import numpy as np

JITTER = 1e-6   # gpflow.default_jitter(), as oracle.cpu_ref.JITTER


def _f64(*a):
    return [np.asarray(x, np.float64) for x in a]


def logits(mu_a, var_a, z=None, jitter=JITTER):
    """[S', N, K]: S' = S sampled logits, or the means alone (S = 0, z None or empty)."""
    mu_a, var_a = _f64(mu_a, var_a)
    if z is None or len(z) == 0:
        return mu_a[None]
    return mu_a[None] + np.asarray(z, np.float64) * np.sqrt(np.maximum(var_a + jitter, 0.0))[None]


def log_softmax(x):
    x = x - x.max(-1, keepdims=True)
    return x - np.log(np.exp(x).sum(-1, keepdims=True))


def weights(mu_a, var_a, z=None, jitter=JITTER):
    """w [N, K]."""
    return np.exp(log_softmax(logits(mu_a, var_a, z, jitter))).mean(0)


def log_normal(y, mu_f, var_f, lik_var):
    """log N(y | mu_f, var_f + lik_var), y broadcast against [N, K]."""
    mu_f, var_f = _f64(mu_f, var_f)
    s2 = var_f + np.asarray(lik_var, np.float64).reshape(1, -1)
    return -0.5 * np.log(2.0 * np.pi * s2) - 0.5 * (np.asarray(y, np.float64) - mu_f) ** 2 / s2


def log_density(mu_f, var_f, mu_a, var_a, lik_var, Y, z=None, jitter=JITTER):
    """[N], by a max-subtracted log-sum-exp over (s, k)."""
    ls = log_softmax(logits(mu_a, var_a, z, jitter))                       # [S', N, K]
    t = ls + log_normal(np.asarray(Y, np.float64).reshape(-1, 1), mu_f, var_f, lik_var)[None]
    t = np.moveaxis(t, 1, 0).reshape(t.shape[1], -1)                        # [N, S' K]
    m = t.max(-1)
    return m + np.log(np.exp(t - m[:, None]).sum(-1)) - np.log(ls.shape[0])


def mean_and_var(mu_f, var_f, lik_var, w):
    """(mix_mean [N], mix_var [N]), the variance in its centred form."""
    mu_f, var_f, w = _f64(mu_f, var_f, w)
    s2 = var_f + np.asarray(lik_var, np.float64).reshape(1, -1)
    mean = (w * mu_f).sum(-1)
    return mean, (w * (s2 + (mu_f - mean[:, None]) ** 2)).sum(-1)


def density_grid(mu_f, var_f, lik_var, w, y_grid):
    """[N, G]."""
    y = np.asarray(y_grid, np.float64).reshape(1, -1, 1)                    # [1, G, 1]
    mu_f, var_f, w = _f64(mu_f, var_f, w)
    ln = log_normal(y, mu_f[:, None, :], var_f[:, None, :], lik_var)       # [N, G, K]
    return (w[:, None, :] * np.exp(ln)).sum(-1)


def predict(mu_f, var_f, mu_a, var_a, lik_var, Y=None, z=None, y_grid=None, jitter=JITTER):
    """Every output at once, as a dict (log_density with Y, density with y_grid)."""
    w = weights(mu_a, var_a, z, jitter)
    mean, var = mean_and_var(mu_f, var_f, lik_var, w)
    out = dict(weights=w, mix_mean=mean, mix_var=var)
    if Y is not None:
        out["log_density"] = log_density(mu_f, var_f, mu_a, var_a, lik_var, Y, z, jitter)
    if y_grid is not None:
        out["density"] = density_grid(mu_f, var_f, lik_var, w, y_grid)
    return out
