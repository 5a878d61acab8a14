"""Float64 statement of the mixture scores (DESIGN "Mixture scores"; include/mgp_hip.h,
mgp_mixture_score / mgp_mixture_quantiles): CDF, survival function, CRPS and quantiles of
p(y | x) = sum_k w_k N(y | mu_k, s_k^2), s_k^2 = var_f,k + lik_var_k.  The reference project
has no counterpart, so this file is the specification the tests hold the kernels to.  Latents
and weights are point-major [N, K] here (the oracle's layout).

    t_k = (Y - mu_k) / s_k
    cdf = sum_k w_k erfc(-t_k / sqrt 2) / 2,     sf = sum_k w_k erfc(+t_k / sqrt 2) / 2
    A(m, v) = m erf(m / sqrt(2 v)) + sqrt(2 v / pi) exp(-m^2 / (2 v))
    crps = sum_i w_i A(Y - mu_i, s_i^2) - 1/2 sum_i sum_j w_i w_j A(mu_i - mu_j, s_i^2 + s_j^2)
    quantile(p): cdf(y) = p for p <= 1/2, sf(y) = 1 - p for p > 1/2

Levels are rounded to float32 once and 1 - p is the float32 subtraction (exact), as on the device.
"""
import numpy as np
from scipy.optimize import brentq
from scipy.special import erf, erfc, ndtri

SQRT2 = np.sqrt(2.0)


def _f64(*a):
    return [np.asarray(x, np.float64) for x in a]


def scales(var_f, lik_var):
    """s [N, K] = sqrt(var_f + lik_var)."""
    var_f, lik_var = _f64(var_f, lik_var)
    return np.sqrt(var_f + lik_var.reshape(1, -1))


def cdf_sf(mu_f, var_f, lik_var, w, Y):
    """(cdf [N], sf [N]), each its own erfc sum."""
    mu_f, w = _f64(mu_f, w)
    t = (np.asarray(Y, np.float64).reshape(-1, 1) - mu_f) / scales(var_f, lik_var)
    return (w * 0.5 * erfc(-t / SQRT2)).sum(-1), (w * 0.5 * erfc(t / SQRT2)).sum(-1)


def A(m, v):
    """E|X| of X ~ N(m, v)."""
    m, v = _f64(m, v)
    return m * erf(m / np.sqrt(2.0 * v)) + np.sqrt(2.0 * v / np.pi) * np.exp(-m * m / (2.0 * v))


def crps_terms(mu_f, var_f, lik_var, w, Y):
    """(sum_i w_i A(Y - mu_i, s_i^2) [N], 1/2 sum_ij w_i w_j A(mu_i - mu_j, s_i^2 + s_j^2) [N])."""
    mu_f, w = _f64(mu_f, w)
    s2 = scales(var_f, lik_var) ** 2
    first = (w * A(np.asarray(Y, np.float64).reshape(-1, 1) - mu_f, s2)).sum(-1)
    pair = (w[:, :, None] * w[:, None, :]
            * A(mu_f[:, :, None] - mu_f[:, None, :], s2[:, :, None] + s2[:, None, :])).sum((-1, -2))
    return first, 0.5 * pair


def crps(mu_f, var_f, lik_var, w, Y):
    first, half_pair = crps_terms(mu_f, var_f, lik_var, w, Y)
    return first - half_pair


def f32_levels(levels):
    """(p, tail, upper): the float32 levels, the tail probability solved for (p, or the float32
    1 - p above 1/2) and which tail, all as float64 values of float32 numbers."""
    p32 = np.asarray(levels, np.float32).reshape(-1)
    if not np.all((p32 > 0) & (p32 < 1)):
        raise ValueError("levels must lie in (0, 1)")
    upper = p32 > np.float32(0.5)
    tail = np.where(upper, np.float32(1) - p32, p32)
    return p32.astype(np.float64), tail.astype(np.float64), upper


def tail_function(mu, s, w, upper):
    """y -> cdf(y) (lower) or sf(y) (upper) of one point's mixture."""
    sign = 1.0 if upper else -1.0
    return lambda y: float((w * 0.5 * erfc(sign * (y - mu) / (s * SQRT2))).sum())


def quantiles(mu_f, var_f, lik_var, w, levels):
    """[N, Q] by brentq on the tail probability, bracketed by the experts' own quantiles."""
    mu_f, w = _f64(mu_f, w)
    s = scales(var_f, lik_var)
    _, tail, upper = f32_levels(levels)
    out = np.empty((mu_f.shape[0], tail.size))
    for q in range(tail.size):
        z = -ndtri(tail[q]) if upper[q] else ndtri(tail[q])
        for n in range(mu_f.shape[0]):
            on = w[n] > 0
            e = mu_f[n, on] + s[n, on] * z
            lo, hi = e.min(), e.max()
            pad = 1e-9 * (abs(lo) + abs(hi) + s[n].max())
            f = tail_function(mu_f[n], s[n], w[n], upper[q])
            g = (lambda y: tail[q] - f(y)) if upper[q] else (lambda y: f(y) - tail[q])   # increasing in y
            lo, hi = lo - pad, hi + pad
            # the weights are float32 roundings and need not sum to 1: widen until the signs differ
            for _ in range(200):
                if g(lo) <= 0.0 <= g(hi):
                    break
                lo, hi = lo - (hi - lo) - s[n].max(), hi + (hi - lo) + s[n].max()
            out[n, q] = lo if g(lo) == 0.0 else hi if g(hi) == 0.0 else brentq(g, lo, hi, xtol=1e-300, rtol=8.9e-16,
                                                                                maxiter=500)
    return out


def tail_residual(mu_f, var_f, lik_var, w, levels, q):
    """[N, Q]: |F(q) - p| / p for p <= 1/2, |SF(q) - (1 - p)| / (1 - p) above, in float64."""
    mu_f, w = _f64(mu_f, w)
    s = scales(var_f, lik_var)
    _, tail, upper = f32_levels(levels)
    q = np.asarray(q, np.float64)
    sign = np.where(upper, 1.0, -1.0)[None, :, None]
    t = (q[:, :, None] - mu_f[:, None, :]) / (s[:, None, :] * SQRT2)
    F = (w[:, None, :] * 0.5 * erfc(sign * t)).sum(-1)
    return np.abs(F - tail[None]) / tail[None]


def score(mu_f, var_f, lik_var, w, Y):
    """cdf, sf, crps as a dict."""
    c, s = cdf_sf(mu_f, var_f, lik_var, w, Y)
    return dict(cdf=c, sf=s, crps=crps(mu_f, var_f, lik_var, w, Y))
