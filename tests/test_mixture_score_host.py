"""CPU tests of the mixture scores: the C-ABI entries' argument checks (all made before any HIP
call, so they run without a GPU) and known answers of the float64 statement
tests/mixture_score_ref.py that the GPU tests compare the kernels with."""
import ctypes
import re

import numpy as np
import pytest
from scipy.special import ndtr, ndtri

from modulatedgps_amd import _lib
from tests import mixture_score_ref as SR

ENTRIES = ("mgp_mixture_score_workspace_bytes", "mgp_mixture_score", "mgp_mixture_quantiles")
MGP_OP_MIXTURE_SCORE = 14
MGP_ERR_WORKSPACE, MGP_ERR_UNSUPPORTED = 1, 3


def test_entries_are_bound_declared_and_exported():
    syms = _lib.header_symbols()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and name in syms and hasattr(raw, name), name
    text = open(_lib.HEADER_PATH).read()
    assert re.search(r"MGP_OP_MIXTURE_SCORE\s*=\s*14\b", text)


def test_workspace_query_matches_the_front():
    lib = _lib.load()
    for N, K in ((1, 1), (64, 3), (65, 3), (1000, 32), (65536, 8)):
        nbytes = lib.mgp_mixture_score_workspace_bytes(N, K)
        assert nbytes == lib.mgp_workspace_bytes(MGP_OP_MIXTURE_SCORE, 0, N, K)
        assert nbytes >= 8 and nbytes % 8 == 0
        assert nbytes >= 8 * -(-N * 4 // 256)   # one double per 256-thread block at 4 lanes per point


def _score(**kw):
    """mgp_mixture_score with valid (never dereferenced) arguments, overridden by kw."""
    lib = _lib.load()
    c = ctypes.c_void_p(256)
    N, K = 100, 3
    base = dict(mu_f=c, var_f=c, ldf=N, lik_var=c, weights=c, Y=c, N=N, K=K, cdf=c, sf=c, crps=c, crps_sum=c,
                workspace=c, workspace_bytes=lib.mgp_mixture_score_workspace_bytes(N, K), stream=None)
    assert len(base) == len(_lib.SIGNATURES["mgp_mixture_score"][1])
    base.update(kw)
    return lib.mgp_mixture_score(*base.values())


def test_score_rejects_bad_arguments_before_any_hip_call():
    assert _score(mu_f=None) == -1 and _score(var_f=None) == -2 and _score(ldf=99) == -3
    assert _score(lik_var=None) == -4 and _score(weights=None) == -5 and _score(Y=None) == -6
    assert _score(K=0) == -8 and _score(K=-1) == -8
    assert _score(K=33) == MGP_ERR_UNSUPPORTED
    nbytes = _lib.load().mgp_mixture_score_workspace_bytes(100, 3)
    assert _score(workspace_bytes=nbytes - 1) == MGP_ERR_WORKSPACE
    assert _score(workspace=None) == MGP_ERR_WORKSPACE
    # N <= 0: nothing to do, after the checks
    assert _score(N=0) == 0 and _score(N=-3) == 0
    assert _score(N=0, K=33) == MGP_ERR_UNSUPPORTED and _score(N=0, Y=None) == -6


def _quantiles(**kw):
    lib = _lib.load()
    c = ctypes.c_void_p(256)
    base = dict(mu_f=c, var_f=c, ldf=100, lik_var=c, weights=c, N=100, K=3, levels=c, Q=9, quantiles=c, ldq=9,
                stream=None)
    assert len(base) == len(_lib.SIGNATURES["mgp_mixture_quantiles"][1])
    base.update(kw)
    return lib.mgp_mixture_quantiles(*base.values())


def test_quantiles_rejects_bad_arguments_before_any_hip_call():
    assert _quantiles(mu_f=None) == -1 and _quantiles(var_f=None) == -2 and _quantiles(ldf=99) == -3
    assert _quantiles(lik_var=None) == -4 and _quantiles(weights=None) == -5
    assert _quantiles(K=0) == -7 and _quantiles(K=33) == MGP_ERR_UNSUPPORTED
    assert _quantiles(levels=None) == -8 and _quantiles(Q=-1) == -9
    assert _quantiles(Q=257, ldq=257) == MGP_ERR_UNSUPPORTED
    assert _quantiles(quantiles=None) == -10 and _quantiles(ldq=8) == -11
    assert _quantiles(N=0) == 0 and _quantiles(Q=0, ldq=0) == 0
    assert _quantiles(N=0, K=33) == MGP_ERR_UNSUPPORTED and _quantiles(Q=0, ldq=0, weights=None) == -5


def test_python_layer_rejects_levels_outside_the_unit_interval():
    """Before anything is uploaded: no device is touched."""
    from modulatedgps_amd import ops
    for bad in ([0.0], [1.0], [0.5, -1e-3], [1.5], [float("nan")], [1 - 1e-9], [[0.1, 0.2]], [0.5] * 257):
        with pytest.raises(ValueError):
            ops.quantile_levels(bad)
    lv = ops.quantile_levels([1e-6, 0.5, 1 - 1e-6])
    assert lv.dtype == np.float32 and lv.shape == (3,)
    with pytest.raises(ValueError):
        SR.quantiles(np.zeros((1, 1)), np.ones((1, 1)), [0.1], np.ones((1, 1)), [0.0])


def test_reference_single_expert_known_answers():
    """K = 1: cdf = Phi(t), quantile = mu + s z_p, crps = s [t (2 Phi(t) - 1) + 2 phi(t) - 1 / sqrt(pi)]."""
    rng = np.random.default_rng(0)
    N = 40
    mu, var_f = rng.normal(size=(N, 1)) * 3, rng.uniform(0.01, 1, (N, 1))
    lik_var, w = np.array([0.3]), np.ones((N, 1))
    s = np.sqrt(var_f[:, 0] + 0.3)
    t = rng.uniform(-6, 6, N)
    Y = mu[:, 0] + t * s
    t = (Y - mu[:, 0]) / s
    out = SR.score(mu, var_f, lik_var, w, Y)
    np.testing.assert_allclose(out["cdf"], ndtr(t), rtol=1e-12)
    np.testing.assert_allclose(out["sf"], ndtr(-t), rtol=1e-12)
    phi = np.exp(-0.5 * t * t) / np.sqrt(2 * np.pi)
    np.testing.assert_allclose(out["crps"], s * (t * (2 * ndtr(t) - 1) + 2 * phi - 1 / np.sqrt(np.pi)), rtol=1e-11)
    levels = np.array([1e-6, 0.025, 0.5, 0.975, 1 - 1e-6])
    p32, tail, upper = SR.f32_levels(levels)
    z = np.where(upper, -ndtri(tail), ndtri(tail))
    q = SR.quantiles(mu, var_f, lik_var, w, levels)
    np.testing.assert_allclose(q, mu + s[:, None] * z[None], rtol=1e-12, atol=1e-12)


def _random_mixture(rng, N, K):
    mu = rng.normal(0, 5, (N, K))
    s = np.exp(rng.uniform(np.log(0.05), 0.0, (N, K)))
    lik_var = np.full(K, 1e-3)
    w = rng.dirichlet(np.full(K, 0.7), N)
    k = rng.integers(0, K, N)
    Y = mu[np.arange(N), k] + rng.uniform(-4, 4, N) * s[np.arange(N), k]
    return mu, s * s - lik_var[None], lik_var, w, Y


def test_reference_crps_is_the_integral_of_the_squared_cdf_error():
    """crps = int (F(u) - 1[u >= y])^2 du = int_{u < y} F^2 + int_{u > y} (1 - F)^2, each half by
    the trapezoid rule on a grid that ends at y (so the jump is no cell's interior), fine beside
    the narrowest expert: s >= 0.05 and spacing h = 1e-3 give a relative error of about
    (h / s)^2 / 12 = 3e-5; the halves are cut 60 away from y, beyond every expert's tail."""
    rng = np.random.default_rng(1)
    mu, var_f, lik_var, w, Y = _random_mixture(rng, 6, 4)
    closed = SR.crps(mu, var_f, lik_var, w, Y)
    assert (closed >= 0).all()
    h = 1e-3
    step = np.arange(0.0, 60.0, h)
    trapezoid = lambda f: np.sum(0.5 * (f[1:] + f[:-1])) * h
    for n in range(6):
        one = lambda a: np.repeat(a[n:n + 1], step.size, 0)
        below = SR.cdf_sf(one(mu), one(var_f), lik_var, one(w), Y[n] - step)[0]
        above = SR.cdf_sf(one(mu), one(var_f), lik_var, one(w), Y[n] + step)[1]
        quad = trapezoid(below ** 2) + trapezoid(above ** 2)
        assert abs(quad - closed[n]) <= 2e-4 * closed[n], (n, quad, closed[n])


def test_reference_quantiles_invert_the_cdf_and_crps_is_non_negative():
    rng = np.random.default_rng(2)
    for K in (1, 3, 8):
        mu, var_f, lik_var, w, Y = _random_mixture(rng, 25, K)
        levels = [1e-6, 1e-3, 0.025, 0.25, 0.5, 0.75, 0.975, 0.999, 1 - 1e-6]
        q = SR.quantiles(mu, var_f, lik_var, w, levels)
        _, tail, _ = SR.f32_levels(levels)
        assert (SR.tail_residual(mu, var_f, lik_var, w, levels, q) * tail[None]).max() <= 1e-12
        assert (np.diff(q, axis=1) > 0).all()
        assert (SR.crps(mu, var_f, lik_var, w, Y) >= 0).all()
        c, s = SR.cdf_sf(mu, var_f, lik_var, w, Y)
        np.testing.assert_allclose(c + s, 1.0, rtol=1e-13)
