"""CPU tests of the mixture predictive: the C-ABI entries' argument checks (all made before
any HIP call, so they run without a GPU) and known answers of the float64 statement
tests/mixture_ref.py that the GPU tests compare the kernels with."""
import ctypes
import re

import numpy as np

from modulatedgps_amd import _lib
from oracle import cpu_ref as R
from tests import mixture_ref as MR
from tests.helpers import load_golden, params_from_golden

ENTRIES = ("mgp_mixture_predict_workspace_bytes", "mgp_mixture_predict", "mgp_mixture_density_grid")
MGP_OP_MIXTURE_PREDICT = 13
MGP_ERR_WORKSPACE, MGP_ERR_UNSUPPORTED = 1, 3


def test_entries_are_bound_declared_and_exported():
    syms = _lib.header_symbols()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and name in syms and hasattr(raw, name), name
    text = open(_lib.HEADER_PATH).read()
    assert re.search(r"MGP_OP_MIXTURE_PREDICT\s*=\s*13\b", text)


def test_workspace_query_matches_the_front():
    lib = _lib.load()
    for N, K in ((1, 1), (64, 3), (65, 3), (1000, 32), (65536, 8)):
        nbytes = lib.mgp_mixture_predict_workspace_bytes(N, K)
        assert nbytes == lib.mgp_workspace_bytes(MGP_OP_MIXTURE_PREDICT, 0, N, K)
        assert nbytes >= 8 and nbytes % 8 == 0


def _predict(**kw):
    """mgp_mixture_predict with valid (never dereferenced) arguments, overridden by kw."""
    lib = _lib.load()
    c = ctypes.c_void_p(256)
    N, K = 100, 3
    base = dict(mu_f=c, var_f=c, mu_a=c, var_a=c, ldf=N, lik_var=c, Y=c, N=N, K=K, S=5, jitter=1e-6, noise_z=None,
                seed=0, n_offset=0, weights=c, mix_mean=c, mix_var=c, log_density=c, log_density_sum=c,
                workspace=c, workspace_bytes=lib.mgp_mixture_predict_workspace_bytes(N, K), stream=None)
    assert len(base) == len(_lib.SIGNATURES["mgp_mixture_predict"][1])
    base.update(kw)
    return lib.mgp_mixture_predict(*base.values())


def test_predict_rejects_bad_arguments_before_any_hip_call():
    assert _predict(K=33) == MGP_ERR_UNSUPPORTED
    assert _predict(jitter=-1.0) == -11
    assert _predict(jitter=float("nan")) == -11
    assert _predict(S=-1) == -10
    nbytes = _lib.load().mgp_mixture_predict_workspace_bytes(100, 3)
    assert _predict(workspace_bytes=nbytes - 1) == MGP_ERR_WORKSPACE
    assert _predict(workspace=None) == MGP_ERR_WORKSPACE
    # log_density / log_density_sum without Y
    assert _predict(Y=None) == -7
    assert _predict(Y=None, log_density_sum=None) == -7
    assert _predict(Y=None, log_density=None) == -7
    # the rest of the documented codes
    assert _predict(mu_f=None) == -1 and _predict(var_f=None) == -2
    assert _predict(mu_a=None) == -3 and _predict(var_a=None) == -4
    assert _predict(ldf=99) == -5 and _predict(lik_var=None) == -6
    assert _predict(K=0) == -9 and _predict(n_offset=-1) == -14
    # N <= 0: nothing to do (after the checks)
    assert _predict(N=0) == 0 and _predict(N=-3) == 0
    assert _predict(N=0, S=-1) == -10


def test_density_grid_rejects_bad_arguments_before_any_hip_call():
    lib = _lib.load()
    c = ctypes.c_void_p(256)
    base = dict(mu_f=c, var_f=c, ldf=100, lik_var=c, weights=c, N=100, K=3, y_grid=c, G=7, density=c, ldd=7,
                stream=None)
    assert len(base) == len(_lib.SIGNATURES["mgp_mixture_density_grid"][1])
    call = lambda **kw: lib.mgp_mixture_density_grid(*{**base, **kw}.values())
    assert call(mu_f=None) == -1 and call(var_f=None) == -2 and call(ldf=99) == -3
    assert call(lik_var=None) == -4 and call(weights=None) == -5
    assert call(K=0) == -7 and call(K=33) == MGP_ERR_UNSUPPORTED
    assert call(y_grid=None) == -8 and call(G=-1) == -9 and call(density=None) == -10 and call(ldd=6) == -11
    assert call(N=0) == 0 and call(G=0, ldd=0) == 0


def test_reference_single_expert_is_the_gaussian_log_pdf():
    """K = 1: the weights are identically 1 and the log density is the expert's Gaussian
    log pdf, for any S and any noise."""
    rng = np.random.default_rng(0)
    N = 50
    mu_f, mu_a = rng.normal(size=(N, 1)) * 3, rng.normal(size=(N, 1)) * 5
    var_f, var_a = rng.uniform(0.01, 1, (N, 1)), rng.uniform(0.01, 3, (N, 1))
    lik_var = np.array([0.3])
    Y = mu_f[:, 0] + rng.normal(size=N) * 5
    s2 = var_f[:, 0] + 0.3
    pdf = -0.5 * np.log(2 * np.pi * s2) - 0.5 * (Y - mu_f[:, 0]) ** 2 / s2
    for S in (0, 1, 7):
        z = rng.normal(size=(S, N, 1)) if S else None
        out = MR.predict(mu_f, var_f, mu_a, var_a, lik_var, Y=Y, z=z, y_grid=Y[:3])
        np.testing.assert_allclose(out["weights"], 1.0, rtol=0, atol=1e-15)
        np.testing.assert_allclose(out["log_density"], pdf, rtol=1e-13)
        np.testing.assert_allclose(out["mix_mean"], mu_f[:, 0], rtol=1e-14)
        np.testing.assert_allclose(out["mix_var"], s2, rtol=1e-14)
        np.testing.assert_allclose(np.log(out["density"][np.arange(3), np.arange(3)]), pdf[:3], rtol=1e-12)


def test_reference_plug_in_weights_are_predict_assign():
    d = load_golden("case_c1.npz")
    p = params_from_golden(d)
    mu_a, var_a = R._layer_f(p.assign, d["Xtest"])
    w = MR.weights(mu_a, var_a)
    np.testing.assert_allclose(w, R.predict_assign(d["Xtest"], p), rtol=1e-13, atol=1e-300)
    np.testing.assert_allclose(w, d["predict_assign"], rtol=1e-9)
    np.testing.assert_allclose(w.sum(-1), 1.0, rtol=1e-14)


def test_reference_log_density_stays_finite_in_the_tails():
    """A point 20 sigma from every expert: log density near -200, where the densities
    themselves are far below float32's range."""
    mu_f = np.array([[0.0, 1.0, -1.0]])
    var_f = np.full((1, 3), 1e-4)
    lik_var = np.array([1e-4, 1e-4, 1e-4])
    mu_a, var_a = np.array([[0.0, -15.0, 15.0]]), np.ones((1, 3))
    Y = np.array([1.0 + 20 * np.sqrt(2e-4)])
    ld = MR.log_density(mu_f, var_f, mu_a, var_a, lik_var, Y)
    w = MR.weights(mu_a, var_a)
    direct = np.log(np.sum(w * np.exp(MR.log_normal(Y.reshape(-1, 1), mu_f, var_f, lik_var))))
    assert np.isfinite(ld).all() and -230 < ld[0] < -190
    np.testing.assert_allclose(ld, direct, rtol=1e-12)
