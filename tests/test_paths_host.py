"""CPU tests of the pathwise-sample feature (csrc/paths.hip, modulatedgps_amd/paths.py): the
C-ABI entry is bound, declared and exported and checks its arguments before any HIP call;
the Python validation raises without a device; and the float64 reference (tests/path_ref.py)
reproduces predict_f's mean exactly and its variance on average over bases."""
import ctypes
import re

import numpy as np
import pytest

from modulatedgps_amd import _lib
from oracle import cpu_ref as R
from tests import path_ref

MGP_OP_PATH_EVAL = 15


def test_path_eval_is_bound_declared_and_exported():
    assert "mgp_path_eval" in _lib.SIGNATURES
    assert "mgp_path_eval" in _lib.header_symbols()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "mgp_path_eval")
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r"\bMGP_OP_PATH_EVAL\s*=\s*15\b", header)
    # the entry needs no workspace
    assert _lib.load().mgp_workspace_bytes(MGP_OP_PATH_EVAL, 1024, 65536, 128) == 0


def test_path_eval_checks_arguments():
    """Every bad argument is rejected with the code documented in mgp_hip.h before any
    pointer is read or HIP call made; N = 0 is a no-op after the checks."""
    lib = _lib.load()
    c = ctypes.c_void_p(256)
    N, D, Rn, M, C = 100, 2, 37, 25, 12
    names = ("X", "ldx", "N", "D", "Om", "ldo", "ph", "R", "A", "lda", "M", "W", "ldw", "C", "out", "ldout", "s")
    base = dict(X=c, ldx=D, N=N, D=D, Om=c, ldo=D, ph=c, R=Rn, A=c, lda=N, M=M, W=c, ldw=C, C=C, out=c, ldout=N,
                s=None)
    assert len(names) == len(_lib.SIGNATURES["mgp_path_eval"][1])
    call = lambda **kw: lib.mgp_path_eval(*[kw.get(n, base[n]) for n in names])
    assert call(X=None) == -1
    assert call(ldx=D - 1) == -2
    assert call(D=0) == -4
    assert call(D=33, ldx=64, ldo=64) == 3
    assert call(D=33, ldx=64, ldo=64, N=0) == 3          # the limit is checked before the no-op
    assert call(Om=None) == -5
    assert call(ldo=D - 1) == -6
    assert call(ph=None) == -7
    assert call(R=0) == -8
    assert call(A=None) == -9
    assert call(lda=N - 4) == -10
    assert call(M=-1) == -11
    assert call(W=None) == -12
    assert call(ldw=C - 4) == -13
    assert call(C=0) == -14
    assert call(out=None) == -15
    assert call(ldout=N - 1) == -16
    # float4 rows of W and A
    assert call(ldw=C + 2) == 2 and call(lda=N + 2) == 2
    assert call(W=ctypes.c_void_p(260)) == 2 and call(A=ctypes.c_void_p(264)) == 2
    # prior only: A and lda are not looked at
    assert call(M=0, A=None, lda=0, N=0) == 0
    assert call(N=0) == 0 and call(N=-1, lda=0, ldout=0) == 0
    assert call(N=0, X=None) == -1 and call(N=0, out=None) == -15


def test_python_validation_raises_without_a_device():
    from modulatedgps_amd import paths
    M, K, D = 20, 3, 2
    assert paths.check_sample_args(4, 64, M, K, D) == (4, 64)
    with pytest.raises(ValueError):
        paths.check_sample_args(0, 64, M, K, D)
    with pytest.raises(ValueError):
        paths.check_sample_args(4, 0, M, K, D)
    zeta, phase = np.zeros((64, D)), np.zeros(64)
    w, eps = np.zeros((4, K, 64)), np.zeros((4, K, M))
    assert paths.check_sample_args(4, 64, M, K, D, basis=(zeta, phase), noise=(w, eps)) == (4, 64)
    for basis in ((zeta[:, :1], phase), (zeta, phase[:-1]), (zeta[:-1], phase), (zeta,)):
        with pytest.raises(ValueError):
            paths.check_sample_args(4, 64, M, K, D, basis=basis)
    for noise in ((w[:3], eps), (w, eps[:, :, :-1]), (w[:, :2], eps), (w.transpose(0, 2, 1), eps), (w,)):
        with pytest.raises(ValueError):
            paths.check_sample_args(4, 64, M, K, D, noise=noise)
    paths.check_points(np.zeros((7, D)), D)
    paths.check_points(np.zeros(7), 1)
    for X in (np.zeros((7, D + 1)), np.zeros(7), np.zeros((2, 7, D))):
        with pytest.raises(ValueError):
            paths.check_points(X, D)
    # the methods exist on the layer and on both mixtures, and MixtureGPs re-exports the classes
    from MixtureGPs.models import SMGP, LayerPaths, MixturePaths, SMGPModified, SVGPModified
    assert callable(SVGPModified.sample_paths) and callable(SMGP.sample_paths)
    assert SMGPModified.sample_paths is SMGP.sample_paths
    assert LayerPaths is paths.LayerPaths and MixturePaths is paths.MixturePaths


def _problem(seed=3, N=40, M=8, K=2, D=1):
    rng = np.random.default_rng(seed)
    L = dict(Z=np.linspace(-2.0, 2.0, M)[:, None] + 0.02 * rng.standard_normal((M, D)), variance=0.8,
             lengthscales=0.7, q_mu=0.5 * rng.standard_normal((M, K)),
             q_sqrt=0.3 * np.eye(M)[None] + np.tril(0.05 * rng.standard_normal((K, M, M))))
    return rng, L, np.linspace(-2.5, 2.5, N)[:, None]


def test_reference_zero_draw_is_predict_f_mean():
    rng, L, X = _problem()
    Rn, S, K, M = 64, 2, 2, L["Z"].shape[0]
    zeta, phase = rng.standard_normal((Rn, 1)), rng.random(Rn)
    f, mean, var = path_ref.layer_paths(X, L, zeta, phase, np.zeros((S, K, Rn)), np.zeros((S, K, M)))
    fm, _ = R.svgp_predict_f(X, L["Z"], L["variance"], L["lengthscales"], L["q_mu"], L["q_sqrt"])
    assert np.abs(f - fm[None]).max() <= 1e-12 * max(1.0, np.abs(fm).max())
    assert np.abs(mean - fm).max() <= 1e-12 * max(1.0, np.abs(fm).max())
    # path_eval is the same function in the stacked form
    w, eps = rng.standard_normal((S, K, Rn)), rng.standard_normal((S, K, M))
    f, _, _ = path_ref.layer_paths(X, L, zeta, phase, w, eps)
    f0, _, _ = path_ref.layer_paths(X, L, zeta, phase, w, np.zeros_like(eps))
    assert np.abs(f - f0).max() > 1e-3


def test_reference_variance_is_unbiased_over_bases():
    """E_basis |g(x)|^2 = var - |A(x)|^2: the analytic variance given the basis, averaged
    over 32 bases, deviates less from predict_f's variance at R = 4096 than at R = 64."""
    _, L, X = _problem()
    _, fv = R.svgp_predict_f(X, L["Z"], L["variance"], L["lengthscales"], L["q_mu"], L["q_sqrt"])
    worst = {}
    for Rn in (64, 4096):
        acc = np.zeros_like(fv)
        for b in range(32):
            rng = np.random.default_rng(1000 + b)
            zeta, phase = rng.standard_normal((Rn, 1)), rng.random(Rn)
            _, _, var = path_ref.layer_paths(X, L, zeta, phase, np.zeros((1, 2, Rn)), np.zeros((1, 2, 8)))
            acc += var
        worst[Rn] = np.abs(acc / 32 / fv - 1.0).max()
        print(f"SCOREERR path_var_bias_R{Rn} {worst[Rn]:.3e}")
    assert worst[4096] < worst[64]
