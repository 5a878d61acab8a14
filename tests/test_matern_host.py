"""CPU tests of the Matern kernels: the float64 reference of tests/matern_ref.py against central
finite differences, and the argument checks of every mgp_matern_* entry through ctypes (all
refused before any pointer is read or HIP call made, so no GPU is needed)."""
import ctypes

import numpy as np
import pytest
import torch

from modulatedgps_amd import _lib
from tests import matern_ref as MR

NU2 = [3, 5]


@pytest.mark.parametrize("nu2", NU2)
def test_reference_diagonal_and_symmetry(nu2):
    rng = np.random.default_rng(nu2)
    Z = rng.standard_normal((17, 3))
    ls = np.array([0.6, 1.1, 1.7])
    K = MR.matern_K(Z, Z, 0.7, ls, nu2)
    assert np.array_equal(K.diagonal(), np.full(17, 0.7))          # K(x, x) = variance
    assert np.array_equal(K, K.T)
    assert np.all(K > 0) and np.all(K <= 0.7)
    Ku = MR.matern_Kuu(Z, 0.7, ls, nu2, 1e-3)
    assert np.array_equal(Ku.diagonal(), np.full(17, 0.7 + 1e-3))
    assert np.linalg.eigvalsh(Ku).min() > 0
    # against the closed form at one distance: r = 2 lengthscales along one axis
    one = MR.matern_K(np.zeros((1, 1)), np.array([[1.0]]), 2.0, 0.5, nu2)[0, 0]
    s = np.sqrt(nu2) * 2.0
    assert one == pytest.approx(2.0 * ((1 + s) if nu2 == 3 else (1 + s + s * s / 3)) * np.exp(-s), rel=1e-15)
    t = MR.torch_matern(torch.tensor(Z), torch.tensor(Z[:5]), torch.tensor(0.7, dtype=torch.float64),
                        torch.tensor(ls), nu2)
    assert np.abs(t.numpy() - K[:, :5]).max() < 1e-15


@pytest.mark.parametrize("nu2", NU2)
def test_reference_gradients_match_finite_differences(nu2):
    """Autograd of sum(gK * K(Z, X)) and of sum(gK * K(Z, Z)) (with a coincident pair X[0] = Z[0])
    against central differences of the numpy reference."""
    rng = np.random.default_rng(10 + nu2)
    M, N, D = 6, 9, 3
    Z, X = rng.standard_normal((M, D)), rng.standard_normal((N, D))
    X[0] = Z[0]
    ls, var = np.array([0.7, 1.0, 1.4]), 0.6
    gK, gU = rng.standard_normal((M, N)), rng.standard_normal((M, M))
    gU = 0.5 * (gU + gU.T)

    def f(Zv, lsv, v):
        return float((gK * MR.matern_K(Zv, X, v, lsv, nu2)).sum() + (gU * MR.matern_K(Zv, Zv, v, lsv, nu2)).sum())

    z, l, v = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (Z, ls, var))
    (((torch.tensor(gK) * MR.torch_matern(z, torch.tensor(X), v, l, nu2)).sum()
      + (torch.tensor(gU) * MR.torch_matern(z, z, v, l, nu2)).sum())).backward()
    assert torch.isfinite(z.grad).all()
    h = 1e-6

    def fd(arr, i, which):
        out = []
        for sgn in (1, -1):
            a = arr.copy()
            a[i] += sgn * h
            out.append(f(a, ls, var) if which == "Z" else f(Z, a, var))
        return (out[0] - out[1]) / (2 * h)
    gz = np.array([[fd(Z, (m, d), "Z") for d in range(D)] for m in range(M)])
    gl = np.array([fd(ls, d, "ls") for d in range(D)])
    gv = (f(Z, ls, var + h) - f(Z, ls, var - h)) / (2 * h)
    assert np.abs(z.grad.numpy() - gz).max() < 1e-7 * max(1.0, np.abs(gz).max())
    assert np.abs(l.grad.numpy() - gl).max() < 1e-7 * max(1.0, np.abs(gl).max())
    assert float(v.grad) == pytest.approx(gv, rel=1e-8)


def test_reference_elbo_with_se_kernels_is_the_oracle():
    """matern_ref.elbo with both families "se" is oracle.grad_ref.elbo (the pinned graph)."""
    from oracle import cpu_ref as R
    from oracle import grad_ref as GR
    X, Y, p = R.synthetic_problem(200, 12, 3, 2, 0.8, state="perturbed", S=4)
    z, u = R.explicit_noise(4, 200, 3, seed=5)
    e, _ = MR.elbo_and_grads(X, Y, p, z, u, ("se", "se"))
    pred, assign, lik = GR.params_from_oracle(p, requires_grad=False)
    f = lambda a: torch.tensor(np.asarray(a, np.float32)).double()
    ref = float(GR.elbo(f(X), f(Y), pred, assign, lik, f(z), f(u), p.num_data))
    assert e == pytest.approx(ref, rel=1e-12)
    e52, g52 = MR.elbo_and_grads(X, Y, p, z, u, ("matern52", "matern32"))
    assert np.isfinite(e52) and e52 != e and all(np.all(np.isfinite(g)) for g in g52.values())


def test_classes_are_exported():
    from MixtureGPs import kernels as mk
    from modulatedgps_amd import kernels as k
    assert mk.Matern32 is k.Matern32 and mk.Matern52 is k.Matern52 and mk.SquaredExponential is k.SquaredExponential
    assert (k.Matern32.nu2, k.Matern52.nu2) == (3, 5)
    assert not issubclass(k.Matern52, k.SquaredExponential)
    for name in ("K", "Kuu", "K_diag", "__call__", "parameters", "__repr__", "kuf_image", "factorise", "backward"):
        assert callable(getattr(k.Matern32, name)) and callable(getattr(k.SquaredExponential, name))


# --------------------------------------------------------------------------- argument checks
P = ctypes.c_void_p(4096)   # never dereferenced: every call below is refused first
BIG = 1 << 30


def _kuf(**kw):
    a = dict(X=P, ldx=8, Z=P, ldz=8, N=100, M=64, D=8, var=P, ls=P, n_ls=1, nu2=5, out=P, ldk=100, s=None)
    a.update(kw)
    return _lib.load().mgp_matern_kuf(*a.values())


def _kuu(**kw):
    a = dict(Z=P, ldz=8, M=64, D=8, var=P, ls=P, n_ls=8, nu2=3, jitter=1e-6, out=P, ldk=64, s=None)
    a.update(kw)
    return _lib.load().mgp_matern_kuu(*a.values())


def _img(**kw):
    a = dict(X=P, ldx=8, Z=P, ldz=8, N=100, M=64, D=8, var=P, ls=P, n_ls=1, nu2=5, out=P, nbytes=BIG, fmt=1, s=None)
    a.update(kw)
    return _lib.load().mgp_matern_kuf_image(*a.values())


def _chol(**kw):
    a = dict(Z=P, ldz=8, M=64, D=8, var=P, ls=P, n_ls=1, nu2=5, jitter=1e-6, L=None, LinvT=P, ldl=64, info=P, ws=P,
             wsb=BIG, s=None)
    a.update(kw)
    return _lib.load().mgp_matern_kuu_potrf_trtri(*a.values())


def _bwd(**kw):
    a = dict(X=P, ldx=8, Z=P, ldz=8, N=100, M=64, D=8, var=P, ls=P, n_ls=1, nu2=5, gK=P, ldg=100, sym=0, acc=0,
             gZ=P, ldgz=8, g_var=P, g_ls=P, ws=P, wsb=BIG, s=None)
    a.update(kw)
    return _lib.load().mgp_matern_backward(*a.values())


def test_entries_refuse_bad_arguments():
    wide = dict(ldx=33, ldz=33)
    for call in (_kuf, _img, _bwd):
        assert call(X=None) == -1 and call(ldx=7) == -2 and call(Z=None) == -3 and call(ldz=7) == -4
        assert call(D=0) == -7 and call(D=33, **wide) == 3
        assert call(var=None) == -8 and call(ls=None) == -9 and call(n_ls=3) == -10
        assert call(nu2=4) == -11 and call(nu2=1) == -11 and call(nu2=0) == -11
        assert call(N=0) == 0 and call(M=0) == 0 and call(N=-1, M=-1) == 0    # nothing to do
    assert _kuf(out=None) == -12 and _kuf(ldk=99) == -13
    assert _kuf(ldk=102) == 2 and _kuf(out=ctypes.c_void_p(4100)) == 2
    assert _img(out=None) == -12 and _img(nbytes=_lib.load().mgp_x6_cols_bytes(64, 100) - 1) == -13
    assert _img(fmt=2) == -14 and _img(fmt=-1) == -14 and _img(out=ctypes.c_void_p(4104)) == 2
    assert _bwd(gK=None) == -12 and _bwd(ldg=99) == -13 and _bwd(gZ=None) == -16 and _bwd(ldgz=7) == -17
    assert _bwd(g_var=None) == -18 and _bwd(g_ls=None) == -19
    assert _bwd(ws=None) == 1 and _bwd(wsb=_lib.load().mgp_matern_backward_workspace_bytes(100, 64, 8) - 1) == 1
    assert _bwd(D=33, ldx=33, ldz=33, ldgz=33) == 3
    assert _kuu(Z=None) == -1 and _kuu(ldz=7) == -2 and _kuu(D=0) == -4 and _kuu(D=33, ldz=33, n_ls=33) == 3
    assert _kuu(var=None) == -5 and _kuu(ls=None) == -6 and _kuu(n_ls=2) == -7 and _kuu(nu2=4) == -8
    assert _kuu(jitter=-1.0) == -9 and _kuu(out=None) == -10 and _kuu(ldk=63) == -11 and _kuu(ldk=66) == 2
    assert _kuu(M=0) == 0
    assert _chol(Z=None) == -1 and _chol(ldz=7) == -2 and _chol(D=0) == -4 and _chol(D=33, ldz=33) == 3
    assert _chol(var=None) == -5 and _chol(ls=None) == -6 and _chol(n_ls=2) == -7 and _chol(nu2=4) == -8
    assert _chol(jitter=-1.0) == -9 and _chol(LinvT=None) == -11 and _chol(ldl=63) == -12 and _chol(info=None) == -13
    assert _chol(M=0) == 0
    assert _chol(ws=None) == 1 and _chol(wsb=_lib.load().mgp_matern_chol_workspace_bytes(64) - 1) == 1
    assert _chol(ldl=66) == 2 and _chol(L=ctypes.c_void_p(4100)) == 2 and _chol(ws=ctypes.c_void_p(4104)) == 2


def test_workspace_helpers():
    lib = _lib.load()
    assert lib.mgp_matern_chol_workspace_bytes(0) == 0 and lib.mgp_matern_chol_workspace_bytes(-3) == 0
    assert lib.mgp_matern_chol_workspace_bytes(130) == lib.mgp_chol_workspace_bytes(130, 1) + 130 * 130 * 8
    for N, M, D in ((100, 0, 8), (100, 64, 0), (100, 64, 33), (-1, 64, 8)):
        assert lib.mgp_matern_backward_workspace_bytes(N, M, D) == 0
    # per chunk of 4096 points: [M][1 + 2 DMAX] doubles, DMAX = D rounded up to a power of two
    assert lib.mgp_matern_backward_workspace_bytes(4097, 64, 3) == 2 * 64 * 9 * 8
    assert lib.mgp_matern_backward_workspace_bytes(0, 64, 32) == 64 * 65 * 8


def test_python_surface_refuses_before_any_launch():
    """ops checks nu2 and SVGPModified the kernel class on the host (no device needed)."""
    from modulatedgps_amd import ops
    with pytest.raises(ValueError, match="nu2"):
        ops._nu2(4)
    assert ops._nu2(3) == 3 and ops._nu2(5) == 5
    from modulatedgps_amd.models import SVGPModified
    with pytest.raises(TypeError, match="Matern32"):
        SVGPModified(object(), None, np.zeros((4, 1)), device="cpu")
