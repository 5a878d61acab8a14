"""SquaredExponential kernel (drop-in for gpflow.kernels.SquaredExponential as used by
the reference demos, e.g. demos/demo_tf2.py:37-38) backed by the gfx950 RBF kernels, and
Matern32 / Matern52 (gpflow.kernels.Matern32 / Matern52) backed by csrc/matern.hip.

Hyper-parameters are stored as constrained float32 device tensors (variance [1],
lengthscales [1] or [D]); the kernels read them through device pointers so no
call synchronises with the host.
"""
import numpy as np
import torch

from . import ops
from .config import default_device, default_jitter


def _param(v, device):
    t = torch.as_tensor(np.asarray(v, dtype=np.float32).reshape(-1), device=device)
    return t.clone()


class _Stationary:
    """What the kernel families share: the constrained parameters, K_diag = variance and the
    GPflow-style call forms.  A family adds K, Kuu and the three operations an SVGP layer needs
    of its kernel (kuf_image, factorise, backward)."""

    def __init__(self, variance=1.0, lengthscales=1.0, device=None):
        dev = device or default_device()
        self.device = torch.device(dev)
        if np.any(np.asarray(variance) <= 0) or np.any(np.asarray(lengthscales) <= 0):
            raise ValueError("variance and lengthscales must be positive")
        self.variance = _param(variance, self.device)
        self.lengthscales = _param(lengthscales, self.device)

    # GPflow-style API ---------------------------------------------------------------
    def K_diag(self, X):
        """Stationary.K_diag: variance broadcast to X.shape[:-1] (models.py:133)."""
        X = torch.as_tensor(X)
        return self.variance.expand(X.shape[:-1])

    def __call__(self, X, X2=None, full_cov=True):
        if not full_cov:
            return self.K_diag(X)
        return self.K(X, X2)

    def _x(self, X):
        """Inputs as float32 device rows with unit innermost stride (numpy views such
        as linspace(...)[:, None] carry a 0 stride on the size-1 axis)."""
        X = torch.as_tensor(X)
        if X.dim() == 1:
            X = X[:, None]
        if X.dtype != torch.float32 or X.device != self.device or X.stride(-1) != 1:
            X = torch.empty(X.shape, dtype=torch.float32, device=self.device).copy_(X)
        return X

    def parameters(self):
        return {"variance": self.variance, "lengthscales": self.lengthscales}

    def __repr__(self):
        return (f"{type(self).__name__}(variance={self.variance.tolist()}, "
                f"lengthscales={self.lengthscales.tolist()})")


class SquaredExponential(_Stationary):
    """k(x, x') = variance * exp(-0.5 * ||(x - x') / lengthscales||^2)."""

    def K(self, A, B=None):
        """K(A, B) [M_A, N_B] (models.py:139 calls K(Z, Xnew))."""
        A = self._x(A)
        if B is None:
            return ops.rbf_kuu(A, self.variance, self.lengthscales, 0.0)
        return ops.rbf_kuf(self._x(B), A, self.variance, self.lengthscales)

    def Kuu(self, Z, jitter=None):
        """covariances.Kuu(Z, kernel, jitter) (models.py:135)."""
        return ops.rbf_kuu(self._x(Z), self.variance, self.lengthscales,
                           default_jitter() if jitter is None else jitter)

    # what an SVGP layer needs of its kernel family ------------------------------------
    def kuf_image(self, X, Z, out=None, fmt="x6"):
        """K1: the fragment image of Kuf = K(Z, X), split-bf16 ("x6") or split-f16 ("f16")."""
        return ops.rbf_kuf_x6(X, Z, self.variance, self.lengthscales, out=out, fmt=fmt)

    def factorise(self, Z, want_L=False):
        """Kuu (float64, default jitter) -> L (or None), (L^-1)^T float32 [1, M, M] and info."""
        return ops.kuu_potrf_trtri([Z], [self.variance], [self.lengthscales], default_jitter(), want_L=want_L)

    def backward(self, X, Z, gK, symmetric=False, accumulate=False, gZ=None, g_var=None, g_ls=None):
        """Reverse mode of K(Z, X) for the cotangent gK: (gZ, g_var, g_ls)."""
        return ops.rbf_backward(X, Z, self.variance, self.lengthscales, gK, symmetric=symmetric,
                                accumulate=accumulate, gZ=gZ, g_var=g_var, g_ls=g_ls)


class _Matern(_Stationary):
    """Matern kernels of half-integer smoothness nu = nu2 / 2 on csrc/matern.hip: with
    s = sqrt(nu2) ||(x - x') / lengthscales||, k = variance * p(s) * exp(-s).  Constructor,
    parameters and methods are SquaredExponential's; every operation runs on the Matern
    entries (direct-difference form, translation invariant bit for bit)."""
    nu2 = None

    def K(self, A, B=None):
        A = self._x(A)
        if B is None:
            return ops.matern_kuu(A, self.variance, self.lengthscales, self.nu2, 0.0)
        return ops.matern_kuf(self._x(B), A, self.variance, self.lengthscales, self.nu2)

    def Kuu(self, Z, jitter=None):
        return ops.matern_kuu(self._x(Z), self.variance, self.lengthscales, self.nu2,
                              default_jitter() if jitter is None else jitter)

    def kuf_image(self, X, Z, out=None, fmt="x6"):
        return ops.matern_kuf_image(X, Z, self.variance, self.lengthscales, self.nu2, out=out, fmt=fmt)

    def factorise(self, Z, want_L=False):
        return ops.matern_kuu_potrf_trtri(Z, self.variance, self.lengthscales, self.nu2, default_jitter(),
                                          want_L=want_L)

    def backward(self, X, Z, gK, symmetric=False, accumulate=False, gZ=None, g_var=None, g_ls=None):
        return ops.matern_backward(X, Z, self.variance, self.lengthscales, self.nu2, gK, symmetric=symmetric,
                                   accumulate=accumulate, gZ=gZ, g_var=g_var, g_ls=g_ls)


class Matern32(_Matern):
    """k(x, x') = variance * (1 + s) * exp(-s), s = sqrt(3) * ||(x - x') / lengthscales||."""
    nu2 = 3


class Matern52(_Matern):
    """k(x, x') = variance * (1 + s + s^2 / 3) * exp(-s), s = sqrt(5) * ||(x - x') / lengthscales||."""
    nu2 = 5
