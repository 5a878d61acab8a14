"""Pathwise posterior function samples (Matheron's rule with a random-Fourier-feature
prior; Wilson et al. 2020) of a whitened SVGP layer and of the SMGP mixture.

A sample is a function, frozen when it is drawn: LayerPaths(X) evaluates the same S x K
functions at any X, at a cost linear in N, and a call on a shard of X returns the bits of
the unsharded call.  The reference has no counterpart (its demos draw independent marginal
points); DESIGN "Pathwise samples" is the specification:

    phi_j(x)   = sqrt(2 var / R) cos(Omega_j . x + 2 pi phase_j),   Omega = zeta / lengthscales
    v          = q_mu[:, k] + tril(q_sqrt[k]) eps          (whitened inducing draw)
    r          = v - L^-1 (Phi(Z) w)                       (whitened residual)
    f_{s,k}(x) = Phi(x) w + A(x)^T r,                      A(x) = L^-1 k(Z, x)

Evaluation runs K1 and K4 (for the f32 A) with the frozen L^-T and then mgp_path_eval
(csrc/paths.hip); the setup runs K3 once, mgp_path_eval at X = Z without A, and forms v and r
from torch ops with the L^-1 product in float64 (M * M * S * K work, off the hot path).
"""
import math

import numpy as np
import torch

from . import ops
from .config import conditional_mode, default_jitter, forward_image_format
from .likelihoods import MultiClass
from .models import _Stage, _splitmix64


def _shape(a):
    return tuple(a.shape) if hasattr(a, "shape") else tuple(np.asarray(a).shape)


def check_sample_args(num_samples, num_features, M, K, D, basis=None, noise=None):
    """Validate sample_paths' arguments on the host (nothing is uploaded): returns (S, R)."""
    S, R = int(num_samples), int(num_features)
    if S < 1:
        raise ValueError(f"num_samples must be >= 1, got {num_samples}")
    if R < 1:
        raise ValueError(f"num_features must be >= 1, got {num_features}")
    if basis is not None:
        if len(basis) != 2 or _shape(basis[0]) != (R, D) or _shape(basis[1]) != (R,):
            raise ValueError(f"basis must be (zeta [{R}, {D}], phase [{R}])")
    if noise is not None:
        if len(noise) != 2 or _shape(noise[0]) != (S, K, R) or _shape(noise[1]) != (S, K, M):
            raise ValueError(f"noise must be (w [{S}, {K}, {R}], eps [{S}, {K}, {M}])")
    return S, R


def check_points(X, D):
    """X [N, D] (a 1-D X is a column when D == 1), validated on the host."""
    shp = _shape(X)
    if len(shp) == 1 and D == 1:
        return
    if len(shp) != 2 or shp[1] != D:
        raise ValueError(f"X must be [N, {D}], got {shp}")


def _dev(x, device, dtype=torch.float32):
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    return t.to(device=device, dtype=dtype)


class LayerPaths:
    """S joint samples of a layer's K latent functions, a snapshot of the layer when it was
    drawn: it holds its own copies of Z, the kernel parameters, L^-T, Omega and W, so
    training the layer afterwards does not change it.  `zeta`, `phase`, `w`, `eps` are the
    draws ([R, D], [R] in turns, [S, K, R], [S, K, M]).  Calling it with X [N, D] returns the
    device tensor [S, N, K]."""

    def __init__(self, layer, num_samples, num_features=1024, seed=None, basis=None, noise=None):
        M, K, D = layer.num_inducing, layer.num_latent_gps, layer.Z.shape[1]
        S, R = check_sample_args(num_samples, num_features, M, K, D, basis, noise)
        dev = layer.device
        self.device, self.S, self.K, self.R, self.M, self.D = dev, S, K, R, M, D
        if basis is None or noise is None:
            key = layer.next_seed() if seed is None else int(seed)
        if basis is None:
            z, u = ops.philox_noise(key, 0, R, D, 1, dev)
            self.zeta, self.phase = z[0], u[0, :, 0].contiguous()
        else:
            self.zeta, self.phase = _dev(basis[0], dev).contiguous(), _dev(basis[1], dev).contiguous()
        if noise is None:
            self.w = ops.philox_normal2(_splitmix64(key ^ 0x77), 0, R, K, S, dev).permute(0, 2, 1)
            self.eps = ops.philox_normal2(_splitmix64(key ^ 0x65), 0, M, K, S, dev).permute(0, 2, 1)
        else:
            self.w, self.eps = _dev(noise[0], dev), _dev(noise[1], dev)
        self.Z = layer.Z.clone()
        self.variance = layer.kernel.variance.clone()
        self.lengthscales = layer.kernel.lengthscales.clone()
        _, LinvT, info = ops.kuu_potrf_trtri([self.Z], [self.variance], [self.lengthscales], default_jitter())
        layer._last_info = info
        ops.check_info(info)
        self.LinvT = LinvT[0]
        self._Tfr = {}
        self._q0 = torch.zeros(M, 1, dtype=torch.float32, device=dev)   # K4's statistics operand (unused)
        f64 = torch.float64
        # Omega in turns: 1 / 2 pi folded in here, so the kernel reduces the argument exactly
        self.Omega = (self.zeta.to(f64) / self.lengthscales.to(f64) / (2.0 * math.pi)).to(torch.float32)
        C = S * K
        W = ops.padded(R + M, C, dev)
        amp = torch.sqrt(2.0 * self.variance.to(f64) / R)
        W[:R].copy_(amp * self.w.to(f64).permute(2, 0, 1).reshape(R, C))
        prior_z = ops.path_eval(self.Z, self.Omega, self.phase, W[:R])              # (Phi(Z) w)^T [C, M]
        Lq = torch.tril(layer.q_sqrt.to(f64))
        v = layer.q_mu.to(f64).t().unsqueeze(0) + torch.einsum("kmj,skj->skm", Lq, self.eps.to(f64))
        r = v.reshape(C, M) - prior_z.to(f64) @ self.LinvT.to(f64)                  # u^T L^-T = (L^-1 u)^T
        W[R:].copy_(r.t())
        self.W = W

    def _tfr(self, fmt):
        if fmt not in self._Tfr:
            self._Tfr[fmt] = ops.split_upper_x6(self.LinvT, fmt=fmt)
        return self._Tfr[fmt]

    def _x(self, X):
        check_points(X, self.D)
        X = X if isinstance(X, torch.Tensor) else torch.as_tensor(np.asarray(X))
        if X.dim() == 1:
            X = X[:, None]
        if X.dtype != torch.float32 or X.device != self.device or X.stride(-1) != 1:
            X = torch.empty(X.shape, dtype=torch.float32, device=self.device).copy_(X)
        return X

    def solve(self, X, timing=None):
        """A = L^-1 k(Z, X) [M, N] in f32 for device rows X: K1 and K4 with the frozen L^-T (K4
        for its f32 A only: one zero q_mu column feeds its statistics)."""
        M, N = self.M, X.shape[0]
        A = ops.padded(M, N, self.device)
        if conditional_mode() == "f32":
            with _Stage(timing, "rbf_kuf"):
                Kuf = ops.rbf_kuf(X, self.Z, self.variance, self.lengthscales)
            with _Stage(timing, "trsm_stats"):
                ops.trsm_stats(self.LinvT, Kuf, self._q0, A=A)
            return A
        fmt = forward_image_format()
        with _Stage(timing, "rbf_kuf"):
            Kfr = ops.rbf_kuf_x6(X, self.Z, self.variance, self.lengthscales, fmt=fmt)
        with _Stage(timing, "trsm_stats"):
            ops.trsm_stats_x6(self._tfr(fmt), Kfr, self._q0, M, N, A=A,
                              f16_variance=self.variance if fmt == "f16" else None, in_fmt=fmt)
        return A

    def __call__(self, X, timing=None):
        X = self._x(X)
        N = X.shape[0]
        if N == 0:
            return torch.empty(self.S, 0, self.K, dtype=torch.float32, device=self.device)
        A = self.solve(X, timing)
        with _Stage(timing, "path_eval"):
            out = ops.path_eval(X, self.Omega, self.phase, self.W, A=A)              # [S K, N]
        return out.unflatten(0, (self.S, self.K)).permute(0, 2, 1)


class MixturePaths:
    """Coherent samples of an SMGP: `.pred` (expert curves f_k) and `.assign` (assignment-logit
    curves a_k), LayerPaths of the two layers drawn with the same S.  Every method takes
    X [N, D] and returns a device tensor."""

    def __init__(self, model, num_samples, num_features=1024, seed=None):
        check_sample_args(num_samples, num_features, 0, 0, 0)
        key = model.next_seed() if seed is None else int(seed)
        self._multiclass = isinstance(model.likelihood.likelihood, MultiClass)
        self.pred = LayerPaths(model.pred_layer, num_samples, num_features, seed=_splitmix64(key ^ 0x70))
        self.assign = LayerPaths(model.assign_layer, num_samples, num_features, seed=_splitmix64(key ^ 0x61))

    def predict_f(self, X):
        """Expert curves [S, N, K]."""
        return self.pred(X)

    def predict_logits(self, X):
        """Assignment-logit curves [S, N, K]."""
        return self.assign(X)

    def predict_weights(self, X):
        """softmax_k of the logit curves [S, N, K]."""
        return torch.softmax(self.assign(X), dim=-1)

    def predict_mean(self, X):
        """sum_k weights_k f_k [S, N]: the mixture's mean curve per sample."""
        if self._multiclass:
            raise NotImplementedError(
                "a MultiClass pred likelihood has no expert mixture: W multiplies one value per point, "
                "and predict_y already returns the class probabilities")
        return (self.predict_weights(X) * self.pred(X)).sum(-1)
