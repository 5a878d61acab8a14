"""float64 statement of the pathwise posterior samples (modulatedgps_amd/paths.py,
csrc/paths.hip; DESIGN "Pathwise samples"), with explicit basis and draws:

    Omega      = zeta / lengthscales,  phi_j(x) = sqrt(2 var / R) cos(Omega_j . x + 2 pi phase_j)
    v          = q_mu[:, k] + tril(q_sqrt[k]) eps[s, k]
    r          = v - L^-1 (Phi(Z) w[s, k]),             L = chol(Kuu + jitter I)
    f_{s,k}(x) = Phi(x) w[s, k] + A(x)^T r,             A(x) = L^-1 k(Z, x)

Given the basis f_{s,k}(x) is Gaussian with mean A(x)^T q_mu[:, k] and variance
|g(x)|^2 + |tril(q_sqrt[k])^T A(x)|^2, g(x) = Phi(x) - Phi(Z)^T L^-T A(x)."""
import numpy as np
import scipy.linalg as sla

from oracle import cpu_ref as R


def features(X, zeta, phase, variance, lengthscales):
    """Phi(X) [N, R] in float64."""
    X = np.asarray(X, np.float64)
    if X.ndim == 1:
        X = X[:, None]
    Omega = np.asarray(zeta, np.float64) / np.asarray(lengthscales, np.float64)
    Rn = Omega.shape[0]
    arg = X @ Omega.T + 2.0 * np.pi * np.asarray(phase, np.float64)[None, :]
    return np.sqrt(2.0 * float(np.asarray(variance).reshape(-1)[0]) / Rn) * np.cos(arg)


def path_eval(X, Omega_turns, phase, W, A=None):
    """mgp_path_eval in float64: out [C, N] from Omega [R, D] and phase [R] in turns,
    W [R + M, C] and A [M, N] (None: prior rows only)."""
    X = np.asarray(X, np.float64)
    W = np.asarray(W, np.float64)
    Rn = np.asarray(Omega_turns).shape[0]
    cosf = np.cos(2.0 * np.pi * (X @ np.asarray(Omega_turns, np.float64).T + np.asarray(phase, np.float64)[None, :]))
    out = W[:Rn].T @ cosf.T
    if A is not None:
        out = out + W[Rn:].T @ np.asarray(A, np.float64)
    return out


def layer_paths(X, L, zeta, phase, w, eps, jitter=None):
    """Paths of a layer L (dict Z, variance, lengthscales, q_mu, q_sqrt) at X [N, D] for the
    basis (zeta [R, D], phase [R] in turns) and draws (w [S, K, R], eps [S, K, M]).
    Returns (f [S, N, K], mean [N, K], var [N, K]): the paths and their analytic mean and
    variance over the draws, given the basis."""
    Z, var, ls = np.asarray(L["Z"], np.float64), L["variance"], L["lengthscales"]
    if Z.ndim == 1:
        Z = Z[:, None]
    X = np.asarray(X, np.float64)
    if X.ndim == 1:
        X = X[:, None]
    w, eps = np.asarray(w, np.float64), np.asarray(eps, np.float64)
    q_mu, Lq = np.asarray(L["q_mu"], np.float64), np.tril(np.asarray(L["q_sqrt"], np.float64))
    Lm = np.linalg.cholesky(R.rbf_Kuu(Z, var, ls, jitter))
    A = sla.solve_triangular(Lm, R.rbf_K(Z, X, var, ls), lower=True)                 # [M, N]
    PhiX, PhiZ = features(X, zeta, phase, var, ls), features(Z, zeta, phase, var, ls)
    v = q_mu.T[None] + np.einsum("kmj,skj->skm", Lq, eps)                             # [S, K, M]
    u = np.einsum("mr,skr->skm", PhiZ, w)                                             # Phi(Z) w
    S, K, M = v.shape
    Linv_u = sla.solve_triangular(Lm, u.reshape(S * K, M).T, lower=True).T.reshape(S, K, M)
    r = v - Linv_u
    f = np.einsum("nr,skr->snk", PhiX, w) + np.einsum("mn,skm->snk", A, r)
    mean = A.T @ q_mu
    G = PhiX - (sla.solve_triangular(Lm, PhiZ, lower=True).T @ A).T                   # g(x)^T rows, [N, R]
    LTA = np.swapaxes(Lq, -1, -2) @ A[None]                                           # [K, M, N]
    var_f = np.sum(G * G, -1)[:, None] + np.sum(LTA * LTA, -2).T
    return f, mean, var_f
