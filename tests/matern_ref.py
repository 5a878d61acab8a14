"""Float64 references for the Matern kernels (tests/test_matern_host.py, tests/test_gpu_matern.py).

    s = sqrt(nu2) sqrt(sum_d ((a_d - b_d) / l_d)^2),  nu2 = 2 nu in {3, 5}
    nu2 = 3: k = var (1 + s) exp(-s)        nu2 = 5: k = var (1 + s + s^2 / 3) exp(-s)

matern_K / matern_Kuu: numpy, differences of the coordinates taken directly (no expanded square
distance, so nothing cancels far from the origin).  torch_kernel(family): the same as a
differentiable torch callable (A, B, variance, lengthscales) -> [M, N]; family "se" is
oracle.grad_ref.rbf.  elbo(): the SMGP / SMGPModified ELBO of oracle.grad_ref with a kernel callable
per layer -- its data term and KL are oracle.grad_ref.data_term and gauss_kl_white, so only the two
covariance builds differ from the pinned SquaredExponential graph."""
import numpy as np
import torch

from oracle import grad_ref as GR

JITTER = 1e-6
FAMILIES = {"se": None, "matern32": 3, "matern52": 5}


def _poly(s, nu2):
    if nu2 == 3:
        return 1.0 + s
    if nu2 == 5:
        return 1.0 + s + s * s / 3.0
    raise ValueError("nu2 must be 3 or 5")


def matern_K(A, B, variance, lengthscales, nu2):
    """K(A, B) [M, N] in float64."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    ls = np.broadcast_to(np.asarray(lengthscales, np.float64).reshape(-1), (A.shape[1],))
    r2 = np.zeros((A.shape[0], B.shape[0]))
    for d in range(A.shape[1]):   # one [M, N] plane at a time: no [M, N, D] array
        r2 += ((A[:, d, None] - B[None, :, d]) / ls[d]) ** 2
    s = np.sqrt(nu2 * r2)
    return float(variance) * _poly(s, nu2) * np.exp(-s)


def matern_Kuu(Z, variance, lengthscales, nu2, jitter=JITTER):
    return matern_K(Z, Z, variance, lengthscales, nu2) + jitter * np.eye(np.shape(Z)[0])


def torch_matern(A, B, variance, lengthscales, nu2):
    """Differentiable K(A, B).  sqrt is taken of max(r2, 1e-36) (GPflow's own guard): at
    coincident points the value is exact to 1e-18 and the gradient is the analytic zero."""
    diff = (A[:, None, :] - B[None, :, :]) / lengthscales
    r2 = (diff ** 2).sum(-1)
    s = torch.sqrt(nu2 * torch.clamp(r2, min=1e-36))
    return variance * _poly(s, nu2) * torch.exp(-s)


def torch_kernel(family):
    nu2 = FAMILIES[family]
    if nu2 is None:
        return GR.rbf
    return lambda A, B, variance, lengthscales: torch_matern(A, B, variance, lengthscales, nu2)


def layer_conditional(X, L, kern):
    """oracle.grad_ref.layer_conditional with the covariance callable `kern`: fmean, fvar [N, K]."""
    Z = L["Z"]
    M = Z.shape[0]
    Kuu = kern(Z, Z, L["variance"], L["lengthscales"]) + JITTER * torch.eye(M, dtype=Z.dtype)
    Lm = torch.linalg.cholesky(Kuu)
    A = torch.linalg.solve_triangular(Lm, kern(Z, X, L["variance"], L["lengthscales"]), upper=False)
    fmean = A.T @ L["q_mu"]
    LTA = torch.tril(L["q_sqrt"]).transpose(1, 2) @ A
    fvar = L["variance"] - (A ** 2).sum(0)[:, None] + (LTA ** 2).sum(1).T
    return fmean, fvar


def elbo(X, Y, pred, assign, lik_var, z, u, num_data, kern_f, kern_a, assign_lik_var=None):
    """The ELBO of oracle.grad_ref.elbo with a kernel callable per layer (float64 scalar tensor)."""
    mu_f, var_f = layer_conditional(X, pred, kern_f)
    mu_a, var_a = layer_conditional(X, assign, kern_a)
    data = GR.data_term(mu_f, var_f, mu_a, var_a, Y, lik_var, z, u, assign_lik_var=assign_lik_var)
    kl = GR.gauss_kl_white(pred["q_mu"], pred["q_sqrt"]) + GR.gauss_kl_white(assign["q_mu"], assign["q_sqrt"])
    return data / X.shape[0] - kl / num_data


def elbo_and_grads(X, Y, p, z, u, families, a_var=None, dtype=torch.float64):
    """(ELBO, {name: gradient}) of an oracle SMGPParams `p` with the kernel families
    (pred, assign), named as SMGP.trainable_parameters(); q_sqrt gradients lower triangular."""
    pred, assign, lik = GR.params_from_oracle(p)
    leaf = lambda t: t.detach().to(dtype).requires_grad_(True)
    pred = {k: leaf(v) for k, v in pred.items()}
    assign = {k: leaf(v) for k, v in assign.items()}
    lik = leaf(lik)
    rnd = lambda a: torch.tensor(np.asarray(a, np.float32)).to(dtype)
    av = None
    if a_var is not None:
        av = leaf(torch.tensor(np.asarray(a_var, np.float32).reshape(-1)))
    e = elbo(rnd(X), rnd(Y), pred, assign, lik, rnd(z), rnd(u), p.num_data, torch_kernel(families[0]),
             torch_kernel(families[1]), assign_lik_var=av)
    e.backward()
    g = {"lik_variance": lik.grad.double().numpy()}
    if av is not None:
        g["assign_lik_variance"] = av.grad.double().numpy()
    for name, L in (("pred", pred), ("assign", assign)):
        for k in GR.LAYER_KEYS:
            gk = L[k].grad.double().numpy()
            g[name + "." + k] = np.tril(gk) if k == "q_sqrt" else gk
    return float(e.detach()), g


def device_kernel(family, variance, lengthscales, device):
    from modulatedgps_amd import kernels
    cls = {"se": kernels.SquaredExponential, "matern32": kernels.Matern32, "matern52": kernels.Matern52}[family]
    return cls(variance=variance, lengthscales=lengthscales, device=device)


def build_model(p, device, families, a_var=None, seed=0):
    """tests.helpers.build_model with a kernel family per layer (SMGPModified when a_var is given)."""
    from modulatedgps_amd.likelihoods import GaussianModified
    from modulatedgps_amd.models import SMGP, SMGPModified, SVGPModified
    K = p.lik_variance.shape[1]
    lik = GaussianModified(variance=p.lik_variance, device=device)
    layers = []
    for L, fam in zip((p.pred, p.assign), families):
        layer = SVGPModified(device_kernel(fam, L["variance"], L["lengthscales"], device), lik, L["Z"],
                             num_latent_gps=K, whiten=True, device=device)
        layer.set_variational(L["q_mu"], L["q_sqrt"])
        layers.append(layer)
    if a_var is None:
        return SMGP(lik, layers[0], layers[1], K=K, num_samples=p.S, num_data=p.num_data, seed=seed)
    return SMGPModified(lik, GaussianModified(variance=a_var, device=device), layers[0], layers[1], K=K,
                        num_samples=p.S, num_data=p.num_data, seed=seed)
