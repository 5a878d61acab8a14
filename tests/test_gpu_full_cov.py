"""Full-covariance predictions and joint posterior samples of an SVGP layer
(SVGPModified.predict_f(Xnew, full_cov=True) / predict_f_samples, csrc/fullcov.hip) against
the float64 semantics of GPflow's base_conditional(full_cov=True, white=True) as the
reference's posterior plugin reaches it (MixtureGPs/models.py:133-143).

Gate: the project's 1e-4 normwise against float64 (tests/test_gpu_api.py), per expert on
cov[k]."""
import functools

import numpy as np
import pytest
import scipy.linalg as sla
import torch

from oracle import cpu_ref as R
from tests.helpers import build_model, load_golden, normwise, params_from_golden, to_np

pytestmark = pytest.mark.gpu

GATE = 1e-4


def full_cov_ref(X, L, jitter=None):
    """float64 mean [N, K] and cov [K, N, N] of base_conditional(Kmn, Kmm, Knn, q_mu,
    full_cov=True, q_sqrt, white=True) with Knn = K(X, X) (no jitter), Kmm = Kuu + jitter I."""
    Z, var, ls = L["Z"], L["variance"], L["lengthscales"]
    Lm = np.linalg.cholesky(R.rbf_Kuu(Z, var, ls, jitter))
    A = sla.solve_triangular(Lm, R.rbf_K(Z, X, var, ls), lower=True)
    Knn = R.rbf_K(X, X, var, ls)
    base = Knn - A.T @ A
    covs = []
    for Lk in np.tril(L["q_sqrt"]):
        C = Lk.T @ A
        covs.append(base + C.T @ C)
    return A.T @ L["q_mu"], np.stack(covs), A


def check_cov(cov, cov_ref, var_ref=None):
    """cov [K, N, N] device tensor: per expert within the gate of cov_ref, bitwise
    symmetric, diagonal within the gate of the marginal variance var_ref [N, K]."""
    assert tuple(cov.shape) == cov_ref.shape
    assert torch.equal(cov, cov.transpose(-1, -2))
    c = to_np(cov)
    for k in range(c.shape[0]):
        err = normwise(c[k], cov_ref[k])
        print(f"expert {k}: cov normwise {err:.3e}")
        assert err < GATE
        if var_ref is not None:
            errd = normwise(np.diag(c[k]), var_ref[:, k])
            print(f"expert {k}: diag normwise {errd:.3e}")
            assert errd < GATE


@functools.lru_cache(maxsize=None)
def golden(case):
    d = load_golden(case + ".npz")
    return d, params_from_golden(d)


@functools.lru_cache(maxsize=None)
def golden_ref(case, layer):
    d, p = golden(case)
    L = getattr(p, layer)
    mean, cov, _ = full_cov_ref(d["Xtest"], L)
    _, var = R.svgp_predict_f(d["Xtest"], L["Z"], L["variance"], L["lengthscales"], L["q_mu"], L["q_sqrt"])
    return mean, cov, var


def _layer(model, name):
    return model.pred_layer if name == "pred" else model.assign_layer


def _dev(x, device):
    return torch.as_tensor(np.asarray(x), dtype=torch.float32, device=device)


# --------------------------------------------------------------------------- 1. kernel alone
@pytest.mark.parametrize("N,M,K,D", [(1, 20, 1, 1), (33, 25, 3, 1), (100, 130, 3, 2), (257, 64, 2, 8),
                                     (2900, 16, 2, 1)])
def test_full_cov_kernel(device, N, M, K, D):
    """(2900, 16, 2, 1): 276 output tiles, more than the 256 CUs -- workgroups that own a
    tile with every expert beside tiles cut by expert (the smaller shapes are all cut)."""
    from modulatedgps_amd import _lib, ops
    rng = np.random.default_rng(100 * N + M)
    X = rng.standard_normal((N, D))
    Z = rng.standard_normal((M, D))
    ls = 0.8 + 0.6 * rng.random(D) if D == 2 else np.float64(0.9 * np.sqrt(D))
    L = dict(Z=Z, variance=0.7, lengthscales=ls, q_mu=0.5 * rng.standard_normal((M, K)),
             q_sqrt=0.5 * np.eye(M)[None] + np.tril(0.1 * rng.standard_normal((K, M, M))))
    _, cov_ref, A64 = full_cov_ref(X, L)
    _, var_ref = R.svgp_predict_f(X, Z, 0.7, ls, L["q_mu"], L["q_sqrt"])

    Xd = _dev(X, device)
    A = ops.as_padded(_dev(A64, device))
    q_sqrt = ops.as_padded(_dev(L["q_sqrt"], device))
    var, lst = _dev([0.7], device), _dev(np.atleast_1d(ls), device)
    ld = (N + 3) // 4 * 4
    sentinel = -12345.0
    buf = torch.full((K, N, ld), sentinel, dtype=torch.float32, device=device)
    nbytes = _lib.load().mgp_full_cov_workspace_bytes(M, N, K)
    assert nbytes >= K * M * N * 4
    guard = 4096
    ws = torch.full((nbytes + guard,), 0xA5, dtype=torch.uint8, device=device)
    cov = ops.full_cov_conditional(Xd, A, q_sqrt, var, lst, out=buf[..., :N], workspace=ws[:nbytes])
    assert cov.data_ptr() == buf.data_ptr() and tuple(cov.shape) == (K, N, N)
    check_cov(cov, cov_ref, var_ref)
    assert bool((buf[..., N:] == sentinel).all())          # padding columns untouched
    assert bool((ws[nbytes:] == 0xA5).all())               # nothing past workspace_bytes
    # allocated by the wrapper: the same bits in a padded [K, N, N] view
    cov2 = ops.full_cov_conditional(Xd, A, q_sqrt, var, lst)
    assert cov2.stride(-2) % 4 == 0 and torch.equal(cov2, cov)


# --------------------------------------------------------------------------- 2. the API
@pytest.mark.parametrize("layer", ["pred", "assign"])
@pytest.mark.parametrize("case", ["case_demo_perturbed", "case_c1"])
def test_predict_f_full_cov(device, case, layer):
    from modulatedgps_amd import config
    d, p = golden(case)
    lay = _layer(build_model(p, device), layer)
    mean_ref, cov_ref, var_ref = golden_ref(case, layer)
    K = cov_ref.shape[0]
    Xd = _dev(d["Xtest"], device)
    mean0, var0 = lay.predict_f(Xd)
    mean, cov = lay.predict_f(Xd, full_cov=True)
    assert tuple(mean.shape) == (100, K) and tuple(cov.shape) == (K, 100, 100)
    assert torch.equal(mean, mean0)
    assert normwise(to_np(mean), mean_ref) < GATE
    check_cov(cov, cov_ref, var_ref)
    # the posterior plugin's entries return the same tensors
    post = lay.posterior()
    for fn in (post._conditional_fused, post.fused_predict_f, post.predict_f):
        m2, c2 = fn(Xd, full_cov=True)
        assert torch.equal(m2, mean) and torch.equal(c2, cov)
    for fn in (post._conditional_fused, post.fused_predict_f, lay.predict_f):
        with pytest.raises(NotImplementedError):
            fn(Xd, full_cov=True, full_output_cov=True)
        with pytest.raises(NotImplementedError):
            fn(Xd, full_output_cov=True)
    # the exact-f32 chain and the split-bf16 images feed the same kernel
    mode, fmt = config.conditional_mode(), config.expert_format()
    try:
        config.set_conditional_mode("f32")
        m3, c3 = lay.predict_f(Xd, full_cov=True)
        assert torch.equal(m3, lay.predict_f(Xd)[0])
        check_cov(c3, cov_ref, var_ref)
        config.set_conditional_mode(mode)
        config.set_expert_format("x6")
        m4, c4 = lay.predict_f(Xd, full_cov=True)
        assert torch.equal(m4, lay.predict_f(Xd)[0])
        check_cov(c4, cov_ref, var_ref)
    finally:
        config.set_conditional_mode(mode)
        config.set_expert_format(fmt)


# --------------------------------------------------------------------------- 3. leading dimensions
def test_full_cov_leading_dimensions(device):
    d, p = golden("case_demo_perturbed")
    lay = build_model(p, device).pred_layer
    mean_ref, cov_ref, var_ref = golden_ref("case_demo_perturbed", "pred")
    X = d["Xtest"]
    N, K, S = X.shape[0], cov_ref.shape[0], 4
    Xe = _dev(X, device)[None].expand(S, *X.shape)
    mean, cov = lay.predict_f(Xe, full_cov=True)
    assert tuple(mean.shape) == (S, N, K) and tuple(cov.shape) == (S, K, N, N)
    assert cov.stride(0) == 0 and mean.stride(0) == 0
    check_cov(cov[S - 1], cov_ref, var_ref)
    # a materialised copy of the tiled rows, declared tiled: computed once, the same bits
    mean_t, cov_t = lay.predict_f(Xe.contiguous(), full_cov=True, tiled=True)
    assert cov_t.stride(0) == 0 and torch.equal(cov_t, cov) and torch.equal(mean_t, mean)
    # a host array of equal copies is recognised as tiled
    assert lay.predict_f(np.tile(X[None], (S, 1, 1)), full_cov=True)[1].stride(0) == 0
    # distinct inputs per leading index: each has its own N x N blocks
    rng = np.random.default_rng(3)
    Xr = X[None] + 0.1 * rng.standard_normal((S,) + X.shape)
    mean_r, cov_r = lay.predict_f(_dev(Xr, device), full_cov=True)
    assert tuple(mean_r.shape) == (S, N, K) and tuple(cov_r.shape) == (S, K, N, N)
    for s in range(S):
        m_ref, c_ref, _ = full_cov_ref(Xr[s], p.pred)
        assert normwise(to_np(mean_r[s]), m_ref) < GATE
        check_cov(cov_r[s], c_ref)
    # two leading dimensions
    m2, c2 = lay.predict_f(_dev(Xr, device).reshape(2, 2, N, -1), full_cov=True)
    assert tuple(c2.shape) == (2, 2, K, N, N) and torch.equal(c2.reshape(S, K, N, N), cov_r)
    assert torch.equal(m2.reshape(S, N, K), mean_r)


# --------------------------------------------------------------------------- 4. samples, deterministic
def _factors_from_identity_noise(lay, Xd, jitter=None):
    """predict_f_samples with noise[s, :, k] = e_s: samples - mean are the columns of
    chol(cov[k] + jitter I).  Returns mean [N, K] and the factors [K, N, N] (host)."""
    N, K = Xd.shape[0], lay.num_latent_gps
    noise = torch.eye(N, device=Xd.device)[:, :, None].expand(N, N, K)
    samples = lay.predict_f_samples(Xd, num_samples=N, noise=noise, jitter=jitter)
    assert tuple(samples.shape) == (N, N, K)
    mean = lay.predict_f(Xd)[0]
    cols = to_np(samples - mean[None])                       # [s, n, k] = L_k[n, s]
    return to_np(mean), np.transpose(cols, (2, 1, 0))


def _check_factors(Ls, cov_ref, jitter):
    N = cov_ref.shape[-1]
    for k, Lk in enumerate(Ls):
        assert np.all(np.triu(Lk, 1) == 0.0)
        err = normwise(Lk @ Lk.T, cov_ref[k] + jitter * np.eye(N))
        print(f"expert {k}: L L^T normwise {err:.3e}")
        assert err < GATE


def test_samples_identity_noise_sparse_points(device):
    """(a) every 4th point of the sorted test inputs (N = 25), default jitter 1e-6: the
    float64 minimum eigenvalue of cov is 4.7e-3."""
    d, p = golden("case_demo_perturbed")
    lay = build_model(p, device).pred_layer
    Xs = np.sort(d["Xtest"], axis=0)[::4]
    assert Xs.shape[0] == 25
    _, cov_ref, _ = full_cov_ref(Xs, p.pred)
    assert np.linalg.eigvalsh(cov_ref).min() > 1e-3
    _, Ls = _factors_from_identity_noise(lay, _dev(Xs, device))
    _check_factors(Ls, cov_ref, 1e-6)


def test_samples_identity_noise_dense_points(device):
    """(b) all 100 test inputs on the assign layer with jitter 1e-4 (the float32
    covariance's most negative eigenvalue at such sizes is about -3.5e-7)."""
    d, p = golden("case_demo_perturbed")
    lay = build_model(p, device).assign_layer
    _, cov_ref, _ = golden_ref("case_demo_perturbed", "assign")
    _, Ls = _factors_from_identity_noise(lay, _dev(d["Xtest"], device), jitter=1e-4)
    _check_factors(Ls, cov_ref, 1e-4)


# --------------------------------------------------------------------------- 5. samples, Philox
def test_samples_philox(device):
    d, p = golden("case_demo_perturbed")
    lay = build_model(p, device).pred_layer
    Xs = np.sort(d["Xtest"], axis=0)[::8]
    N, K = Xs.shape[0], lay.num_latent_gps
    assert N == 13
    Xd = _dev(Xs, device)
    mean_ref, cov_ref, _ = full_cov_ref(Xs, p.pred)
    a = lay.predict_f_samples(Xd, 5, seed=11)
    assert tuple(a.shape) == (5, N, K)
    assert torch.equal(a, lay.predict_f_samples(Xd, 5, seed=11))
    assert not torch.equal(a, lay.predict_f_samples(Xd, 5, seed=12))
    # without a seed every call draws a fresh key of the layer
    assert not torch.equal(lay.predict_f_samples(Xd, 5), lay.predict_f_samples(Xd, 5))
    one = lay.predict_f_samples(Xd, seed=11)
    assert tuple(one.shape) == (N, K) and torch.equal(one, lay.predict_f_samples(Xd, 1, seed=11)[0])
    # leading dimensions: [..., S, N, K]
    Xe = Xd[None].expand(2, N, -1)
    assert tuple(lay.predict_f_samples(Xe, 3, seed=5).shape) == (2, 3, N, K)
    assert tuple(lay.predict_f_samples(Xe, seed=5).shape) == (2, N, K)
    # the marginal draw
    z = torch.as_tensor(np.random.default_rng(0).standard_normal((4, N, K)), dtype=torch.float32, device=device)
    mean, var = lay.predict_f(Xd)
    diag = lay.predict_f_samples(Xd, 4, full_cov=False, noise=z)
    expect = mean[None] + torch.sqrt(var[None] + 1e-6) * z
    assert torch.allclose(diag, expect, rtol=1e-6, atol=1e-7)
    with pytest.raises(NotImplementedError):
        lay.predict_f_samples(Xd, 4, full_output_cov=True)
    with pytest.raises(ValueError):
        lay.predict_f_samples(Xd, 4, noise=z[:3])
    # moments of S = 16384 joint draws: the normwise error of an empirical covariance of S
    # Gaussian draws has expectation sqrt((|C|_F^2 + tr(C)^2) / S) / |C|_F <= sqrt((1 + N) / S)
    # and the mean's 2-norm error sqrt(tr(C) / S); the bounds are four times those
    S = 16384
    smp = to_np(lay.predict_f_samples(Xd, S, seed=2024))
    for k in range(K):
        C = cov_ref[k] + 1e-6 * np.eye(N)
        emp = np.cov(smp[:, :, k], rowvar=False)
        err_c = normwise(emp, C)
        err_m = np.linalg.norm(smp[:, :, k].mean(0) - mean_ref[:, k])
        print(f"expert {k}: empirical cov normwise {err_c:.3e} (bound {4 * np.sqrt((1 + N) / S):.3e}), "
              f"mean error {err_m:.3e} (bound {4 * np.sqrt(np.trace(C) / S):.3e})")
        assert err_c < 4 * np.sqrt((1 + N) / S)
        assert err_m < 4 * np.sqrt(np.trace(C) / S)


# --------------------------------------------------------------------------- 6. failure is loud
def test_samples_rank_deficient_raises(device):
    """The same point 8 times: cov[k] is a constant matrix (rank 1); without jitter its
    factorisation meets a non-positive pivot, reported by K3's info."""
    from modulatedgps_amd._lib import MGPLinAlgError
    d, p = golden("case_demo_perturbed")
    lay = build_model(p, device).pred_layer
    Xd = _dev(np.repeat(d["Xtest"][40:41], 8, axis=0), device)
    with pytest.raises(MGPLinAlgError, match="jitter"):
        lay.predict_f_samples(Xd, 2, seed=1, jitter=0.0)


# --------------------------------------------------------------------------- 7. K > 8
def k9_problem():
    """9 experts on 24 grid points 1.25 lengthscales apart (D = 2, lengthscale 1.5)."""
    _, _, p = R.synthetic_problem(64, 32, 9, 2, 1.5)
    g0, g1 = np.meshgrid(np.arange(6) - 2.5, np.arange(4) - 1.5, indexing="ij")
    Xs = 1.25 * 1.5 * np.stack([g0.ravel(), g1.ravel()], axis=1)
    mean_ref, cov_ref, _ = full_cov_ref(Xs, p.pred)
    return p, Xs, mean_ref, cov_ref


def test_nine_experts_two_chunk_cholesky(device):
    p, Xs, mean_ref, cov_ref = k9_problem()
    assert Xs.shape == (24, 2) and cov_ref.shape == (9, 24, 24)
    dist = np.linalg.norm(Xs[:, None] - Xs[None], axis=-1) + 1e9 * np.eye(24)
    assert dist.min() >= 1.5                                   # at least one lengthscale apart
    assert np.linalg.eigvalsh(cov_ref).min() >= 1e-3
    lay = build_model(p, device).pred_layer
    Xd = _dev(Xs, device)
    mean, cov = lay.predict_f(Xd, full_cov=True)
    assert normwise(to_np(mean), mean_ref) < GATE
    check_cov(cov, cov_ref)
    _, Ls = _factors_from_identity_noise(lay, Xd, jitter=1e-4)
    assert Ls.shape == (9, 24, 24)
    _check_factors(Ls, cov_ref, 1e-4)
