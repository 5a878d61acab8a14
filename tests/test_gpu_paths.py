"""Pathwise posterior function samples (SVGPModified.sample_paths, SMGP.sample_paths,
ops.path_eval / mgp_path_eval, csrc/paths.hip) against the float64 statement in
tests/path_ref.py, with the same basis and draws.

Gate: the project's 1e-4 normwise against float64.  Every measured error is printed
(`SCOREERR <quantity> <value>`); tools/bench_path_samples.py collects the worst of each."""
import functools

import numpy as np
import pytest
import scipy.linalg as sla
import torch

from oracle import cpu_ref as R
from tests import path_ref
from tests.helpers import build_model, load_golden, normwise, params_from_golden, to_np

pytestmark = pytest.mark.gpu

GATE = 1e-4


def _score(name, value):
    print(f"SCOREERR {name} {value:.3e}")
    return value


def _dev(x, device):
    return torch.as_tensor(np.asarray(x), dtype=torch.float32, device=device)


@functools.lru_cache(maxsize=None)
def golden(case):
    d = load_golden(case + ".npz")
    return d, params_from_golden(d)


def _layer(model, name):
    return model.pred_layer if name == "pred" else model.assign_layer


def _draws(L, X, S, Rn, seed):
    """float32-representable basis and draws for layer parameters L."""
    rng = np.random.default_rng(seed)
    M, K = L["q_mu"].shape
    D = np.asarray(X).shape[-1]
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    return (f32(rng.standard_normal((Rn, D))), f32(rng.random(Rn)), f32(rng.standard_normal((S, K, Rn))),
            f32(rng.standard_normal((S, K, M))))


# --------------------------------------------------------------------------- 1. kernel alone
KERNEL_SHAPES = [(1, 20, 1, 1, 1), (129, 25, 37, 3, 1), (257, 0, 64, 129, 2), (100, 130, 256, 12, 8),
                 (65, 64, 33, 5, 32)]


@pytest.mark.parametrize("N,M,Rn,C,D", KERNEL_SHAPES)
def test_path_eval_kernel(device, N, M, Rn, C, D):
    """(N, M, R, C, D): one point, one feature, one column; R, M no multiples of the 16-row
    chunk and N one past a tile; prior only (A = NULL) with ARD and two column tiles; two
    row tiles of A; the top of the D range.  The reference takes the unrounded float64
    operands (A = L^-1 Kuf in float64; the device gets it rounded, as test_full_cov_kernel)."""
    from modulatedgps_amd import ops
    rng = np.random.default_rng(1000 * N + M + Rn)
    X = rng.standard_normal((N, D))
    ls = 0.8 + 0.6 * rng.random(D) if D == 2 else np.float64(0.9 * np.sqrt(D))
    var = 0.7
    Omega = rng.standard_normal((Rn, D)) / ls / (2 * np.pi)       # in turns
    phase = rng.random(Rn)
    W = rng.standard_normal((Rn + M, C))
    W[:Rn] *= np.sqrt(2 * var / Rn)
    A64 = None
    if M:
        Z = rng.standard_normal((M, D))
        Lm = np.linalg.cholesky(R.rbf_Kuu(Z, var, ls))
        A64 = sla.solve_triangular(Lm, R.rbf_K(Z, X, var, ls), lower=True)
    ref = path_ref.path_eval(X, Omega, phase, W, A64)

    Xd, Od, pd, Wd = _dev(X, device), _dev(Omega, device), _dev(phase, device), ops.as_padded(_dev(W, device))
    Ad = ops.as_padded(_dev(A64, device)) if M else None
    ld = (N + 3) // 4 * 4 + 4
    sentinel = -12345.0
    buf = torch.full((C + 1, ld), sentinel, dtype=torch.float32, device=device)
    out = ops.path_eval(Xd, Od, pd, Wd, A=Ad, out=buf[:C, :N])
    assert out.data_ptr() == buf.data_ptr() and tuple(out.shape) == (C, N)
    err = _score("path_eval_kernel", normwise(to_np(out), ref))
    assert err < GATE
    assert bool((buf[:C, N:] == sentinel).all()) and bool((buf[C] == sentinel).all())   # padding untouched
    # a second call, into storage of the wrapper's own: the same bits
    out2 = ops.path_eval(Xd, Od, pd, Wd, A=Ad)
    assert torch.equal(out2, out)
    # a shard returns the bits of the unsharded call: cuts off and on tile edges
    cuts = [(N // 3, N - N // 4)] + ([(128, N), (0, 128)] if N > 128 else [])
    for a, b in cuts:
        if b <= a:
            continue
        part = ops.path_eval(Xd[a:b], Od, pd, Wd, A=Ad[:, a:b] if M else None)
        assert torch.equal(part, out[:, a:b]), (a, b)


# --------------------------------------------------------------------------- 2. through the layer
@pytest.mark.parametrize("layer", ["pred", "assign"])
@pytest.mark.parametrize("case", ["case_demo_perturbed", "case_c1"])
def test_layer_paths(device, case, layer):
    d, p = golden(case)
    L = getattr(p, layer)
    lay = _layer(build_model(p, device), layer)
    X = d["Xtest"]
    S, Rn = 4, 256
    zeta, phase, w, eps = _draws(L, X, S, Rn, seed=11)
    paths = lay.sample_paths(S, Rn, basis=(zeta, phase), noise=(w, eps))
    for got, want in ((paths.zeta, zeta), (paths.phase, phase), (paths.w, w), (paths.eps, eps)):
        assert np.array_equal(to_np(got), want)
    K = L["q_mu"].shape[1]
    f = paths(_dev(X, device))
    assert tuple(f.shape) == (S, X.shape[0], K)
    f_ref, mean_ref, _ = path_ref.layer_paths(X, L, zeta, phase, w, eps)
    assert _score("layer_paths", normwise(to_np(f), f_ref)) < GATE
    # zero draws: the path is predict_f's mean, for any basis
    zero = lay.sample_paths(S, Rn, basis=(zeta, phase), noise=(np.zeros_like(w), np.zeros_like(eps)))
    f0 = to_np(zero(_dev(X, device)))
    mean_dev = to_np(lay.predict_f(_dev(X, device))[0])
    for s in range(S):
        assert _score("layer_paths_zero_draw", normwise(f0[s], mean_dev)) < GATE
        assert _score("layer_paths_zero_draw_ref", normwise(f0[s], mean_ref)) < GATE


def test_layer_paths_other_chains(device):
    """K1 and K4 on the exact-f32 chain and on the split-bf16 images feed the same kernel."""
    from modulatedgps_amd import config
    d, p = golden("case_c1")
    lay = build_model(p, device).pred_layer
    X = d["Xtest"]
    zeta, phase, w, eps = _draws(p.pred, X, 2, 64, seed=12)
    f_ref, _, _ = path_ref.layer_paths(X, p.pred, zeta, phase, w, eps)
    paths = lay.sample_paths(2, 64, basis=(zeta, phase), noise=(w, eps))
    mode, fmt = config.conditional_mode(), config.expert_format()
    try:
        config.set_conditional_mode("f32")
        assert _score("layer_paths_f32_chain", normwise(to_np(paths(_dev(X, device))), f_ref)) < GATE
        config.set_conditional_mode(mode)
        config.set_expert_format("x6")
        assert _score("layer_paths_x6_chain", normwise(to_np(paths(_dev(X, device))), f_ref)) < GATE
    finally:
        config.set_conditional_mode(mode)
        config.set_expert_format(fmt)


# --------------------------------------------------------------------------- 3. function semantics
def test_paths_are_functions(device):
    d, p = golden("case_demo_perturbed")
    lay = build_model(p, device).pred_layer
    X = _dev(d["Xtest"], device)
    paths = lay.sample_paths(3, 64, seed=5)
    full = paths(X)
    for cut in (37, 64):
        assert torch.equal(paths(X[:cut]), full[:, :cut]) and torch.equal(paths(X[cut:]), full[:, cut:])
    assert torch.equal(paths(torch.cat([X[:cut], X[cut:]])), full)
    # the same seed is the same function, another seed another
    again = lay.sample_paths(3, 64, seed=5)
    assert torch.equal(again(X), full)
    other = lay.sample_paths(3, 64, seed=6)
    assert not torch.equal(other(X), full)
    # keyed by the layer: two draws without a seed differ
    assert not torch.equal(lay.sample_paths(3, 64)(X), lay.sample_paths(3, 64)(X))
    # a snapshot: new variational values do not reach the old object, a new object has them
    q_mu, q_sqrt = lay.q_mu.clone(), lay.q_sqrt.clone()
    lay.set_variational(q_mu + 0.25, 0.5 * q_sqrt)
    assert torch.equal(paths(X), full)
    assert not torch.equal(lay.sample_paths(3, 64, seed=5)(X), full)
    with pytest.raises(ValueError):
        paths(torch.zeros(5, X.shape[1] + 1, device=device))
    with pytest.raises(ValueError):
        lay.sample_paths(0, 64)
    with pytest.raises(ValueError):
        lay.sample_paths(3, 0)


# --------------------------------------------------------------------------- 4. moments
def test_path_moments(device):
    """Philox draws on one basis, S = 4096: per point and expert the sample mean and variance
    against the analytic mean m and variance v given that basis.  Both bounds are six standard
    deviations of the sampling distributions: sd(mean_S) = sqrt(v / S), sd(var_S / v) =
    sqrt(2 / (S - 1))."""
    d, p = golden("case_demo_perturbed")
    lay = build_model(p, device).pred_layer
    X = d["Xtest"]
    S, Rn = 4096, 256
    paths = lay.sample_paths(S, Rn, seed=2024)
    f = to_np(paths(_dev(X, device)))                              # [S, N, K]
    M, K = p.pred["q_mu"].shape
    _, m, v = path_ref.layer_paths(X, p.pred, to_np(paths.zeta), to_np(paths.phase), np.zeros((1, K, Rn)),
                                   np.zeros((1, K, M)))
    zmean = np.abs(f.mean(0) - m) / np.sqrt(v / S)
    ratio = f.var(0, ddof=1) / v
    _score("path_moments_mean_sigmas", zmean.max())
    _score("path_moments_var_ratio_min", ratio.min())
    _score("path_moments_var_ratio_max", ratio.max())
    assert zmean.max() <= 6.0
    assert np.abs(ratio - 1.0).max() <= 6.0 * np.sqrt(2.0 / (S - 1))


# --------------------------------------------------------------------------- 5. mixture
def _mixture_ref(mp, p, X):
    out = []
    for lp, L in ((mp.pred, p.pred), (mp.assign, p.assign)):
        f, _, _ = path_ref.layer_paths(X, L, to_np(lp.zeta), to_np(lp.phase), to_np(lp.w), to_np(lp.eps))
        out.append(f)
    f, a = out
    e = np.exp(a - a.max(-1, keepdims=True))
    wts = e / e.sum(-1, keepdims=True)
    return f, a, wts, (wts * f).sum(-1)


def test_mixture_paths(device):
    d, p = golden("case_demo_perturbed")
    model = build_model(p, device)
    X = d["Xtest"]
    Xd = _dev(X, device)
    S, Rn = 4, 256
    mp = model.sample_paths(S, Rn, seed=7)
    f_ref, a_ref, w_ref, m_ref = _mixture_ref(mp, p, X)
    K = f_ref.shape[-1]
    got = dict(f=mp.predict_f(Xd), logits=mp.predict_logits(Xd), weights=mp.predict_weights(Xd),
               mean=mp.predict_mean(Xd))
    assert tuple(got["f"].shape) == tuple(got["logits"].shape) == tuple(got["weights"].shape) == (S, X.shape[0], K)
    assert tuple(got["mean"].shape) == (S, X.shape[0])
    for name, ref in (("f", f_ref), ("logits", a_ref), ("weights", w_ref), ("mean", m_ref)):
        assert _score("mixture_paths_" + name, normwise(to_np(got[name]), ref)) < GATE
    assert torch.equal(model.sample_paths(S, Rn, seed=7).predict_mean(Xd), got["mean"])
    assert not torch.equal(model.sample_paths(S, Rn).predict_mean(Xd), model.sample_paths(S, Rn).predict_mean(Xd))
    # SMGPModified inherits the method: the same layers and seed, the same curves
    from modulatedgps_amd.likelihoods import GaussianModified
    from modulatedgps_amd.models import SMGPModified
    mod = SMGPModified(model.likelihood.likelihood, GaussianModified(variance=np.linspace(0.3, 0.9, K)[None], device=device),
                       model.pred_layer, model.assign_layer, K=K, num_samples=p.S, num_data=p.num_data)
    assert torch.equal(mod.sample_paths(S, Rn, seed=7).predict_mean(Xd), got["mean"])


def test_mixture_paths_multiclass_raises(device):
    from modulatedgps_amd.kernels import SquaredExponential
    from modulatedgps_amd.likelihoods import MultiClass, RobustMax
    from modulatedgps_amd.models import SMGP, SVGPModified
    X, _, p = R.synthetic_problem(64, 8, 3, 1, 1.0, state="perturbed", S=3)
    lik = MultiClass(num_classes=3, invlink=RobustMax(3, epsilon=1e-3, device=device), device=device)
    layers = []
    for L in (p.pred, p.assign):
        kern = SquaredExponential(variance=L["variance"], lengthscales=L["lengthscales"], device=device)
        layer = SVGPModified(kern, lik, L["Z"], num_latent_gps=3, whiten=True, device=device)
        layer.set_variational(L["q_mu"], L["q_sqrt"])
        layers.append(layer)
    model = SMGP(lik, layers[0], layers[1], K=3, num_samples=3, num_data=64)
    mp = model.sample_paths(2, 32, seed=1)
    Xd = _dev(X, device)
    assert tuple(mp.predict_f(Xd).shape) == tuple(mp.predict_weights(Xd).shape) == (2, 64, 3)
    with pytest.raises(NotImplementedError):
        mp.predict_mean(Xd)
