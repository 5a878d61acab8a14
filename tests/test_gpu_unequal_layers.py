"""Models whose two SVGP layers differ: another number of inducing points and / or
another kind of lengthscale (scalar against ARD) per layer.

cluster.kmeans drops empty clusters and inducing.greedy_variance stops early, so
Z and Z_assign of different M come out of the project's own initialisers.  With
Mf != Ma SMGP sizes its buffers by max(Mf, Ma) and slices them per layer, factorises
each Kuu on its own (no batched K3, no prep event inside it, no bounded L^-T images,
no K1 inside K3), and runs the tril(q_sqrt) images, K4, K5 and the backward tail per
layer; with equal M but mixed lengthscale counts (case g) the forward stays batched
with a mixed n_ls array and only the backward tail goes per layer.

Cases (tests/helpers.py UNEQUAL_CASES; cond(Kuu + 1e-6 I) pred / assign in float64):
a both M <= 64, pred ARD (6e3 / 4e2); b two row tiles against one, assign ARD
(1e5 / 5e3); c = b with the larger layer second; d K = 5 (7e1 / 4e3); e 129 against
128, the stats tile counts differ by one; f an M = 1 layer; g equal M, mixed n_ls.

Tolerances are the existing ones: ELBO 1e-4 relative, conditionals normwise
max(1e-4, 10 sqrt(cond) 1.2e-7) (test_gpu_properties), gradients max(3e-4, 1.5 x float32
autograd's error) (test_gpu_training; 4 x for the degenerate case f, as the drawn-shapes
gradient test holds degenerate shapes, for the reason its docstring gives)."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref as R
from tests.helpers import UNEQUAL_CASES, build_model, dev_noise, normwise, to_np, unequal_problem

pytestmark = pytest.mark.gpu

FORMATS = ["f16", "x6", "f16x8"]


class _Format:
    """Set the image format as test_elbo_and_grad does; restore it on exit."""

    def __init__(self, fmt):
        self.fmt = fmt

    def __enter__(self):
        from modulatedgps_amd import config
        self.old = (config.expert_format(), config.expert_cross())
        config.set_expert_format("x6" if self.fmt == "x6" else "f16")
        config.set_expert_cross("f8" if self.fmt == "f16x8" else "f16")

    def __exit__(self, *exc):
        from modulatedgps_amd import config
        config.set_expert_format(self.old[0])
        config.set_expert_cross(self.old[1])


_REF = {}


def _reference(case):
    """(X, Y, p, z, u, elbo, parts) of a case, computed once and left unchanged."""
    if case not in _REF:
        N, Mf, Ma, K, D, ls_f, ls_a, S = UNEQUAL_CASES[case]
        X, Y, p = unequal_problem(N, Mf, Ma, K, D, ls_f, ls_a, S)
        z, u = R.explicit_noise(S, N, K, seed=7)
        ref, parts = R.smgp_elbo(X, Y, p, z, u, return_parts=True)
        _REF[case] = (X, Y, p, z, u, ref, parts)
    return _REF[case]


def check_elbo_and_conditionals(device, X, Y, p, z, u, ref, parts, tag):
    """ELBO at 1e-4 relative; the four conditionals normwise at the conditioning-scaled
    tolerance of test_elbo_and_conditionals_random_shapes; every output has its layer's shape."""
    model = build_model(p, device)
    Xd = torch.as_tensor(X, dtype=torch.float32, device=device)
    e = float(model._build_likelihood(Xd, Y, noise=dev_noise(z, u, device)).cpu())
    assert e == pytest.approx(ref, rel=1e-4), (tag, e, ref)
    N, K = X.shape[0], p.lik_variance.shape[1]
    mu_f, var_f, mu_a, var_a = model.conditionals(Xd)
    for got, name, L in ((mu_f, "mu_f", p.pred), (var_f, "var_f", p.pred), (mu_a, "mu_a", p.assign),
                         (var_a, "var_a", p.assign)):
        assert tuple(got.shape) == (K, N), (tag, name, got.shape)
        cond = np.linalg.cond(R.rbf_Kuu(L["Z"], L["variance"], L["lengthscales"]))
        tol = max(1e-4, 10 * np.sqrt(cond) * 1.2e-7)
        want = parts[name]
        if np.abs(want).max() == 0:
            assert np.abs(to_np(got)).max() < 1e-6, (tag, name)
        else:
            err = normwise(to_np(got).T, want)
            print(f"{tag} {name}: cond {cond:.1e} normwise {err:.2e} (tol {tol:.1e})", flush=True)
            assert err < tol, (tag, name, cond, err)
    return model


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("case", sorted(UNEQUAL_CASES))
def test_elbo_and_conditionals(device, case, fmt):
    with _Format(fmt):
        check_elbo_and_conditionals(device, *_reference(case), tag=(case, fmt))


def test_modified_elbo(device):
    """Case a as SMGPModified (the assignment likelihood has its own variances)."""
    from tests.test_gpu_training import _model
    X, Y, p, z, u, _, _ = _reference("a")
    a_var = np.linspace(0.3, 0.9, p.lik_variance.shape[1])[None, :]
    ref = R.smgp_modified_elbo(X, Y, p, a_var, z, u)
    model = _model(p, device, a_var)
    Xd = torch.as_tensor(X, dtype=torch.float32, device=device)
    e = float(model._build_likelihood(Xd, Y, noise=dev_noise(z, u, device)).cpu())
    assert e == pytest.approx(ref, rel=1e-4), (e, ref)


@pytest.mark.parametrize("case", ["b", "e"])
def test_predictions(device, case):
    """predict_y / predict_assign on 97 held-out points, the close criterion of
    test_elbo_and_conditionals_random_shapes."""
    X, Y, p, *_ = _reference(case)
    D = X.shape[1]
    model = build_model(p, device)
    cond = max(np.linalg.cond(R.rbf_Kuu(L["Z"], L["variance"], L["lengthscales"])) for L in (p.pred, p.assign))
    tol = max(1e-4, 10 * np.sqrt(cond) * 1.2e-7)
    Xt = np.random.default_rng(11).standard_normal((97, D))
    Xt64 = Xt.astype(np.float32).astype(np.float64)
    Xtd = torch.as_tensor(Xt, dtype=torch.float32, device=device)
    close = lambda got, ref: np.linalg.norm(np.asarray(got, np.float64) - ref) <= tol * max(
        np.linalg.norm(ref), 1e-3 * np.sqrt(ref.size))
    ym, yv = model.predict_y(Xtd)
    rm, rv = R.predict_y(Xt64, p)
    assert close(ym, rm), (case, "predict_y mean")
    assert close(yv, rv), (case, "predict_y var")
    assert close(model.predict_assign(Xtd), R.predict_assign(Xt64, p)), (case, "predict_assign")


def _grad(device, case, modified=False, floors=None, factor=1.5):
    from tests.test_gpu_training import _check_elbo_and_grad
    N, Mf, Ma, K, D, ls_f, ls_a, S = UNEQUAL_CASES[case]
    _, grads = _check_elbo_and_grad(device, N, max(Mf, Ma), K, D, None, S, modified, floors=floors, factor=factor,
                                    problem=unequal_problem(N, Mf, Ma, K, D, ls_f, ls_a, S))
    for name, M, ls in (("pred", Mf, ls_f), ("assign", Ma, ls_a)):   # each layer's blocks, that layer's shapes
        assert tuple(grads[name + ".Z"].shape) == (M, D)
        assert tuple(grads[name + ".q_mu"].shape) == (M, K)
        assert tuple(grads[name + ".q_sqrt"].shape) == (K, M, M)
        assert grads[name + ".lengthscales"].numel() == np.size(ls)
        assert grads[name + ".variance"].numel() == 1


@pytest.mark.parametrize("fmt", ["f16", "x6"])
@pytest.mark.parametrize("case", ["a", "b", "c", "d", "e", "g"])
def test_elbo_and_grad(device, case, fmt):
    with _Format(fmt):
        _grad(device, case)


def test_elbo_and_grad_modified(device):
    _grad(device, "a", modified=True)


def test_elbo_and_grad_f16x8(device):
    """Case b with the e4m3 cross terms, at that format's floors of test_gpu_training."""
    with _Format("f16x8"):
        _grad(device, "b", floors={"assign.variance": 4e-4})


@pytest.mark.parametrize("fmt", ["f16", "x6"])
def test_elbo_and_grad_degenerate_layer(device, fmt):
    """Case f, an M = 1 pred layer: 4 x float32 autograd's error, what
    test_elbo_and_grad_random_shapes holds degenerate shapes to."""
    with _Format(fmt):
        _grad(device, "f", factor=4.0)


def _read_back(model, p):
    """The device model's parameters as an oracle SMGPParams."""
    layers = []
    for layer in (model.pred_layer, model.assign_layer):
        ls = to_np(layer.kernel.lengthscales).reshape(-1)
        layers.append(dict(Z=to_np(layer.Z), variance=float(to_np(layer.kernel.variance).reshape(-1)[0]),
                           lengthscales=float(ls[0]) if ls.size == 1 else ls, q_mu=to_np(layer.q_mu),
                           q_sqrt=np.tril(to_np(layer.q_sqrt))))
    lik = to_np(model.likelihood.likelihood.variance).reshape(1, -1)
    return R.SMGPParams(layers[0], layers[1], lik, p.num_data, p.S)


@pytest.mark.parametrize("optimiser", ["adam", "natgrad_adam"])
def test_state_after_training(device, optimiser):
    """Five optimiser iterations on case a, then the ELBO at the parameters read back from
    the device against the oracle at those parameters: an image, factor or bound that stays
    stale after an update on the per-layer path shows here."""
    from utils.data import Dataset
    from utils.training_utils import run_adam, run_natgrad_adam
    X, Y, p, z, u, ref0, _ = _reference("a")
    N = X.shape[0]
    model = build_model(p, device)
    Xd = torch.as_tensor(X, dtype=torch.float32, device=device)
    Yd = torch.as_tensor(Y, dtype=torch.float32, device=device)
    noise = dev_noise(z, u, device)
    e0 = float(model._build_likelihood(Xd, Y, noise=noise).cpu())
    assert e0 == pytest.approx(ref0, rel=1e-4)
    it = iter(Dataset.from_tensor_slices((Xd, Yd)).batch(N).repeat())
    iters, elbos = (run_adam if optimiser == "adam" else run_natgrad_adam)(model, 5, it, 0.01)
    assert iters == [5] and np.all(np.isfinite(elbos))
    assert int(model.last_info.abs().max().cpu()) == 0
    e1 = float(model._build_likelihood(Xd, Y, noise=noise).cpu())
    assert int(model.last_info.abs().max().cpu()) == 0
    p1 = _read_back(model, p)
    assert p1.pred["Z"].shape == p.pred["Z"].shape and p1.assign["q_sqrt"].shape == p.assign["q_sqrt"].shape
    assert np.abs(p1.pred["q_mu"] - p.pred["q_mu"]).max() > 0   # the steps moved the parameters
    ref1 = R.smgp_elbo(X, Y, p1, z, u)
    print(f"{optimiser}: elbo {e0:.6f} -> {e1:.6f}; oracle at the read-back parameters {ref1:.6f}", flush=True)
    assert e1 == pytest.approx(ref1, rel=1e-4), (e1, ref1)
    assert np.isfinite(e1) and e1 > e0, (e0, e1)
