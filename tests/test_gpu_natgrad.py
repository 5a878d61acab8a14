"""GPU tests of the natural-gradient step on (q_mu, q_sqrt): ops.natgrad_step
(mgp_natgrad_step, csrc/natgrad.hip) against the float64 direct-route reference of
tests/natgrad_ref.py, its defined edge cases (step = 0, a step that does not exist), the
conjugate one-step property from host-made and from elbo_and_grad's gradients, and
training.NaturalGradient / run_natgrad_adam end to end.

Gates: the project's 1e-4 normwise gate for the op and rel 1e-4 for an ELBO.  The two
conjugate comparisons against the closed-form optimum are bounded by 2 x the error of the
yardstick, the specified step (float64 arithmetic, outputs rounded to float32 once) computed
on the CPU from float32-rounded gradients -- the float32 gradients pass through B^-1, so no
fixed bound fits.  Measured on the MI355X (GPU / yardstick, normwise against the optimum):
host-made gradients, M = 70: S 4.5e-7 / 4.3e-7, mu 6.8e-7 / 6.9e-7; end to end, K = 1,
M = 64, N = 2049 (yardstick from float32 autograd of oracle/grad_ref.py): S 6.5e-5 / 6.4e-3,
mu 1.6e-4 / 6.3e-3 (the float32 gradients are multiplied by step = 2049 on their way through B^-1)."""
import functools

import numpy as np
import pytest
import torch

from oracle import cpu_ref as R
from oracle import grad_ref as GR
from tests import natgrad_ref as NR
from tests.helpers import build_model, dev_noise, to_np

pytestmark = pytest.mark.gpu

GATE = 1e-4


def _dev(a, device, dtype=torch.float32):
    from modulatedgps_amd import ops
    a = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a), dtype=dtype)
    return ops.as_padded(a, device=device, dtype=dtype)


@functools.lru_cache(maxsize=None)
def _case(M, K, step, kind):
    q_mu, q_sqrt, g_mu, g_sqrt = NR.draw_case(M, K, step, kind)
    mu_ref, L_ref, ok = NR.step_direct(q_mu, q_sqrt, g_mu, g_sqrt, step)
    assert ok.all()
    return q_mu, q_sqrt, g_mu, g_sqrt, mu_ref, L_ref


def _gram(L):
    return np.einsum("kij,klj->kil", L, L)


@pytest.mark.parametrize("step", NR.STEPS)
@pytest.mark.parametrize("K", NR.SHAPES_K)
@pytest.mark.parametrize("M", NR.SHAPES_M)
def test_natgrad_step_matches_reference(device, M, K, step):
    """plain: loss gradients, grad_sign +1; negdiag: ELBO gradients (negated), grad_sign -1;
    illcond: float64 gradients.  q_mu', q_sqrt', L' L'^T, the sign rule, the zero upper
    triangle and info."""
    from modulatedgps_amd import ops
    for kind in NR.KINDS:
        q_mu, q_sqrt, g_mu, g_sqrt, mu_ref, L_ref = _case(M, K, step, kind)
        sign = -1.0 if kind == "negdiag" else 1.0
        gdt = torch.float64 if kind == "illcond" else torch.float32
        mu_d, L_d = _dev(q_mu, device), _dev(q_sqrt, device)
        info = ops.natgrad_step(mu_d, L_d, _dev(sign * g_mu, device, gdt), _dev(sign * g_sqrt, device, gdt), step,
                                grad_sign=sign)
        assert info.dtype == torch.int32 and info.cpu().tolist() == [0] * K, kind
        mu, L = to_np(mu_d), to_np(L_d)
        errs = (NR.normwise(mu, mu_ref), NR.normwise(L, L_ref), NR.normwise(_gram(L), _gram(L_ref)))
        print(kind, ["%.1e" % e for e in errs])
        assert np.all(np.triu(L, 1) == 0.0), kind
        assert np.all(np.sign(np.diagonal(L, axis1=1, axis2=2)) == np.sign(np.diagonal(q_sqrt, axis1=1, axis2=2)))
        assert max(errs) < GATE, (kind, errs)


def test_step_zero_is_the_identity(device):
    from modulatedgps_amd import ops
    q_mu, q_sqrt, g_mu, g_sqrt, _, _ = _case(70, 3, 1.0, "negdiag")
    mu_d, L_d = _dev(q_mu, device), _dev(q_sqrt, device)
    mu0, L0 = mu_d.clone(), L_d.clone()
    info = torch.full((3,), 7, dtype=torch.int32, device=device)
    out = ops.natgrad_step(mu_d, L_d, _dev(g_mu, device), _dev(g_sqrt, device), 0.0, info=info)
    assert out is info and info.cpu().tolist() == [0, 0, 0]
    assert torch.equal(mu_d.view(torch.int32), mu0.view(torch.int32))
    assert torch.equal(L_d.view(torch.int32), L0.view(torch.int32))


def test_two_calls_give_the_same_bits(device):
    from modulatedgps_amd import ops
    q_mu, q_sqrt, g_mu, g_sqrt, _, _ = _case(130, 9, 1.0, "plain")
    outs = []
    for _ in range(2):
        mu_d, L_d = _dev(q_mu, device), _dev(q_sqrt, device)
        ops.natgrad_step(mu_d, L_d, _dev(g_mu, device), _dev(g_sqrt, device), 1.0, grad_sign=1.0)
        outs.append((mu_d, L_d))
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))
    assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))


def test_failed_step_leaves_its_expert_unchanged(device):
    """Expert 1: L = I, g_L = -(2 / step) I, so B = -I: an error code, the expert bitwise
    unchanged, the others as the reference, nothing NaN."""
    from modulatedgps_amd import ops
    M, K, step = 25, 3, 1.0
    q_mu, q_sqrt, g_mu, g_sqrt, _, _ = _case(M, K, step, "plain")
    q_sqrt, g_sqrt = q_sqrt.copy(), g_sqrt.copy()
    q_sqrt[1] = np.eye(M)
    g_sqrt[1] = -(2.0 / step) * np.eye(M)
    mu_ref, L_ref, ok = NR.step_direct(q_mu, q_sqrt, g_mu, g_sqrt, step)
    assert list(ok) == [True, False, True]
    mu_d, L_d = _dev(q_mu, device), _dev(q_sqrt, device)
    mu0, L0 = mu_d.clone(), L_d.clone()
    info = ops.natgrad_step(mu_d, L_d, _dev(g_mu, device), _dev(g_sqrt, device), step, grad_sign=1.0).cpu().tolist()
    assert info[0] == 0 and info[2] == 0 and info[1] != 0
    assert torch.equal(mu_d[:, 1].view(torch.int32), mu0[:, 1].view(torch.int32))
    assert torch.equal(L_d[1].view(torch.int32), L0[1].view(torch.int32))
    mu, L = to_np(mu_d), to_np(L_d)
    assert np.all(np.isfinite(mu)) and np.all(np.isfinite(L))
    for k in (0, 2):
        assert NR.normwise(mu[:, k], mu_ref[:, k]) < GATE and NR.normwise(L[k], L_ref[k]) < GATE


def test_conjugate_step_from_host_made_gradients(device):
    """M = 70, N = 200: one step at step = 1 from a perturbed start reaches S*, mu*; at most
    2 x the yardstick's error (module docstring; measured S 4.5e-7 / 4.3e-7, mu 6.8e-7 / 6.9e-7)."""
    from modulatedgps_amd import ops
    c = NR.conjugate_case()
    mu_y, L_y, ok = NR.step_direct(c["mu"][:, None], c["L"][None], c["g_mu"][:, None], c["g_L"][None], 1.0)
    assert ok.all()
    mu_y, L_y = NR.f32(mu_y[:, 0]), NR.f32(L_y[0])
    y_S, y_mu = NR.normwise(L_y @ L_y.T, c["S_star"]), NR.normwise(mu_y, c["mu_star"])
    mu_d, L_d = _dev(c["mu"][:, None], device), _dev(c["L"][None], device)
    info = ops.natgrad_step(mu_d, L_d, _dev(c["g_mu"][:, None], device), _dev(c["g_L"][None], device), 1.0,
                            grad_sign=1.0)
    assert info.cpu().tolist() == [0]
    mu, L = to_np(mu_d)[:, 0], to_np(L_d)[0]
    e_S, e_mu = NR.normwise(L @ L.T, c["S_star"]), NR.normwise(mu, c["mu_star"])
    print(f"conjugate host-made: S {e_S:.2e} / {y_S:.2e}, mu {e_mu:.2e} / {y_mu:.2e}")
    assert e_S <= 2.0 * y_S and e_mu <= 2.0 * y_mu


def _oracle(X, Y, p, z, u, dtype=torch.float64):
    """ELBO and its gradients w.r.t. (q_mu, q_sqrt) of both layers by autograd of
    oracle/grad_ref.py (float64, or float32 as the yardstick)."""
    pred, assign, lik = GR.params_from_oracle(p)
    leaf = lambda t: t.detach().to(dtype).requires_grad_(True)
    pred = {k: leaf(v) for k, v in pred.items()}
    assign = {k: leaf(v) for k, v in assign.items()}
    f = lambda a: torch.tensor(np.asarray(a, np.float32)).to(dtype)
    e = GR.elbo(f(X), f(Y), pred, assign, leaf(lik), f(z), f(u), p.num_data)
    e.backward()
    g = {}
    for name, L in (("pred", pred), ("assign", assign)):
        g[name + ".q_mu"] = L["q_mu"].grad.double().numpy()
        g[name + ".q_sqrt"] = np.tril(L["q_sqrt"].grad.double().numpy())
    return float(e.detach()), g


def _stepped(p, g, step):
    """The oracle parameters after the reference step from the ELBO gradients g."""
    layers = {}
    for name, L in (("pred", p.pred), ("assign", p.assign)):
        mu, Ls, ok = NR.step_direct(NR.f32(L["q_mu"]), NR.f32(L["q_sqrt"]), -g[name + ".q_mu"], -g[name + ".q_sqrt"],
                                    step)
        assert ok.all()
        layers[name] = dict(L, q_mu=mu, q_sqrt=Ls)
    return R.SMGPParams(layers["pred"], layers["assign"], p.lik_variance, p.num_data, p.S)


def test_conjugate_model_end_to_end(device):
    """K = 1: the mixture weight is 1 and the model is conjugate, so one
    NaturalGradient(gamma = 1) step on elbo_and_grad's gradients reaches the collapsed SGPR
    (Titsias) bound, returns the assignment layer to its prior and puts the prediction layer
    at the closed-form optimum (2 x the float32-autograd yardstick; measured S 6.5e-5 / 6.4e-3,
    mu 1.6e-4 / 6.3e-3; ELBO -0.62386465 against the bound -0.62386470)."""
    from modulatedgps_amd.training import NaturalGradient
    N, M, S = 2049, 64, 3
    X, Y, p = R.synthetic_problem(N, M, 1, 2, 0.8, state="perturbed", S=S)
    z, u = R.explicit_noise(S, N, 1, seed=5)
    # the closed forms, float64 on the float32-rounded inputs, Kuu with the default jitter
    X32, y = NR.f32(X), NR.f32(Y).reshape(-1)
    Z32 = NR.f32(p.pred["Z"])
    var, ls = float(NR.f32(p.pred["variance"])), NR.f32(p.pred["lengthscales"])
    s2 = float(NR.f32(p.lik_variance).reshape(-1)[0])
    Lm = np.linalg.cholesky(R.rbf_Kuu(Z32, var, ls))
    A = np.linalg.solve(Lm, R.rbf_K(Z32, X32, var, ls))
    Bm = np.eye(M) + A @ A.T / s2
    S_star = np.linalg.inv(Bm)
    mu_star = S_star @ A @ y / s2
    LB = np.linalg.cholesky(Bm)
    c = np.linalg.solve(LB, A @ y) / s2
    bound = (-0.5 * N * np.log(2 * np.pi * s2) - np.log(np.diag(LB)).sum() - 0.5 * y @ y / s2 + 0.5 * c @ c
             - 0.5 * (N * var - np.sum(A * A)) / s2) / N
    # the yardstick: the reference step from float32 autograd's gradients
    _, g32 = _oracle(X, Y, p, z, u, dtype=torch.float32)
    py = _stepped(p, g32, float(N))
    Ly, muy = NR.f32(py.pred["q_sqrt"][0]), NR.f32(py.pred["q_mu"][:, 0])
    y_S, y_mu = NR.normwise(Ly @ Ly.T, S_star), NR.normwise(muy, mu_star)

    model = build_model(p, device)
    Xd = torch.as_tensor(X, dtype=torch.float32, device=device)
    noise = dev_noise(z, u, device)
    _, grads = model.elbo_and_grad(Xd, Y, noise=noise)
    ng = NaturalGradient(gamma=1.0)
    ng.step(model, grads)
    assert ng.skipped() == 0
    elbo = float(model._build_likelihood(Xd, Y, noise=noise).cpu())
    print(f"K=1 conjugate: elbo {elbo:.8f} bound {bound:.8f}")
    assert elbo == pytest.approx(bound, rel=1e-4)
    qa, La = to_np(model.assign_layer.q_mu), to_np(model.assign_layer.q_sqrt)[0]
    assert np.abs(qa).max() < 1e-5
    assert NR.normwise(La @ La.T, np.eye(M)) < 1e-5
    Lf, muf = to_np(model.pred_layer.q_sqrt)[0], to_np(model.pred_layer.q_mu)[:, 0]
    e_S, e_mu = NR.normwise(Lf @ Lf.T, S_star), NR.normwise(muf, mu_star)
    print(f"K=1 conjugate: S {e_S:.2e} / {y_S:.2e}, mu {e_mu:.2e} / {y_mu:.2e}")
    assert e_S <= 2.0 * y_S and e_mu <= 2.0 * y_mu


def test_model_step_end_to_end(device):
    """K = 3, the loop test's problem: NaturalGradient.step is bitwise ops.natgrad_step on the
    same gradients, and after one step at gamma = 0.1 the ELBO under the same noise equals the
    oracle's at the reference-stepped parameters (oracle: -1.5450 -> -0.8768; measured -1.5450 -> -0.8768) and has risen."""
    from modulatedgps_amd import ops
    from modulatedgps_amd.training import NaturalGradient
    N, K, S, gamma = 1000, 3, 5, 0.1
    X, Y, p = R.synthetic_problem(N, 25, K, 1, 0.5, state="init", S=S)
    z, u = R.explicit_noise(S, N, K, seed=5)
    e_before, g64 = _oracle(X, Y, p, z, u)
    e_after = R.smgp_elbo(X, Y, _stepped(p, g64, gamma * N), z, u)
    assert e_after > e_before
    model = build_model(p, device)
    Xd = torch.as_tensor(X, dtype=torch.float32, device=device)
    noise = dev_noise(z, u, device)
    e0, grads = model.elbo_and_grad(Xd, Y, noise=noise)
    e0 = float(e0.cpu())
    grads = {k: v.clone() for k, v in grads.items()}
    manual = []
    for name, layer in (("pred", model.pred_layer), ("assign", model.assign_layer)):
        mu, L = _dev(layer.q_mu.clone(), device), _dev(layer.q_sqrt.clone(), device)
        ops.natgrad_step(mu, L, grads[name + ".q_mu"], grads[name + ".q_sqrt"], gamma * N)
        manual.append((mu, L))
    ng = NaturalGradient(gamma)
    infos = ng.step(model, grads)
    assert ng.skipped() == 0 and all(i.cpu().tolist() == [0] * K for i in infos)
    for (mu, L), layer in zip(manual, (model.pred_layer, model.assign_layer)):
        assert torch.equal(mu.view(torch.int32), layer.q_mu.view(torch.int32))
        assert torch.equal(L.view(torch.int32), layer.q_sqrt.view(torch.int32))
    e1 = float(model._build_likelihood(Xd, Y, noise=noise).cpu())
    print(f"K=3 step: elbo {e0:.6f} -> {e1:.6f}; oracle {e_before:.6f} -> {e_after:.6f}")
    assert e1 == pytest.approx(e_after, rel=1e-4)
    assert e1 > e0


def test_run_natgrad_adam_beats_run_adam(device):
    """60 full-batch iterations from the same start and seed: run_natgrad_adam(gamma = 0.1)
    ends above run_adam (CPU oracle: about -0.68 against -0.85; measured -0.723 against -0.895,
    a gap of 0.172), with no skipped step."""
    from utils.data import Dataset
    from utils.training_utils import run_adam, run_natgrad_adam
    from modulatedgps_amd.training import NaturalGradient
    X, Y, p = R.synthetic_problem(1000, 25, 3, 1, 0.5, state="init", S=5)
    Xd = torch.as_tensor(X, dtype=torch.float32, device=device)
    Yd = torch.as_tensor(Y, dtype=torch.float32, device=device)
    out = {}
    for name in ("adam", "natgrad"):
        model = build_model(p, device, seed=0)
        it = iter(Dataset.from_tensor_slices((Xd, Yd)).shuffle(buffer_size=1000, seed=0).batch(1000).repeat())
        if name == "adam":
            out[name] = run_adam(model, 60, it, 0.01)
        else:
            ng = NaturalGradient(0.1)
            out[name] = run_natgrad_adam(model, 60, it, 0.01, gamma=ng)
            assert ng.skipped() == 0
    for iters, elbos in out.values():
        assert iters == list(range(5, 61, 5))
        assert np.all(np.isfinite(elbos))
    gap = np.mean(out["natgrad"][1][-3:]) - np.mean(out["adam"][1][-3:])
    print(f"run_natgrad_adam - run_adam, mean of the last three ELBOs: {gap:.4f}")
    assert gap > 0
