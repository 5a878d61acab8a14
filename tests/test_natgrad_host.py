"""CPU tests of the natural-gradient step (mgp_natgrad_step, csrc/natgrad.hip): the float64
reference of tests/natgrad_ref.py (direct route) against the closed form the kernel uses, the
conjugate one-step property, and the C-ABI's argument checks without a GPU."""
import ctypes

import numpy as np
import pytest

from modulatedgps_amd import _lib
from tests import natgrad_ref as NR


def step_closed(q_mu, q_sqrt, g_mu, g_sqrt, step):
    """The kernel's closed form in numpy float64: B = I + step (P + P^T), J B J = C C^T,
    W = J C^T J, L' = L W^-1, mu' = mu - step L' (L'^T g_mu).  No inverse of L or S."""
    M, K = q_mu.shape
    mu_new, L_new = q_mu.copy(), np.tril(q_sqrt).copy()
    for k in range(K):
        L = np.tril(q_sqrt[k])
        P = NR.phi(L.T @ np.tril(g_sqrt[k]))
        B = np.eye(M) + step * (P + P.T)
        C = np.linalg.cholesky(B[::-1, ::-1])
        W = C.T[::-1, ::-1]
        assert np.allclose(np.triu(W, 1), 0.0)
        Ln = np.linalg.solve(W.T, L.T).T
        L_new[k] = Ln
        mu_new[:, k] = q_mu[:, k] - step * Ln @ (Ln.T @ g_mu[:, k])
    return mu_new, L_new


@pytest.mark.parametrize("kind", NR.KINDS)
@pytest.mark.parametrize("step", NR.STEPS)
def test_direct_route_equals_closed_form(step, kind):
    """Over every shape of the GPU test: the reference step exists for every expert (so no GPU
    case is excused), lambda_min(B) keeps its margin after the float32 rounding of g_L, and
    the two routes agree.  Bound: the direct route inverts L and the new precision explicitly,
    so it carries about eps64 cond(S) cond(B) (cond(S) up to 1e8 in the ill-conditioned draws,
    measured 3.3e-8 at worst there and 8.5e-13 elsewhere); the closed form carries eps64 cond(B)."""
    for M in NR.SHAPES_M:
        for K in NR.SHAPES_K:
            q_mu, q_sqrt, g_mu, g_sqrt = NR.draw_case(M, K, step, kind)
            assert all(NR.min_eig_B(q_sqrt[k], g_sqrt[k], step) > 0.4 for k in range(K))
            mu_d, L_d, ok = NR.step_direct(q_mu, q_sqrt, g_mu, g_sqrt, step)
            assert ok.all(), (M, K)
            mu_c, L_c = step_closed(q_mu, q_sqrt, g_mu, g_sqrt, step)
            tol = 1e-6 if kind == "illcond" else 1e-10
            assert NR.normwise(L_d, L_c) < tol, (M, K, NR.normwise(L_d, L_c))
            assert NR.normwise(mu_d, mu_c) < tol, (M, K, NR.normwise(mu_d, mu_c))
            assert np.all(np.sign(np.diagonal(L_d, axis1=1, axis2=2)) == np.sign(np.diagonal(q_sqrt, axis1=1, axis2=2)))
            assert np.all(np.sign(np.diagonal(L_c, axis1=1, axis2=2)) == np.sign(np.diagonal(q_sqrt, axis1=1, axis2=2)))


def test_step_zero_and_failure_in_reference():
    q_mu, q_sqrt, g_mu, g_sqrt = NR.draw_case(25, 3, 1.0, "plain")
    mu0, L0, ok = NR.step_direct(q_mu, q_sqrt, g_mu, g_sqrt, 0.0)
    assert ok.all() and NR.normwise(L0, q_sqrt) < 1e-12 and NR.normwise(mu0, q_mu) < 1e-12
    q_sqrt[1] = np.eye(25)
    g_sqrt[1] = -2.0 * np.eye(25)       # B = -I at step 1
    _, _, ok = NR.step_direct(q_mu, q_sqrt, g_mu, g_sqrt, 1.0)
    assert list(ok) == [True, False, True]


def test_conjugate_model_is_solved_in_one_step():
    """One step at step = 1 from the float64 gradients lands on the conjugate optimum."""
    c = NR.conjugate_case()
    for route in (NR.step_direct, step_closed):
        out = route(c["mu"][:, None], c["L"][None], c["g_mu64"][:, None], c["g_L64"][None], 1.0)
        mu, L = out[0][:, 0], out[1][0]
        assert NR.normwise(L @ L.T, c["S_star"]) < 1e-12
        assert NR.normwise(mu, c["mu_star"]) < 1e-12


def _call(lib, **kw):
    c = ctypes.c_void_p(256)
    M, K = kw.get("M", 70), kw.get("K", 3)
    d = dict(q_mu=c, ldq=4, q_sqrt=c, ldqs=72, strideq=72 * 70, g_q_mu=c, ldg=4, g_q_sqrt=c, ldgs=72,
             strideg=72 * 70, dbl=0, M=M, K=K, step=1.0, sign=-1.0, info=c, ws=c,
             wsb=lib.mgp_natgrad_workspace_bytes(70, 3), stream=None)
    d.update(kw)
    return lib.mgp_natgrad_step(*[d[k] for k in ("q_mu", "ldq", "q_sqrt", "ldqs", "strideq", "g_q_mu", "ldg",
                                                 "g_q_sqrt", "ldgs", "strideg", "dbl", "M", "K", "step", "sign",
                                                 "info", "ws", "wsb", "stream")])


def test_argument_checks_before_any_hip_call():
    """Every violation has a code of its own (mgp_hip.h) and is refused before a HIP call or a
    pointer read: the pointers here are not mapped, and there is no GPU."""
    lib = _lib.load()
    assert _call(lib, q_mu=None) == -1
    assert _call(lib, ldq=2) == -2
    assert _call(lib, q_sqrt=None) == -3
    assert _call(lib, ldqs=69) == -4
    assert _call(lib, strideq=72 * 70 - 1) == -5
    assert _call(lib, g_q_mu=None) == -6
    assert _call(lib, ldg=2) == -7
    assert _call(lib, g_q_sqrt=None) == -8
    assert _call(lib, ldgs=69) == -9
    assert _call(lib, strideg=72 * 70 - 1) == -10
    assert _call(lib, dbl=2) == -11
    assert _call(lib, M=0) == -12
    assert _call(lib, K=0) == -13
    for bad in (-0.5, float("inf"), float("nan")):
        assert _call(lib, step=bad) == -14
    assert _call(lib, sign=float("nan")) == -15 and _call(lib, sign=float("inf")) == -15
    assert _call(lib, info=None) == -16
    assert _call(lib, M=(1 << 20) + 1, ldqs=1 << 21, ldgs=1 << 21) == 3
    assert _call(lib, ws=None) == 1
    assert _call(lib, wsb=lib.mgp_natgrad_workspace_bytes(70, 3) - 1) == 1
    assert _call(lib, ws=ctypes.c_void_p(264)) == 2
    # a single expert needs no stride
    assert _call(lib, K=1, strideq=0, strideg=0, wsb=0) == 1


def test_workspace_size_formula():
    """J B J / L' (float64) + C^-T (float32, rows padded to 4) + K3's workspace for
    min(K, 8) matrices + t and mu' (float64), each rounded up to 256 bytes."""
    lib = _lib.load()
    up = lambda x: (x + 255) // 256 * 256
    M, K = 70, 3
    want = up(K * M * M * 8) + up(K * M * 72 * 4) + up(lib.mgp_chol_workspace_bytes(M, K)) + 2 * up(K * M * 8)
    assert lib.mgp_natgrad_workspace_bytes(M, K) == want == 1165056
    M, K = 1024, 9
    want = up(K * M * M * 8) + up(K * M * M * 4) + up(lib.mgp_chol_workspace_bytes(M, 8)) + 2 * up(K * M * 8)
    assert lib.mgp_natgrad_workspace_bytes(M, K) == want
    assert lib.mgp_natgrad_workspace_bytes(0, 3) == 0 and lib.mgp_natgrad_workspace_bytes(70, 0) == 0


def test_natural_gradient_needs_a_scale():
    from modulatedgps_amd.training import NaturalGradient

    class Model:
        num_data = None
    with pytest.raises(ValueError):
        NaturalGradient(0.1).step(Model(), {})
    assert NaturalGradient(0.1, scale=10.0).skipped() == 0
