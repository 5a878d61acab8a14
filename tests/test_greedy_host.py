"""CPU tests of the greedy conditional-variance selection: the float64 statement
tests/greedy_ref.py is a pivoted Cholesky, the C-ABI entries' argument checks and size limits
and the Python argument checks (all made before any HIP call, so they run without a GPU), and
the suitability of the inputs the GPU tests (tests/test_gpu_greedy.py) rely on."""
import ctypes

import numpy as np
import pytest

from modulatedgps_amd import _lib, inducing
from modulatedgps_amd.kernels import SquaredExponential
from tests import greedy_ref as GR

ENTRIES = ("mgp_greedy_workspace_bytes", "mgp_greedy_init", "mgp_greedy_steps", "mgp_greedy_result")
MGP_ERR_WORKSPACE, MGP_ERR_ALIGN, MGP_ERR_UNSUPPORTED = 1, 2, 3
NMAX = 2 ** 31 - 1


def test_entries_are_bound_declared_and_exported():
    syms = _lib.header_symbols()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and name in syms and hasattr(raw, name), name
    import MixtureGPs.inducing as drop_in
    for name in ("greedy_variance", "greedy_variance_device", "ConditionalVariance"):
        assert getattr(drop_in, name) is getattr(inducing, name)


# ------------------------------------------------------------------ the C-ABI
def _call(name, base, **kw):
    assert len(base) == len(_lib.SIGNATURES[name][1]), name
    return getattr(_lib.load(), name)(*{**base, **kw}.values())


def _ws(N, M, D):
    return _lib.load().mgp_greedy_workspace_bytes(N, M, D)


def test_workspace_query_and_limits():
    assert _ws(1500, 128, 2) > 0 and _ws(1500, 128, 2) % 256 == 0
    assert _ws(65536, 1024, 8) > _ws(65536, 1, 8) > 65536 * 8
    assert _ws(100, 100, 32) > 0 and _ws(NMAX, 1, 1) > 0 and _ws(1, 1, 1) > 0
    # one past each limit, and nonsense sizes: 0
    assert _ws(100, 10, 33) == 0 and _ws(100, 101, 8) == 0 and _ws(NMAX + 1, 10, 8) == 0
    assert _ws(0, 1, 1) == 0 and _ws(10, 0, 1) == 0 and _ws(10, 1, 0) == 0


def test_entries_reject_bad_arguments_before_any_hip_call():
    c = ctypes.c_void_p(256)
    N, M, D = 100, 10, 8
    wsb = _ws(N, M, D)
    init = dict(N=N, D=D, variance=c, thr=1e-4, ws=c, wsb=wsb, stream=None)
    call = lambda **kw: _call("mgp_greedy_init", init, **kw)
    assert call(N=-1) == -1 and call(D=0) == -2 and call(variance=None) == -3
    assert call(thr=-1e-9) == -4 and call(thr=float("nan")) == -4
    assert call(D=33) == call(N=NMAX + 1) == MGP_ERR_UNSUPPORTED
    assert call(N=0) == 0 and call(N=0, ws=None) == 0          # nothing to do
    assert call(wsb=_ws(N, 1, D) - 1) == call(ws=None) == MGP_ERR_WORKSPACE
    assert call(ws=ctypes.c_void_p(264)) == MGP_ERR_ALIGN

    steps = dict(X=c, ldx=D, N=N, D=D, variance=c, ls=c, n_ls=1, M=M, B=4, L=c, ldl=N, ws=c, wsb=wsb, state=c,
                 stream=None)
    call = lambda **kw: _call("mgp_greedy_steps", steps, **kw)
    assert call(X=None) == -1 and call(ldx=D - 1) == -2 and call(N=-1) == -3 and call(D=0) == -4
    assert call(variance=None) == -5 and call(ls=None) == -6 and call(n_ls=2) == -7 and call(n_ls=0) == -7
    assert call(M=0) == -8 and call(B=0) == -9 and call(L=None) == -10 and call(ldl=N - 1) == -11
    assert call(state=None) == -14
    assert call(D=33, ldx=33, n_ls=33) == call(N=NMAX + 1) == call(M=N + 1) == MGP_ERR_UNSUPPORTED
    assert call(N=0) == 0
    assert call(wsb=wsb - 1) == call(ws=None) == MGP_ERR_WORKSPACE
    assert call(ldl=N + 2) == call(L=ctypes.c_void_p(260)) == call(ws=ctypes.c_void_p(264)) == MGP_ERR_ALIGN
    assert call(n_ls=D, wsb=wsb - 1) == MGP_ERR_WORKSPACE      # ARD passes the n_ls check

    res = dict(X=c, ldx=D, N=N, D=D, M=M, ws=c, wsb=wsb, indices=c, Z=c, ldz=D, dmax=c, trace=c, residual=None,
               info=c, stream=None)
    call = lambda **kw: _call("mgp_greedy_result", res, **kw)
    assert call(X=None) == -1 and call(ldx=D - 1) == -2 and call(N=-1) == -3 and call(D=0) == -4
    assert call(M=0) == -5 and call(indices=None) == -8 and call(Z=None) == -9 and call(ldz=D - 1) == -10
    assert call(dmax=None) == -11 and call(trace=None) == -12 and call(info=None) == -14
    assert call(D=33, ldx=33, ldz=33) == call(N=NMAX + 1) == call(M=N + 1) == MGP_ERR_UNSUPPORTED
    assert call(N=0) == 0
    assert call(wsb=wsb - 1) == call(ws=None) == MGP_ERR_WORKSPACE
    assert call(ws=ctypes.c_void_p(264)) == MGP_ERR_ALIGN


def test_python_argument_checks_need_no_device():
    """Every check raises ValueError before anything is uploaded (the kernel's parameters
    live on the CPU here, and no device exists)."""
    k1 = SquaredExponential(1.0, 0.5, device="cpu")
    k3 = SquaredExponential(1.0, [0.5, 0.6, 0.7], device="cpu")
    X = np.linspace(-1.0, 1.0, 40).reshape(20, 2)
    bad = [
        dict(X=np.array([[0.0], [np.nan]]), M=1, kernel=k1),
        dict(X=np.array([[0.0], [np.inf]]), M=1, kernel=k1),
        dict(X=X, M=0, kernel=k1), dict(X=X, M=21, kernel=k1), dict(X=X, M=2.5, kernel=k1),
        dict(X=np.zeros((40, 33)), M=4, kernel=k1),
        dict(X=np.zeros((4, 3, 2)), M=2, kernel=k1),
        dict(X=X, M=4, kernel=k3),                          # 3 lengthscales, 2 columns
        dict(X=X[:, 0], M=4, kernel=k3),                    # 1-D is [N, 1]
        dict(X=X, M=4, kernel=object()),
        dict(X=X, M=4, kernel=k1, threshold=-1e-6), dict(X=X, M=4, kernel=k1, threshold=float("nan")),
        dict(X=X, M=4, kernel=k1, threshold=float("inf")),
        dict(X=X, M=4, kernel=k1, block=0), dict(X=X, M=4, kernel=k1, block=1.5),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            inducing.greedy_variance_device(**kw)
    with pytest.raises(ValueError):
        inducing.greedy_variance(X, 0, k1)
    with pytest.raises(ValueError):
        inducing.ConditionalVariance(threshold=-1.0).compute_initialisation(X, 4, k1)
    with pytest.raises(ValueError):
        inducing.ConditionalVariance().compute_initialisation(X, 4, "SquaredExponential")


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("case", GR.CASES, ids=lambda c: c.name)
def test_reference_is_a_pivoted_cholesky(case):
    """On the chosen rows L^T L reproduces Kff, residual = diag(Kff) - sum L^2 >= 0, dmax is
    the residual diagonal at each pivot and does not increase, trace is the residual's sum."""
    X, _, variance, ls = case.args()
    var, lsd = GR.hyper(variance, ls)
    r = GR.case_reference(case.name)
    m, p, L = len(r.indices), r.indices, r.factor
    assert len(set(p.tolist())) == m
    K = GR.kernel_matrix(X[p], X, var, lsd)                 # [m, N]
    np.testing.assert_allclose(L.T[p] @ L, K, rtol=0, atol=1e-12 * var)
    np.testing.assert_allclose(r.residual, var - (L * L).sum(axis=0), rtol=0, atol=1e-12 * var)
    assert r.residual.min() >= 0.0 and np.all(r.residual[p] <= 1e-12 * var)
    assert np.all(np.diff(r.dmax) <= 1e-12 * var) and r.dmax[0] == var
    assert r.trace[-1] == r.residual.sum()
    # pivoted: step t leaves nothing on the rows chosen before it, and sqrt(dmax[t]) on its own
    T = L[:, p]
    assert np.abs(np.tril(T, -1)).max() <= 1e-10 and np.allclose(np.diag(T), np.sqrt(r.dmax), rtol=1e-10)


# ------------------------------------------------------------------ input suitability
def test_gpu_test_inputs_are_suitable():
    """What tests/test_gpu_greedy.py relies on, for the inputs of tests/greedy_ref.py: the
    emulation of the device's number formats takes the float64 reference's pivots on every
    exact-sequence case, the reference takes as many steps as the case claims, and the
    emulation's |d - d_ref| / variance -- of which the GPU gate is 4 x -- is the 1e-7 that a
    float32 factor allows (a few 2^-24 per subtracted square)."""
    for c in GR.CASES:
        r, e = GR.case_reference(c.name), GR.case_emulation(c.name)
        assert len(r.indices) == c.m and r.stopped == c.stopped, (c.name, len(r.indices), r.stopped)
        assert len(r.indices) >= (c.m if c.stopped else c.M)
        assert np.array_equal(e.indices, r.indices) and e.stopped == r.stopped, c.name
    worst = GR.emulation_d_error()
    print(f"GREEDY emulation max|d - d_ref|/variance {worst:.3e} gate {GR.gate():.3e}")
    assert 2.0 ** -24 < worst < 4e-7
    # the first input: after the first pivot (row 0) rows in several workgroup tiles still hold
    # d == variance exactly, and the lowest of them is the second pivot
    tie = GR.case_reference("tie")
    var = GR.hyper(GR.CASES[0].variance, 1.0)[0]
    tied = np.flatnonzero(tie.d_steps[0] == var)
    assert tie.indices[0] == 0 and len(set((tied // 256).tolist())) >= 2 and tie.indices[1] == tied[0]
    # duplicates: equal rows are neighbours (2 r, 2 r + 1)
    X = GR.case_inputs()["duplicates"]
    assert np.array_equal(X[0::2], X[1::2]) and len(np.unique(X, axis=0)) == 300
    # the edge inputs: the emulation keeps the reference's pivots there too
    for N in GR.EDGE_SIZES:
        args = (GR.edge_input(N), min(N, 8), *GR.EDGE_KERNEL)
        assert np.array_equal(GR.emulation(*args).indices, GR.reference(*args).indices), N
    x = GR.smooth_input()[:, None]
    r, e = GR.reference(x, GR.SMOOTH_N, 1.0, [1.0]), GR.emulation(x, GR.SMOOTH_N, 1.0, [1.0])
    assert r.stopped and len(r.indices) < 30 and np.array_equal(e.indices, r.indices)
    X = GR.case_inputs()["f64kernel"]
    assert np.array_equal(GR.emulation(X, 64, 1.0, [0.8]).indices, GR.reference(X, 64, 1.0, [0.8]).indices)
    # the inputs of the two other kernel paths: all M steps run, and the emulation's error
    # along its own pivots is within the worst of the cases above, so their gate holds here
    for name, N, D, M, *_ in GR.PATH_CASES:
        err, short, m = GR.path_case_emulation_error(name)
        print(f"GREEDY emulation on {name}: m {m} max|d - d_ref|/variance {err:.3e} shortfall/variance {short:.3e}")
        assert m == M and err <= worst and short <= worst
    assert GR.PATH_CASES[0][1] > 1024 * 256 and GR.PATH_CASES[1][3] > 1024
    # the run below the default threshold goes beyond 1e-5 * variance and has no duplicates
    e, r, sub = GR.low_threshold_emulation()
    print(f"GREEDY emulation at threshold {GR.LOW_THRESHOLD:g}: m {len(e.indices)} worst suboptimality {sub:.3e}")
    assert len(e.indices) > 160 and len(set(e.indices.tolist())) == len(e.indices) and 0.0 <= sub < 0.3
