"""CPU tests of the data-association entries (csrc/mixture_assign.hip): the C-ABI entries'
argument checks (all made before any HIP call, so they run without a GPU), known answers of the
float64 statement tests/mixture_assign_ref.py, and the conditions on the inputs of
tests/test_gpu_mixture_assign.py that the reference alone has to meet."""
import ctypes
import re

import numpy as np
import pytest

from modulatedgps_amd import _lib
from tests import mixture_assign_ref as AR

ENTRIES = ("mgp_mixture_responsibilities_workspace_bytes", "mgp_mixture_responsibilities", "mgp_mixture_modes")
MGP_OP_MIXTURE_RESPONSIBILITIES, MGP_OP_MIXTURE_MODES = 16, 17
MGP_ERR_WORKSPACE, MGP_ERR_UNSUPPORTED = 1, 3


def test_entries_are_bound_declared_and_exported():
    syms = _lib.header_symbols()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and name in syms and hasattr(raw, name), name
    text = open(_lib.HEADER_PATH).read()
    assert re.search(r"MGP_OP_MIXTURE_RESPONSIBILITIES\s*=\s*16\b", text)
    assert re.search(r"MGP_OP_MIXTURE_MODES\s*=\s*17\b", text)
    from modulatedgps_amd import ops
    from modulatedgps_amd.models import SMGP, SMGPModified
    assert callable(ops.mixture_responsibilities) and callable(ops.mixture_modes)
    for name in ("predict_responsibilities", "predict_labels", "predict_assignment_entropy", "expert_usage",
                 "predict_modes", "predict_map"):
        for cls in (SMGP, SMGPModified):
            assert callable(getattr(cls, name)) and callable(getattr(cls, name + "_device")), name


def test_workspace_query_matches_the_front():
    lib = _lib.load()
    for N, K in ((1, 1), (256, 3), (257, 3), (1000, 32), (65536, 8)):
        nbytes = lib.mgp_mixture_responsibilities_workspace_bytes(N, K)
        assert nbytes == lib.mgp_workspace_bytes(MGP_OP_MIXTURE_RESPONSIBILITIES, 0, N, K)
        assert nbytes == 8 * K * -(-N // 256)   # one double per (256-point workgroup, expert)
        assert lib.mgp_workspace_bytes(MGP_OP_MIXTURE_MODES, 0, N, K) == 0


def _resp(**kw):
    """mgp_mixture_responsibilities with valid (never dereferenced) arguments, overridden by kw."""
    lib = _lib.load()
    c = ctypes.c_void_p(256)
    N, K = 100, 3
    base = dict(mu_f=c, var_f=c, ldf=N, lik_var=c, weights=c, Y=c, N=N, K=K, resp=c, ldr=K, labels=c, entropy=c,
                usage=c, workspace=c, workspace_bytes=lib.mgp_mixture_responsibilities_workspace_bytes(N, K),
                stream=None)
    assert len(base) == len(_lib.SIGNATURES["mgp_mixture_responsibilities"][1])
    base.update(kw)
    return lib.mgp_mixture_responsibilities(*base.values())


def test_responsibilities_rejects_bad_arguments_before_any_hip_call():
    assert _resp(mu_f=None) == -1 and _resp(var_f=None) == -2 and _resp(ldf=99) == -3
    assert _resp(lik_var=None) == -4 and _resp(weights=None) == -5 and _resp(Y=None) == -6
    assert _resp(K=0) == -8 and _resp(K=-1) == -8
    assert _resp(K=33, ldr=33) == MGP_ERR_UNSUPPORTED
    assert _resp(ldr=2) == -10
    nbytes = _lib.load().mgp_mixture_responsibilities_workspace_bytes(100, 3)
    assert _resp(workspace_bytes=nbytes - 1) == MGP_ERR_WORKSPACE
    assert _resp(workspace=None) == MGP_ERR_WORKSPACE
    # N <= 0: nothing to do, after the checks
    assert _resp(N=0) == 0 and _resp(N=-3) == 0
    assert _resp(N=0, K=33, ldr=33) == MGP_ERR_UNSUPPORTED and _resp(N=0, Y=None) == -6 and _resp(N=0, ldr=2) == -10


def _modes(**kw):
    lib = _lib.load()
    c = ctypes.c_void_p(256)
    base = dict(mu_f=c, var_f=c, ldf=100, lik_var=c, weights=c, N=100, K=3, modes=c, mode_density=c, ldm=3, count=c,
                stream=None)
    assert len(base) == len(_lib.SIGNATURES["mgp_mixture_modes"][1])
    base.update(kw)
    return lib.mgp_mixture_modes(*base.values())


def test_modes_rejects_bad_arguments_before_any_hip_call():
    assert _modes(mu_f=None) == -1 and _modes(var_f=None) == -2 and _modes(ldf=99) == -3
    assert _modes(lik_var=None) == -4 and _modes(weights=None) == -5
    assert _modes(K=0) == -7 and _modes(K=33, ldm=33) == MGP_ERR_UNSUPPORTED
    assert _modes(ldm=2) == -10 and _modes(ldm=2, modes=None) == -10
    assert _modes(N=0) == 0 and _modes(N=-1) == 0
    assert _modes(N=0, K=33, ldm=33) == MGP_ERR_UNSUPPORTED and _modes(N=0, weights=None) == -5


# --------------------------------------------------------------------------- known answers
def test_reference_single_expert_known_answers():
    """K = 1: resp 1, entropy 0, one mode at mu with density 1 / (s sqrt(2 pi))."""
    rng = np.random.default_rng(0)
    N = 40
    mu, var_f = rng.normal(size=(N, 1)) * 3, rng.uniform(0.01, 1, (N, 1))
    lik_var, w = np.array([0.3]), np.ones((N, 1))
    s = np.sqrt(var_f[:, 0] + 0.3)
    Y = mu[:, 0] + rng.uniform(-30, 30, N) * s
    args = (mu, var_f, lik_var, w)
    assert np.array_equal(AR.responsibilities(*args, Y), np.ones((N, 1)))
    assert np.array_equal(AR.entropy(*args, Y), np.zeros(N))
    assert np.array_equal(AR.labels(*args, Y), np.zeros(N, int))
    assert np.array_equal(AR.usage(*args, Y), [N])
    for modes in (AR.modes_climb(*args), AR.modes_grid(*args), AR.climb_f32(*args)):
        for n, (y, dens) in enumerate(modes):
            assert y.shape == (1,) and abs(y[0] - mu[n, 0]) <= 1e-6 * abs(mu[n, 0])
            assert abs(dens[0] * s[n] * np.sqrt(2 * np.pi) - 1.0) <= 1e-10


@pytest.mark.parametrize("ratio,count", [(1.9, 1), (2.5, 2)])
def test_reference_two_equal_experts_are_bimodal_beyond_two_sigma(ratio, count):
    """Equal weights and a common s at -d / 2 and +d / 2: two modes exactly when d > 2 s."""
    s = np.array([0.3, 0.7, 1.1])
    mu = np.stack([-0.5 * ratio * s, 0.5 * ratio * s], 1) + np.array([[0.0], [2.0], [-5.0]])
    var_f, lik_var, w = np.repeat((s * s - 0.01)[:, None], 2, 1), np.array([0.01, 0.01]), np.full((3, 2), 0.5)
    for modes in (AR.modes_climb(mu, var_f, lik_var, w), AR.modes_grid(mu, var_f, lik_var, w),
                  AR.climb_f32(mu, var_f, lik_var, w)):
        for n, (y, dens) in enumerate(modes):
            assert y.size == count, (ratio, n, y)
            centre = mu[n].mean()
            if count == 1:
                assert abs(y[0] - centre) <= 1e-3 * s[n]
            else:
                assert abs(y.sum() - 2 * centre) <= 1e-6 * s[n] and mu[n, 0] < y.min() < centre < y.max() < mu[n, 1]
            assert np.allclose(dens, AR.density(mu[n:n + 1], var_f[n:n + 1], lik_var, w[n:n + 1], y[None])[0], rtol=1e-12)


def test_reference_zero_weight_and_coincident_experts():
    mu = np.array([[0.0, 1.0, 9.0], [2.0, 2.0, 2.0]])
    var_f, lik_var = np.array([[0.2, 0.1, 0.01], [0.3, 0.3, 0.3]]), np.array([0.05, 0.05, 0.05])
    w = np.array([[0.6, 0.4, 0.0], [0.2, 0.5, 0.3]])
    Y = np.array([9.0, 2.5])
    r = AR.responsibilities(mu, var_f, lik_var, w, Y)
    assert r[0, 2] == 0.0 and abs(r[0].sum() - 1) < 1e-15
    np.testing.assert_allclose(r[1], w[1], rtol=1e-14)
    climb, grid = AR.modes_climb(mu, var_f, lik_var, w), AR.modes_grid(mu, var_f, lik_var, w)
    assert all(y.max() < 2.0 for y, _ in (climb[0], grid[0]))   # the zero-weight expert at 9 is no start
    assert climb[1][0].tolist() == [2.0] and grid[1][0].tolist() == [2.0]
    none = AR.responsibilities(mu[:1], var_f[:1], lik_var, np.zeros((1, 3)), Y[:1])
    assert np.isnan(none).all() and AR.labels(mu[:1], var_f[:1], lik_var, np.zeros((1, 3)), Y[:1])[0] == -1


def test_reference_far_tails_stay_finite():
    """25 sigma from every expert every linear-domain density has underflowed in float32 (and
    at 40 sigma in float64); the log-domain statement still sums to 1."""
    d = AR.far_case(8)
    args = (d["mu_f"], d["var_f"], d["lik_var"], d["w"], d["Y"])
    t = np.abs(d["Y"].astype(np.float64)[:, None] - d["mu_f"]) / AR.scales(d["var_f"], d["lik_var"])
    assert t.min() >= 25.0
    assert np.exp(-0.5 * t.min() ** 2) < np.finfo(np.float32).tiny
    r = AR.responsibilities(*args)
    # |a| is about 25^2 / 2 here and larger for the other experts: its float64 rounding, some
    # 1e3 * 2^-52, is the error of a row's sum
    assert np.isfinite(r).all() and np.abs(r.sum(-1) - 1).max() < 1e-12
    assert np.isfinite(AR.entropy(*args)).all()


@pytest.mark.parametrize("K", AR.KS)
def test_reference_usage_sums_to_n_and_entropy_is_bounded(K):
    d = AR.case(K)
    args = (d["mu_f"], d["var_f"], d["lik_var"], d["w"], d["Y"])
    assert abs(AR.usage(*args).sum() - AR.N_CASE) <= 1e-9 * AR.N_CASE
    e = AR.entropy(*args)
    assert (e >= -1e-12).all() and (e <= np.log(K) + 1e-12).all()
    r = AR.responsibilities(*args)
    with np.errstate(divide="ignore", invalid="ignore"):
        direct = -np.where(r > 0, r * np.log(r), 0.0).sum(-1)
    np.testing.assert_allclose(e, direct, atol=1e-10)


# --------------------------------------------------------------------------- conditions on the GPU inputs
@pytest.mark.parametrize("K", AR.KS)
def test_gpu_inputs_meet_the_conditions(K):
    """On every generated case: climb and grid agree in count and position to 1e-9, distinct
    modes lie at least 0.05 min s apart, the float32 climb finds the same count, and the two
    largest a_k are at least 1e-3 apart at every point (far tails included)."""
    d = AR.case(K)
    smin = AR.scales(d["var_f"], d["lik_var"]).min(-1)
    climb, grid, emu = AR.case_modes(K)
    for n in range(AR.N_CASE):
        yc, yg, ye = np.sort(climb[n][0]), np.sort(grid[n][0]), np.sort(emu[n][0])
        assert 1 <= yc.size <= K
        assert yc.size == yg.size and np.abs(yc - yg).max() <= 1e-9, (n, yc, yg)
        assert ye.size == yc.size, (n, yc, ye)
        assert yc.size == 1 or np.diff(yc).min() >= 0.05 * smin[n], (n, yc)
        assert (np.diff(climb[n][1]) <= 0).all()
    assert AR.label_gap(d["mu_f"], d["var_f"], d["lik_var"], d["w"], d["Y"]).min() >= 1e-3
    f = AR.far_case(K)
    assert AR.label_gap(f["mu_f"], f["var_f"], f["lik_var"], f["w"], f["Y"]).min() >= 1e-3
    err = AR.f32_position_error(K)
    print(f"ASSIGNERR f32_climb_position_over_min_s_K{K} {err:.3e}")
    assert err <= 1.25 * AR.F32_POSITION_ERROR   # the margin: another libm's float32 exp
