"""GPU tests of the greedy conditional-variance selection (csrc/greedy.hip;
modulatedgps_amd.inducing) against the float64 statement tests/greedy_ref.py.

Tolerances (none taken from the code under test):
  pivots    the float64 reference's sequence, m and stopped exactly on the cases of
            greedy_ref.CASES -- tests/test_greedy_host.py asserts that the emulation of the
            device's number formats (float64 kernel values and d, float32 factor) keeps it.
  gate      GR.gate() = 4 x the emulation's worst |d - d_ref| / variance over those cases
            (1.5e-7, so 5.9e-7); the 4 x covers the device's exp, its fused multiply-adds
            and the order of its float64 dot against NumPy's.  It bounds, along the device's
            own pivots, the shortfall of every pivot against the float64 maximum and the
            residual; dmax and trace to the relative error it implies at the last dmax.
            The same gate on greedy_ref.PATH_CASES (a workgroup sweeping two tiles; more steps
            than one LDS chunk), where the host test asserts the emulation's error is no larger.
  below the default threshold (1e-6): the relative shortfall of each pivot, 4 x the
            emulation's worst on the same input.
Every measured figure is printed (`GREEDY <quantity> <value>`) before it is asserted."""
import functools

import numpy as np
import pytest
import torch

from modulatedgps_amd import inducing, ops
from modulatedgps_amd.kernels import SquaredExponential
from tests import greedy_ref as GR

pytestmark = pytest.mark.gpu

CASE_IDS = [c.name for c in GR.CASES]


def _kernel(variance, ls, device):
    return SquaredExponential(variance=variance, lengthscales=np.asarray(ls), device=device)


def _host(r):
    """A GreedyVarianceResult as numpy arrays."""
    return dict(Z=r.Z.cpu().numpy(), indices=r.indices.cpu().numpy(), dmax=r.dmax.cpu().numpy(),
                trace=r.trace.cpu().numpy(), residual=r.residual.cpu().numpy(),
                factor=None if r.factor is None else r.factor.cpu().numpy(), stopped=r.stopped)


def _same_bits(a, b, fields=("Z", "indices", "dmax", "trace", "residual", "factor")):
    return a["stopped"] == b["stopped"] and all(
        a[f].shape == b[f].shape and a[f].tobytes() == b[f].tobytes() for f in fields)


@functools.lru_cache(maxsize=None)
def _device_run(name):
    """One device selection per case at the default threshold (computed once, with the factor)."""
    c = {c.name: c for c in GR.CASES}[name]
    dev = torch.device("cuda", 0)
    X, M, variance, ls = c.args()
    return _host(inducing.greedy_variance_device(X, M, _kernel(variance, ls, dev), want_factor=True))


# ------------------------------------------------------------------ 1. the exact pivot sequence
@pytest.mark.parametrize("name", CASE_IDS)
def test_pivots_are_the_float64_sequence(device, name):
    c = {c.name: c for c in GR.CASES}[name]
    ref, got = GR.case_reference(name), _device_run(name)
    m = len(got["indices"])
    first_diff = next((i for i, (a, b) in enumerate(zip(got["indices"], ref.indices)) if a != b), None)
    print(f"GREEDY {name} m {m} (reference {len(ref.indices)}) stopped {got['stopped']} first difference {first_diff}")
    assert m == c.m and got["stopped"] == c.stopped
    assert got["indices"].dtype == np.int64 and np.array_equal(got["indices"], ref.indices)
    X = c.X()
    assert got["Z"].dtype == np.float32 and np.array_equal(got["Z"], X[ref.indices])
    if name == "tie":
        assert got["indices"][0] == 0 and got["indices"][1] == ref.indices[1]
    if name == "duplicates":
        rows = got["indices"] // 2                      # rows 2 r and 2 r + 1 are equal
        assert len(set(rows.tolist())) == m


# ------------------------------------------------------------------ 2. optimal along its own path
@pytest.mark.parametrize("name", CASE_IDS)
def test_every_pivot_is_the_float64_maximum_to_the_gate(device, name):
    c = {c.name: c for c in GR.CASES}[name]
    got = _device_run(name)
    X, _, variance, ls = c.args()
    var = GR.hyper(variance, 1.0)[0]
    gate = GR.gate()
    ref = GR.reference(X, len(got["indices"]), variance, ls, path=got["indices"])
    short = float(((ref.top - ref.dmax) / var).max())
    res = float(np.abs(got["residual"] - ref.residual).max() / var)
    rel = gate * var / ref.dmax[-1]
    e_dmax = float((np.abs(got["dmax"] - ref.dmax) / ref.dmax).max())
    e_trace = float((np.abs(got["trace"] - ref.trace) / ref.trace).max())
    print(f"GREEDY {name} gate {gate:.3e} shortfall/variance {short:.3e} residual error/variance {res:.3e} "
          f"dmax rel {e_dmax:.3e} trace rel {e_trace:.3e} (allowed {rel:.3e})")
    assert short <= gate
    assert res <= gate
    assert got["residual"].dtype == np.float64 and got["residual"].min() >= 0.0
    assert np.all(np.diff(got["dmax"]) <= 0.0)
    assert e_dmax <= rel and e_trace <= rel
    assert got["trace"][-1] == pytest.approx(got["residual"].sum(), rel=1e-12)


@pytest.mark.parametrize("name", [c[0] for c in GR.PATH_CASES])
def test_more_tiles_than_workgroups_and_more_steps_than_one_chunk(device, name):
    """The step kernel's two other paths (greedy_ref.PATH_CASES), along the device's pivots."""
    X, M, variance, ls = GR.path_case(name)
    var = GR.hyper(variance, 1.0)[0]
    got = _host(inducing.greedy_variance_device(X, M, _kernel(variance, ls, device), block=M, want_factor=True))
    p = got["indices"]
    ref = GR.along(X, p, variance, ls)
    short = float(((ref.top - ref.dmax) / var).max())
    res = float(np.abs(got["residual"] - ref.residual).max() / var)
    print(f"GREEDY {name} m {len(p)} shortfall/variance {short:.3e} residual error/variance {res:.3e} "
          f"(gate {GR.gate():.3e})")
    assert len(p) == M and not got["stopped"] and len(set(p.tolist())) == M
    assert short <= GR.gate() and res <= GR.gate()
    assert got["residual"].min() >= 0.0 and np.all(np.diff(got["dmax"]) <= 0.0)
    assert got["trace"][-1] == pytest.approx(got["residual"].sum(), rel=1e-12)


# ------------------------------------------------------------------ 3. bitwise determinism
def test_results_do_not_depend_on_the_call_the_block_or_the_leading_dimensions(device):
    c = GR.CASES[0]
    X, M, variance, ls = c.args()
    kern = _kernel(variance, ls, device)
    base = _device_run(c.name)
    assert _same_bits(base, _host(inducing.greedy_variance_device(X, M, kern, want_factor=True)))
    for block in (1, 7, 64, M):
        assert _same_bits(base, _host(inducing.greedy_variance_device(X, M, kern, block=block, want_factor=True))), block
    # rows of X three floats apart from the next
    wide = torch.zeros(c.N, c.D + 3, device=device)
    wide[:, :c.D] = torch.as_tensor(X, device=device)
    assert _same_bits(base, _host(inducing.greedy_variance_device(wide[:, :c.D], M, kern, want_factor=True)))
    # a factor with rows 8 floats longer than round4(N), through the ops layer
    Xd = torch.as_tensor(X, device=device)
    ws = ops.greedy_workspace(c.N, M, c.D, device)
    store = torch.full((M, (c.N + 3) // 4 * 4 + 8), float("nan"), device=device)
    factor = store[:, :c.N]
    state = torch.zeros(2, dtype=torch.int32, device=device)
    ops.greedy_init(c.N, c.D, kern.variance, 1e-4, ws)
    ops.greedy_steps(Xd, kern.variance, kern.lengthscales, M, M, factor, ws, state)
    indices, Z, dmax, trace, residual, info = ops.greedy_result(Xd, M, ws)
    m, stopped = (int(v) for v in info.cpu())
    assert state.cpu().tolist() == [m, stopped]
    padded = dict(Z=Z[:m].cpu().numpy(), indices=indices[:m].cpu().numpy(), dmax=dmax[:m].cpu().numpy(),
                  trace=trace[:m].cpu().numpy(), residual=residual.cpu().numpy(),
                  factor=factor[:m].contiguous().cpu().numpy(), stopped=bool(stopped))
    assert _same_bits(base, padded)
    # without the factor: the same selection
    plain = inducing.greedy_variance_device(X, M, kern)
    assert plain.factor is None and np.array_equal(plain.indices.cpu().numpy(), base["indices"])


# ------------------------------------------------------------------ 4. below the default threshold
def test_below_the_default_threshold(device):
    c = GR.CASES[0]
    X, _, variance, ls = c.args()
    var = GR.hyper(variance, 1.0)[0]
    emu, _, emu_worst = GR.low_threshold_emulation()
    got = _host(inducing.greedy_variance_device(X, GR.LOW_M, _kernel(variance, ls, device),
                                                threshold=GR.LOW_THRESHOLD, want_factor=True))
    m = len(got["indices"])
    ref = GR.reference(X, m, variance, ls, path=got["indices"])
    sub = GR.suboptimality(ref)
    print(f"GREEDY threshold {GR.LOW_THRESHOLD:g}: m {m} (emulation {len(emu.indices)}) worst relative shortfall "
          f"{sub.max():.3e} (emulation {emu_worst:.3e}, allowed {4 * emu_worst:.3e})")
    for thr in (1e-4, 3e-5, 1e-5, 3e-6, 1e-6):
        k = int((ref.top > thr * var).sum())
        print(f"GREEDY   down to {thr:g} x variance: {k} steps, worst relative shortfall {sub[:k].max():.3e}")
    assert len(set(got["indices"].tolist())) == m
    assert all(np.isfinite(got[f]).all() for f in ("Z", "dmax", "trace", "residual", "factor"))
    assert got["residual"].min() >= 0.0 and np.all(np.diff(got["dmax"]) <= 0.0)
    assert got["dmax"][-1] > GR.LOW_THRESHOLD * var
    assert sub.max() <= 4 * emu_worst


# ------------------------------------------------------------------ 5. edges
@pytest.mark.parametrize("N", GR.EDGE_SIZES)
def test_sizes_around_the_wave_and_the_tile(device, N):
    X, M = GR.edge_input(N), min(N, 8)
    ref = GR.reference(X, M, *GR.EDGE_KERNEL)
    got = _host(inducing.greedy_variance_device(X, M, _kernel(*GR.EDGE_KERNEL, device), want_factor=True))
    var = GR.hyper(GR.EDGE_KERNEL[0], 1.0)[0]
    assert np.array_equal(got["indices"], ref.indices) and got["stopped"] == ref.stopped
    assert got["factor"].shape == (len(ref.indices), N)
    assert np.abs(got["residual"] - ref.residual).max() <= GR.gate() * var
    assert np.abs(got["dmax"] - ref.dmax).max() <= GR.gate() * var
    assert got["dmax"][0] == var


def test_one_point_and_every_point(device):
    X = GR.edge_input(257)
    kern = _kernel(1.0, [0.5], device)
    one = inducing.greedy_variance_device(X, 1, kern)
    assert one.indices.cpu().tolist() == [0] and not one.stopped and tuple(one.Z.shape) == (1, 2)
    assert float(one.trace.cpu()[0]) == pytest.approx(float(one.residual.sum().cpu()), rel=1e-12)
    # M = N on a smooth 1-D input: the threshold ends it long before N
    x = GR.smooth_input()
    ref = GR.reference(x[:, None], GR.SMOOTH_N, 1.0, [1.0])
    r = inducing.greedy_variance_device(x, GR.SMOOTH_N, _kernel(1.0, [1.0], device))
    m = len(r.indices)
    print(f"GREEDY smooth 1-D input: m {m} of {GR.SMOOTH_N} (reference {len(ref.indices)})")
    assert r.stopped and m == len(ref.indices) < 30 and tuple(r.Z.shape) == (m, 1)
    assert np.array_equal(r.indices.cpu().numpy(), ref.indices)
    assert float(r.residual.max().cpu()) <= 1e-4 + GR.gate()


def test_scalar_and_equal_ard_lengthscales_give_the_same_bits(device):
    X = GR.case_inputs()["f64kernel"]
    a = _host(inducing.greedy_variance_device(X, 64, _kernel(1.0, [0.8], device), want_factor=True))
    b = _host(inducing.greedy_variance_device(X, 64, _kernel(1.0, [0.8, 0.8, 0.8], device), want_factor=True))
    assert _same_bits(a, b)


# ------------------------------------------------------------------ 6. the factor
@pytest.mark.parametrize("name", CASE_IDS)
def test_factor_reproduces_the_kernel_on_the_chosen_rows(device, name):
    c = {c.name: c for c in GR.CASES}[name]
    got = _device_run(name)
    X, _, variance, ls = c.args()
    var, lsd = GR.hyper(variance, ls)
    p = got["indices"]
    F = got["factor"].astype(np.float64)
    assert got["factor"].dtype == np.float32 and F.shape == (len(p), c.N)
    K = GR.kernel_matrix(X[p], X[p], var, lsd)
    e_k = float(np.abs(F[:, p].T @ F[:, p] - K).max() / var)
    e_r = float(np.abs(np.maximum(var - (F * F).sum(axis=0), 0.0) - got["residual"]).max() / var)
    print(f"GREEDY {name} factor: |F^T F - K|/variance {e_k:.3e} |variance - sum F^2 - residual|/variance {e_r:.3e}")
    assert e_k <= GR.gate() and e_r <= GR.gate()


# ------------------------------------------------------------------ 7. use
def test_selection_feeds_the_svgp_layer_with_pivots_above_the_threshold(device):
    from MixtureGPs.inducing import ConditionalVariance, greedy_variance
    from modulatedgps_amd.config import default_jitter
    from modulatedgps_amd.likelihoods import GaussianModified
    from modulatedgps_amd.models import SVGPModified
    c = GR.CASES[0]
    X, M, variance, ls = c.args()
    kern = _kernel(variance, ls, device)
    Z, indices = greedy_variance(X, M, kern)
    assert isinstance(Z, np.ndarray) and Z.dtype == np.float64 and Z.shape == (c.m, c.D)
    assert indices.dtype == np.int64 and np.array_equal(Z, X[indices].astype(np.float64))
    lik = GaussianModified(variance=np.full((1, 3), 0.1), device=device)
    layer = SVGPModified(kern, lik, inducing_variable=Z, num_latent_gps=3, whiten=True, device=device)
    Zt = layer.inducing_variable
    assert tuple(Zt.shape) == (c.m, c.D)
    _, _, info = ops.kuu_potrf_trtri([ops.as_padded(Zt)], [kern.variance], [kern.lengthscales], default_jitter())
    assert info.cpu().tolist() == [0]
    var, lsd = GR.hyper(variance, ls)
    pivots = np.diag(np.linalg.cholesky(GR.kernel_matrix(Z, Z, var, lsd))) ** 2      # no jitter
    print(f"GREEDY smallest squared Cholesky pivot of K(Z, Z) / variance {pivots.min() / var:.3e}")
    assert pivots.min() >= 1e-4 * var * (1 - 1e-3)
    Z2, i2 = ConditionalVariance().compute_initialisation(X, M, kern)
    assert np.array_equal(Z2, Z) and np.array_equal(i2, indices)
