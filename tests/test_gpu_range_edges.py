"""Every kernel family at the top of its supported D and K range, and one past it.

The kernels are compiled once per bucket of the input dimension (DMAX = 1, 2, 4, 8, 16,
32) and of the expert count (KMAX = 4 .. 32); the per-kernel modules stop at D = 16 and,
for most of K6, at K = 16.  Here the largest instantiations and the ragged sizes inside a
bucket (D = 7, 13, 17, 31; K = 9, 17, 31) run against float64 references on the
float32-rounded inputs, with the tolerances of the neighbouring per-kernel tests:

  Kuf / Kuu            elementwise 2e-6 * variance               (test_rbf_kuf_kuu)
  Kuf images           2e-6 var + k ln2 8 2^-24 (|z'|^2 + |x'|^2)  (test_kuf_and_trsm_images)
  L, L^-1 of Kuu       normwise 1e-6 + cond(Kuu) 1e-15           (test_kuu_factorisation_ill_conditioned)
  RBF backward         normwise / relative 1e-4                  (test_rbf_backward)
  full covariance      normwise 1e-4 per expert                  (test_full_cov_kernel)
  K6 data term         rel 1e-4, abs 1e-3                        (test_elbo_terms_explicit_and_philox)
  K6 backward          normwise 1e-4 per block                   (test_elbo_terms_backward)
  conditionals         normwise 1e-4 at cond(Kuu) < 1e6          (test_conditional_split_bf16)

Non-vacuity: with unit lengthscales at D = 32 every K(z, x) is ~e^-32 and an absolute
bound passes for a kernel that returns zeros, so the lengthscales grow with sqrt(D) (ARD:
sqrt(D) U(0.7, 1.4)) and every Kuf / Kuu case first asserts on its float64 reference that
median(Kuf) >= 0.05 var and cond(Kuu + 1e-6 I) < 1e6.

The limits the C-ABI enforces (include/mgp_hip.h): D <= 32 for the RBF
entries, the Kuf side job and the full covariance (mgp_kuu_potrf_trtri without the side
job takes any D); K <= 16 for K4 and the conditional backward; K <= 32 for K5, K6, the
full covariance and the §8(b) front.  One past each limit the entry returns
MGP_ERR_UNSUPPORTED and leaves its outputs untouched."""
import functools
import math
import types

import numpy as np
import pytest
import scipy.linalg as sla
import torch

from oracle import cpu_ref as R
from oracle import grad_ref as GR
from oracle import philox
from tests.helpers import build_model, decode_cols_f16, decode_cols_image, normwise, to_np

pytestmark = pytest.mark.gpu

VAR = float(np.float32(0.7))
EPS = 1e-3                 # RobustMax epsilon
UNSUPPORTED = 3            # MGP_ERR_UNSUPPORTED
EDGE_D = [7, 13, 17, 31, 32]
EDGE_K = [17, 31, 32]


def _r(a):
    """float64 array of the float32-rounded values (what the device sees)."""
    return np.asarray(a, np.float32).astype(np.float64)


def _t(x, dev):
    return torch.as_tensor(np.array(x, dtype=np.float32), device=dev)   # a copy: the cached cases are read-only


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


# =========================================================================== 1. the RBF family
def rbf_inputs(D, ard, N, M, scale=1.0):
    """X [N, D], Z [M, D] ~ N(0, 1) and lengthscales ~ scale sqrt(D) (ARD: a spread around it)."""
    rng = np.random.default_rng(1000 * D + 10 * M + int(ard))
    X = _r(rng.standard_normal((N, D)))
    Z = _r(rng.standard_normal((M, D)))
    ls = _r(scale * np.sqrt(D) * (rng.uniform(0.7, 1.4, D) if ard else np.ones(1)))
    return X, Z, ls


@functools.lru_cache(maxsize=None)
def rbf_case(D, ard, N, M, scale=1.0):
    """Inputs and float64 references (shared, read-only); the non-vacuity conditions hold."""
    X, Z, ls = rbf_inputs(D, ard, N, M, scale)
    Kuf = R.rbf_K(Z, X, VAR, ls)
    Kuu = R.rbf_Kuu(Z, VAR, ls)            # + 1e-6 I
    cond = np.linalg.cond(Kuu)
    assert np.median(Kuf) >= 0.05 * VAR, np.median(Kuf)
    assert cond < 1e6, cond
    return _frozen(X, Z, ls, Kuf, Kuu) + (cond,)


@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("D", EDGE_D)
def test_rbf_kuf_kuu_edges(device, D, ard):
    """stat_tile_kernel<FamSE, 8 / 16 / 32> at ragged D: N = 1100 crosses the 1024-column tile (a second
    column block of 76, the last thread's float4 cut), M = 70 the 64-row tile."""
    from modulatedgps_amd import ops
    N, M = 1100, 70
    X, Z, ls, Kuf_ref, Kuu_ref, _ = rbf_case(D, ard, N, M)
    var, lst = _t([VAR], device), _t(ls, device)
    Kuf = to_np(ops.rbf_kuf(_t(X, device), _t(Z, device), var, lst))
    assert np.abs(Kuf - Kuf_ref).max() <= 2e-6 * VAR
    Kuu = to_np(ops.rbf_kuu(_t(Z, device), var, lst, 1e-6))
    assert np.abs(Kuu - Kuu_ref).max() <= 2e-6 * VAR
    assert np.array_equal(Kuu, Kuu.T)


@pytest.mark.parametrize("fmt", ["x6", "f16"])
@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("D", EDGE_D)
def test_kuf_image_edges(device, D, ard, fmt):
    """kuf_image_block<8 / 16 / 32> (split-bf16 and split-f16 Kuf images) against float64.
    N = 300 crosses the 256-column image tile (and the 128-column block), M = 130 the
    128-row block; the image's padding rows and columns are written as zeros."""
    from modulatedgps_amd import ops
    N, M = 300, 130
    X, Z, ls, k64, _, _ = rbf_case(D, ard, N, M)
    img = torch.full((ops.x6_cols_bytes(M, N),), 0x7F, dtype=torch.uint8, device=device)
    ops.rbf_kuf_x6(_t(X, device), _t(Z, device), _t([VAR], device), _t(ls, device), out=img, fmt=fmt)
    Mp, Np = -(-M // 128) * 128, -(-N // 256) * 256
    if fmt == "x6":
        full = decode_cols_image(img, Mp, Np)
    else:
        full = decode_cols_f16(img, Mp, Np, float(ops.image_bound(img, M, N=N).cpu()))
    # expanded form |z'|^2 + |x'|^2 - 2 z'.x' with z'_d = z_d sqrt(0.5 log2 e) / l_d: its f32
    # rounding error is a few eps32 (|z'|^2 + |x'|^2) in the exponent
    c2 = 0.5 * np.log2(np.e) / np.broadcast_to(ls, (D,)) ** 2
    norms = (Z ** 2 @ c2)[:, None] + (X ** 2 @ c2)[None, :]
    bound = 2e-6 * VAR + k64 * np.log(2.0) * 8 * 2.0 ** -24 * norms
    assert np.all(np.abs(full[:M, :N] - k64) <= bound)
    assert not full[M:].any() and not full[:, N:].any()


@pytest.mark.parametrize("fmt", ["x6", "f16"])
@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("D", [17, 32])
def test_kuf_side_job_edges(device, D, ard, fmt):
    """The Kuf side job of K3's step launches (M = 130 > 64: there are step launches to carry
    it) writes the bytes of mgp_rbf_kuf_x6 / _f16 at DMAX = 32, ragged and full."""
    from modulatedgps_amd import ops
    N, M = 300, 130
    X, Z0, ls0 = rbf_inputs(D, ard, N, M)
    _, Z1, ls1 = rbf_inputs(D, ard, N, M + 1)
    X, Zs = _t(X, device), [_t(Z0, device), _t(Z1[:M], device)]
    var, ls = [_t([0.7], device), _t([0.3], device)], [_t(ls0, device), _t(ls1, device)]
    nbytes = ops.x6_cols_bytes(M, N)
    ref = [torch.zeros(nbytes, dtype=torch.uint8, device=device) for _ in range(2)]
    got = [torch.zeros(nbytes, dtype=torch.uint8, device=device) for _ in range(2)]
    for b in range(2):
        ops.rbf_kuf_x6(X, Zs[b], var[b], ls[b], out=ref[b], fmt=fmt)
    _, LinvT0, info0 = ops.kuu_potrf_trtri(Zs, var, ls, 1e-6)
    _, LinvT1, info1 = ops.kuu_potrf_trtri(Zs, var, ls, 1e-6, kuf=(X, got, fmt))
    torch.cuda.synchronize()
    for b in range(2):
        assert torch.equal(got[b], ref[b]), b
    assert torch.equal(LinvT1, LinvT0) and torch.equal(info1, info0)


@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("D", [17, 32, 33, 40])
def test_kuu_factorisation_edges(device, D, ard):
    """The fused float64 Kuu build of K3: the staged build at D = 17, 32 and the generic one
    at D = 33, 40 (mgp_kuu_potrf_trtri takes any D), L and L^-1 against float64 LAPACK.
    M = 130: three 64-row tiles, the last of 2 rows."""
    from modulatedgps_amd import ops
    M = 130
    cases = [rbf_case(D, ard, 130, M), rbf_case(D, ard, 131, M)]     # two layers, two Z
    L, LinvT, info = ops.kuu_potrf_trtri([_t(c[1], device) for c in cases], [_t([VAR], device)] * 2,
                                         [_t(c[2], device) for c in cases], 1e-6, want_L=True)
    assert (info.cpu() == 0).all()
    for b, (_, Z, ls, _, Kuu, cond) in enumerate(cases):
        Lr = np.linalg.cholesky(Kuu)
        Li = sla.solve_triangular(Lr, np.eye(M), lower=True)
        eL, eI = normwise(to_np(L[b]), Lr), normwise(to_np(LinvT[b]).T, Li)
        print(f"D={D} cond(Kuu)={cond:.2e} L {eL:.2e} Linv {eI:.2e}")
        assert eL < 1e-6 + cond * 1e-15
        assert eI < 1e-6 + cond * 1e-15


def _rows_of(a, ld, device):
    """a [n, D] as the first D columns of rows of ld floats; the spare columns hold NaN,
    which must not enter any result."""
    if ld == a.shape[1]:
        return _t(a, device)
    buf = torch.full((a.shape[0], ld), float("nan"), dtype=torch.float32, device=device)
    buf[:, :a.shape[1]] = _t(a, device)
    return buf[:, :a.shape[1]]


# (D, ldx): both point-load paths of the DMAX = 16 and DMAX = 32 buckets
BWD_LAYOUTS = [(13, 16), (13, 13), (20, 32), (17, 17), (32, 32), (31, 31)]


@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("D,ldx", BWD_LAYOUTS)
def test_rbf_backward_edges(device, D, ldx, ard, sym):
    """stat_bwd_rows / finish<FamSE, 16>, <FamSE, 32> against float64 autograd.  D = 13 in rows of 16, D = 20
    in rows of 32 and D = 32 take the dwordx4 point loads (ldx % 4 == 0, ldx >= DMAX); ldx =
    13, 17, 31 the dword loads.  N = 1100: four full 256-point sweeps and a tail of 76 (one
    64-point step and 12 lanes); M = 70: nine 8-row workgroups, the last with 6 rows."""
    from modulatedgps_amd import ops
    N, M = 1100, 70
    X, Z, ls = rbf_inputs(D, ard, N, M)
    if sym:
        X, N = Z, M
    rng = np.random.default_rng(12 + D)
    gK = _r(rng.standard_normal((M, N)))
    if sym:
        gK = _r(0.5 * (gK + gK.T))
    gZ, gv, gl = ops.rbf_backward(_rows_of(X, ldx, device), _t(Z, device), _t([VAR], device), _t(ls, device),
                                  ops.as_padded(_t(gK, device)), symmetric=sym)
    z64 = torch.tensor(Z, requires_grad=True)
    v64 = torch.tensor(VAR, dtype=torch.float64, requires_grad=True)
    l64 = torch.tensor(ls, requires_grad=True)
    x64 = z64 if sym else torch.tensor(X)
    (GR.rbf(z64, x64, v64, l64) * torch.tensor(gK)).sum().backward()
    assert normwise(to_np(gZ), z64.grad.numpy()) < 1e-4
    assert float(gv.cpu()) == pytest.approx(float(v64.grad), rel=1e-4)
    assert normwise(gl.cpu().numpy(), l64.grad.numpy()) < 1e-4


@pytest.mark.parametrize("accumulate", [0, 1, 2])
@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("D", [17, 32])
def test_rbf_backward_batch_edges(device, D, ard, accumulate):
    """mgp_rbf_backward_batch at DMAX = 32 (D = 17: dword loads, D = 32: dwordx4) equals the
    per-call path bit for bit in its three accumulate modes (0: everything overwritten, 1:
    everything added to, 2: gZ / g_ls overwritten and g_var added to)."""
    from modulatedgps_amd import ops
    N, M, batch = 333, 70, 2
    rng = np.random.default_rng(D + 7 * accumulate)
    X, Z0, ls0 = rbf_inputs(D, ard, N, M)
    _, Z1, ls1 = rbf_inputs(D, ard, N, M + 1)
    Xd, Zs = _t(X, device), [_t(Z0, device), _t(Z1[:M], device)]
    var, ls = [_t([0.6], device), _t([0.8], device)], [_t(ls0, device), _t(ls1, device)]
    gKuf = [ops.as_padded(_t(rng.standard_normal((M, N)), device)) for _ in range(batch)]
    gKuu = []
    for _ in range(batch):
        g = rng.standard_normal((M, M))
        gKuu.append(ops.as_padded(_t(0.5 * (g + g.T), device)))
    nan = float("nan")
    init_Z = [_t(rng.standard_normal((M, D)), device) for _ in range(batch)]
    init_v = [torch.tensor([0.25 * b - 0.3], dtype=torch.float64, device=device) for b in range(batch)]
    init_l = [torch.as_tensor(rng.standard_normal(ls0.size), dtype=torch.float64, device=device) for _ in range(batch)]
    start = {0: lambda t: torch.full_like(t, nan), 1: lambda t: t.clone(), 2: lambda t: torch.full_like(t, nan)}
    ref = []
    for b in range(batch):
        if accumulate == 1:
            gZ, gv, gl = init_Z[b].clone(), init_v[b].clone(), init_l[b].clone()
        elif accumulate == 2:
            gZ, gv, gl = torch.zeros_like(init_Z[b]), init_v[b].clone(), torch.zeros_like(init_l[b])
        else:
            gZ, gv, gl = (torch.full_like(t, nan) for t in (init_Z[b], init_v[b], init_l[b]))
        ops.rbf_backward(Xd, Zs[b], var[b], ls[b], gKuf[b], accumulate=accumulate != 0, gZ=gZ, g_var=gv, g_ls=gl)
        ops.rbf_backward(Zs[b], Zs[b], var[b], ls[b], gKuu[b], symmetric=True, accumulate=True, gZ=gZ, g_var=gv,
                         g_ls=gl)
        ref.append((gZ, gv, gl))
    gZs, gls = [start[accumulate](t) for t in init_Z], [start[accumulate](t) for t in init_l]
    gvs = [torch.full_like(t, nan) if accumulate == 0 else t.clone() for t in init_v]
    ops.rbf_backward_batch(Xd, Zs, var, ls, gKuf, gKuu, gZs, gvs, gls, accumulate=accumulate)
    torch.cuda.synchronize()
    for b in range(batch):
        assert torch.isfinite(ref[b][0]).all() and torch.isfinite(ref[b][2]).all()
        assert torch.equal(gZs[b], ref[b][0]), b
        assert torch.equal(gvs[b], ref[b][1]), b
        assert torch.equal(gls[b], ref[b][2]), b


@pytest.mark.parametrize("D,K", [(17, 2), (32, 3), (2, 17), (3, 32)])
def test_full_cov_edges(device, D, K):
    """mgp_full_cov_conditional at D > 8 (the X tiles' LDS pitch comes from the D limit) and at
    K > 3 (the expert cut of the output tiles), N = 130 (three 64-point tiles, the last of
    2), M = 40: per expert against float64, bitwise symmetric, the diagonal equal to the
    marginal variance; nothing written beside the output.  A = L^-1 Kuf is an input here
    (float64 on the host), so cond(Kuu) does not enter; Kuf is not vanishing."""
    from modulatedgps_amd import ops
    N, M = 130, 40
    X, Z, ls = rbf_inputs(D, True, N, M, scale=1.0 if D > 8 else 0.6)
    Kuf, Kuu = R.rbf_K(Z, X, VAR, ls), R.rbf_Kuu(Z, VAR, ls)
    assert np.median(Kuf) >= 0.05 * VAR
    rng = np.random.default_rng(100 * D + K)
    q_sqrt = _r(0.5 * np.eye(M)[None] + np.tril(0.1 * rng.standard_normal((K, M, M))))
    A64 = sla.solve_triangular(np.linalg.cholesky(Kuu), Kuf, lower=True)
    base = R.rbf_K(X, X, VAR, ls) - A64.T @ A64
    cov_ref = np.stack([base + (Lk.T @ A64).T @ (Lk.T @ A64) for Lk in np.tril(q_sqrt)])
    _, var_ref = R.svgp_predict_f_dedup(X, Z, VAR, ls, np.zeros((M, K)), q_sqrt)
    ld = (N + 3) // 4 * 4
    sentinel = -12345.0
    buf = torch.full((K, N, ld), sentinel, dtype=torch.float32, device=device)
    cov = ops.full_cov_conditional(_t(X, device), ops.as_padded(_t(A64, device)), ops.as_padded(_t(q_sqrt, device)),
                                   _t([VAR], device), _t(ls, device), out=buf[..., :N])
    assert torch.equal(cov, cov.transpose(-1, -2))
    c = to_np(cov)
    for k in range(K):
        assert normwise(c[k], cov_ref[k]) < 1e-4, k
        assert normwise(np.diag(c[k]), var_ref[:, k]) < 1e-4, k
    assert bool((buf[..., N:] == sentinel).all())


# =========================================================================== 2. K6 and the epilogues
LIKS = ["gauss", "modified", "multiclass", "multiclass_modified"]


@functools.lru_cache(maxsize=None)
def k6_case(N, K, S):
    """Random conditionals [N, K], targets, class labels covering 0 and K - 1, likelihood
    variances and explicit noise -- float64 arrays of float32 values, read-only."""
    rng = np.random.default_rng(100 * K + S)
    c = types.SimpleNamespace(N=N, K=K, S=S)
    c.mu_f, c.mu_a = _r(0.5 * rng.standard_normal((N, K))), _r(rng.standard_normal((N, K)))
    c.var_f, c.var_a = _r(rng.uniform(0.3, 1.2, (N, K))), _r(rng.uniform(0.05, 1.0, (N, K)))
    c.Y = _r(rng.standard_normal(N))
    c.Yc = rng.integers(0, K, N).astype(np.float64)
    c.Yc[0], c.Yc[1] = 0.0, K - 1.0
    c.lv, c.av = _r(rng.uniform(0.2, 1.0, K)), _r(np.linspace(0.3, 0.9, K))
    z, u = R.explicit_noise(S, N, K, seed=3)
    c.z, c.u = _r(z), _r(u)
    # the MultiClass cases are informative: most points sit away from p_y = 0 and 1
    p_y = R.robustmax_prob_is_largest(c.Yc, c.mu_f, c.var_f, K).reshape(-1)
    assert 0.0 in c.Yc and K - 1.0 in c.Yc
    assert np.mean((p_y > 1e-3) & (p_y < 1 - 1e-3)) >= 0.5
    _frozen(*vars(c).values())
    return c


def k6_data_ref(c, z, u, lik):
    """sum_n of SMGP.E_log_p_Y (SMGPModified: plus the assignment term) in float64."""
    mc, mod = lik.startswith("multiclass"), lik.endswith("modified")
    Y = (c.Yc if mc else c.Y).reshape(-1, 1)
    p = R.SMGPParams(None, None, c.lv, c.N, c.S, multiclass_eps=EPS if mc else None)
    W = R.assignment_weights(c.mu_a[None], c.var_a[None], z, u)
    val = R.e_log_p_y(c.mu_f[None], c.var_f[None], Y, p.lik_variance, W, c.S, p=p)
    if mod:
        ve_a = R.gaussian_var_exp(c.mu_a[None], c.var_a[None], Y[None], c.av[None])
        val = val + R._logsumexp0(np.sum(ve_a * W, 2)) - np.log(c.S)
    return float(np.sum(val))


def k6_device_args(c, lik, device):
    """(mu_f, var_f, mu_a, var_a, Y, lik_var, S) and the keyword arguments of ops.elbo_terms."""
    from modulatedgps_amd import ops
    mc, mod = lik.startswith("multiclass"), lik.endswith("modified")
    conds = [ops.as_padded(_t(a.T, device)) for a in (c.mu_f, c.var_f, c.mu_a, c.var_a)]
    args = (*conds, _t(c.Yc if mc else c.Y, device), None if mc else _t(c.lv, device), c.S)
    kw = {}
    if mc:
        kw["multiclass_eps"] = EPS
    if mod:
        kw["assign_lik_var"] = _t(c.av, device)
    return args, kw


# every likelihood at K = 17, 31, 32; MultiClass also at K = 9, 16 (its KMAX = 16 bucket)
FWD_CASES = [(K, lik) for K in EDGE_K for lik in LIKS] + [(K, lik) for K in (9, 16) for lik in LIKS[2:]]


@pytest.mark.parametrize("S", [3, 5])
@pytest.mark.parametrize("K,lik", FWD_CASES)
def test_elbo_terms_edges(device, K, S, lik):
    """K6 forward (plain, modified, MultiClass) at KMAX = 32, ragged and full, with explicit
    noise and with Philox ((K + 3) / 4 counter blocks: K = 17 uses one word of its fifth).
    MultiClass also at K = 9, 16 (KMAX = 16).  N = 257: two 64-point workgroups at four
    lanes per point (one 256-point workgroup for MultiClass) and one point more."""
    from modulatedgps_amd import ops
    c = k6_case(257, K, S)
    args, kw = k6_device_args(c, lik, device)
    out = float(ops.elbo_terms(*args, noise=(_t(c.z, device), _t(c.u, device)), **kw).cpu())
    assert out == pytest.approx(k6_data_ref(c, c.z, c.u, lik), rel=1e-4, abs=1e-3)
    seed, n = 99 + K, np.arange(c.N)
    out2 = float(ops.elbo_terms(*args, seed=seed, **kw).cpu())
    ref2 = k6_data_ref(c, philox.noise_normal(seed, S, n, K), philox.noise_uniform(seed, S, n, K), lik)
    assert out2 == pytest.approx(ref2, rel=1e-4, abs=1e-3)


def test_philox_stream_k17(device):
    """The noise streams at K = 17: five counter blocks per (s, n), the fifth used for one
    word.  Uniforms bit-exact with oracle/philox.py, normals (both streams) within 2e-5."""
    from modulatedgps_amd import ops
    seed, S, N, K, off = 0x1234ABCD9876, 3, 257, 17, 500
    z, u = ops.philox_noise(seed, off, N, K, S, device)
    n = np.arange(off, off + N)
    assert np.array_equal(to_np(u), philox.noise_uniform(seed, S, n, K).astype(np.float32).astype(np.float64))
    assert np.abs(to_np(z) - philox.noise_normal(seed, S, n, K)).max() < 2e-5
    z2 = ops.philox_normal2(seed, off, N, K, S, device)
    assert np.abs(to_np(z2) - philox.noise_normal(seed, S, n, K, stream=2)).max() < 2e-5


def _data_term_grads_f32(c, lik):
    """float32 autograd (CPU) of the same data term: the float32 floor of its gradients."""
    mc, mod = lik.startswith("multiclass"), lik.endswith("modified")
    f = lambda a: torch.tensor(np.array(a), dtype=torch.float32)
    leaves = [f(a).requires_grad_(True) for a in (c.mu_f, c.var_f, c.mu_a, c.var_a)]
    dt = GR.data_term(*leaves, f(c.Yc if mc else c.Y), None if mc else f(c.lv), f(c.z), f(c.u),
                      assign_lik_var=f(c.av) if mod else None, multiclass_eps=EPS if mc else None)
    (dt / c.N).backward()
    return [t.grad.double().numpy() for t in leaves]


@pytest.mark.parametrize("lik", LIKS)
@pytest.mark.parametrize("K", EDGE_K)
def test_elbo_terms_backward_edges(device, K, lik):
    """K6 backward of the three likelihoods at KMAX = 32 against float64 autograd of the data
    term at the same float32 inputs: all four planes of G, and every one of the K entries
    of the likelihood-variance gradients (partial sums strided by 2 KMAX).  N = 257: one
    256-point workgroup and one point more.

    MultiClass without the assignment likelihood: the assignment gradients vanish in exact
    arithmetic (ve (1 - sum_k W_k) / tau), and what float32 leaves of them grows with K and
    with |log(eps / (K - 1))|.  Measured |g_mu_a| / |g_var_a| of the kernel, of float32
    autograd of the same formula on the CPU, and the sibling test's absolute bound
    1e-5 |g_mu_f| (float64 autograd: 1.7e-15):
      K = 17   6.44e-7 / 7.07e-7   5.97e-7 / 4.52e-7   8.47e-7
      K = 31   7.48e-7 / 7.68e-7   7.48e-7 / 6.97e-7   6.36e-7
      K = 32   6.99e-7 / 6.55e-7   6.59e-7 / 6.88e-7   6.27e-7
    At K = 31, 32 the sibling's bound is below float32's own floor, so the bound is the larger
    of the sibling's and 1.5 x the float32 evaluation."""
    from modulatedgps_amd import ops
    c = k6_case(257, K, 3)
    mc, mod = lik.startswith("multiclass"), lik.endswith("modified")
    leaves = [torch.tensor(np.array(a), requires_grad=True) for a in (c.mu_f, c.var_f, c.mu_a, c.var_a)]
    lv = None if mc else torch.tensor(np.array(c.lv), requires_grad=True)
    av = torch.tensor(np.array(c.av), requires_grad=True) if mod else None
    dt = GR.data_term(*leaves, torch.tensor(np.array(c.Yc if mc else c.Y)), lv, torch.tensor(np.array(c.z)),
                      torch.tensor(np.array(c.u)), assign_lik_var=av, multiclass_eps=EPS if mc else None)
    (dt / c.N).backward()
    args, kw = k6_device_args(c, lik, device)
    G, glv, glva = ops.elbo_terms_backward(*args, noise=(_t(c.z, device), _t(c.u, device)), scale=1.0 / c.N, **kw)
    scale_ref = np.linalg.norm(leaves[0].grad.numpy())
    for i, name in enumerate(("mu_f", "var_f", "mu_a", "var_a")):
        got, ref = to_np(G[i])[:, :c.N].T, leaves[i].grad.numpy()
        if np.linalg.norm(ref) < 1e-12 * scale_ref:
            # SMGP with MultiClass: sum_k W_sk = 1, the data term does not depend on the
            # assignment layer and both gradients are roundoff (test_gpu_multiclass.py)
            assert mc and not mod, name
            noise32 = np.linalg.norm(_data_term_grads_f32(c, lik)[i])
            print(f"K={K} {name}: |g| {np.linalg.norm(got):.3e}, float32 autograd {noise32:.3e}, "
                  f"1e-5 scale {1e-5 * scale_ref:.3e}")
            assert np.linalg.norm(got) < max(1e-5 * scale_ref, 1.5 * noise32), name
        else:
            assert normwise(got, ref) < 1e-4, name
    for got, leaf, name in ((glv, lv, "g_lik_var"), (glva, av, "g_assign_lik_var")):
        if leaf is None:
            assert got is None, name
            continue
        got, ref = got.cpu().numpy(), leaf.grad.numpy()
        assert got.shape == (K,) and np.all(ref != 0.0)
        assert normwise(got, ref) < 1e-4, name
        assert np.all(np.abs(got - ref) <= 1e-4 * np.abs(ref).max()), name   # entry by entry


@pytest.mark.parametrize("K", EDGE_K)
def test_predictive_epilogues_edges(device, K):
    """predict_samples (explicit noise), predict_epilogue and multiclass_predict at KMAX = 32
    against the oracle functions of the same names (1e-4 normwise, as the model-level
    prediction tests); N = 257 is one 256-thread workgroup and one point more."""
    from modulatedgps_amd import ops
    N, S = 257, 3
    c = k6_case(N, K, S)
    conds = [ops.as_padded(_t(a.T, device)) for a in (c.mu_f, c.var_f, c.mu_a, c.var_a)]
    lv = _t(c.lv, device)
    rng = np.random.default_rng(9 + K)
    zy = _r(rng.standard_normal((S, N, K)))
    W = R.assignment_weights(c.mu_a[None], c.var_a[None], c.z, c.u)
    mean, var = R.gaussian_predict_mean_and_var(c.mu_f, c.var_f, c.lv[None])
    sy_ref = np.sum(R.reparameterize(mean[None], var[None], zy) * W, 2)
    sf_ref = np.sum(R.reparameterize(c.mu_f[None], c.var_f[None], zy) * W, 2)
    sy, sf = ops.predict_samples(*conds, lv, S, noise=[_t(a, device) for a in (c.z, c.u, zy)])
    assert normwise(to_np(sy), sy_ref) < 1e-4
    assert normwise(to_np(sf), sf_ref) < 1e-4
    ym, yv, asg = ops.predict_epilogue(conds[0], conds[1], conds[2], lv, want_y=True, want_assign=True)
    e = np.exp(c.mu_a - c.mu_a.max(-1, keepdims=True))
    assert normwise(to_np(ym), mean) < 1e-4 and normwise(to_np(yv), var) < 1e-4
    assert normwise(to_np(asg), e / e.sum(-1, keepdims=True)) < 1e-4
    pm, pv = ops.multiclass_predict(conds[0], conds[1], EPS)
    pm_ref, pv_ref = R.multiclass_predict_mean_and_var(c.mu_f, c.var_f, K, EPS)
    assert normwise(to_np(pm), pm_ref) < 1e-4 and normwise(to_np(pv), pv_ref) < 1e-4


@pytest.mark.parametrize("lik", ["gauss", "modified"])
@pytest.mark.parametrize("K", EDGE_K)
def test_methods_compose_edges(device, K, lik):
    """assign_logits -> relaxed_onehot_sample -> e_log_p_y with one Philox key draw K6's own
    noise streams: their composition equals elbo_terms with that key (per point, the
    tolerance of test_methods_compose_to_build_likelihood), and the sampled weights are the
    oracle's relaxed one-hot sample of the device's logits."""
    from modulatedgps_amd import ops
    N, S, seed = 257, 3, 1234567 + K
    c = k6_case(N, K, S)
    args, kw = k6_device_args(c, lik, device)
    mu_f, var_f, mu_a, var_a, Yd, lvd, _ = args
    logits = ops.assign_logits(mu_a, var_a, S, N, seed=seed)
    W = ops.relaxed_onehot_sample(logits, S, N, seed=seed)
    n = np.arange(N)
    W_ref = R.relaxed_onehot_sample(to_np(logits), philox.noise_uniform(seed, S, n, K))
    assert normwise(to_np(W).reshape(S, N, K), W_ref) < 1e-4
    per = ops.e_log_p_y(mu_f, var_f, Yd, lvd, W, S, N, mu_a=mu_a, var_a=var_a, assign_lik_var=kw.get("assign_lik_var"))
    fused = float(ops.elbo_terms(*args, seed=seed, **kw).cpu()) / N
    assert float(per.double().mean().cpu()) == pytest.approx(fused, rel=2e-6, abs=1e-6)


# =========================================================================== 3. K5 and the front above K = 16
@functools.lru_cache(maxsize=None)
def cond_case(N, M, K, D):
    """One layer's state, float64 A = L^-1 Kuf and the K4 column statistics computed on the
    host (K4 itself stops at K = 16), and the float64 conditional."""
    ls = float(np.float32(round(0.9 * math.sqrt(D), 2)))
    X, _, p = R.synthetic_problem(N, M, K, D, ls, state="perturbed", S=2)
    L = p.pred
    c = types.SimpleNamespace(N=N, M=M, K=K, D=D, ls=ls, var=float(np.float32(L["variance"])))
    c.X, c.Z, c.q_mu, c.q_sqrt = _r(X), _r(L["Z"]), _r(L["q_mu"]), _r(L["q_sqrt"])
    Kuu = R.rbf_Kuu(c.Z, c.var, ls)
    assert np.linalg.cond(Kuu) < 1e6      # the 1e-4 branch of test_conditional_split_bf16's tolerance
    c.A = _r(sla.solve_triangular(np.linalg.cholesky(Kuu), R.rbf_K(c.Z, c.X, c.var, ls), lower=True))
    c.mu_ref, c.var_ref = R.svgp_predict_f_dedup(c.X, c.Z, c.var, ls, c.q_mu, c.q_sqrt)
    T = -(-M // 64)
    c.stats = np.zeros((T, K + 1, N))
    for t in range(T):
        rows = slice(64 * t, min(64 * t + 64, M))
        c.stats[t, 0] = np.sum(c.A[rows] ** 2, axis=0)
        c.stats[t, 1:] = c.q_mu[rows].T @ c.A[rows]
    _frozen(*vars(c).values())
    return c


# N = 301: one 256-column image tile and 45 columns; M = 70 / 130: past the 64-row stats
# tile / past the 128-row image block (three stats tiles, the last of 2 rows)
COND_SHAPES = [(301, 70, 17, 5), (301, 130, 32, 8)]


@pytest.mark.parametrize("N,M,K,D", COND_SHAPES)
def test_expert_conditional_edges(device, N, M, K, D):
    """K5 above K4's limit: the f32 kernel and the split-bf16 / split-f16 image kernels at
    K = 17, 32 on host-computed column statistics, against the float64 conditional with
    test_conditional_split_bf16's tolerances."""
    from modulatedgps_amd import ops
    c = cond_case(N, M, K, D)
    assert ops.stats_tiles(M) == c.stats.shape[0]
    A, qs, var = ops.as_padded(_t(c.A, device)), ops.as_padded(_t(c.q_sqrt, device)), _t([c.var], device)
    stats = ops.padded(c.stats.shape[0] * (K + 1), N, device).unflatten(0, (-1, K + 1))
    stats.copy_(_t(c.stats, device))
    fm32, fv32 = ops.expert_conditional(A, qs, stats, var)
    assert normwise(to_np(fm32).T, c.mu_ref) < 1e-4
    assert normwise(to_np(fv32).T, c.var_ref) < 1e-4
    fm, fv = ops.expert_conditional_x6(ops.split_cols_x6(A), ops.split_lower_x6(qs), stats, var, M, N, K)
    assert torch.equal(fm[:, :N], fm32[:, :N])
    assert normwise(to_np(fv).T, to_np(fv32).T) < 2e-6
    assert normwise(to_np(fm).T, c.mu_ref) < 1e-4
    assert normwise(to_np(fv).T, c.var_ref) < 1e-4
    fm, fv = ops.expert_conditional_x6(ops.split_cols_x6(A, fmt="f16"), ops.split_lower_x6(qs, fmt="f16"), stats, var,
                                       M, N, K, fmt="f16", cross="f16")
    assert normwise(to_np(fm).T, c.mu_ref) < 1e-4
    assert normwise(to_np(fv).T, c.var_ref) < 1e-4


def _front_expert_conditional(c, device, fmean, fvar):
    """mgp_expert_conditional (the §8(b) front's K5: images, col_stats_kernel, split-f16 K5)."""
    from modulatedgps_amd import _lib, ops
    lib = _lib.load()
    A, qm = ops.as_padded(_t(c.A, device)), _t(c.q_mu, device)
    qs, var = ops.as_padded(_t(c.q_sqrt, device)), _t([c.var], device)
    ws = torch.empty(max(lib.mgp_workspace_bytes(5, c.M, c.N, c.K), 16), dtype=torch.uint8, device=device)
    return lib.mgp_expert_conditional(A.data_ptr(), A.stride(0), qm.data_ptr(), qm.stride(0), qs.data_ptr(),
                                      qs.stride(1), qs.stride(0), var.data_ptr(), c.M, c.N, c.K, fmean.data_ptr(),
                                      fvar.data_ptr(), fmean.stride(0), ws.data_ptr(), ws.numel(),
                                      torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("N,M,K,D", COND_SHAPES)
def test_front_expert_conditional_edges(device, N, M, K, D):
    """The front's mgp_expert_conditional at K = 17, 32 (col_stats_kernel<32>, ragged and full)
    against the float64 conditional, 1e-4 normwise."""
    from modulatedgps_amd import ops
    c = cond_case(N, M, K, D)
    fmean, fvar = ops.padded(K, N, device), ops.padded(K, N, device)
    assert _front_expert_conditional(c, device, fmean, fvar) == 0
    assert normwise(to_np(fmean).T, c.mu_ref) < 1e-4
    assert normwise(to_np(fvar).T, c.var_ref) < 1e-4


# =========================================================================== 4. the limits
def _refused(call, outputs):
    """`call` raises MGPError(MGP_ERR_UNSUPPORTED) and writes none of the sentinel-filled
    `outputs` (tensors, each filled with one value of its dtype)."""
    from modulatedgps_amd import _lib
    before = [t.clone() for t in outputs]
    with pytest.raises(_lib.MGPError) as e:
        call()
    assert e.value.status == UNSUPPORTED, e.value
    torch.cuda.synchronize()
    for t, b in zip(outputs, before):
        assert torch.equal(t, b)


def _sent(shape, device, dtype=torch.float32, value=-12345.0):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), value, dtype=dtype, device=device)


def test_refuses_d33(device):
    """D = 33 is one past the RBF entries' limit: MGP_ERR_UNSUPPORTED, outputs untouched."""
    from modulatedgps_amd import ops
    N, M, D, K = 130, 40, 33, 2
    X, Z, ls = rbf_inputs(D, True, N, M)
    X, Z, var, ls = _t(X, device), _t(Z, device), _t([VAR], device), _t(ls, device)
    out = _sent((M, 132), device)
    _refused(lambda: ops.rbf_kuf(X, Z, var, ls, out=out[:, :N]), [out])
    out = _sent((M, M), device)
    _refused(lambda: ops.rbf_kuu(Z, var, ls, 1e-6, out=out), [out])
    for fmt in ("x6", "f16"):
        img = _sent(ops.x6_cols_bytes(M, N), device, torch.uint8, 0x5A)
        _refused(lambda: ops.rbf_kuf_x6(X, Z, var, ls, out=img, fmt=fmt), [img])
        LinvT, info = _sent((1, M, M), device), _sent(1, device, torch.int32, 77)
        _refused(lambda: ops.kuu_potrf_trtri([Z], [var], [ls], 1e-6, LinvT=LinvT, info=info, kuf=(X, [img], fmt)),
                 [img, LinvT, info])
    gK, gKuu = ops.as_padded(torch.ones(M, N, device=device)), ops.as_padded(torch.ones(M, M, device=device))
    gZ, gv, gl = _sent((M, D), device), _sent(1, device, torch.float64), _sent(D, device, torch.float64)
    _refused(lambda: ops.rbf_backward(X, Z, var, ls, gK, gZ=gZ, g_var=gv, g_ls=gl), [gZ, gv, gl])
    _refused(lambda: ops.rbf_backward_batch(X, [Z], [var], [ls], [gK], [gKuu], [gZ], [gv], [gl]), [gZ, gv, gl])
    A, qs = ops.as_padded(torch.zeros(M, N, device=device)), ops.as_padded(torch.zeros(K, M, M, device=device))
    cov = _sent((K, N, 132), device)
    _refused(lambda: ops.full_cov_conditional(X, A, qs, var, ls, out=cov[..., :N]), [cov])


def test_refuses_k33(device):
    """K = 33 is one past the limit of K6, the method-level entries, the predictive epilogues,
    the full covariance and the front's mgp_expert_conditional."""
    from modulatedgps_amd import _lib, ops
    N, K, S, M = 130, 33, 2, 40
    rng = np.random.default_rng(33)
    conds = [ops.as_padded(_t(a, device)) for a in (rng.standard_normal((K, N)), rng.uniform(0.1, 1.0, (K, N)),
                                                    rng.standard_normal((K, N)), rng.uniform(0.1, 1.0, (K, N)))]
    Y, Yc = _t(rng.standard_normal(N), device), _t(rng.integers(0, K, N), device)
    lv, av = _t(rng.uniform(0.2, 1.0, K), device), _t(np.linspace(0.3, 0.9, K), device)
    for kw in ({}, {"assign_lik_var": av}, {"multiclass_eps": EPS}):
        mc = "multiclass_eps" in kw
        out = _sent(1, device, torch.float64)
        _refused(lambda: ops.elbo_terms(*conds, Yc if mc else Y, None if mc else lv, S, seed=1, out=out, **kw), [out])
        G = ops.padded(4 * K, N, device).unflatten(0, (4, K))
        G.fill_(-12345.0)
        _refused(lambda: ops.elbo_terms_backward(*conds, Yc if mc else Y, None if mc else lv, S, seed=1, G=G, **kw), [G])
    # the entries below allocate their outputs: the refusal alone
    logits, W = torch.zeros(S * N, K, device=device), torch.full((S * N, K), 1.0 / K, device=device)
    _refused(lambda: ops.relaxed_onehot_sample(logits, S, N, seed=1), [])
    _refused(lambda: ops.e_log_p_y(conds[0], conds[1], Y, lv, W, S, N), [])
    _refused(lambda: ops.e_log_p_y(conds[0], conds[1], Yc, None, W, S, N, multiclass_eps=EPS), [])
    _refused(lambda: ops.predict_samples(*conds, lv, S, seed=1), [])
    _refused(lambda: ops.predict_samples(*conds, None, S, seed=1, multiclass_eps=EPS), [])
    _refused(lambda: ops.multiclass_predict(conds[0], conds[1], EPS), [])
    X, var, ls = _t(rng.standard_normal((N, 2)), device), _t([VAR], device), _t([1.0], device)
    A, qs = ops.as_padded(torch.zeros(M, N, device=device)), ops.as_padded(torch.zeros(K, M, M, device=device))
    cov = _sent((K, N, 132), device)
    _refused(lambda: ops.full_cov_conditional(X, A, qs, var, ls, out=cov[..., :N]), [cov])
    c = types.SimpleNamespace(N=N, M=M, K=K, A=np.zeros((M, N)), q_mu=np.zeros((M, K)), q_sqrt=np.zeros((K, M, M)),
                              var=VAR)
    fmean, fvar = _sent((K, 132), device), _sent((K, 132), device)

    def front():
        _lib.check("mgp_expert_conditional", _front_expert_conditional(c, device, fmean, fvar))
    _refused(front, [fmean, fvar])


def test_refuses_k17_in_k4_and_conditional_backward(device):
    """K = 17 is one past the limit of K4 (mgp_trsm_stats*) and of the conditional backward."""
    from modulatedgps_amd import ops
    N, M, K = 130, 40, 17
    z = lambda *s: torch.zeros(*s, device=device)
    LinvT, Kuf, q_mu, var = ops.as_padded(z(M, M)), ops.as_padded(z(M, N)), ops.as_padded(z(M, K)), _t([VAR], device)
    T = ops.stats_tiles(M)
    new_stats = lambda: _sent((T, K + 1, 132), device)
    A, st = _sent((M, 132), device), new_stats()
    _refused(lambda: ops.trsm_stats(LinvT, Kuf, q_mu, A=A[:, :N], stats=st[..., :N]), [A, st])
    cb, lb = ops.x6_cols_bytes(M, N), ops.x6_lower_bytes(M, 1)
    Tfr, Kfr = torch.zeros(lb, dtype=torch.uint8, device=device), torch.zeros(cb, dtype=torch.uint8, device=device)
    for kw in ({}, {"f16_variance": var}, {"f16_variance": var, "in_fmt": "f16", "cross": "f16"},
               {"f16_variance": var, "in_fmt": "f16", "cross": "f8"}):
        Afr, st = _sent(cb, device, torch.uint8, 0x5A), new_stats()
        _refused(lambda: ops.trsm_stats_x6(Tfr, Kfr, q_mu, M, N, Afr=Afr, stats=st[..., :N], **kw), [Afr, st])
    Afr, st = _sent(cb, device, torch.uint8, 0x5A), new_stats()
    _refused(lambda: ops.trsm_stats_f16_batch([Tfr], [Kfr], [q_mu], M, N, [Afr], [st[..., :N]], [var]), [Afr, st])
    qs, Gmu, Gv = ops.as_padded(z(K, M, M)), ops.as_padded(z(K, N)), ops.as_padded(z(K, N))
    Acols = ops.as_padded(z(M, N))

    def outs():
        return {"g_q_mu": _sent((M, 20), device)[:, :K], "g_q_sqrt": _sent((K, M, M), device),
                "g_Kuf": _sent((M, 132), device)[:, :N], "g_Lm": _sent((M, M), device),
                "g_var": _sent(1, device, torch.float64)}
    for fmt, cross in (("x6", None), ("f16", "f16"), ("f16", "f8")):
        o = outs()
        _refused(lambda: ops.conditional_backward_x6(Kfr, Acols, qs, q_mu, LinvT, Gmu, Gv, M, N, out=o, fmt=fmt,
                                                     cross=cross), list(o.values()))
    one = torch.ones(1, device=device)
    Cfr = torch.zeros(max(int(ops.c_images_bytes(M, N, K)), 16), dtype=torch.uint8, device=device)
    o = outs()
    _refused(lambda: ops.conditional_backward_x6(Kfr, Acols, qs, q_mu, LinvT, Gmu, Gv, M, N, out=o, fmt="f16",
                                                 cross="f16", c_images=(Cfr, one, one)), list(o.values()))
    _refused(lambda: ops.conditional_backward_prep(qs, one), [])


@pytest.mark.parametrize("fmt", ["f16", "x6"])
def test_model_refuses_k17(device, fmt):
    """The Python model with 17 experts: the conditional path needs K4, so _build_likelihood,
    conditionals and predict_y raise an error that names the K <= 16 limit, in both image
    formats, and return nothing."""
    from modulatedgps_amd import config
    N, M, K, D = 130, 40, 17, 2
    X, Y, p = R.synthetic_problem(N, M, K, D, 1.0, state="perturbed", S=2)
    old = config.expert_format()
    config.set_expert_format(fmt)
    try:
        model = build_model(p, device)
        Xd = _t(X, device)
        for call in (lambda: model._build_likelihood(Xd, Y, seed=3), lambda: model.conditionals(Xd),
                     lambda: model.predict_y(Xd), lambda: model.elbo_and_grad(Xd, Y, seed=3)):
            with pytest.raises(ValueError, match=r"K = 17.*K <= 16"):
                call()
    finally:
        config.set_expert_format(old)


@pytest.mark.parametrize("fmt", ["f16", "x6"])
@pytest.mark.parametrize("N,M,K,D", [(301, 40, 3, 32), (301, 40, 3, 17)])
def test_model_at_d32(device, N, M, K, D, fmt):
    """The model end to end at the top of the D range (lengthscale ~ sqrt(D)): the ELBO and the
    conditionals against the float64 oracle, the training gradient against float64 autograd
    with test_elbo_and_grad's bound (FLOOR, 1.5 x float32 autograd)."""
    from modulatedgps_amd import config
    from tests.test_gpu_training import _check_elbo_and_grad
    ls, S = round(0.9 * math.sqrt(D), 2), 3
    X, Y, p = R.synthetic_problem(N, M, K, D, ls, state="perturbed", S=S)
    z, u = R.explicit_noise(S, N, K, seed=5)
    for L in (p.pred, p.assign):
        assert np.median(R.rbf_K(L["Z"], X, L["variance"], ls)) >= 0.05 * L["variance"]
        assert np.linalg.cond(R.rbf_Kuu(L["Z"], L["variance"], ls)) < 1e6
    ref, parts = R.smgp_elbo(X, Y, p, z, u, return_parts=True)
    old, old_cross = config.expert_format(), config.expert_cross()
    config.set_expert_format(fmt)
    config.set_expert_cross("f16")
    try:
        model = build_model(p, device)
        Xd = _t(X, device)
        conds = [c.clone() for c in model.conditionals(Xd)]
        for got, name in zip(conds, ("mu_f", "var_f", "mu_a", "var_a")):
            assert normwise(to_np(got)[:, :N].T, parts[name]) < 1e-4, name
        e = float(model._build_likelihood(Xd, Y, noise=(_t(z, device), _t(u, device))).cpu())
        assert e == pytest.approx(ref, rel=1e-4)
        _check_elbo_and_grad(device, N, M, K, D, ls, S, False, factor=1.5)
    finally:
        config.set_expert_format(old)
        config.set_expert_cross(old_cross)

