"""Translation invariance of the RBF kernels: K(Z + c, X + c) = K(Z, X).

1. Bit identity on grid-exact cases (tests/translation_ref.py: coordinates on a 2^-10 grid in
   [-4, 4], per-axis offsets on that grid up to 4096): every shifted coordinate and every
   difference of two of them is exact in float32, so a kernel that differences the raw
   coordinates before any scaling, squaring or product returns the same bits for (X, Z) and
   (X + c, Z + c).  No tolerance.  N = 301 (no multiple of 32), M = 130 (two 128-row blocks,
   the second ragged), D in {1, 3, 8, 32} (the DMAX 1, 4, 8, 32 instantiations), ARD on / off;
   offsets: zero (the control: two calls agree), +1024 on every axis, and a mixed one.
2. Accuracy on shifted inputs that are on no grid (standard normal + 1000; a calendar axis
   in [2000, 2020] at lengthscale 1) against float64 of the float32 inputs, with the bounds
   the suite already uses: 2e-6 variance elementwise for mgp_rbf_kuf / mgp_rbf_kuu
   (test_rbf_kuf_kuu); for the decoded images the bound of test_kuf_and_trsm_images with its
   norms term about the point the kernel subtracts (translation_ref.image_bound) and, split-f16,
   normwise < 5e-7 and max < 2e-6 max|ref| (test_kuf_f16_image_any_variance); every decoded
   entry finite and <= variance (1 + 2^-20).
3. The model on a snapped synthetic problem moved by the mixed offset: ELBO (rel 1e-4),
   predict_y (normwise 1e-4) and elbo_and_grad (test_gpu_training's criterion) against the
   oracle on the UNSHIFTED problem, and the shifted ELBO bit-equal to the unshifted one.

Which of these the load-time reference subtraction fixed (they fail on the commit before it:
coordinates scaled first, the image's expanded form on raw scaled coordinates) and which pin
behaviour that was already right is listed per test."""
import functools

import numpy as np
import pytest
import scipy.linalg as sla
import torch

from oracle import cpu_ref as R
from tests import translation_ref as T
from tests.helpers import build_model, decode_cols_f16, decode_cols_image, dev_noise, normwise, to_np

pytestmark = pytest.mark.gpu

N, M = 301, 130
CASES = [(1, False), (1, True), (3, False), (3, True), (8, False), (8, True), (32, False), (32, True)]
CASE_IDS = [f"D{D}-{'ard' if ard else 'iso'}" for D, ard in CASES]
SHIFTS = ("zero", "plus1024", "mixed")
JITTER = 1e-6


def _t(x, device, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x), dtype=dtype, device=device)


@functools.lru_cache(maxsize=None)
def _host_case(D, ard):
    return T.grid_case(N, M, D, ard)


def _shifted(D, ard, kind, device):
    """Device X, Z of the case moved by the offset `kind`, and the offset."""
    X, Z, _, _ = _host_case(D, ard)
    c = T.offset_vector(kind, D)
    return _t(T.shift(X, c), device), _t(T.shift(Z, c), device), c


def _hyper(D, ard, device):
    _, _, var, ls = _host_case(D, ard)
    return _t([var], device), _t(ls, device)


def _image(X, Z, var, ls, fmt):
    from modulatedgps_amd import ops
    # zero-filled: plane 2 of a split-f16 image is never written
    img = torch.zeros(ops.x6_cols_bytes(Z.shape[0], X.shape[0]), dtype=torch.uint8, device=X.device)
    return ops.rbf_kuf_x6(X, Z, var, ls, out=img, fmt=fmt)


# ---------------------------------------------------------------------- 1. bit identity
@pytest.mark.parametrize("fmt", ["x6", "f16"])
@pytest.mark.parametrize("D,ard", CASES, ids=CASE_IDS)
def test_kuf_image_bits(device, D, ard, fmt):
    """mgp_rbf_kuf_x6 / mgp_rbf_kuf_f16 (fixed: failed before the reference subtraction)."""
    from modulatedgps_amd import ops
    var, ls = _hyper(D, ard, device)
    X0, Z0, _ = _shifted(D, ard, "zero", device)
    img0 = _image(X0, Z0, var, ls, fmt)
    for kind in SHIFTS:
        Xs, Zs, _ = _shifted(D, ard, kind, device)
        img = _image(Xs, Zs, var, ls, fmt)
        assert torch.equal(img, img0), kind
        if fmt == "f16":
            assert float(ops.image_bound(img, M, N=N).cpu()) == float(var.cpu())


@pytest.mark.parametrize("fmt", ["x6", "f16"])
@pytest.mark.parametrize("D,ard", CASES, ids=CASE_IDS)
def test_kuf_side_job_and_factorisation_bits(device, D, ard, fmt):
    """The same images written by K3's step launches (mgp_kuu_potrf_trtri_kuf), two layers with
    their own Z[0]: bit-equal to the stand-alone launch on the same inputs and to the unshifted
    images (fixed); L, L^-T and info of the float64 Kuu bit-equal under the shift (already
    right: K3 differences the raw coordinates in float64)."""
    from modulatedgps_amd import ops
    var, ls = _hyper(D, ard, device)
    var2 = _t([0.3], device)

    def run(kind):
        X, Z, _ = _shifted(D, ard, kind, device)
        Zs = [Z, torch.flip(Z, dims=(0,)).contiguous()]     # layer 1: the rows reversed
        vs = [var, var2]
        side = [torch.zeros(ops.x6_cols_bytes(M, N), dtype=torch.uint8, device=device) for _ in range(2)]
        L, LinvT, info = ops.kuu_potrf_trtri(Zs, vs, [ls, ls], JITTER, want_L=True, kuf=(X, side, fmt))
        own = [_image(X, Zs[b], vs[b], ls, fmt) for b in range(2)]
        torch.cuda.synchronize()
        for b in range(2):
            assert torch.equal(side[b], own[b]), (kind, b)
        return side, L, LinvT, info

    side0, L0, LinvT0, info0 = run("zero")
    assert (info0.cpu() == 0).all()
    for kind in SHIFTS[1:]:
        side, L, LinvT, info = run(kind)
        for b in range(2):
            assert torch.equal(side[b], side0[b]), (kind, b)
        assert torch.equal(L, L0) and torch.equal(LinvT, LinvT0) and torch.equal(info, info0), kind


@pytest.mark.parametrize("D,ard", CASES, ids=CASE_IDS)
def test_kuu_factorisation_bits(device, D, ard):
    """mgp_kuu_potrf_trtri alone: L, L^-T and info (already right: K3 builds Kuu in float64
    from differences of the raw coordinates)."""
    from modulatedgps_amd import ops
    var, ls = _hyper(D, ard, device)

    def run(kind):
        _, Z, _ = _shifted(D, ard, kind, device)
        return ops.kuu_potrf_trtri([Z, torch.flip(Z, dims=(0,)).contiguous()], [var, var], [ls, ls], JITTER,
                                   want_L=True)

    L0, LinvT0, info0 = run("zero")
    assert (info0.cpu() == 0).all() and float(LinvT0.abs().max()) > 0.0
    for kind in SHIFTS:
        L, LinvT, info = run(kind)
        assert torch.equal(L, L0) and torch.equal(LinvT, LinvT0) and torch.equal(info, info0), kind


@pytest.mark.parametrize("D,ard", CASES, ids=CASE_IDS)
def test_rbf_kuf_kuu_bits(device, D, ard):
    """mgp_rbf_kuf, mgp_rbf_kuu with its jitter diagonal, and the front's mgp_rbf_kuu_jitter
    (fixed: the f32 tile kernel scaled each coordinate before the difference)."""
    from modulatedgps_amd import _lib, ops
    var, ls = _hyper(D, ard, device)

    def run(kind):
        X, Z, _ = _shifted(D, ard, kind, device)
        Kuf = ops.rbf_kuf(X, Z, var, ls)
        Kuu = ops.rbf_kuu(Z, var, ls, JITTER)
        Kj = ops.padded(M, M, device)
        _lib.call("mgp_rbf_kuu_jitter", Z.data_ptr(), ops._ld(Z), M, D, var.data_ptr(), ls.data_ptr(), ls.numel(),
                  JITTER, Kj.data_ptr(), ops._ld(Kj), ops._stream())
        return Kuf, Kuu, Kj

    Kuf0, Kuu0, Kj0 = run("zero")
    assert torch.equal(Kj0, Kuu0)
    v32 = np.float32(float(var.cpu()))
    assert np.array_equal(to_np(Kuu0).diagonal(), np.full(M, np.float64(v32 + np.float32(JITTER))))
    for kind in SHIFTS:
        Kuf, Kuu, Kj = run(kind)
        assert torch.equal(Kuf, Kuf0) and torch.equal(Kuu, Kuu0) and torch.equal(Kj, Kuu0), kind


@pytest.mark.parametrize("D,ard", CASES, ids=CASE_IDS)
def test_rbf_backward_bits(device, D, ard):
    """mgp_rbf_backward (Kuf cotangent, and the symmetric Kuu one) and mgp_rbf_backward_batch,
    the same cotangents given to both calls (already right: FamSE::bwd_point differences the
    raw coordinates)."""
    from modulatedgps_amd import ops
    var, ls = _hyper(D, ard, device)
    rng = np.random.default_rng(D)
    gKuf = ops.as_padded(_t(rng.standard_normal((M, N)), device))
    g = rng.standard_normal((M, M))
    gKuu = ops.as_padded(_t(0.5 * (g + g.T), device))

    def run(kind):
        X, Z, _ = _shifted(D, ard, kind, device)
        out = list(ops.rbf_backward(X, Z, var, ls, gKuf))
        out += list(ops.rbf_backward(Z, Z, var, ls, gKuu, symmetric=True))
        Zs = [Z, torch.flip(Z, dims=(0,)).contiguous()]
        gZs = [torch.zeros(M, D, device=device) for _ in range(2)]
        gvs = [torch.zeros(1, dtype=torch.float64, device=device) for _ in range(2)]
        gls = [torch.zeros(ls.numel(), dtype=torch.float64, device=device) for _ in range(2)]
        ops.rbf_backward_batch(X, Zs, [var, var], [ls, ls], [gKuf, gKuf], [gKuu, gKuu], gZs, gvs, gls)
        return out + gZs + gvs + gls

    ref = run("zero")
    assert all(bool(torch.isfinite(t).all()) for t in ref) and float(ref[0].abs().max()) > 0.0
    for kind in SHIFTS:
        for i, (a, b) in enumerate(zip(run(kind), ref)):
            assert torch.equal(a, b), (kind, i)


@pytest.mark.parametrize("D,ard", CASES, ids=CASE_IDS)
def test_full_cov_bits(device, D, ard):
    """mgp_full_cov_conditional with A = L^-1 Kuf computed once (float64, unshifted) and given to
    both calls: only the Knn tile sees X (fixed: it scaled each coordinate before the difference)."""
    from modulatedgps_amd import ops
    X, Z, v, l = _host_case(D, ard)
    K = 2
    A64 = sla.solve_triangular(np.linalg.cholesky(T.rbf_Kuu_ref(Z, v, l, JITTER)), T.rbf_K_ref(Z, X, v, l), lower=True)
    rng = np.random.default_rng(D + 1)
    q_sqrt = 0.5 * np.eye(M)[None] + np.tril(0.1 * rng.standard_normal((K, M, M)))
    A, qs = ops.as_padded(_t(A64, device)), ops.as_padded(_t(q_sqrt, device))
    var, ls = _hyper(D, ard, device)
    cov0 = ops.full_cov_conditional(_shifted(D, ard, "zero", device)[0], A, qs, var, ls)
    # the reference of this A and q_sqrt: the unshifted call is right to the suite's gate
    base = T.rbf_K_ref(X, X, v, l) - A64.T @ A64
    for k in range(K):
        C = np.tril(q_sqrt[k]).T @ A64
        assert normwise(to_np(cov0[k]), base + C.T @ C) < 1e-4
    for kind in SHIFTS:
        cov = ops.full_cov_conditional(_shifted(D, ard, kind, device)[0], A, qs, var, ls)
        assert torch.equal(cov, cov0), kind


@pytest.mark.parametrize("name", ["stops", "duplicates"])
def test_greedy_bits(device, name):
    """mgp_greedy_*: the smallest case of tests/greedy_ref.py (and its smallest 2-D one), snapped
    to the grid: the same indices, dmax, trace, residual and factor, Z moved by c (already right:
    greedy.hip differences the raw coordinates in float64)."""
    from modulatedgps_amd import inducing
    from modulatedgps_amd.kernels import SquaredExponential
    from tests import greedy_ref as GR
    case = {c.name: c for c in GR.CASES}[name]
    X, Mg, variance, ls = case.args()
    X = T.snap(X)
    kern = SquaredExponential(variance=variance, lengthscales=np.asarray(ls), device=device)
    r0 = inducing.greedy_variance_device(X, Mg, kern, want_factor=True)
    assert len(r0.indices) > 1
    for kind in SHIFTS:
        c = T.offset_vector(kind, case.D)
        r = inducing.greedy_variance_device(T.shift(X, c), Mg, kern, want_factor=True)
        assert r.stopped == r0.stopped and torch.equal(r.indices, r0.indices), kind
        assert np.array_equal((to_np(r.Z) - c).astype(np.float32), r0.Z.cpu().numpy()), kind
        for f in ("dmax", "trace", "residual", "factor"):
            assert torch.equal(getattr(r, f), getattr(r0, f)), (kind, f)


# ---------------------------------------------------------------------- 2. accuracy off the grid
@functools.lru_cache(maxsize=None)
def _accuracy_case(name):
    """-> X [N, D], Z [M, D] (float32), variance, lengthscales, and the float64 Kuf / Kuu."""
    rng = np.random.default_rng(11)
    if name == "calendar":                      # a time axis in years, lengthscale one year
        X = rng.uniform(2000.0, 2020.0, (N, 1))
        Z = X[rng.choice(N, M, replace=False)]
        ls = np.array([1.0])
    else:                                       # "normal1000-D<d>"
        D = int(name.rsplit("D", 1)[1])
        X = rng.standard_normal((N, D)) + 1000.0
        Z = rng.standard_normal((M, D)) + 1000.0
        ls = np.array([0.7 * np.sqrt(D)])
    X, Z, ls, var = X.astype(np.float32), Z.astype(np.float32), ls.astype(np.float32), 0.7
    return X, Z, var, ls, T.rbf_K_ref(Z, X, var, ls), T.rbf_Kuu_ref(Z, var, ls, JITTER)


ACCURACY = ["normal1000-D1", "normal1000-D3", "normal1000-D8", "normal1000-D32", "calendar"]


@pytest.mark.parametrize("name", ACCURACY)
def test_rbf_kuf_kuu_far_from_origin(device, name):
    """(fixed: 3e-5 variance at offset 1000 when the coordinates were scaled first)"""
    from modulatedgps_amd import ops
    X, Z, var, ls, k64, u64 = _accuracy_case(name)
    vt, lt = _t([var], device), _t(ls, device)
    Kuf = to_np(ops.rbf_kuf(_t(X, device), _t(Z, device), vt, lt))
    Kuu = to_np(ops.rbf_kuu(_t(Z, device), vt, lt, JITTER))
    ef, eu = np.abs(Kuf - k64).max() / var, np.abs(Kuu - u64).max() / var
    print(f"TRANSLATION {name} rbf_kuf max|err|/variance {ef:.3e} rbf_kuu {eu:.3e} (bound 2e-6)")
    assert ef <= 2e-6 and eu <= 2e-6
    assert np.array_equal(Kuu, Kuu.T)


@pytest.mark.parametrize("fmt", ["x6", "f16"])
@pytest.mark.parametrize("name", ACCURACY)
def test_kuf_image_far_from_origin(device, name, fmt):
    """The decoded Kuf image (fixed: before, errors of several per cent of the variance and
    entries above it on these inputs).  The calendar case spans 20 lengthscales: K1's expanded
    form about any reference point is ~1.4e-6 normwise and 7.8e-6 max|ref| off there (measured,
    and a float32 NumPy emulation agrees), outside the split-f16 class bounds below, so D = 1
    takes the difference z' - x' itself on the MFMA and squares it (kuf_image.hpp): 1.4e-7 and
    4.4e-7 measured."""
    from modulatedgps_amd import ops
    X, Z, var, ls, k64, _ = _accuracy_case(name)
    vt, lt = _t([var], device), _t(ls, device)
    img = _image(_t(X, device), _t(Z, device), vt, lt, fmt)
    v32 = float(np.float32(var))
    if fmt == "f16":
        bound = float(ops.image_bound(img, M, N=N).cpu())
        assert bound == v32
        kd = decode_cols_f16(img, M, N, bound)
    else:
        kd = decode_cols_image(img, M, N)
    err = np.abs(kd - k64)
    ratio = float(np.max(err / T.image_bound(Z, X, var, ls, k64)))
    nw, mx = normwise(kd, k64), float(err.max() / np.abs(k64).max())
    print(f"TRANSLATION {name} {fmt} image: err/bound {ratio:.3f} normwise {nw:.3e} max/max|ref| {mx:.3e} "
          f"max entry/variance {kd.max() / v32:.9f}")
    assert np.all(np.isfinite(kd)) and kd.max() <= v32 * (1.0 + 2.0 ** -20)
    assert ratio <= 1.0
    if fmt == "f16":
        assert nw < 5e-7
        assert mx < 2e-6


# ---------------------------------------------------------------------- 3. the model
MODEL = dict(N=1000, M=64, K=3, D=2, ls=0.7, S=3)


@functools.lru_cache(maxsize=None)
def _model_problem():
    X, Y, p = T.snapped_problem(MODEL["N"], MODEL["M"], MODEL["K"], MODEL["D"], MODEL["ls"], MODEL["S"])
    c = T.offset_vector("mixed", MODEL["D"])
    z, u = R.explicit_noise(MODEL["S"], MODEL["N"], MODEL["K"], seed=5)
    ref = dict(elbo=R.smgp_elbo(X, Y, p, z, u), predict_y=R.predict_y(X, p))
    return X, Y, p, T.shift(X, c), T.shifted_params(p, c), z, u, ref


@pytest.fixture(params=["f16", "x6"])
def chain_fmt(request):
    from modulatedgps_amd import config
    old = config.expert_format()
    config.set_expert_format(request.param)
    yield request.param
    config.set_expert_format(old)


def test_model_elbo_and_predict_far_from_origin(device, chain_fmt):
    """ELBO with explicit noise and predict_y of the shifted model against the oracle on the
    unshifted problem (fixed: the Kuf image of the shifted inputs was wrong by per cents)."""
    X, Y, p, Xs, ps, z, u, ref = _model_problem()
    model = build_model(ps, device)
    Xd = _t(Xs, device)
    elbo = float(model._build_likelihood(Xd, Y, noise=dev_noise(z, u, device)).cpu())
    ym, yv = model.predict_y(Xd)
    em, ev = normwise(np.asarray(ym), ref["predict_y"][0]), normwise(np.asarray(yv), ref["predict_y"][1])
    print(f"TRANSLATION model {chain_fmt}: elbo {elbo:.7f} ref {ref['elbo']:.7f} predict_y mean {em:.2e} var {ev:.2e}")
    assert elbo == pytest.approx(ref["elbo"], rel=1e-4)
    assert em < 1e-4 and ev < 1e-4


def test_model_elbo_and_grad_far_from_origin(device, chain_fmt):
    """elbo_and_grad of the shifted model by test_gpu_training's criterion: float64 and float32
    autograd of the oracle graph on the unshifted problem (fixed)."""
    from tests.test_gpu_training import _check_elbo_and_grad
    X, Y, p, Xs, ps, _, _, _ = _model_problem()
    _check_elbo_and_grad(device, MODEL["N"], MODEL["M"], MODEL["K"], MODEL["D"], MODEL["ls"], MODEL["S"], False,
                         problem=(X, Y, p), device_problem=(Xs, ps))


def test_model_step_bits(device, chain_fmt):
    """Where two elbo_and_grad calls on the same input return the same bits, the shifted step
    returns them too (fixed); skipped, with the reason, where the step is not deterministic."""
    X, Y, p, Xs, ps, z, u, _ = _model_problem()
    model = build_model(p, device)
    Xd = _t(X, device)
    e0, g0 = model.elbo_and_grad(Xd, Y, noise=dev_noise(z, u, device))
    e1, g1 = model.elbo_and_grad(Xd, Y, noise=dev_noise(z, u, device))
    if not torch.equal(e0, e1):
        pytest.skip(f"two elbo_and_grad calls on the same input differ ({float(e0)!r} vs {float(e1)!r}: a "
                    "reduction whose order is not fixed), so the shifted ELBO cannot be asserted bit-equal")
    e_s, g_s = build_model(ps, device).elbo_and_grad(_t(Xs, device), Y, noise=dev_noise(z, u, device))
    assert torch.equal(e_s, e0)
    for n in g0:
        if torch.equal(g0[n], g1[n]):           # the gradient blocks that are deterministic as well
            assert torch.equal(g_s[n], g0[n]), n
