"""GPU tests of the Matern32 / Matern52 kernels (csrc/matern.hip) from the C-ABI entries up to
the models, against the float64 references of tests/matern_ref.py.  Tolerances are the suite's
own for the SquaredExponential counterparts:
  Kuf / Kuu and the decoded Kuf images: elementwise |err| <= 2e-6 * variance
  L, L^-1 of the float64 factorisation: normwise < 1e-6 (cond(Kuu) < 1e6 asserted)
  backward: gZ, g_ls normwise < 1e-4, g_var rel 1e-4;  predict_f normwise < 1e-4;  ELBO rel 1e-4
  elbo_and_grad per block: normwise < max(3e-4, 1.5 x float32 torch autograd of the same graph)."""
import functools

import numpy as np
import pytest
import scipy.linalg as sla
import torch

from oracle import cpu_ref as R
from tests import matern_ref as MR
from tests import translation_ref as T
from tests.helpers import decode_cols_f16, decode_cols_image, dev_noise, normwise, to_np, unequal_problem

pytestmark = pytest.mark.gpu

NU2 = [3, 5]
FAMILY = {3: "matern32", 5: "matern52"}
JITTER = 1e-6


def _t(x, dev):
    return torch.as_tensor(np.asarray(x), dtype=torch.float32, device=dev)


def _r32(a):
    return np.asarray(a, np.float32).astype(np.float64)


# --------------------------------------------------------------------------- 1. Kuf / Kuu
@pytest.mark.parametrize("nu2", NU2)
@pytest.mark.parametrize("N,M,D,ard", [(1000, 37, 1, False), (4099, 256, 2, False), (2048, 130, 8, True),
                                       (3, 5, 16, True), (1500, 64, 3, True), (515, 129, 32, True)])
def test_matern_kuf_kuu(device, N, M, D, ard, nu2):
    from modulatedgps_amd import ops
    rng = np.random.default_rng(N + M)
    X, Z = rng.standard_normal((N, D)), rng.standard_normal((M, D))
    ls = rng.uniform(0.5, 2.0, D) * (np.sqrt(D) if D == 32 else 1.0) if ard else np.array([0.8])
    var = 0.7
    Xd, Zd, vd, ld = _t(X, device), _t(Z, device), _t([var], device), _t(ls, device)
    Kuf = to_np(ops.matern_kuf(Xd, Zd, vd, ld, nu2))
    ref = MR.matern_K(_r32(Z), _r32(X), np.float32(var), _r32(ls), nu2)
    ef = np.abs(Kuf - ref).max() / var
    Kuu = to_np(ops.matern_kuu(Zd, vd, ld, nu2, JITTER))
    eu = np.abs(Kuu - MR.matern_Kuu(_r32(Z), np.float32(var), _r32(ls), nu2, JITTER)).max() / var
    print(f"MATERN nu2={nu2} N={N} M={M} D={D}: kuf max|err|/variance {ef:.3e} kuu {eu:.3e} (bound 2e-6)")
    assert ef <= 2e-6 and eu <= 2e-6
    assert np.array_equal(Kuu, Kuu.T)
    assert np.array_equal(Kuu.diagonal(), np.full(M, np.float64(np.float32(var) + np.float32(JITTER))))


# --------------------------------------------------------------------------- 2. images
def _image(X, Z, var, ls, nu2, fmt):
    """The image written into a buffer of 0xFF bytes (NaN patterns: nothing may stay unwritten)."""
    from modulatedgps_amd import _lib, ops
    M, N = Z.shape[0], X.shape[0]
    out = torch.full((_lib.load().mgp_x6_cols_bytes(M, N),), 0xFF, dtype=torch.uint8, device=X.device)
    img = ops.matern_kuf_image(X, Z, var, ls, nu2, out=out, fmt=fmt)
    assert img.data_ptr() == out.data_ptr()
    return img


def _decode(img, M, N, fmt, bound):
    Mp, Np = -(-M // 128) * 128, -(-N // 256) * 256
    full = decode_cols_f16(img, Mp, Np, bound) if fmt == "f16" else decode_cols_image(img, Mp, Np)
    return full[:M, :N], full


@pytest.mark.parametrize("nu2", NU2)
@pytest.mark.parametrize("fmt", ["x6", "f16"])
@pytest.mark.parametrize("N,M,D,ard", [(777, 130, 3, True), (3, 1, 1, False), (256, 128, 8, True)])
def test_matern_kuf_image(device, N, M, D, ard, fmt, nu2):
    from modulatedgps_amd import ops
    rng = np.random.default_rng(N + M + D)
    X, Z = rng.standard_normal((N, D)), rng.standard_normal((M, D))
    ls = rng.uniform(0.5, 2.0, D) if ard else np.array([0.8])
    var = 0.1   # not a power of two: the split-f16 scale and the variance do not fold into an exact multiplier
    img = _image(_t(X, device), _t(Z, device), _t([var], device), _t(ls, device), nu2, fmt)
    v32 = float(np.float32(var))
    assert float(ops.image_bound(img, M, N=N).cpu()) == v32                   # the trailer's scale bound
    tr = img[img.numel() - 256:].view(torch.float32).cpu().numpy()
    assert np.array_equal(tr[32:64], np.zeros(32, np.float32))                # no reference point
    kd, full = _decode(img, M, N, fmt, v32)
    assert np.all(np.isfinite(full))
    assert not full[M:].any() and not full[:, N:].any()                       # padding exactly zero
    ref = MR.matern_K(_r32(Z), _r32(X), np.float32(var), _r32(ls), nu2)
    err = np.abs(kd - ref).max() / var
    print(f"MATERN nu2={nu2} {fmt} image N={N} M={M} D={D}: max|err|/variance {err:.3e} (bound 2e-6)")
    assert err <= 2e-6
    assert kd.max() <= v32 * (1.0 + 2.0 ** -20)


# --------------------------------------------------------------------------- 3. translation
TN, TM = 300, 70
SHIFTS = ("plus1024", "mixed")


@pytest.mark.parametrize("nu2", NU2)
@pytest.mark.parametrize("D,ard", [(1, False), (3, True), (8, True)])
def test_matern_translation_bits(device, D, ard, nu2):
    """Grid-exact inputs and their exactly shifted copies (tests/translation_ref.py) give the same
    bits from every Matern entry: only differences of raw coordinates are formed."""
    from modulatedgps_amd import ops
    X0, Z0, var, ls = T.grid_case(TN, TM, D, ard)
    vd, ld = _t([var], device), _t(ls, device)
    rng = np.random.default_rng(D)
    gKuf = ops.as_padded(_t(rng.standard_normal((TM, TN)), device))
    g = rng.standard_normal((TM, TM))
    gKuu = ops.as_padded(_t(0.5 * (g + g.T), device))

    def run(kind):
        c = T.offset_vector(kind, D)
        X, Z = _t(T.shift(X0, c), device), _t(T.shift(Z0, c), device)
        out = [_image(X, Z, vd, ld, nu2, "x6"), _image(X, Z, vd, ld, nu2, "f16"),
               ops.matern_kuf(X, Z, vd, ld, nu2), ops.matern_kuu(Z, vd, ld, nu2, JITTER)]
        L, LinvT, info = ops.matern_kuu_potrf_trtri(Z, vd, ld, nu2, JITTER, want_L=True)
        out += [L, LinvT, info]
        out += list(ops.matern_backward(X, Z, vd, ld, nu2, gKuf))
        out += list(ops.matern_backward(Z, Z, vd, ld, nu2, gKuu, symmetric=True))
        return out

    ref = run("zero")
    assert int(ref[6].cpu()[0]) == 0 and float(ref[5].abs().max()) > 0.0 and float(ref[7].abs().max()) > 0.0
    for kind in SHIFTS:
        for i, (a, b) in enumerate(zip(run(kind), ref)):
            assert torch.equal(a, b), (kind, i)


@pytest.mark.parametrize("nu2", NU2)
@pytest.mark.parametrize("D", [1, 3, 8, 32])
def test_matern_far_from_origin(device, D, nu2):
    """Unit spread at an offset of 1e4: the 2e-6 variance bound still holds against float64 of the
    float32-rounded inputs, for the f32 entries and both images."""
    from modulatedgps_amd import ops
    rng = np.random.default_rng(D)
    X = (rng.standard_normal((TN, D)) + 1e4).astype(np.float32)
    Z = (rng.standard_normal((TM, D)) + 1e4).astype(np.float32)
    ls, var = np.array([0.7 * np.sqrt(D)], np.float32), 0.7
    Xd, Zd, vd, ld = _t(X, device), _t(Z, device), _t([var], device), _t(ls, device)
    ref = MR.matern_K(_r32(Z), _r32(X), np.float32(var), _r32(ls), nu2)
    refu = MR.matern_Kuu(_r32(Z), np.float32(var), _r32(ls), nu2, JITTER)
    errs = {"kuf": np.abs(to_np(ops.matern_kuf(Xd, Zd, vd, ld, nu2)) - ref).max() / var,
            "kuu": np.abs(to_np(ops.matern_kuu(Zd, vd, ld, nu2, JITTER)) - refu).max() / var}
    for fmt in ("x6", "f16"):
        kd, _ = _decode(_image(Xd, Zd, vd, ld, nu2, fmt), TM, TN, fmt, float(np.float32(var)))
        errs[fmt] = np.abs(kd - ref).max() / var
    print(f"MATERN nu2={nu2} D={D} offset 1e4: " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert all(v <= 2e-6 for v in errs.values()), errs


# --------------------------------------------------------------------------- 4. factorisation
@pytest.mark.parametrize("nu2", NU2)
@pytest.mark.parametrize("M", [25, 64, 130, 256])
def test_matern_kuu_potrf_trtri(device, M, nu2):
    from modulatedgps_amd import ops
    rng = np.random.default_rng(M)
    Z = rng.standard_normal((M, 3)).astype(np.float32)
    var, ls = 0.5, np.array([0.5, 1.0, 1.5], np.float32)
    Kuu = MR.matern_Kuu(_r32(Z), np.float32(var), _r32(ls), nu2, JITTER)
    cond = np.linalg.cond(Kuu)
    assert cond < 1e6, cond
    L, LinvT, info = ops.matern_kuu_potrf_trtri(_t(Z, device), _t([var], device), _t(ls, device), nu2, JITTER,
                                                want_L=True)
    assert int(info.cpu()[0]) == 0
    Lr = np.linalg.cholesky(Kuu)
    Li = sla.solve_triangular(Lr, np.eye(M), lower=True)
    Lg, Lt = to_np(L[0]), to_np(LinvT[0])
    assert not np.triu(Lg, 1).any() and not np.tril(Lt, -1).any()
    eL, eI = normwise(Lg, Lr), normwise(Lt.T, Li)
    print(f"MATERN nu2={nu2} M={M}: cond {cond:.1e} L {eL:.2e} L^-1 {eI:.2e} (bound 1e-6)")
    assert eL < 1e-6 and eI < 1e-6
    # without L: the same inverse
    _, LinvT2, info2 = ops.matern_kuu_potrf_trtri(_t(Z, device), _t([var], device), _t(ls, device), nu2, JITTER)
    assert torch.equal(LinvT2, LinvT) and int(info2.cpu()[0]) == 0


# --------------------------------------------------------------------------- 5. backward
@pytest.mark.parametrize("nu2", NU2)
@pytest.mark.parametrize("N,M,D,ard", [(1000, 37, 1, False), (777, 130, 3, True), (300, 64, 32, True)])
def test_matern_backward(device, N, M, D, ard, nu2):
    """The Kuf cotangent, then the symmetric Kuu cotangent accumulated onto it, against float64
    autograd of both terms; two calls give the same bits."""
    from modulatedgps_amd import ops
    rng = np.random.default_rng(12 + D)
    Z = rng.standard_normal((M, D)).astype(np.float32)
    X = rng.standard_normal((N, D)).astype(np.float32)
    ls = ((np.linspace(0.7, 1.3, D) if ard else np.array([0.9])) * np.sqrt(D)).astype(np.float32)
    gK = rng.standard_normal((M, N)).astype(np.float32)
    gU = rng.standard_normal((M, M)).astype(np.float32)
    gU = 0.5 * (gU + gU.T)
    Xd, Zd, vd, ld = _t(X, device), _t(Z, device), _t([0.6], device), _t(ls, device)
    gKd, gUd = ops.as_padded(_t(gK, device)), ops.as_padded(_t(gU, device))

    def run():
        gZ, gv, gl = ops.matern_backward(Xd, Zd, vd, ld, nu2, gKd)
        first = (gZ.clone(), gv.clone(), gl.clone())
        ops.matern_backward(Zd, Zd, vd, ld, nu2, gUd, symmetric=True, accumulate=True, gZ=gZ, g_var=gv, g_ls=gl)
        return first, (gZ, gv, gl)

    first, both = run()
    z64 = torch.tensor(Z.astype(np.float64), requires_grad=True)
    v64 = torch.tensor(float(np.float32(0.6)), dtype=torch.float64, requires_grad=True)
    l64 = torch.tensor(ls.astype(np.float64), requires_grad=True)
    kuf = (MR.torch_matern(z64, torch.tensor(X.astype(np.float64)), v64, l64, nu2) * torch.tensor(gK.astype(np.float64))).sum()
    gf = torch.autograd.grad(kuf, (z64, v64, l64), retain_graph=True)
    kuu = (MR.torch_matern(z64, z64, v64, l64, nu2) * torch.tensor(gU.astype(np.float64))).sum()
    gu = torch.autograd.grad(kuu, (z64, v64, l64))
    for name, got, ref in (("Kuf", first, gf), ("Kuf + Kuu", both, [a + b for a, b in zip(gf, gu)])):
        eZ, eL = normwise(to_np(got[0]), ref[0].numpy()), normwise(got[2].cpu().numpy(), ref[2].numpy())
        print(f"MATERN nu2={nu2} backward {name} N={N} M={M} D={D}: gZ {eZ:.2e} g_ls {eL:.2e}")
        assert eZ < 1e-4 and eL < 1e-4
        assert float(got[1].cpu()) == pytest.approx(float(ref[1]), rel=1e-4)
    again_first, again_both = run()
    for a, b in zip(first + both, again_first + again_both):
        assert torch.equal(a, b)


@pytest.mark.parametrize("nu2", NU2)
def test_matern_backward_coincident_points(device, nu2):
    """X rows equal to Z rows: nothing divides by s, so the output is finite and matches autograd."""
    from modulatedgps_amd import ops
    rng = np.random.default_rng(3)
    M, N, D = 37, 200, 3
    Z = rng.standard_normal((M, D)).astype(np.float32)
    X = rng.standard_normal((N, D)).astype(np.float32)
    X[:M] = Z
    ls = np.array([0.7, 1.0, 1.3], np.float32)
    gK = rng.standard_normal((M, N)).astype(np.float32)
    gZ, gv, gl = ops.matern_backward(_t(X, device), _t(Z, device), _t([0.6], device), _t(ls, device), nu2,
                                     ops.as_padded(_t(gK, device)))
    assert all(bool(torch.isfinite(t).all()) for t in (gZ, gv, gl))
    z64 = torch.tensor(Z.astype(np.float64), requires_grad=True)
    l64 = torch.tensor(ls.astype(np.float64), requires_grad=True)
    v64 = torch.tensor(float(np.float32(0.6)), dtype=torch.float64)
    (MR.torch_matern(z64, torch.tensor(X.astype(np.float64)), v64, l64, nu2) * torch.tensor(gK.astype(np.float64))).sum().backward()
    assert normwise(to_np(gZ), z64.grad.numpy()) < 1e-4 and normwise(gl.cpu().numpy(), l64.grad.numpy()) < 1e-4


# --------------------------------------------------------------------------- 6. predict_f
@functools.lru_cache(maxsize=None)
def _layer_case(N, M, K, D, ard, nu2):
    X, _, p = R.synthetic_problem(N, M, K, D, 1.0, state="perturbed", S=2)
    L = p.pred
    ls = np.linspace(0.8, 1.6, D) if ard else np.array([0.9])
    Z32, X32 = _r32(L["Z"]), _r32(X)
    Kuu = MR.matern_Kuu(Z32, np.float32(L["variance"]), _r32(ls), nu2, JITTER)
    Kuf = MR.matern_K(Z32, X32, np.float32(L["variance"]), _r32(ls), nu2)
    Knn = np.full(N, float(np.float32(L["variance"])))
    mu, var = R.base_conditional_white(Kuf, Kuu, Knn, _r32(L["q_mu"]), _r32(L["q_sqrt"]))
    return X, L, ls, np.linalg.cond(Kuu), mu, var


def _set_chain(config, chain):
    config.set_conditional_mode("f32" if chain == "f32" else "x6")
    config.set_expert_format("x6" if chain == "x6" else "f16")
    config.set_expert_cross("f8" if chain == "f16x8" else "f16")


@pytest.fixture
def chain_config():
    from modulatedgps_amd import config
    old = (config.conditional_mode(), config.expert_format(), config.expert_cross())
    yield config
    config.set_conditional_mode(old[0]), config.set_expert_format(old[1]), config.set_expert_cross(old[2])


@pytest.mark.parametrize("nu2", NU2)
@pytest.mark.parametrize("chain", ["f16", "x6", "f16x8", "f32"])
@pytest.mark.parametrize("N,M,K,D,ard", [(2048, 130, 4, 8, True), (1500, 64, 3, 3, False)])
def test_matern_predict_f(device, chain_config, N, M, K, D, ard, chain, nu2):
    from modulatedgps_amd.models import SVGPModified
    X, L, ls, cond, mu_ref, var_ref = _layer_case(N, M, K, D, ard, nu2)
    assert cond < 1e6, cond
    _set_chain(chain_config, chain)
    layer = SVGPModified(MR.device_kernel(FAMILY[nu2], L["variance"], ls, device), None, L["Z"], num_latent_gps=K,
                         device=device)
    layer.set_variational(L["q_mu"], L["q_sqrt"])
    mu, var = layer.predict_f(_t(X, device))
    assert int(layer._last_info.cpu()[0]) == 0
    em, ev = normwise(to_np(mu), mu_ref), normwise(to_np(var), var_ref)
    print(f"MATERN nu2={nu2} predict_f {chain} N={N} M={M}: cond {cond:.1e} mean {em:.2e} var {ev:.2e} (bound 1e-4)")
    assert em < 1e-4 and ev < 1e-4


# --------------------------------------------------------------------------- 7. ELBO
def _problem(N, Mf, Ma, K, D, S):
    if Mf == Ma:
        return R.synthetic_problem(N, Mf, K, D, 0.8, ls_assign=1.1, state="perturbed", S=S)
    return unequal_problem(N, Mf, Ma, K, D, 0.8, np.linspace(0.7, 1.3, D), S)


ELBO_CASES = [("smgp", ("matern52", "matern52"), 130, 130), ("modified", ("matern32", "se"), 130, 130),
              ("smgp", ("matern52", "matern32"), 130, 64), ("modified", ("se", "matern52"), 64, 130)]


@pytest.mark.parametrize("kind,families,Mf,Ma", ELBO_CASES)
def test_matern_elbo(device, kind, families, Mf, Ma):
    N, K, D, S = 777, 3, 3, 5
    X, Y, p = _problem(N, Mf, Ma, K, D, S)
    z, u = R.explicit_noise(S, N, K, seed=5)
    a_var = np.linspace(0.3, 0.9, K)[None, :] if kind == "modified" else None
    with torch.no_grad():
        e_ref, _ = _ref_elbo(X, Y, p, z, u, families, a_var)
    model = MR.build_model(p, device, families, a_var=a_var)
    e = float(model._build_likelihood(_t(X, device), Y, noise=dev_noise(z, u, device)).cpu())
    model.check_linalg()
    print(f"MATERN elbo {kind} {families} M=({Mf}, {Ma}): {e:.6f} reference {e_ref:.6f}")
    assert e == pytest.approx(e_ref, rel=1e-4)


def _ref_elbo(X, Y, p, z, u, families, a_var):
    from oracle import grad_ref as GR
    pred, assign, lik = GR.params_from_oracle(p, requires_grad=False)
    f = lambda a: torch.tensor(np.asarray(a, np.float32)).double()
    av = None if a_var is None else f(np.asarray(a_var).reshape(-1))
    e = MR.elbo(f(X), f(Y), pred, assign, lik, f(z), f(u), p.num_data, MR.torch_kernel(families[0]),
                MR.torch_kernel(families[1]), assign_lik_var=av)
    return float(e), None


# --------------------------------------------------------------------------- 8. elbo_and_grad
FLOOR, FACTOR = 3e-4, 1.5


@functools.lru_cache(maxsize=None)
def _grad_case(N, M, K, D, S, families):
    X, Y, p = R.synthetic_problem(N, M, K, D, 0.8 if D == 2 else 1.0, state="perturbed", S=S)
    z, u = R.explicit_noise(S, N, K, seed=5)
    e64, g64 = MR.elbo_and_grads(X, Y, p, z, u, families)
    _, g32 = MR.elbo_and_grads(X, Y, p, z, u, families, dtype=torch.float32)
    return X, Y, p, z, u, e64, g64, g32


@pytest.mark.parametrize("families", [("matern52", "matern52"), ("matern32", "se")], ids=["m52-m52", "m32-se"])
@pytest.mark.parametrize("fmt", ["f16", "x6"])
@pytest.mark.parametrize("N,M,K,D,S", [(2049, 64, 4, 2, 7), (777, 130, 3, 3, 5)])
def test_matern_elbo_and_grad(device, chain_config, N, M, K, D, S, fmt, families):
    """tests/test_gpu_training.py's criterion on the Matern graph: per parameter block, normwise
    error against float64 autograd < max(3e-4, 1.5 x the error of float32 autograd of the same
    graph, measured here)."""
    X, Y, p, z, u, e64, g64, g32 = _grad_case(N, M, K, D, S, families)
    _set_chain(chain_config, fmt)
    model = MR.build_model(p, device, families)
    e, grads = model.elbo_and_grad(_t(X, device), Y, noise=dev_noise(z, u, device))
    model.check_linalg()
    assert float(e.cpu()) == pytest.approx(e64, rel=1e-4)
    names = [n for n, _, _ in model.trainable_parameters()]
    assert sorted(names) == sorted(g64)
    errs, errs32 = {}, {}
    for n in names:
        got = to_np(grads[n])
        got = got.reshape(-1) if n.endswith(("variance", "lengthscales")) else got
        ref = g64[n].reshape(got.shape)
        errs[n], errs32[n] = normwise(got, ref), normwise(g32[n].reshape(got.shape), ref)
    print(f"MATERN grad {families} {fmt} N={N} M={M}: " + str({k: f"{v:.1e}/{errs32[k]:.1e}" for k, v in errs.items()}))
    for n, err in errs.items():
        assert err < max(FLOOR, FACTOR * errs32[n]), (n, err, errs32[n])


def test_matern_sharded_gradient(device, tmp_path):
    """N-sharded elbo_and_grad (n_offset / n_total, through a one-rank process group): the
    kernel-parameter gradients of the two shards, which carry no KL part, add up to the
    whole batch's."""
    import torch.distributed as dist
    N, M, K, D, S = 777, 64, 3, 3, 5
    families = ("matern52", "matern32")
    X, Y, p = R.synthetic_problem(N, M, K, D, 1.0, state="perturbed", S=S)
    z, u = R.explicit_noise(S, N, K, seed=5)
    model = MR.build_model(p, device, families)
    Xd = _t(X, device)
    _, whole = model.elbo_and_grad(Xd, Y, noise=dev_noise(z, u, device))
    whole = {k: to_np(v) for k, v in whole.items()}
    own = not dist.is_initialized()
    if own:
        dist.init_process_group("gloo", init_method=f"file://{tmp_path}/store", rank=0, world_size=1)
    try:
        parts = []
        for lo, hi in ((0, 400), (400, N)):
            _, g = model.elbo_and_grad(Xd[lo:hi], Y[lo:hi], noise=dev_noise(z[:, lo:hi], u[:, lo:hi], device),
                                       n_offset=lo, n_total=N, process_group=dist.group.WORLD)
            parts.append({k: to_np(v) for k, v in g.items()})
    finally:
        if own:
            dist.destroy_process_group()
    for name in ("pred.Z", "pred.variance", "pred.lengthscales", "assign.Z", "assign.variance",
                 "assign.lengthscales", "lik_variance"):
        assert normwise(parts[0][name] + parts[1][name], whole[name]) < 1e-4, name


# --------------------------------------------------------------------------- 9. training
def _toy(device, seed=0):
    X, Y, p = R.synthetic_problem(1000, 25, 3, 1, 0.5, state="init", S=5)
    model = MR.build_model(p, device, ("matern52", "matern52"), seed=seed)
    return X, Y, model


@pytest.mark.parametrize("runner", ["run_adam", "run_natgrad_adam"])
def test_matern_training_raises_the_elbo(device, runner):
    """20 full-batch iterations on a Matern52 toy model: the ELBO under one fixed noise rises."""
    from utils import training_utils
    from utils.data import Dataset
    X, Y, model = _toy(device)
    Xd, Yd = _t(X, device), _t(Y, device)
    z, u = R.explicit_noise(5, 1000, 3, seed=5)
    noise = dev_noise(z, u, device)
    e0 = float(model._build_likelihood(Xd, Y, noise=noise).cpu())
    it = iter(Dataset.from_tensor_slices((Xd, Yd)).shuffle(buffer_size=1000, seed=0).batch(1000).repeat())
    iters, elbos = getattr(training_utils, runner)(model, 20, it, 0.01)
    e1 = float(model._build_likelihood(Xd, Y, noise=noise).cpu())
    print(f"MATERN {runner}: elbo {e0:.4f} -> {e1:.4f}; reported {np.round(elbos, 4).tolist()}")
    assert iters == [5, 10, 15, 20] and np.all(np.isfinite(elbos))
    assert e1 > e0


# --------------------------------------------------------------------------- 10. surfaces
def test_squared_exponential_model_keeps_its_path(device):
    """Both kernels SquaredExponential: the two-layer launches as before."""
    X, Y, p = R.synthetic_problem(777, 130, 3, 3, 1.0, state="perturbed", S=3)
    model = MR.build_model(p, device, ("se", "se"))
    model._build_likelihood(_t(X, device), Y, seed=1)
    assert model.layers_per_launch == 2
    assert "LinvT2" in model._buffers(777) and model._tail_batchable()
    mixed = MR.build_model(p, device, ("se", "matern52"))
    mixed._build_likelihood(_t(X, device), Y, seed=1)
    assert "LinvT2" not in mixed._buffers(777) and not mixed._tail_batchable()


def test_matern_only_surfaces_raise(device):
    from modulatedgps_amd.inducing import greedy_variance
    X, Y, p = R.synthetic_problem(300, 25, 3, 2, 1.0, state="perturbed", S=3)
    model = MR.build_model(p, device, ("matern32", "matern52"))
    Xd = _t(X, device)
    layer = model.pred_layer
    with pytest.raises(NotImplementedError, match="Matern32"):
        layer.predict_f(Xd[:50], full_cov=True)
    with pytest.raises(NotImplementedError, match="Matern32"):
        layer.predict_f_samples(Xd[:50], 2, full_cov=True)
    with pytest.raises(NotImplementedError, match="Matern32"):
        layer.sample_paths(2, num_features=64)
    with pytest.raises(NotImplementedError, match="Matern"):
        model.sample_paths(2, num_features=64)
    with pytest.raises(NotImplementedError, match="Matern52"):
        model.assign_layer.predict_f(Xd[:50], full_cov=True)
    with pytest.raises(ValueError, match="SquaredExponential"):
        greedy_variance(Xd, 10, layer.kernel)
    s = layer.predict_f_samples(Xd[:50], 2, full_cov=False, seed=3)   # the marginal draw works
    assert tuple(s.shape) == (2, 50, 3) and bool(torch.isfinite(s).all())
    assert repr(layer.kernel).startswith("Matern32(variance=[0.5")
    with pytest.raises(TypeError):
        from modulatedgps_amd.models import SVGPModified
        SVGPModified(object(), None, np.zeros((4, 1)), device=device)


# --------------------------------------------------------------------------- predictions
@functools.lru_cache(maxsize=None)
def _predict_case():
    N, M, K, D = 500, 64, 3, 2
    X, Y, p = R.synthetic_problem(N, M, K, D, 0.8, ls_assign=1.1, state="perturbed", S=3)
    out = {}
    for name, L, nu2 in (("f", p.pred, 5), ("a", p.assign, 3)):
        Z32, X32, v = _r32(L["Z"]), _r32(X), np.float32(L["variance"])
        ls = _r32([L["lengthscales"]])
        out[name] = R.base_conditional_white(MR.matern_K(Z32, X32, v, ls, nu2), MR.matern_Kuu(Z32, v, ls, nu2, JITTER),
                                             np.full(N, float(v)), _r32(L["q_mu"]), _r32(L["q_sqrt"]))
    return X, Y, p, out


def test_matern_predict_y_assign_samples(device):
    X, Y, p, ref = _predict_case()
    model = MR.build_model(p, device, ("matern52", "matern32"))
    lik = _r32(p.lik_variance).reshape(-1)
    ym, yv = model.predict_y(X)
    assert ym.shape == (1, 500, 3)
    assert normwise(ym[0], ref["f"][0]) < 1e-4 and normwise(yv[0], ref["f"][1] + lik) < 1e-4
    asg = model.predict_assign(X)
    mu_a = ref["a"][0]
    soft = np.exp(mu_a - mu_a.max(1, keepdims=True))
    assert normwise(asg, soft / soft.sum(1, keepdims=True)) < 1e-4
    sy, sf = model.predict_samples(X, S=4, seed=11)
    assert sy.shape == (4, 500, 1) and sf.shape == (4, 500, 1)
    assert np.all(np.isfinite(sy)) and np.all(np.isfinite(sf))
    sy2, _ = model.predict_samples(X, S=4, seed=11)
    assert np.array_equal(sy, sy2)


def test_matern_mixture_predictive(device):
    """The mixture predictive on Matern layers: plug-in weights, mean and variance against the
    float64 conditionals; quantiles, CDF and CRPS consistent with each other."""
    X, Y, p, ref = _predict_case()
    model = MR.build_model(p, device, ("matern52", "matern32"))
    lik = _r32(p.lik_variance).reshape(-1)
    mu_f, var_f, mu_a = ref["f"][0], ref["f"][1] + lik, ref["a"][0]
    w = np.exp(mu_a - mu_a.max(1, keepdims=True))
    w /= w.sum(1, keepdims=True)
    assert normwise(model.predict_mixture_weights(X), w) < 1e-4
    mean = (w * mu_f).sum(1, keepdims=True)
    var = (w * (var_f + (mu_f - mean) ** 2)).sum(1, keepdims=True)
    m, v = model.predict_mixture_mean_and_var(X)
    assert normwise(m, mean) < 1e-4 and normwise(v, var) < 1e-4
    dens = np.log((w * np.exp(-0.5 * (Y - mu_f) ** 2 / var_f) / np.sqrt(2 * np.pi * var_f)).sum(1))
    assert normwise(model.predict_log_density(X, Y), dens) < 1e-4
    assert model.log_predictive_density(X, Y) == pytest.approx(dens.mean(), rel=1e-4)
    grid = np.linspace(-3, 3, 7)
    assert model.predict_density(X, grid).shape == (500, 7)
    levels = [0.1, 0.5, 0.9]
    q = model.predict_quantiles(X, levels)
    assert q.shape == (500, 3) and np.all(np.diff(q, axis=1) > 0)
    for j, lv in enumerate(levels):
        assert np.abs(model.predict_cdf(X, q[:, j]) - lv).max() < 1e-4
    cdf = model.predict_cdf(X, Y)
    assert np.all((cdf >= 0) & (cdf <= 1))
    assert np.abs(cdf + model.predict_cdf(X, Y, tail="upper") - 1.0).max() < 1e-5
    crps = model.predict_crps(X, Y)
    assert crps.shape == (500,) and np.all(crps > 0) and np.all(np.isfinite(crps))
    assert model.crps(X, Y) == pytest.approx(crps.mean(), rel=1e-5)
