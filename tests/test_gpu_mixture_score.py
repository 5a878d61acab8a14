"""GPU tests of the mixture scores (csrc/mixture_score.hip: mgp_mixture_score,
mgp_mixture_quantiles; SMGP.predict_cdf / predict_quantiles / predict_crps / crps) against the
float64 statement tests/mixture_score_ref.py.

Criteria (the project's 1e-4 gate; a float32 evaluation of the same formulas stays inside each):
  cdf, sf    relative error <= 1e-4 wherever the reference is >= 1e-30; below that the output
             lies in [0, 1e-29]
  crps       normwise <= 1e-4, and per point |err| <= 1e-5 * sum_i w_i A(Y - mu_i, s_i^2), the
             size of the positive terms being summed (margin over K * 2^-24); crps_sum equals
             the float64 sum of the returned values to 1e-12; two calls return the same bits
  quantiles  every output finite and (a) tail-relative residual under the float64 reference
             <= 1e-4 (|F(q) - p| / p for p <= 1/2, |SF(q) - (1 - p)| / (1 - p) above), or (b) the
             float64 root within 2 float32 ulps of q; nothing is excused another way
Every measured error is printed (`SCOREERR <quantity> <value>`); tools/bench_mixture_score.py
--errors-from collects the worst of each into profiles/mixture_score_bench.json."""
import functools

import numpy as np
import pytest
import torch

from oracle import cpu_ref as R
from tests import mixture_ref as MR
from tests import mixture_score_ref as SR
from tests.helpers import build_model, load_golden, normwise, params_from_golden, to_np

pytestmark = pytest.mark.gpu

GATE = 1e-4
LEVELS = (1e-6, 1e-3, 0.025, 0.25, 0.5, 0.75, 0.975, 0.999, 1 - 1e-6)

# (N, K, Q): N across the wave (16 points) and workgroup (64 points) edges at 4 lanes per
# point; K pads and fills every KMAX instance 1, 2, 4, 8, 16, 32; Q = 1, 3, 9
SHAPES = [(1, 1, 1), (63, 2, 3), (64, 3, 9), (65, 5, 9), (257, 8, 3), (1000, 9, 1), (64, 17, 9), (65, 32, 3),
          (257, 4, 9), (63, 16, 1)]


def _err(name, value):
    print(f"SCOREERR {name} {value:.3e}")
    return value


def _levels(Q):
    return {1: (0.5,), 3: (0.025, 0.5, 0.975), 9: LEVELS}[Q]


@functools.lru_cache(maxsize=None)
def _generic(N, K):
    """Float32 inputs, point-major [N, K]: mu ~ N(0, 5^2), s in [0.01, 1], Dirichlet(0.7)
    weights, Y = mu_k + t s_k with t ~ U(-12, 12)."""
    rng = np.random.default_rng(100 * N + K)
    f32 = lambda a: np.asarray(a, np.float32)
    s = np.exp(rng.uniform(np.log(0.01), 0.0, (N, K)))
    lik_var = f32(rng.uniform(2e-5, 8e-5, K))
    d = dict(mu_f=f32(rng.normal(0, 5, (N, K))), lik_var=lik_var, var_f=f32(s * s - lik_var[None].astype(np.float64)),
             w=f32(rng.dirichlet(np.full(K, 0.7), N)))
    k = rng.integers(0, K, N)
    s32 = SR.scales(d["var_f"], lik_var)
    d["Y"] = f32(d["mu_f"][np.arange(N), k] + rng.uniform(-12, 12, N) * s32[np.arange(N), k])
    return d


def _hard():
    """Each a way a kernel fails; (name, mu [K], s [K], w [K], Y values)."""
    return [
        # the median sits where the CDF is flat to float32 between the branches
        ("flat_between_branches", [-25.0, 25.0], [1e-3, 1e-3], [0.5, 0.5], [-25.0, -24.999, 0.0, 25.0005, 30.0]),
        ("zero_weight_far_expert", [0.0, 1.0, 1e4], [0.5, 0.3, 0.1], [0.6, 0.4, 0.0], [-2.0, 0.5, 3.0, 1e4]),
        ("identical_experts", [2.0] * 4, [0.7] * 4, [0.25] * 4, [-3.0, 2.0, 2.1, 9.0]),
        # output resolution (an ulp of 1000 is 6e-5, s / 160) limits the answer
        ("mu_near_1000", [1000.0, 1000.05], [0.01, 0.01], [0.3, 0.7], [999.9, 1000.0, 1000.03, 1000.06, 1000.2]),
    ]


def _hard_inputs(mu, s, w, Y):
    f32 = lambda a: np.asarray(a, np.float32)
    n, s2 = len(Y), np.asarray(s, np.float64) ** 2
    lik_var = f32(0.25 * s2)
    return dict(mu_f=np.tile(f32(mu), (n, 1)), var_f=np.tile(f32(s2 - lik_var.astype(np.float64)), (n, 1)),
                lik_var=lik_var, w=np.tile(f32(w), (n, 1)), Y=f32(Y))


def _dev(a, device):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=device)


def _device_inputs(d, device):
    """mu_f, var_f as expert-major [K, N] views of one NaN-filled [2, K, ld] buffer, ld > N."""
    N, K = d["mu_f"].shape
    ld = (N + 3) // 4 * 4 + 4
    buf = torch.full((2, K, ld), float("nan"), dtype=torch.float32, device=device)
    buf[0, :, :N] = _dev(d["mu_f"].T, device)
    buf[1, :, :N] = _dev(d["var_f"].T, device)
    return buf[0, :, :N], buf[1, :, :N], _dev(d["lik_var"], device), _dev(d["w"], device)


def _check_cdf(name, got, ref):
    big = ref >= 1e-30
    assert np.isfinite(got).all(), name
    rel = np.abs(got[big] - ref[big]) / ref[big]
    worst = _err(name, rel.max() if rel.size else 0.0)
    assert worst <= GATE, (name, worst)
    assert ((got[~big] >= 0) & (got[~big] <= 1e-29)).all(), name


def _check_score(d, out, tag=""):
    ref = SR.score(d["mu_f"], d["var_f"], d["lik_var"], d["w"], d["Y"])
    _check_cdf(tag + "cdf_rel", to_np(out["cdf"]), ref["cdf"])
    _check_cdf(tag + "sf_rel", to_np(out["sf"]), ref["sf"])
    got = to_np(out["crps"])
    first, _ = SR.crps_terms(d["mu_f"], d["var_f"], d["lik_var"], d["w"], d["Y"])
    assert np.isfinite(got).all()
    assert _err(tag + "crps_normwise", normwise(got, ref["crps"])) <= GATE
    assert _err(tag + "crps_point_over_first", (np.abs(got - ref["crps"]) / first).max()) <= 1e-5
    total, direct = float(out["crps_sum"].cpu()), float(out["crps"].double().sum().cpu())
    assert abs(total - direct) <= 1e-12 * abs(direct)


def _ulps(q, k):
    q = q.astype(np.float32)
    for _ in range(abs(k)):
        q = np.nextafter(q, np.float32(np.inf if k > 0 else -np.inf))
    return q.astype(np.float64)


def _check_quantiles(d, levels, got, tag="", monotone=False):
    """(a) or (b) of the module docstring for every (point, level)."""
    got = to_np(got)
    assert got.shape == (d["mu_f"].shape[0], len(levels)) and np.isfinite(got).all()
    args = (d["mu_f"], d["var_f"], d["lik_var"], d["w"], levels)
    resid = SR.tail_residual(*args, got)
    # h(y) = cdf(y) - p or (1 - p) - sf(y) increases in y: the float64 root lies in
    # [q - 2 ulp, q + 2 ulp] exactly when h changes sign over it
    _, tail, upper = SR.f32_levels(levels)
    mu, w, s = d["mu_f"].astype(np.float64), d["w"].astype(np.float64), SR.scales(d["var_f"], d["lik_var"])
    sign = np.where(upper, 1.0, -1.0)[None, :, None]

    def h(y):
        F = (w[:, None, :] * 0.5 * SR.erfc(sign * (y[:, :, None] - mu[:, None, :]) / (s[:, None, :] * SR.SQRT2))).sum(-1)
        return np.where(upper[None], tail[None] - F, F - tail[None])
    near = (h(_ulps(got, -2)) <= 0) & (h(_ulps(got, 2)) >= 0)
    ok = (resid <= GATE) | near
    _err(tag + "quantile_tail_residual_where_not_within_2ulp", np.where(near, 0.0, resid).max())
    _err(tag + "quantile_fraction_by_ulp_rule", float((near & ~(resid <= GATE)).mean()))
    assert ok.all(), (tag, np.argwhere(~ok)[:5], resid[~ok][:5])
    if monotone:
        assert (np.diff(got, axis=1) >= 0).all()


@pytest.mark.parametrize("N,K,Q", SHAPES)
def test_kernels_against_float64(device, N, K, Q):
    from modulatedgps_amd import ops
    d = _generic(N, K)
    mu_f, var_f, lik_var, w = _device_inputs(d, device)
    Y = _dev(d["Y"], device)
    out = ops.mixture_score(mu_f, var_f, lik_var, w, Y)
    assert sorted(out) == sorted(ops.SCORE_OUTPUTS)
    assert all(tuple(out[n].shape) == (N,) and out[n].dtype == torch.float32 for n in ("cdf", "sf", "crps"))
    _check_score(d, out)
    # two calls return the same bits; NULL outputs are honoured, one output at a time
    again = ops.mixture_score(mu_f, var_f, lik_var, w, Y)
    for name in ops.SCORE_OUTPUTS:
        assert torch.equal(again[name], out[name]), name
        one = ops.mixture_score(mu_f, var_f, lik_var, w, Y, want=(name,))
        assert list(one) == [name] and torch.equal(one[name], out[name]), name
    levels = _levels(Q)
    q = ops.mixture_quantiles(mu_f, var_f, lik_var, w, levels)
    assert tuple(q.shape) == (N, Q) and q.dtype == torch.float32
    _check_quantiles(d, levels, q, monotone=True)
    assert torch.equal(ops.mixture_quantiles(mu_f, var_f, lik_var, w, levels), q)


def test_quantiles_into_a_padded_output(device):
    """ldq > Q: the rows land at their stride and the padding is not written."""
    from modulatedgps_amd import ops
    N, K = 65, 5
    d = _generic(N, K)
    mu_f, var_f, lik_var, w = _device_inputs(d, device)
    buf = torch.full((N, len(LEVELS) + 3), -7.0, dtype=torch.float32, device=device)
    q = ops.mixture_quantiles(mu_f, var_f, lik_var, w, LEVELS, out=buf[:, :len(LEVELS)])
    assert q.data_ptr() == buf.data_ptr()
    assert torch.equal(q, ops.mixture_quantiles(mu_f, var_f, lik_var, w, LEVELS))
    assert (buf[:, len(LEVELS):] == -7.0).all()


@pytest.mark.parametrize("name,mu,s,w,Y", _hard(), ids=[h[0] for h in _hard()])
def test_hard_inputs(device, name, mu, s, w, Y):
    from modulatedgps_amd import ops
    d = _hard_inputs(mu, s, w, Y)
    mu_f, var_f, lik_var, wd = _device_inputs(d, device)
    out = ops.mixture_score(mu_f, var_f, lik_var, wd, _dev(d["Y"], device))
    _check_score(d, out, tag=name + "_")
    q = ops.mixture_quantiles(mu_f, var_f, lik_var, wd, LEVELS)
    _check_quantiles(d, LEVELS, q, tag=name + "_")
    assert (np.diff(to_np(q), axis=1) >= 0).all()


def test_levels_outside_the_unit_interval(device):
    """The Python layer raises before the upload; the entry itself writes NaN for such a level."""
    import ctypes
    from modulatedgps_amd import _lib, ops
    d = _generic(63, 2)
    mu_f, var_f, lik_var, w = _device_inputs(d, device)
    for bad in ([0.0], [1.0], [0.5, -0.1], [float("nan")], [1 - 1e-9]):
        with pytest.raises(ValueError):
            ops.mixture_quantiles(mu_f, var_f, lik_var, w, bad)
    lv = _dev([0.5, 0.0, 1.0, float("nan"), 0.25], device)
    q = torch.zeros(63, 5, dtype=torch.float32, device=device)
    _lib.call("mgp_mixture_quantiles", mu_f.data_ptr(), var_f.data_ptr(), mu_f.stride(0), lik_var.data_ptr(),
              w.data_ptr(), 63, 2, lv.data_ptr(), 5, q.data_ptr(), 5, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    q = to_np(q)
    assert np.isnan(q[:, 1:4]).all() and np.isfinite(q[:, [0, 4]]).all()
    assert np.array_equal(q[:, [0, 4]], to_np(ops.mixture_quantiles(mu_f, var_f, lik_var, w, [0.5, 0.25])))


def test_shards_are_bitwise_the_one_call(device):
    from modulatedgps_amd import ops
    N, K, a = 257, 8, 100
    d = _generic(N, K)
    mu_f, var_f, lik_var, w = _device_inputs(d, device)
    Y = _dev(d["Y"], device)
    full = ops.mixture_score(mu_f, var_f, lik_var, w, Y)
    fq = ops.mixture_quantiles(mu_f, var_f, lik_var, w, LEVELS)
    parts, pq = [], []
    for lo, hi in ((0, a), (a, N)):
        sl = (mu_f[:, lo:hi], var_f[:, lo:hi], lik_var, w[lo:hi].contiguous())
        parts.append(ops.mixture_score(*sl, Y[lo:hi].contiguous()))
        pq.append(ops.mixture_quantiles(*sl, LEVELS))
    for name in ("cdf", "sf", "crps"):
        assert torch.equal(torch.cat([p[name] for p in parts]), full[name]), name
    assert torch.equal(torch.cat(pq), fq)
    tot, two = float(full["crps_sum"].cpu()), sum(float(p["crps_sum"].cpu()) for p in parts)
    assert abs(two - tot) <= 1e-12 * abs(tot)


# ------------------------------------------------------------------ model level
CASES = ["case_c1", "case_demo_perturbed", "case_demo_init"]
MODEL_LEVELS = (0.05, 0.2, 0.35, 0.5, 0.65, 0.8, 0.95)


@functools.lru_cache(maxsize=None)
def _case(name):
    """The golden case, its oracle parameters and the float64 latents at X and Xtest."""
    d = load_golden(name + ".npz")
    p = params_from_golden(d)
    lat = {key: R._layer_f(p.pred, d[key]) + R._layer_f(p.assign, d[key]) for key in ("X", "Xtest")}
    return d, p, lat


_MODELS = {}


def _model(name, device):
    if name not in _MODELS:
        _MODELS[name] = build_model(_case(name)[1], device)
    return _MODELS[name]


def _probability_residual(lat, lik_var, w, q):
    """max |F(q) - p| over points and levels, F the float64 mixture CDF on the latents `lat`."""
    _, tail, _ = SR.f32_levels(MODEL_LEVELS)
    return (SR.tail_residual(lat[0], lat[1], lik_var, w, MODEL_LEVELS, q) * tail[None]).max()


@pytest.mark.parametrize("S", [0, 8])
@pytest.mark.parametrize("case", CASES)
def test_model_methods_against_the_oracle_latents(device, case, S):
    """Gates: cdf and crps normwise 1e-4, quantiles by residual in probability <= 1e-4 absolute,
    against the reference on the float64 oracle latents.  The float32 conditionals set an error
    floor that contains no code under test: the reference on the device's own float32 latents
    against the reference on the oracle latents.  A case whose floor exceeds 1e-4 is gated at
    twice its floor."""
    d, p, lat = _case(case)
    model = _model(case, device)
    X, Y, Xt = d["X"], d["Y"][:, 0], d["Xtest"]
    z = d["z"][:8] if S else None
    kw = dict(noise_z=z) if S else {}
    lik_var = p.lik_variance[0]
    # cdf and crps on the training inputs
    w_ref = MR.weights(lat["X"][2], lat["X"][3], z)
    ref = SR.score(lat["X"][0], lat["X"][1], lik_var, w_ref, Y)
    dl = [to_np(t).T for t in model.conditionals(model.pred_layer.kernel._x(X))]
    model.check_linalg()
    floor = SR.score(dl[0], dl[1], lik_var, MR.weights(dl[2], dl[3], z), Y)
    N = X.shape[0]
    cdf, sf, crps = model.predict_cdf(X, Y, S, **kw), model.predict_cdf(X, Y, S, tail="upper", **kw), model.predict_crps(X, Y, S, **kw)
    for name, got in (("cdf", cdf), ("sf", sf), ("crps", crps)):
        assert got.shape == (N,) and got.dtype == np.float64 and np.isfinite(got).all()
        fl = _err(f"model_{case}_S{S}_{name}_floor", normwise(floor[name], ref[name]))
        e = _err(f"model_{case}_S{S}_{name}", normwise(got, ref[name]))
        assert e <= (GATE if fl <= GATE else 2 * fl), (name, e, fl)
    mean = model.crps(X, Y, S, **kw)
    assert isinstance(mean, float)
    assert abs(mean - crps.mean()) <= 1e-6 * crps.mean()   # the same float32 values, summed in float64
    # quantiles on the held-out inputs (no noise array of that size: S = 0 there, Philox otherwise)
    if S == 0:
        lt = lat["Xtest"]
        w_ref = MR.weights(lt[2], lt[3])
        q = model.predict_quantiles(Xt, MODEL_LEVELS)
        assert q.shape == (Xt.shape[0], len(MODEL_LEVELS)) and q.dtype == np.float64 and np.isfinite(q).all()
        assert (np.diff(q, axis=1) > 0).all()
        dt = [to_np(t).T for t in model.conditionals(model.pred_layer.kernel._x(Xt))]
        q_floor = SR.quantiles(dt[0], dt[1], lik_var, MR.weights(dt[2], dt[3]), MODEL_LEVELS)
        fl = _err(f"model_{case}_quantile_probability_floor", _probability_residual(lt, lik_var, w_ref, q_floor))
        e = _err(f"model_{case}_quantile_probability", _probability_residual(lt, lik_var, w_ref, q))
        assert e <= (GATE if fl <= GATE else 2 * fl), (e, fl)
    else:
        q = model.predict_quantiles(X, MODEL_LEVELS, S, **kw)
        w_ref = MR.weights(lat["X"][2], lat["X"][3], z)
        fl_w = MR.weights(dl[2], dl[3], z)
        q_floor = SR.quantiles(dl[0][::5], dl[1][::5], lik_var, fl_w[::5], MODEL_LEVELS)
        sub = [a[::5] for a in lat["X"]]
        fl = _err(f"model_{case}_S{S}_quantile_probability_floor", _probability_residual(sub, lik_var, w_ref[::5], q_floor))
        e = _err(f"model_{case}_S{S}_quantile_probability", _probability_residual(lat["X"], lik_var, w_ref, q))
        assert e <= (GATE if fl <= GATE else 2 * fl), (e, fl)


def test_device_twins_return_float32_device_tensors(device):
    d, _, _ = _case("case_c1")
    model = _model("case_c1", device)
    X, Y = d["X"], d["Y"]
    N = X.shape[0]
    outs = [(model.predict_cdf_device(X, Y, 3, seed=1), (N,), model.predict_cdf(X, Y, 3, seed=1)),
            (model.predict_cdf_device(X, Y, 3, seed=1, tail="upper"), (N,), model.predict_cdf(X, Y, 3, seed=1, tail="upper")),
            (model.predict_crps_device(X, Y, 3, seed=1), (N,), model.predict_crps(X, Y, 3, seed=1)),
            (model.predict_quantiles_device(X, [0.1, 0.9], 3, seed=1), (N, 2), model.predict_quantiles(X, [0.1, 0.9], 3, seed=1))]
    for t, shape, host in outs:
        assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == shape
        assert np.array_equal(to_np(t), host)
    s = model.crps_device(X, Y, 3, seed=1)
    assert s.is_cuda and s.dtype == torch.float64 and s.dim() == 0
    assert float(s.cpu()) == model.crps(X, Y, 3, seed=1)
    # tail="upper" is the survival function: with the lower tail it sums to one
    lower, upper = model.predict_cdf(X, Y), model.predict_cdf(X, Y, tail="upper")
    assert np.abs(lower + upper - 1.0).max() < 1e-6
    assert np.array_equal(upper, to_np(model._score(X, Y, 0, ("sf",))[0]["sf"]))
    with pytest.raises(ValueError):
        model.predict_cdf(X, Y, tail="both")
    for bad in ([0.0], [0.5, 1.0], [1.5], [float("nan")]):
        with pytest.raises(ValueError):
            model.predict_quantiles(X, bad)


def test_smgp_modified_inherits_the_methods_unchanged(device):
    from modulatedgps_amd.likelihoods import GaussianModified
    from modulatedgps_amd.models import SMGPModified
    d, p, _ = _case("case_c1")
    base = _model("case_c1", device)
    K = p.lik_variance.shape[1]
    mod = SMGPModified(base.likelihood.likelihood, GaussianModified(variance=np.linspace(0.3, 0.9, K)[None], device=device),
                       base.pred_layer, base.assign_layer, K=K, num_samples=p.S, num_data=p.num_data)
    X, Y = d["X"], d["Y"]
    for S, kw in ((0, {}), (8, dict(seed=5))):
        assert torch.equal(mod.predict_cdf_device(X, Y, S, **kw), base.predict_cdf_device(X, Y, S, **kw))
        assert torch.equal(mod.predict_crps_device(X, Y, S, **kw), base.predict_crps_device(X, Y, S, **kw))
        assert torch.equal(mod.predict_quantiles_device(X, MODEL_LEVELS, S, **kw),
                           base.predict_quantiles_device(X, MODEL_LEVELS, S, **kw))
        assert mod.crps(X, Y, S, **kw) == base.crps(X, Y, S, **kw)


def test_multiclass_has_no_expert_mixture(device):
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
    Y = np.zeros((64, 1))
    calls = {"predict_cdf": (X, Y), "predict_quantiles": (X, [0.5]), "predict_crps": (X, Y), "crps": (X, Y)}
    for name, args in calls.items():
        for fn in (name, name + "_device"):
            with pytest.raises(NotImplementedError, match="MultiClass"):
                getattr(model, fn)(*args)


def test_crps_sharded(device, tmp_path):
    """Two halves with n_offset / n_total add up to the one-call value; a world-size-1 process
    group gives the plain call's bits."""
    import torch.distributed as dist
    d, _, _ = _case("case_c1")
    model = _model("case_c1", device)
    X, Y = d["X"], d["Y"]
    N, h = X.shape[0], 301
    plain = model.crps(X, Y, 8, seed=9)
    two = (model.crps(X[:h], Y[:h], 8, seed=9, n_offset=0, n_total=N)
           + model.crps(X[h:], Y[h:], 8, seed=9, n_offset=h, n_total=N))
    _err("crps_halves_sum", abs(two - plain) / abs(plain))
    assert abs(two - plain) <= 1e-15 * abs(plain)
    dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        via = model.crps(X, Y, 8, seed=9, process_group=dist.group.WORLD)
        half = model.crps(X[:h], Y[:h], 8, seed=9, n_total=N, process_group=dist.group.WORLD)
    finally:
        dist.destroy_process_group()
    assert via == plain
    assert half == model.crps(X[:h], Y[:h], 8, seed=9, n_total=N)
