"""GPU tests of the mixture predictive (csrc/mixture.hip: mgp_mixture_predict,
mgp_mixture_density_grid; SMGP.predict_log_density and its siblings) against the float64
statement tests/mixture_ref.py.

Gate: the project's own, 1e-4 normwise (tests/test_gpu_api.py), on each of
weights, log_density, mix_mean, mix_var and density; the mean log density within
1e-4 * mean|log_density_ref| (normalised by the mean magnitude, so a mean near zero cannot
make it unreachable).  No point is left out of any comparison.  A float32 numpy evaluation
of the same formula sits at 6e-8 .. 2.5e-7 normwise on these inputs and golden latents
perturbed by 1e-5 normwise at 2e-6, so the gate has three orders of room.  Every measured
error is printed (`MIXERR <quantity> <value>`); tools/bench_mixture_predict.py --errors-from
collects the worst of each into profiles/mixture_predict_bench.json."""
import functools

import numpy as np
import pytest
import torch

from oracle import cpu_ref as R
from tests import mixture_ref as MR
from tests.helpers import build_model, load_golden, normwise, params_from_golden, to_np

pytestmark = pytest.mark.gpu

GATE = 1e-4
PER_POINT = ("weights", "mix_mean", "mix_var", "log_density")

# (N, K, S, G): N across block (64 points) and wave (16 points) boundaries; S = 0, below,
# equal to and not a multiple of the 4 lanes of a point; K across the KMAX steps 1, 2, 4, 8,
# 16, 32; G = 1 and G across the grid kernel's 32 / 64 threads per point
SHAPES = [(1, 1, 0, 1), (65, 3, 1, 7), (257, 3, 25, 33), (130, 16, 5, 64), (64, 17, 3, 5), (1000, 32, 2, 3),
          (37, 2, 4, 2), (100, 7, 8, 129)]


def _gate(name, got, ref):
    e = normwise(got, ref)
    print(f"MIXERR {name} {e:.3e}")
    assert np.isfinite(np.asarray(got)).all(), name
    assert e < GATE, (name, e)
    return e


def _gate_mean(got, ld_ref):
    d = abs(got - ld_ref.mean()) / np.abs(ld_ref).mean()
    print(f"MIXERR mean_log_density {d:.3e}")
    assert np.isfinite(got) and d <= GATE, d


@functools.lru_cache(maxsize=None)
def _synthetic(N, K, S, G):
    """Float32 latents (point-major [N, K]), Y, explicit z and the grid of one shape."""
    rng = np.random.default_rng(1000 * N + 10 * K + S)
    f32 = lambda a: np.asarray(a, np.float32)
    logu = lambda lo, hi, shape: np.exp(rng.uniform(np.log(lo), np.log(hi), shape))
    d = dict(mu_f=f32(rng.normal(0, 3, (N, K))), var_f=f32(logu(1e-4, 1, (N, K))), lik_var=f32(logu(1e-3, 1, K)),
             mu_a=f32(rng.uniform(-15, 15, (N, K))), var_a=f32(logu(1e-4, 3, (N, K))))
    # Y within +-20 predictive sigma of a random expert; the first points sit at the ends
    k = rng.integers(0, K, N)
    t = rng.uniform(-20, 20, N)
    t[:2] = (20.0, -20.0)[:min(N, 2)]
    s2 = d["var_f"].astype(np.float64) + d["lik_var"].astype(np.float64)[None]
    d["Y"] = f32(d["mu_f"][np.arange(N), k] + t * np.sqrt(s2[np.arange(N), k]))
    d["z"] = f32(rng.normal(size=(S, N, K)))
    d["y_grid"] = f32(np.linspace(-6, 6, G)) if G > 1 else f32([0.5])
    return d


def _device_latents(d, device):
    """mu_f, var_f, mu_a, var_a as expert-major [K, N] views of one [4, K, ld] buffer, ld > N."""
    N, K = d["mu_f"].shape
    ld = (N + 3) // 4 * 4 + 4
    buf = torch.full((4, K, ld), float("nan"), dtype=torch.float32, device=device)
    for i, name in enumerate(("mu_f", "var_f", "mu_a", "var_a")):
        buf[i, :, :N] = torch.as_tensor(d[name].T.copy(), device=device)
    return [buf[i, :, :N] for i in range(4)]


def _dev(a, device):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=device)


@pytest.mark.parametrize("mode", ["explicit", "philox"])
@pytest.mark.parametrize("N,K,S,G", SHAPES)
def test_kernel_against_float64(device, N, K, S, G, mode):
    from modulatedgps_amd import ops
    d = _synthetic(N, K, S, G)
    lat = _device_latents(d, device)
    lik_var, Y, grid = _dev(d["lik_var"], device), _dev(d["Y"], device), _dev(d["y_grid"], device)
    if mode == "explicit":
        kw = dict(noise_z=_dev(d["z"], device) if S else None)
        z = d["z"]
    else:
        kw = dict(seed=0x1234567890ABCDEF, n_offset=1000003)
        z = to_np(ops.philox_noise(kw["seed"], kw["n_offset"], N, K, S, device, want_u=False)[0]) if S else None
    out = ops.mixture_predict(*lat, lik_var, S, Y=Y, **kw)
    dens = ops.mixture_density_grid(lat[0], lat[1], lik_var, out["weights"], grid)
    ref = MR.predict(d["mu_f"], d["var_f"], d["mu_a"], d["var_a"], d["lik_var"], Y=d["Y"], z=z, y_grid=d["y_grid"])
    for name in PER_POINT:
        assert tuple(out[name].shape) == ref[name].shape
        _gate(name, to_np(out[name]), ref[name])
    assert tuple(dens.shape) == (N, G)
    _gate("density", to_np(dens), ref["density"])
    _gate_mean(float(out["log_density_sum"].cpu()) / N, ref["log_density"])
    # NULL outputs are honoured: one output at a time, bitwise the all-outputs call
    for name in ops.MIXTURE_OUTPUTS:
        one = ops.mixture_predict(*lat, lik_var, S, Y=Y, want=(name,), **kw)
        assert list(one) == [name] and torch.equal(one[name], out[name]), name
    # without Y: the weights and moments alone, bitwise the same
    noy = ops.mixture_predict(*lat, lik_var, S, **kw)
    assert sorted(noy) == ["mix_mean", "mix_var", "weights"]
    assert all(torch.equal(noy[n], out[n]) for n in noy)


def test_philox_shards_are_bitwise_the_one_call(device):
    """N = 257 in one call and as the halves [0, 128), [128, 257) with n_offset 0 and 128."""
    from modulatedgps_amd import ops
    N, K, S = 257, 3, 25
    d = _synthetic(N, K, S, 33)
    lat = _device_latents(d, device)
    lik_var, Y = _dev(d["lik_var"], device), _dev(d["Y"], device)
    full = ops.mixture_predict(*lat, lik_var, S, Y=Y, seed=77)
    parts = [ops.mixture_predict(*[t[:, lo:hi] for t in lat], lik_var, S, Y=Y[lo:hi].contiguous(), seed=77,
                                 n_offset=lo) for lo, hi in ((0, 128), (128, 257))]
    for name in PER_POINT:
        assert torch.equal(torch.cat([p[name] for p in parts]), full[name]), name
    # 257 float64 terms regrouped: at most N * 2.2e-16 relative to the sum of magnitudes
    tot = float(full["log_density_sum"].cpu())
    two = sum(float(p["log_density_sum"].cpu()) for p in parts)
    print(f"MIXERR shard_sum {abs(two - tot) / abs(tot):.3e}")
    assert abs(two - tot) <= 1e-12 * abs(tot)
    assert tot == pytest.approx(float(full["log_density"].double().sum().cpu()), rel=1e-12)


def test_grid_density_is_the_exponential_of_log_density(device):
    """log(density[:, g]) equals log_density for Y == y_grid[g].  Inputs keep every value
    inside float32's range, so that no logarithm of an underflowed density is taken:
    s2 >= 1 and |y - mu_f| <= 9 bound the exponent by 81 / 2 (+ the log weight, >= -30)."""
    from modulatedgps_amd import ops
    N, K, S, G = 130, 5, 3, 9
    rng = np.random.default_rng(3)
    f32 = lambda a: np.asarray(a, np.float32)
    mu_f, var_f = f32(np.clip(rng.normal(0, 3, (N, K)), -6, 6)), f32(rng.uniform(0.5, 1, (N, K)))
    mu_a, var_a = f32(rng.uniform(-15, 15, (N, K))), f32(rng.uniform(1e-4, 3, (N, K)))
    d = dict(mu_f=mu_f, var_f=var_f, mu_a=mu_a, var_a=var_a)
    lat = _device_latents(d, device)
    lik_var, z = _dev(rng.uniform(0.5, 1, K), device), _dev(rng.normal(size=(S, N, K)), device)
    grid = np.linspace(-3, 3, G)
    w = ops.mixture_predict(*lat, lik_var, S, noise_z=z, want=("weights",))["weights"]
    dens = to_np(ops.mixture_density_grid(lat[0], lat[1], lik_var, w, _dev(grid, device)))
    assert (dens > 0).all()
    for g in range(G):
        Y = torch.full((N,), float(np.float32(grid[g])), dtype=torch.float32, device=device)
        ld = ops.mixture_predict(*lat, lik_var, S, Y=Y, noise_z=z, want=("log_density",))["log_density"]
        _gate("log_of_density", np.log(dens[:, g]), to_np(ld))


# ------------------------------------------------------------------ model level
CASES = ["case_c1", "case_demo_perturbed", "case_demo_init"]


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


@pytest.mark.parametrize("S", [0, 8])
@pytest.mark.parametrize("case", CASES)
def test_model_methods_against_the_oracle_latents(device, case, S):
    d, p, lat = _case(case)
    model = _model(case, device)
    X, Y = d["X"], d["Y"][:, 0]
    grid = np.linspace(-3, 3, 33)
    z = d["z"][:8] if S else None
    kw = dict(noise_z=z) if S else {}
    ref = MR.predict(*lat["X"], p.lik_variance[0], Y=Y, z=z, y_grid=grid)
    N, K = lat["X"][0].shape
    w = model.predict_mixture_weights(X, S, **kw)
    assert w.shape == (N, K) and w.dtype == np.float64
    _gate("weights", w, ref["weights"])
    m, v = model.predict_mixture_mean_and_var(X, S, **kw)
    assert m.shape == (N, 1) and v.shape == (N, 1)
    if case == "case_demo_init":   # its mean is identically zero: no normwise denominator
        assert np.abs(ref["mix_mean"]).max() == 0 and np.abs(m).max() < 1e-6
    else:
        _gate("mix_mean", m[:, 0], ref["mix_mean"])
    _gate("mix_var", v[:, 0], ref["mix_var"])
    ld = model.predict_log_density(X, Y, S, **kw)
    assert ld.shape == (N,)
    _gate("log_density", ld, ref["log_density"])
    lpd = model.log_predictive_density(X, Y, S, **kw)
    assert isinstance(lpd, float)
    _gate_mean(lpd, ref["log_density"])
    dens = model.predict_density(X, grid, S, **kw)
    assert dens.shape == (N, 33)
    _gate("density", dens, ref["density"])
    if S == 0:
        # held-out inputs; the plug-in weights are predict_assign
        rt = MR.predict(*lat["Xtest"], p.lik_variance[0], y_grid=grid)
        _gate("density", model.predict_density(d["Xtest"], grid), rt["density"])
        wt = model.predict_mixture_weights(d["Xtest"])
        _gate("weights", wt, d["predict_assign"])
        _gate("weights", wt, to_np(model.predict_assign(d["Xtest"])))


def test_device_twins_return_float32_device_tensors(device):
    d, p, _ = _case("case_c1")
    model = _model("case_c1", device)
    X, Y, grid = d["X"], d["Y"], np.linspace(-3, 3, 5)
    N, K = X.shape[0], p.lik_variance.shape[1]
    outs = [(model.predict_mixture_weights_device(X, 3, seed=1), (N, K), model.predict_mixture_weights(X, 3, seed=1)),
            (model.predict_log_density_device(X, Y, 3, seed=1), (N,), model.predict_log_density(X, Y, 3, seed=1)),
            (model.predict_density_device(X, grid, 3, seed=1), (N, 5), model.predict_density(X, grid, 3, seed=1))]
    outs += list(zip(model.predict_mixture_mean_and_var_device(X, 3, seed=1), [(N, 1)] * 2,
                     model.predict_mixture_mean_and_var(X, 3, seed=1)))
    for t, shape, host in outs:
        assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == shape
        assert np.array_equal(to_np(t), host)
    s = model.log_predictive_density_device(X, Y, 3, seed=1)
    assert s.is_cuda and s.dtype == torch.float64 and s.dim() == 0
    assert float(s.cpu()) == model.log_predictive_density(X, Y, 3, seed=1)
    with pytest.raises(ValueError):
        model.predict_density_device(X, grid[:, None])


def test_philox_seeds(device):
    """Equal seeds give bitwise equal results; seed=None advances the model's key stream."""
    d, _, _ = _case("case_demo_perturbed")
    model = _model("case_demo_perturbed", device)
    X, Y = d["X"], d["Y"]
    a, b = (model.predict_log_density_device(X, Y, 8, seed=42) for _ in range(2))
    assert torch.equal(a, b)
    c, e = (model.predict_log_density_device(X, Y, 8) for _ in range(2))
    assert not torch.equal(c, e) and not torch.equal(a, c)
    draws = model._draws
    model.predict_log_density_device(X, Y, 0)            # S = 0 draws nothing
    model.predict_log_density_device(X, Y, 8, seed=42)   # nor does an explicit seed
    assert model._draws == draws


def test_smgp_modified_inherits_the_methods_unchanged(device):
    """SMGPModified's assign likelihood is a training device only: the same layers give
    bitwise the same mixture predictive."""
    from modulatedgps_amd.likelihoods import GaussianModified
    from modulatedgps_amd.models import SMGPModified
    d, p, _ = _case("case_c1")
    base = _model("case_c1", device)
    K = p.lik_variance.shape[1]
    mod = SMGPModified(base.likelihood.likelihood, GaussianModified(variance=np.linspace(0.3, 0.9, K)[None], device=device),
                       base.pred_layer, base.assign_layer, K=K, num_samples=p.S, num_data=p.num_data)
    X, Y, grid = d["X"], d["Y"], np.linspace(-3, 3, 33)
    for S, kw in ((0, {}), (8, dict(seed=5))):
        assert torch.equal(mod.predict_mixture_weights_device(X, S, **kw), base.predict_mixture_weights_device(X, S, **kw))
        assert torch.equal(mod.predict_log_density_device(X, Y, S, **kw), base.predict_log_density_device(X, Y, S, **kw))
        assert torch.equal(mod.predict_density_device(X, grid, S, **kw), base.predict_density_device(X, grid, S, **kw))
        for a, b in zip(mod.predict_mixture_mean_and_var_device(X, S, **kw),
                        base.predict_mixture_mean_and_var_device(X, S, **kw)):
            assert torch.equal(a, b)
        assert mod.log_predictive_density(X, Y, S, **kw) == base.log_predictive_density(X, Y, S, **kw)


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
    Y, grid = np.zeros((64, 1)), np.linspace(-1, 1, 3)
    calls = {"predict_mixture_weights": (X,), "predict_mixture_mean_and_var": (X,), "predict_log_density": (X, Y),
             "predict_density": (X, grid), "log_predictive_density": (X, Y)}
    for name, args in calls.items():
        for fn in (name, name + "_device"):
            with pytest.raises(NotImplementedError, match="MultiClass"):
                getattr(model, fn)(*args)


def test_log_predictive_density_sharded(device, tmp_path):
    """A world-size-1 process group equals the plain call; two halves with n_offset / n_total
    add up to the one-call value."""
    import torch.distributed as dist
    d, _, _ = _case("case_c1")
    model = _model("case_c1", device)
    X, Y = d["X"], d["Y"]
    N, h = X.shape[0], 301
    plain = model.log_predictive_density(X, Y, 8, seed=9)
    two = (model.log_predictive_density(X[:h], Y[:h], 8, seed=9, n_offset=0, n_total=N)
           + model.log_predictive_density(X[h:], Y[h:], 8, seed=9, n_offset=h, n_total=N))
    print(f"MIXERR halves_sum {abs(two - plain) / abs(plain):.3e}")
    assert abs(two - plain) <= 1e-12 * abs(plain)
    dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        via = model.log_predictive_density(X, Y, 8, seed=9, process_group=dist.group.WORLD)
        half = model.log_predictive_density(X[:h], Y[:h], 8, seed=9, n_total=N, process_group=dist.group.WORLD)
    finally:
        dist.destroy_process_group()
    assert via == plain
    assert half == model.log_predictive_density(X[:h], Y[:h], 8, seed=9, n_total=N)
