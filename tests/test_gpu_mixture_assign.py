"""GPU tests of the data-association entries (csrc/mixture_assign.hip:
mgp_mixture_responsibilities, mgp_mixture_modes; SMGP.predict_responsibilities / predict_labels /
predict_assignment_entropy / expert_usage / predict_modes / predict_map) against the float64
statement tests/mixture_assign_ref.py.  tests/test_mixture_assign_host.py checks, on the CPU,
the conditions the generated inputs have to meet.

Criteria (the project's 1e-4 gate, as for cdf and sf in tests/test_gpu_mixture_score.py):
  resp       relative error <= 1e-4 wherever the reference is >= 1e-30; below that the output
             lies in [0, 1e-29]; rows sum to 1 within 1e-6
  labels     equal to the reference (its two largest a_k are at least 1e-3 apart on these inputs)
  entropy    |err| <= 1e-4 (1 + |ref|)
  usage      within 1e-12 relative of the float64 sum of the returned resp, 1e-4 of the reference
  modes      count equal to the reference; for every returned mode y the float64 derivative
             changes sign over [y - h, y + h], h = POSITION_GATE min_k s_k; density within 1e-4
             relative of the float64 density at the float64 mode; decreasing density; NaN from
             count on
Every measured error is printed (`ASSIGNERR <quantity> <value>`); tools/bench_mixture_assign.py
--errors-from collects the worst of each into profiles/mixture_assign_bench.json."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import cpu_ref as R
from tests import matern_ref as MTR
from tests import mixture_assign_ref as AR
from tests.helpers import to_np

pytestmark = pytest.mark.gpu

GATE = 1e-4
UNSUPPORTED = 3
# Four times the worst |y32 - y64| / min_k s_k of the reference's float32 climb on these cases,
# 8.22e-6 (AR.F32_POSITION_ERROR, measured on the CPU; test_mixture_assign_host.py measures it
# again).  The margin covers the device's summation order and its exp and log.
POSITION_GATE = 4 * AR.F32_POSITION_ERROR


def _err(name, value):
    print(f"ASSIGNERR {name} {value:.3e}")
    return value


def _dev(a, device, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=device)


def _device_inputs(d, device):
    """mu_f, var_f as expert-major [K, N] views of one NaN-filled [2, K, ld] buffer, ld > N."""
    N, K = d["mu_f"].shape
    ld = (N + 3) // 4 * 4 + 4
    buf = torch.full((2, K, ld), float("nan"), dtype=torch.float32, device=device)
    buf[0, :, :N] = _dev(d["mu_f"].T, device)
    buf[1, :, :N] = _dev(d["var_f"].T, device)
    return buf[0, :, :N], buf[1, :, :N], _dev(d["lik_var"], device), _dev(d["w"], device)


def _bits(t):
    return t.contiguous().view(torch.int32)


# --------------------------------------------------------------------------- responsibilities
def _check_resp(d, out, tag, labels=True):
    args = (d["mu_f"], d["var_f"], d["lik_var"], d["w"], d["Y"])
    ref = AR.responsibilities(*args)
    got = to_np(out["resp"])
    assert got.shape == ref.shape and np.isfinite(got).all()
    big = ref >= 1e-30
    assert _err(tag + "resp_rel", (np.abs(got[big] - ref[big]) / ref[big]).max()) <= GATE
    assert ((got[~big] >= 0) & (got[~big] <= 1e-29)).all()
    assert _err(tag + "resp_row_sum", np.abs(got.sum(-1) - 1).max()) <= 1e-6
    if labels:
        assert np.array_equal(to_np(out["labels"]), AR.labels(*args))
    eref = AR.entropy(*args)
    assert _err(tag + "entropy", (np.abs(to_np(out["entropy"]) - eref) / (1 + np.abs(eref))).max()) <= GATE
    own = out["resp"].double().sum(0)
    use = out["usage"]
    assert use.dtype == torch.float64 and tuple(use.shape) == (ref.shape[1],)
    assert _err(tag + "usage_vs_own_resp", float(((use - own).abs() / own.abs().clamp_min(1e-300)).max().cpu())) <= 1e-12
    uref = AR.usage(*args)   # 0 for an expert of weight 0, and then 0 on the device
    assert _err(tag + "usage_rel", (np.abs(to_np(use) - uref) / np.where(uref > 0, uref, 1.0)).max()) <= GATE


@pytest.mark.parametrize("K", AR.KS)
def test_responsibilities_against_float64(device, K):
    from modulatedgps_amd import ops
    d = AR.case(K)
    mu_f, var_f, lik_var, w = _device_inputs(d, device)
    Y = _dev(d["Y"], device)
    out = ops.mixture_responsibilities(mu_f, var_f, lik_var, w, Y, want=ops.RESP_OUTPUTS)
    assert sorted(out) == sorted(ops.RESP_OUTPUTS)
    assert out["labels"].dtype == torch.int32 and out["entropy"].dtype == torch.float32
    _check_resp(d, out, f"K{K}_")
    if K == 1:
        assert (out["resp"] == 1).all() and (out["entropy"] == 0).all()
    # the default is resp alone; NULL outputs are honoured, one output at a time
    assert list(ops.mixture_responsibilities(mu_f, var_f, lik_var, w, Y)) == ["resp"]
    for name in ops.RESP_OUTPUTS:
        one = ops.mixture_responsibilities(mu_f, var_f, lik_var, w, Y, want=(name,))
        assert list(one) == [name] and torch.equal(one[name], out[name]), name


@pytest.mark.parametrize("K", AR.KS)
def test_far_tails_stay_finite(device, K):
    """Y 25 sigma from every mean: every linear-domain density has underflowed in float32."""
    from modulatedgps_amd import ops
    d = AR.far_case(K)
    mu_f, var_f, lik_var, w = _device_inputs(d, device)
    out = ops.mixture_responsibilities(mu_f, var_f, lik_var, w, _dev(d["Y"], device), want=ops.RESP_OUTPUTS)
    got = to_np(out["resp"])
    assert np.isfinite(got).all() and np.isfinite(to_np(out["entropy"])).all() and np.isfinite(to_np(out["usage"])).all()
    assert _err(f"K{K}_far_row_sum", np.abs(got.sum(-1) - 1).max()) <= 1e-6
    assert np.array_equal(to_np(out["labels"]), AR.labels(d["mu_f"], d["var_f"], d["lik_var"], d["w"], d["Y"]))
    _check_resp(d, out, f"K{K}_far_")


def _special():
    f32 = lambda a: np.asarray(a, np.float32)
    zero = dict(mu_f=f32([[0.0, 1.0, 9.0]] * 4), var_f=f32([[0.2, 0.1, 0.01]] * 4), lik_var=f32([0.05, 0.05, 0.05]),
                w=f32([[0.6, 0.4, 0.0]] * 4), Y=f32([-1.0, 0.7, 9.0, 40.0]))
    same = dict(mu_f=f32([[2.0, 2.0, 2.0]] * 3), var_f=f32([[0.3, 0.3, 0.3]] * 3), lik_var=f32([0.05, 0.05, 0.05]),
                w=f32([[0.2, 0.5, 0.3]] * 3), Y=f32([2.0, 2.5, -30.0]))
    return zero, same


def test_zero_weight_and_coincident_experts(device):
    from modulatedgps_amd import ops
    zero, same = _special()
    for d in (zero, same):
        mu_f, var_f, lik_var, w = _device_inputs(d, device)
        d["out"] = ops.mixture_responsibilities(mu_f, var_f, lik_var, w, _dev(d["Y"], device), want=ops.RESP_OUTPUTS)
        d["modes"] = ops.mixture_modes(mu_f, var_f, lik_var, w)
        _check_resp(d, d["out"], "special_", labels=d is zero)
    # a zero weight: resp exactly 0 (also at its own mean), never the label, never a start
    r = to_np(zero["out"]["resp"])
    assert (r[:, 2] == 0).all() and (to_np(zero["out"]["labels"]) != 2).all()
    modes, dens, count = (to_np(t) for t in zero["modes"])
    ref = AR.modes_climb(zero["mu_f"], zero["var_f"], zero["lik_var"], zero["w"])
    assert np.array_equal(count, [ref[0][0].size] * 4) and np.nanmax(modes) < 2.0
    # coincident experts: one mode at the common mean, resp split as w (so the label is the largest weight's)
    np.testing.assert_allclose(to_np(same["out"]["resp"]), same["w"].astype(np.float64), rtol=1e-6)
    assert np.array_equal(to_np(same["out"]["labels"]), [1, 1, 1])
    modes, dens, count = (to_np(t) for t in same["modes"])
    assert np.array_equal(count, [1, 1, 1]) and (modes[:, 0] == 2.0).all() and np.isnan(modes[:, 1:]).all()
    assert np.abs(dens[:, 0] * np.sqrt(2 * np.pi * 0.35) - 1).max() <= GATE
    # no positive weight: NaN, label -1, no mode
    none = dict(zero, w=np.zeros_like(zero["w"]))
    mu_f, var_f, lik_var, w = _device_inputs(none, device)
    out = ops.mixture_responsibilities(mu_f, var_f, lik_var, w, _dev(none["Y"], device), want=("resp", "labels", "entropy"))
    assert torch.isnan(out["resp"]).all() and torch.isnan(out["entropy"]).all() and (out["labels"] == -1).all()
    modes, dens, count = ops.mixture_modes(mu_f, var_f, lik_var, w)
    assert (count == 0).all() and torch.isnan(modes).all() and torch.isnan(dens).all()


# --------------------------------------------------------------------------- modes
def _check_modes(d, got, ref, tag):
    """got: the device's (modes, density, count) as arrays; ref: per point (modes, densities)."""
    modes, dens, count = got[0], got[1], np.asarray(got[2]).astype(int)
    N, K = d["mu_f"].shape
    assert modes.shape == (N, K) and dens.shape == (N, K) and count.shape == (N,)
    assert np.array_equal(count, [r[0].size for r in ref])
    col = np.arange(K)[None]
    live = col < count[:, None]
    assert np.isnan(modes[~live]).all() and np.isnan(dens[~live]).all()
    assert np.isfinite(modes[live]).all() and np.isfinite(dens[live]).all()
    with np.errstate(invalid="ignore"):
        assert (np.diff(dens, axis=1)[live[:, 1:]] <= 0).all()           # decreasing density
    smin = AR.scales(d["var_f"], d["lik_var"]).min(-1)
    h = POSITION_GATE * smin[:, None]
    y = np.where(live, modes, d["mu_f"][:, :1].astype(np.float64))        # a finite stand-in in the dead slots
    args = (d["mu_f"], d["var_f"], d["lik_var"], d["w"])
    below, above = AR.dp(*args, y - h), AR.dp(*args, y + h)
    assert ((below > 0) & (above < 0))[live].all(), tag
    worst_y, worst_d = 0.0, 0.0
    for n in range(N):
        c = count[n]
        o, r = np.argsort(modes[n, :c]), np.argsort(ref[n][0])
        worst_y = max(worst_y, float(np.abs(modes[n, :c][o] - ref[n][0][r]).max() / smin[n]))
        worst_d = max(worst_d, float((np.abs(dens[n, :c][o] - ref[n][1][r]) / ref[n][1][r]).max()))
    _err(tag + "mode_position_over_min_s", worst_y)
    assert _err(tag + "mode_density_rel", worst_d) <= GATE


@pytest.mark.parametrize("K", AR.KS)
def test_modes_against_float64(device, K):
    from modulatedgps_amd import ops
    d = AR.case(K)
    mu_f, var_f, lik_var, w = _device_inputs(d, device)
    modes, dens, count = ops.mixture_modes(mu_f, var_f, lik_var, w)
    assert modes.dtype == torch.float32 and dens.dtype == torch.float32 and count.dtype == torch.int32
    _check_modes(d, (to_np(modes), to_np(dens), to_np(count)), AR.case_climb(K), f"K{K}_")


# --------------------------------------------------------------------------- sharding, repeatability
@pytest.mark.parametrize("K", [3, 32])
def test_shards_are_bitwise_the_one_call_and_calls_repeat(device, K):
    from modulatedgps_amd import ops
    d = AR.case(K)
    N, a = AR.N_CASE, 500
    mu_f, var_f, lik_var, w = _device_inputs(d, device)
    Y = _dev(d["Y"], device)
    full = ops.mixture_responsibilities(mu_f, var_f, lik_var, w, Y, want=ops.RESP_OUTPUTS)
    fm = ops.mixture_modes(mu_f, var_f, lik_var, w)
    again = ops.mixture_responsibilities(mu_f, var_f, lik_var, w, Y, want=ops.RESP_OUTPUTS)
    for name in ops.RESP_OUTPUTS:
        assert torch.equal(again[name], full[name]), name
    for t, u in zip(ops.mixture_modes(mu_f, var_f, lik_var, w), fm):
        assert torch.equal(_bits(t), _bits(u))
    parts, pm = [], []
    for lo, hi in ((0, a), (a, N)):
        sl = (mu_f[:, lo:hi], var_f[:, lo:hi], lik_var, w[lo:hi].contiguous())
        parts.append(ops.mixture_responsibilities(*sl, Y[lo:hi].contiguous(), want=ops.RESP_OUTPUTS))
        pm.append(ops.mixture_modes(*sl))
    for name in ("resp", "labels", "entropy"):
        assert torch.equal(torch.cat([p[name] for p in parts]), full[name]), name
    for i in range(3):
        assert torch.equal(_bits(torch.cat([p[i] for p in pm])), _bits(fm[i])), i
    two = parts[0]["usage"] + parts[1]["usage"]
    assert _err(f"K{K}_usage_shards", float(((two - full["usage"]).abs() / full["usage"]).max().cpu())) <= 1e-12


# --------------------------------------------------------------------------- refusals
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


def test_refuses_k33_and_accepts_n0(device):
    from modulatedgps_amd import _lib
    N, K = 70, 33
    lat = torch.rand(2, K, 72, device=device) + 0.1
    lik_var, w, Y = torch.full((K,), 0.1, device=device), torch.full((N, K), 1.0 / K, device=device), torch.zeros(N, device=device)
    resp, lab, ent = _sent((N, 36), device), _sent(N, device, torch.int32, 77), _sent(N, device)
    use, ws = _sent(K, device, torch.float64), _sent(1 << 16, device, torch.uint8, 0x5A)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _refused(lambda: _lib.call("mgp_mixture_responsibilities", lat[0], lat[1], 72, lik_var, w, Y, N, K, resp, 36, lab,
                               ent, use, ws, ws.numel(), stream), [resp, lab, ent, use, ws])
    modes, dens, count = _sent((N, 36), device), _sent((N, 36), device), _sent(N, device, torch.int32, 77)
    _refused(lambda: _lib.call("mgp_mixture_modes", lat[0], lat[1], 72, lik_var, w, N, K, modes, dens, 36, count, stream),
             [modes, dens, count])
    # N = 0: accepted, nothing written
    for K0 in (3, 32):
        assert _lib.call("mgp_mixture_responsibilities", lat[0], lat[1], 72, lik_var, w, Y, 0, K0, resp, 36, lab, ent,
                         use, ws, ws.numel(), stream) is None
        assert _lib.call("mgp_mixture_modes", lat[0], lat[1], 72, lik_var, w, 0, K0, modes, dens, 36, count, stream) is None
    torch.cuda.synchronize()
    assert (resp == -12345.0).all() and (lab == 77).all() and (use == -12345.0).all() and (modes == -12345.0).all()


# --------------------------------------------------------------------------- model level
FAMILIES = [("se", "se"), ("matern32", "matern52")]


@functools.lru_cache(maxsize=None)
def _problem():
    X, Y, p = R.synthetic_problem(300, 25, 3, 2, 1.0, state="perturbed", S=3)
    z, _ = R.explicit_noise(3, 300, 3, seed=5)
    return X, Y[:, 0] if Y.ndim == 2 else Y, p, z


_MODELS = {}


def _model(families, device):
    if families not in _MODELS:
        _MODELS[families] = MTR.build_model(_problem()[2], device, families)
    return _MODELS[families]


@pytest.mark.parametrize("S", [0, 3])
@pytest.mark.parametrize("families", FAMILIES, ids=["se", "matern"])
def test_model_methods_against_the_reference_on_the_models_own_latents(device, families, S):
    """Every method against the float64 statement evaluated on the model's own float32
    conditionals and weights (so the conditionals' error is no part of the comparison): the
    kernel gates.  Labels are compared where the reference's two largest a_k are at least 1e-3
    apart (these inputs are not chosen; that is all but a few points)."""
    X, Y, p, z = _problem()
    model = _model(families, device)
    kw = dict(noise_z=z) if S else {}
    N, K = X.shape[0], 3
    mu_f, var_f, _, _ = model.conditionals(model.pred_layer.kernel._x(X))
    d = dict(mu_f=to_np(mu_f).T.astype(np.float32), var_f=to_np(var_f).T.astype(np.float32),
             lik_var=to_np(model.likelihood.likelihood.variance.reshape(-1)).astype(np.float32),
             w=to_np(model.predict_mixture_weights_device(X, S, **kw)).astype(np.float32), Y=Y.astype(np.float32))
    model.check_linalg()
    args = (d["mu_f"], d["var_f"], d["lik_var"], d["w"], d["Y"])
    tag = f"model_{families[0]}_S{S}_"
    resp, lab, ent = (model.predict_responsibilities(X, Y, S, **kw), model.predict_labels(X, Y, S, **kw),
                      model.predict_assignment_entropy(X, Y, S, **kw))
    use = model.expert_usage(X, Y, S, **kw)
    assert resp.shape == (N, K) and resp.dtype == np.float64 and lab.shape == (N,) and lab.dtype.kind == "i"
    assert ent.shape == (N,) and use.shape == (K,) and use.dtype == np.float64
    ref = AR.responsibilities(*args)
    big = ref >= 1e-30
    assert _err(tag + "resp_rel", (np.abs(resp[big] - ref[big]) / ref[big]).max()) <= GATE
    assert ((resp[~big] >= 0) & (resp[~big] <= 1e-29)).all() and np.abs(resp.sum(-1) - 1).max() <= 1e-6
    clear = AR.label_gap(*args) >= 1e-3
    assert clear.mean() >= 0.95 and np.array_equal(np.asarray(lab)[clear], AR.labels(*args)[clear])
    eref = AR.entropy(*args)
    assert _err(tag + "entropy", (np.abs(ent - eref) / (1 + np.abs(eref))).max()) <= GATE
    assert _err(tag + "usage_rel", (np.abs(use - AR.usage(*args)) / AR.usage(*args)).max()) <= GATE
    assert abs(use.sum() - N) <= 1e-5 * N
    # modes and the MAP prediction
    modes, dens, count = model.predict_modes(X, S, **kw)
    assert modes.dtype == np.float64 and count.dtype.kind == "i"
    _check_modes(d, (np.asarray(modes), np.asarray(dens), np.asarray(count)), AR.modes_climb(*args[:4]), tag)
    assert np.array_equal(model.predict_map(X, S, **kw), modes[:, 0])
    # host and device variants agree
    twins = [(model.predict_responsibilities_device(X, Y, S, **kw), torch.float32, resp),
             (model.predict_labels_device(X, Y, S, **kw), torch.int32, lab),
             (model.predict_assignment_entropy_device(X, Y, S, **kw), torch.float32, ent),
             (model.expert_usage_device(X, Y, S, **kw), torch.float64, use),
             (model.predict_map_device(X, S, **kw), torch.float32, modes[:, 0])]
    twins += [(t, dt, h) for t, dt, h in zip(model.predict_modes_device(X, S, **kw),
                                             (torch.float32, torch.float32, torch.int32), (modes, dens, count))]
    for t, dtype, host in twins:
        assert t.is_cuda and t.dtype == dtype
        assert np.array_equal(to_np(t), np.asarray(host), equal_nan=dtype != torch.int32)


def test_expert_usage_sharded_and_inherited(device, tmp_path):
    """Two shards with n_offset add up to the whole; a world-size-1 process group gives the
    plain call's bits; SMGPModified inherits the methods unchanged."""
    import torch.distributed as dist
    from modulatedgps_amd.likelihoods import GaussianModified
    from modulatedgps_amd.models import SMGPModified
    X, Y, p, _ = _problem()
    model = _model(FAMILIES[0], device)
    N, a = X.shape[0], 131
    for S, kw in ((0, {}), (3, dict(seed=9))):
        whole = model.expert_usage(X, Y, S, **kw)
        two = model.expert_usage(X[:a], Y[:a], S, n_offset=0, **kw) + model.expert_usage(X[a:], Y[a:], S, n_offset=a, **kw)
        assert _err(f"model_usage_shards_S{S}", (np.abs(two - whole) / whole).max()) <= 1e-12
    dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        via = model.expert_usage(X, Y, 3, seed=9, process_group=dist.group.WORLD)
    finally:
        dist.destroy_process_group()
    assert np.array_equal(via, model.expert_usage(X, Y, 3, seed=9))
    mod = SMGPModified(model.likelihood.likelihood, GaussianModified(variance=np.linspace(0.3, 0.9, 3)[None], device=device),
                       model.pred_layer, model.assign_layer, K=3, num_samples=p.S, num_data=p.num_data)
    assert torch.equal(mod.predict_responsibilities_device(X, Y, 3, seed=4), model.predict_responsibilities_device(X, Y, 3, seed=4))
    for t, u in zip(mod.predict_modes_device(X), model.predict_modes_device(X)):
        assert torch.equal(_bits(t), _bits(u))


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
    calls = {"predict_responsibilities": (X, Y), "predict_labels": (X, Y), "predict_assignment_entropy": (X, Y),
             "expert_usage": (X, Y), "predict_modes": (X,), "predict_map": (X,)}
    for name, args in calls.items():
        for fn in (name, name + "_device"):
            with pytest.raises(NotImplementedError, match="MultiClass"):
                getattr(model, fn)(*args)
