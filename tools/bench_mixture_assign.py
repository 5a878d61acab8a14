"""Timing of the data-association kernels (csrc/mixture_assign.hip) against the same formulas
composed from PyTorch-ROCm float32 ops on the same inputs -- the lines a user would otherwise write:
  ops.mixture_responsibilities  vs  log terms, torch.logsumexp, exp, argmax and a float64 column sum
  ops.mixture_modes             vs  a fixed count of plain mean-shift steps (MEAN_SHIFT_STEPS, in the
                                    log domain via softmax) from the same starts, without the merge
                                    and the ordering
at N = 65536, K = 8 and at the demo shape N = 1500, K = 3.  HIP events, 3 warm-up calls, median of
10 timed calls, the candidates' calls taken in turn, one process.  No speed figure is a condition.
The worst errors against float64 (torch float64 on the device: the responsibilities and entropy
directly; each returned mode polished by float64 Newton steps on p') are recorded beside the
times, and the source of the mode-position gate of tests/test_gpu_mixture_assign.py.
Usage: python tools/bench_mixture_assign.py [--N 65536 --K 8] [--errors-from pytest.log]
           [--out profiles/mixture_assign_bench.json]
--errors-from: a log of `pytest -s tests/test_gpu_mixture_assign.py`; the worst of each
`ASSIGNERR <quantity> <value>` line it printed is recorded as worst_errors."""
import argparse
import json
import math
import os
import re
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modulatedgps_amd import ops  # noqa: E402

MEAN_SHIFT_STEPS = 100
# tests/mixture_assign_ref.py F32_POSITION_ERROR: the worst |y32 - y64| / min_k s_k of the float32
# climb on the test cases, measured on the CPU; the position gate is four times this
F32_POSITION_ERROR = 8.22e-6


def timeit_all(fns, warmup=3, reps=10):
    """{name: {median, min}} of the calls in `fns`, their timed repetitions taken in turn
    (a, b, a, b, ...) so that a drift of the machine falls on all of them alike."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts[name].append(e0.elapsed_time(e1))
    return {name: {"median": float(np.median(t)), "min": float(np.min(t))} for name, t in ts.items()}


def torch_responsibilities(mu_f, var_f, lik_var, w, Y, dtype=torch.float32):
    """resp, labels, entropy, usage with torch kernels in `dtype`; latents expert-major [K, N]."""
    mf, s2, w, Y = mu_f.t().to(dtype), (var_f.t().to(dtype) + lik_var[None].to(dtype)), w.to(dtype), Y.to(dtype)
    a = torch.log(w) - 0.5 * torch.log(s2) - 0.5 * (Y[:, None] - mf) ** 2 / s2
    lse = torch.logsumexp(a, -1)
    resp = torch.exp(a - lse[:, None])
    ent = lse - torch.where(resp == 0, torch.zeros_like(a), resp * a).sum(-1)
    return resp, a.argmax(-1), ent, resp.double().sum(0)


def torch_mean_shift(mu_f, var_f, lik_var, w, steps=MEAN_SHIFT_STEPS):
    """[N, K]: `steps` plain mean-shift steps from every expert mean, float32."""
    mf, s2 = mu_f.t(), var_f.t() + lik_var[None]
    lc = (torch.log(w) - 0.5 * torch.log(s2))[:, None, :]
    inv = (1.0 / s2)[:, None, :]
    y = mf.clone()
    for _ in range(steps):
        d = mf[:, None, :] - y[:, :, None]
        r = torch.softmax(lc - 0.5 * d * d * inv, -1) * inv
        y = (r * mf[:, None, :]).sum(-1) / r.sum(-1)
    return y


def polish_f64(mu_f, var_f, lik_var, w, y, steps=6):
    """(y64, density at y64, min_k s_k): float64 Newton steps on p' from the returned modes y [N, K]
    (NaN slots stay NaN)."""
    mf, s2 = mu_f.t().double(), var_f.t().double() + lik_var[None].double()
    lc = (torch.log(w.double()) - 0.5 * torch.log(s2))[:, None, :]
    inv = (1.0 / s2)[:, None, :]
    y = y.double()
    for it in range(steps + 1):
        d = mf[:, None, :] - y[:, :, None]
        c = lc - 0.5 * d * d * inv
        mx = c.amax(-1, keepdim=True)
        u = torch.exp(c - mx)
        if it == steps:
            return y, torch.exp(mx[..., 0]) * u.sum(-1) / math.sqrt(2 * math.pi), s2.sqrt().amin(-1)
        ui = u * inv
        y = y - (ui * d).sum(-1) / (ui * (inv * d * d - 1)).sum(-1)


def worst_errors(path):
    worst = {}
    for name, val in re.findall(r"\bASSIGNERR (\S+) (\S+)$", open(path).read(), flags=re.M):
        worst[name] = max(worst.get(name, 0.0), float(val))
    return worst


def bench_shape(N, K, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    lat = ops.padded(2 * K, N, dev)
    mu_f, var_f = lat[:K], lat[K:]
    mu_f.copy_(2.0 * torch.randn(K, N, device=dev, generator=g))
    s2 = torch.exp(2.0 * (-1.0 + 0.7 * torch.randn(K, N, device=dev, generator=g)))
    lik_var = 0.3 * s2.amin(1)
    var_f.copy_(s2 - lik_var[:, None])
    w = torch.distributions.Dirichlet(torch.ones(K, device=dev)).sample((N,)).contiguous()
    pick = torch.randint(0, K, (N,), device=dev, generator=g)
    cols = torch.arange(N, device=dev)
    t = 8.0 * torch.rand(N, device=dev, generator=g) - 4.0
    Y = (mu_f[pick, cols] + t * torch.sqrt(var_f[pick, cols] + lik_var[pick])).contiguous()
    ws = torch.empty(max(int(ops._lib.load().mgp_mixture_responsibilities_workspace_bytes(N, K)), 16),
                     dtype=torch.uint8, device=dev)
    out = ops.mixture_responsibilities(mu_f, var_f, lik_var, w, Y, want=ops.RESP_OUTPUTS, workspace=ws)
    modes, dens, count = ops.mixture_modes(mu_f, var_f, lik_var, w)
    # errors against float64
    r64, l64, e64, u64 = torch_responsibilities(mu_f, var_f, lik_var, w, Y, torch.float64)
    big = r64 >= 1e-30
    y64, d64, smin = polish_f64(mu_f, var_f, lik_var, w, modes)
    live = ~torch.isnan(modes)
    err = {"resp_rel_where_ref_ge_1e-30": float(((out["resp"].double() - r64).abs() / r64)[big].max()),
           "resp_row_sum": float((out["resp"].double().sum(-1) - 1).abs().max()),
           "labels_differing": int((out["labels"].long() != l64).sum()),
           "entropy_over_1_plus_ref": float(((out["entropy"].double() - e64).abs() / (1 + e64.abs())).max()),
           "usage_rel": float(((out["usage"] - u64).abs() / u64).max()),
           "mode_position_over_min_s": float(((modes.double() - y64).abs() / smin[:, None])[live].max()),
           "mode_density_rel": float(((dens.double() - d64).abs() / d64)[live].max())}
    res ={"N": N, "K": K, "mean_modes_per_point": float(count.double().mean()), "max_modes": int(count.max())}
    res.update(timeit_all({
        "mixture_responsibilities_ms": lambda: ops.mixture_responsibilities(mu_f, var_f, lik_var, w, Y, want=ops.RESP_OUTPUTS,
                                                                            workspace=ws, out=out),
        "torch_f32_responsibilities_composition_ms": lambda: torch_responsibilities(mu_f, var_f, lik_var, w, Y),
        "mixture_modes_ms": lambda: ops.mixture_modes(mu_f, var_f, lik_var, w),
        "torch_f32_mean_shift_ms": lambda: torch_mean_shift(mu_f, var_f, lik_var, w)}))
    res["torch_mean_shift_steps"] = MEAN_SHIFT_STEPS
    res["responsibilities_speedup_vs_torch"] = (res["torch_f32_responsibilities_composition_ms"]["median"]
                                                / res["mixture_responsibilities_ms"]["median"])
    res["modes_speedup_vs_torch"] = res["torch_f32_mean_shift_ms"]["median"] / res["mixture_modes_ms"]["median"]
    res["errors_vs_float64"] = err
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=65536)
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--errors-from", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"large": bench_shape(a.N, a.K, dev), "demo": bench_shape(1500, 3, dev),
           "method": "HIP events, 3 warm-ups, median of 10, candidates taken in turn, one process",
           "baselines": "torch float32 compositions of the same formulas; the modes baseline is "
                        f"{MEAN_SHIFT_STEPS} plain mean-shift steps from the same starts, without merge and ordering",
           "mode_position_gate": {"f32_climb_position_error_over_min_s": F32_POSITION_ERROR,
                                  "gate_over_min_s": 4 * F32_POSITION_ERROR,
                                  "source": "tests/mixture_assign_ref.py f32_position_error, measured on the CPU"}}
    if a.errors_from:
        res["worst_errors"] = worst_errors(a.errors_from)
        res["worst_errors_gate"] = 1e-4
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
