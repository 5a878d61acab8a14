"""Timing of the mixture scores (csrc/mixture_score.hip) against the same formulas composed
from PyTorch-ROCm float32 ops on the same inputs -- the lines a user would otherwise write:
  ops.mixture_score      vs  torch.special.erfc sums and a K x K broadcast for the CRPS pair term
  ops.mixture_quantiles  vs  a fixed 40-step bisection of the tail probability from the same bracket
at N = 65536, K = 8, Q = 9 and at the demo shape N = 1500, K = 3.  HIP events, 3 warm-up calls,
median of 10 timed calls, the candidates' calls taken in turn, one process.  Inputs are about
6 MB at the large shape: the kernels are bound by erfc / exp, not by HBM, so no HBM fraction is
stated.  The condition is that each fused call is faster than its composition at the large shape.
Usage: python tools/bench_mixture_score.py [--N 65536 --K 8 --Q 9] [--errors-from pytest.log]
           [--kernel-stats kernel_stats.csv] [--out profiles/mixture_score_bench.json]
--errors-from: a log of `pytest -s tests/test_gpu_mixture_score.py`; the worst of each
`SCOREERR <quantity> <value>` line it printed is recorded as worst_errors.
--kernel-stats: the kernel statistics CSV of a kernel trace of this tool, taken in a run of its
own (`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/bench_mixture_score.py`);
the kernels' own times are recorded as kernel_alone_us (KMAX = 8: the large shape, 4: the demo's)."""
import argparse
import csv
import json
import math
import os
import re
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modulatedgps_amd import ops  # noqa: E402

LEVELS9 = (1e-6, 1e-3, 0.025, 0.25, 0.5, 0.75, 0.975, 0.999, 1 - 1e-6)
# the compiler's resource-usage remarks (-Rpass-analysis=kernel-resource-usage), KMAX = 1 .. 32
VGPRS = {"mixture_score_kernel": [18, 23, 26, 40, 78, 126], "mixture_quantiles_kernel": [27, 33, 41, 57, 75, 123],
         "scratch_bytes": 0}


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


def _A(m, v):
    return m * torch.erf(m / torch.sqrt(2.0 * v)) + torch.sqrt(2.0 * v / math.pi) * torch.exp(-m * m / (2.0 * v))


def torch_score(mu_f, var_f, lik_var, w, Y):
    """cdf, sf, crps and its float64 sum with torch float32 kernels; latents expert-major [K, N]."""
    mf, s2 = mu_f.t(), var_f.t() + lik_var[None]
    t = (Y[:, None] - mf) / torch.sqrt(s2) * math.sqrt(0.5)
    cdf = (w * 0.5 * torch.special.erfc(-t)).sum(-1)
    sf = (w * 0.5 * torch.special.erfc(t)).sum(-1)
    first = (w * _A(Y[:, None] - mf, s2)).sum(-1)
    pair = (w[:, :, None] * w[:, None, :] * _A(mf[:, :, None] - mf[:, None, :], s2[:, :, None] + s2[:, None, :]))
    crps = first - 0.5 * pair.sum((-1, -2))
    return cdf, sf, crps, crps.double().sum()


def torch_quantiles(mu_f, var_f, lik_var, w, levels, steps=40):
    """[N, Q] by `steps` bisections of the tail probability from the kernel's bracket."""
    mf, s = mu_f.t(), torch.sqrt(var_f.t() + lik_var[None])
    upper = levels > 0.5
    pt = torch.where(upper, 1.0 - levels, levels)
    zp = torch.special.ndtri(pt) * torch.where(upper, -1.0, 1.0)
    e = mf[:, None, :] + s[:, None, :] * zp[None, :, None]
    lo, hi, smax = e.amin(-1), e.amax(-1), s.amax(-1)[:, None]
    a, b = lo - 4e-6 * (lo.abs() + smax), hi + 4e-6 * (hi.abs() + smax)
    r = (math.sqrt(0.5) / s)[:, None, :] * torch.where(upper, 1.0, -1.0)[None, :, None]
    for _ in range(steps):
        y = 0.5 * (a + b)
        F = (w[:, None, :] * 0.5 * torch.special.erfc((y[:, :, None] - mf[:, None, :]) * r)).sum(-1)
        neg = torch.where(upper[None], pt[None] - F, F - pt[None]) < 0
        a, b = torch.where(neg, y, a), torch.where(neg, b, y)
    return 0.5 * (a + b)


def worst_errors(path):
    worst = {}
    for name, val in re.findall(r"\bSCOREERR (\S+) (\S+)$", open(path).read(), flags=re.M):
        worst[name] = max(worst.get(name, 0.0), float(val))
    return worst


def kernel_alone(path):
    out = {}
    for row in csv.DictReader(open(path)):
        m = re.search(r"mixscore::(\w+<\d+>|\w+)\(", row["Name"])
        if m:
            out[m.group(1)] = {"calls": int(row["Calls"]), "average": float(row["AverageNs"]) / 1e3,
                               "min": float(row["MinNs"]) / 1e3}
    return out


def bench_shape(N, K, Q, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    rand = lambda *shape: torch.rand(*shape, device=dev, generator=g)
    lat = ops.padded(2 * K, N, dev)
    mu_f, var_f = lat[:K], lat[K:]
    mu_f.copy_(5.0 * torch.randn(K, N, device=dev, generator=g))
    lik_var = 2e-5 + 6e-5 * rand(K)
    var_f.copy_(torch.exp(math.log(1e-4) * rand(K, N)) - lik_var[:, None])   # s in [0.01, 1]
    w = torch.distributions.Dirichlet(torch.full((K,), 0.7, device=dev)).sample((N,)).contiguous()
    pick = torch.randint(0, K, (N,), device=dev, generator=g)
    cols = torch.arange(N, device=dev)
    Y = (mu_f[pick, cols] + (8.0 * rand(N) - 4.0) * torch.sqrt(var_f[pick, cols] + lik_var[pick])).contiguous()
    levels = list(LEVELS9[:Q]) if Q <= 9 else list(np.linspace(0.01, 0.99, Q))
    lv = torch.tensor(levels, dtype=torch.float32, device=dev)
    ws = torch.empty(max(int(ops._lib.load().mgp_mixture_score_workspace_bytes(N, K)), 16), dtype=torch.uint8,
                     device=dev)
    out = ops.mixture_score(mu_f, var_f, lik_var, w, Y, workspace=ws)
    q = ops.mixture_quantiles(mu_f, var_f, lik_var, w, levels)
    ref = torch_score(mu_f, var_f, lik_var, w, Y)
    nw = lambda x, r: float((x.double() - r.double()).norm() / r.double().norm())
    diff = {n: nw(out[n], r) for n, r in zip(ops.SCORE_OUTPUTS, ref)}
    diff["quantiles_vs_40_bisections"] = nw(q, torch_quantiles(mu_f, var_f, lik_var, w, lv))
    res = {"N": N, "K": K, "Q": Q}
    res.update(timeit_all({
        "mixture_score_ms": lambda: ops.mixture_score(mu_f, var_f, lik_var, w, Y, workspace=ws, out=out),
        "torch_f32_score_composition_ms": lambda: torch_score(mu_f, var_f, lik_var, w, Y),
        "mixture_quantiles_ms": lambda: ops.mixture_quantiles(mu_f, var_f, lik_var, w, levels, out=q),
        "torch_f32_bisection40_ms": lambda: torch_quantiles(mu_f, var_f, lik_var, w, lv)}))
    res["score_speedup_vs_torch"] = res["torch_f32_score_composition_ms"]["median"] / res["mixture_score_ms"]["median"]
    res["quantiles_speedup_vs_torch"] = res["torch_f32_bisection40_ms"]["median"] / res["mixture_quantiles_ms"]["median"]
    res["normwise_vs_torch_f32"] = diff
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=65536)
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--Q", type=int, default=9)
    ap.add_argument("--errors-from", default="")
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"large": bench_shape(a.N, a.K, a.Q, dev), "demo": bench_shape(1500, 3, a.Q, dev),
           "method": "HIP events, 3 warm-ups, median of 10, candidates taken in turn, one process",
           "bound": "erfc / exp (about 6 MB of inputs at the large shape); no HBM fraction stated",
           "vgprs_kmax_1_2_4_8_16_32": VGPRS}
    res["acceptance"] = {"score_faster_than_torch_composition": res["large"]["score_speedup_vs_torch"] > 1.0,
                         "quantiles_faster_than_torch_bisection": res["large"]["quantiles_speedup_vs_torch"] > 1.0}
    if a.errors_from:
        res["worst_errors"] = worst_errors(a.errors_from)
        res["worst_errors_gate"] = 1e-4
    if a.kernel_stats:
        res["kernel_alone_us"] = kernel_alone(a.kernel_stats)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
