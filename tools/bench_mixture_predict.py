"""Timing of the mixture predictive (csrc/mixture.hip) in Philox mode against (a) the same
formula composed from PyTorch-ROCm float32 elementwise ops on the same latents, with z
generated beforehand and outside the timed region -- the lines a user would otherwise
write -- and (b) the K6 forward (ops.elbo_terms) at the same N, K, S, which does strictly
more per sample (a uniform draw and two logarithms per expert for the Gumbels); and of
SMGP.log_predictive_density end to end at c3's shapes.  HIP events, 3 warm-up calls,
median of 10 timed calls (the three candidates' calls taken in turn).  Compulsory traffic at the default shape is about 10 MB (four
latent arrays in, the outputs back): the kernel is bound by Philox and the
transcendentals, not by HBM, so no HBM fraction is stated.
Usage: python tools/bench_mixture_predict.py [--N 65536 --K 8 --S 25 --G 256] [--no-model]
           [--errors-from pytest.log] [--out profiles/mixture_predict_bench.json]
--errors-from: a log of `pytest -s tests/test_gpu_mixture_predict.py`; the worst of each
`MIXERR <quantity> <value>` line it printed is recorded as worst_errors."""
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
from modulatedgps_amd.config import default_jitter  # noqa: E402


def timeit_all(fns, warmup=3, reps=10):
    """{name: {median, min}} of the calls in `fns`, their timed repetitions taken in turn
    (a, b, c, a, b, c, ...) so that a drift of the machine falls on all of them alike."""
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


def timeit(fn, warmup=3, reps=10):
    return timeit_all({"fn": fn}, warmup, reps)["fn"]


def torch_mixture(mu_f, var_f, mu_a, var_a, lik_var, Y, z, jitter):
    """weights, mix_mean, mix_var, log_density and its float64 sum with torch float32 kernels;
    latents expert-major [K, N], z [S, N, K]."""
    S, N, K = z.shape
    logits = mu_a.t()[None] + z * torch.sqrt(torch.clamp(var_a.t() + jitter, min=0.0))[None]
    ls = torch.log_softmax(logits, -1)
    w = ls.exp().mean(0)
    mf, s2 = mu_f.t(), var_f.t() + lik_var[None]
    ln = -0.5 * torch.log(2.0 * math.pi * s2) - 0.5 * (Y[:, None] - mf).square() / s2
    ld = torch.logsumexp((ls + ln[None]).permute(1, 0, 2).reshape(N, S * K), -1) - math.log(S)
    mean = (w * mf).sum(-1)
    var = (w * (s2 + (mf - mean[:, None]).square())).sum(-1)
    return w, mean, var, ld, ld.double().sum()


def torch_grid(mu_f, var_f, lik_var, w, grid):
    mf, s2 = mu_f.t()[:, None, :], (var_f.t() + lik_var[None])[:, None, :]
    pdf = torch.exp(-0.5 * (grid[None, :, None] - mf).square() / s2) / torch.sqrt(2.0 * math.pi * s2)
    return (w[:, None, :] * pdf).sum(-1)


def worst_errors(path):
    worst = {}
    for name, val in re.findall(r"\bMIXERR (\S+) (\S+)$", open(path).read(), flags=re.M):
        worst[name] = max(worst.get(name, 0.0), float(val))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=65536)
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--S", type=int, default=25)
    ap.add_argument("--G", type=int, default=256)
    ap.add_argument("--no-model", action="store_true", help="skip the end-to-end c3 timing")
    ap.add_argument("--errors-from", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    N, K, S, G = a.N, a.K, a.S, a.G
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    rand = lambda *shape: torch.rand(*shape, device=dev, generator=g)
    lat = ops.padded(4 * K, N, dev)
    mu_f, var_f, mu_a, var_a = (lat[i * K:(i + 1) * K] for i in range(4))
    mu_f.copy_(3.0 * torch.randn(K, N, device=dev, generator=g))
    var_f.copy_(torch.exp(math.log(1e-4) * rand(K, N)))
    mu_a.copy_(30.0 * rand(K, N) - 15.0)
    var_a.copy_(3.0 * torch.exp(math.log(1e-4 / 3.0) * rand(K, N)))
    lik_var = torch.exp(math.log(1e-3) * rand(K))
    pick = torch.randint(0, K, (N,), device=dev, generator=g)
    cols = torch.arange(N, device=dev)
    Y = (mu_f[pick, cols] + (6.0 * rand(N) - 3.0) * torch.sqrt(var_f[pick, cols] + lik_var[pick])).contiguous()
    grid = torch.linspace(-6.0, 6.0, G, device=dev)
    seed, jitter = 1234, default_jitter()
    ws = torch.empty(max(int(ops._lib.load().mgp_mixture_predict_workspace_bytes(N, K)), 16), dtype=torch.uint8,
                     device=dev)
    kws = torch.empty(max(int(ops._lib.load().mgp_elbo_workspace_bytes(N)), 16), dtype=torch.uint8, device=dev)
    ksum = torch.empty(1, dtype=torch.float64, device=dev)

    out = ops.mixture_predict(mu_f, var_f, mu_a, var_a, lik_var, S, Y=Y, seed=seed, workspace=ws)
    # outputs and workspace allocated once, as for the K6 call below
    fused = lambda: ops.mixture_predict(mu_f, var_f, mu_a, var_a, lik_var, S, Y=Y, seed=seed, workspace=ws, out=out)
    z = ops.philox_noise(seed, 0, N, K, S, dev, want_u=False)[0]
    ref = torch_mixture(mu_f, var_f, mu_a, var_a, lik_var, Y, z, jitter)
    nw = lambda x, r: float((x.double() - r.double()).norm() / r.double().norm())
    diff = {n: nw(out[n], r) for n, r in zip(ops.MIXTURE_OUTPUTS, ref)}
    dens = ops.mixture_density_grid(mu_f, var_f, lik_var, out["weights"], grid)
    diff["density"] = nw(dens, torch_grid(mu_f, var_f, lik_var, out["weights"], grid))

    res = {"N": N, "K": K, "S": S, "G": G, "mode": "philox"}
    res.update(timeit_all({
        "mixture_predict_ms": fused,
        "torch_f32_composition_ms": lambda: torch_mixture(mu_f, var_f, mu_a, var_a, lik_var, Y, z, jitter),
        "k6_forward_elbo_terms_ms": lambda: ops.elbo_terms(mu_f, var_f, mu_a, var_a, Y, lik_var, S, seed=seed,
                                                           out=ksum, workspace=kws)}))
    res.update({
        "mixture_density_grid_ms": timeit(lambda: ops.mixture_density_grid(mu_f, var_f, lik_var, out["weights"], grid)),
        "torch_f32_density_grid_ms": timeit(lambda: torch_grid(mu_f, var_f, lik_var, out["weights"], grid)),
        "normwise_vs_torch_f32": diff,
        "bound": "Philox and transcendentals (about 10 MB of compulsory traffic); no HBM fraction stated"})
    t = res["mixture_predict_ms"]["median"]
    res["speedup_vs_torch"] = res["torch_f32_composition_ms"]["median"] / t
    res["speedup_vs_k6_forward"] = res["k6_forward_elbo_terms_ms"]["median"] / t
    res["grid_speedup_vs_torch"] = (res["torch_f32_density_grid_ms"]["median"]
                                    / res["mixture_density_grid_ms"]["median"])
    res["acceptance"] = {"not_slower_than_torch_composition": res["speedup_vs_torch"] >= 1.0,
                         "not_slower_than_k6_forward": res["speedup_vs_k6_forward"] >= 1.0}
    if not a.no_model:
        import bench
        cfg = bench.CONFIGS["c3"]
        X_np, Y_np, layers = bench.synthetic(cfg, 0, dev)
        model = bench.build_model(cfg, layers, dev, num_data=cfg[0])
        Xd, Yd = torch.from_numpy(X_np).to(dev), torch.from_numpy(Y_np).to(dev)
        res["c3"] = dict(zip(("N", "M", "K", "D", "lengthscale", "S"), cfg))
        res["c3"]["log_predictive_density"] = model.log_predictive_density(Xd, Yd, cfg[5], seed=seed)
        res["c3"]["log_predictive_density_ms"] = timeit(
            lambda: model.log_predictive_density_device(Xd, Yd, cfg[5], seed=seed))
        res["c3"]["build_likelihood_ms"] = timeit(lambda: model._build_likelihood(Xd, Yd, seed=seed))
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
