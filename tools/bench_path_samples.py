"""Timing of the pathwise-sample evaluation (csrc/paths.hip) against the same formula composed
from PyTorch-ROCm float32 ops on the same A -- the materialised cos(X Omega^T + b) and two
matmuls, the lines a user would otherwise write -- and of LayerPaths(X) end to end with the
share of K1 and K4.  HIP events, 3 warm-up calls, median of 10 timed calls, the candidates
taken in turn.  Also the largest N at which predict_f_samples(full_cov=True), which this
replaces for large N, still factorises with the default jitter on a dense 1-D grid.  With
--test-log (the output of `pytest tests/test_gpu_paths.py -s`), the worst of every
`SCOREERR <quantity> <value>` line is recorded as worst_errors.
Usage: python tools/bench_path_samples.py [--N 65536 --M 1024 --D 8 --K 8 --S 16 --R 1024]
           [--test-log LOG] [--out profiles/path_samples_bench.json]"""
import argparse
import json
import math
import os
import re
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modulatedgps_amd import _lib, ops  # noqa: E402
from modulatedgps_amd.kernels import SquaredExponential  # noqa: E402
from modulatedgps_amd.models import SVGPModified  # noqa: E402

F32_MFMA_PEAK = 157.3e12   # v_mfma_f32_32x32x2_f32, MI355X


def time_in_turn(fns, warmup=3, reps=10):
    """{name: (median, min)} ms; every repetition times each candidate once, in turn."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return {k: {"median": float(np.median(v)), "min": float(np.min(v))} for k, v in ts.items()}


def largest_full_cov_n(dev):
    """predict_f_samples(full_cov=True) of a one-expert layer on a dense grid of [-3, 3]:
    the last N of the doubling sequence that factorises with the default jitter, and the
    first that does not (None: every N tried ran)."""
    kern = SquaredExponential(variance=1.0, lengthscales=1.0, device=dev)
    layer = SVGPModified(kern, None, torch.linspace(-3, 3, 32, device=dev)[:, None], num_latent_gps=1, device=dev)
    good, bad = None, None
    for N in (128, 256, 512, 1024, 2048, 4096):
        X = torch.linspace(-3, 3, N, device=dev)[:, None]
        try:
            layer.predict_f_samples(X, num_samples=2, seed=1)
            good = N
        except _lib.MGPLinAlgError:
            bad = N
            break
    return good, bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=65536)
    ap.add_argument("--M", type=int, default=1024)
    ap.add_argument("--D", type=int, default=8)
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--S", type=int, default=16)
    ap.add_argument("--R", type=int, default=1024)
    ap.add_argument("--test-log", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    N, M, D, K, S, Rn = a.N, a.M, a.D, a.K, a.S, a.R
    C = S * K
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn(N, D, device=dev, generator=g)
    kern = SquaredExponential(variance=0.5, lengthscales=float(np.sqrt(D)), device=dev)
    layer = SVGPModified(kern, None, X[:M].clone(), num_latent_gps=K, device=dev)
    layer.set_variational(0.5 * torch.randn(M, K, device=dev, generator=g),
                          0.5 * torch.eye(M, device=dev) + 0.1 * torch.randn(K, M, M, device=dev, generator=g))
    paths = layer.sample_paths(S, Rn, seed=1)
    A = paths.solve(X)
    out = ops.padded(C, N, dev)
    W1t, W2t = paths.W[:Rn].t().contiguous(), paths.W[Rn:].t().contiguous()
    Om_t, b = (2 * math.pi * paths.Omega).t().contiguous(), 2 * math.pi * paths.phase

    def fused():
        return ops.path_eval(X, paths.Omega, paths.phase, paths.W, A=A, out=out)

    def composed():
        Phi = torch.cos(torch.addmm(b, X, Om_t))                  # [N, R], materialised
        return torch.addmm(W1t @ Phi.t(), W2t, A)

    diff = float((fused() - composed()).norm() / composed().norm())
    t = time_in_turn({"path_eval": fused, "torch_f32_composition": composed, "layer_paths": lambda: paths(X)})
    stages = {}
    for _ in range(10):
        paths(X, timing=stages)
    torch.cuda.synchronize()
    share = {k: float(np.median([e0.elapsed_time(e1) for e0, e1 in v])) for k, v in stages.items()}
    flops = 2.0 * (Rn + M) * N * C
    good, bad = largest_full_cov_n(dev)
    res = {"N": N, "M": M, "D": D, "K": K, "S": S, "R": Rn, "C": C, "flops_counted": flops,
           "path_eval_ms": t["path_eval"], "torch_f32_composition_ms": t["torch_f32_composition"],
           "layer_paths_ms": t["layer_paths"], "layer_paths_stage_ms": share,
           "tflops": flops / (t["path_eval"]["median"] * 1e-3) / 1e12,
           "fraction_of_f32_mfma_peak": flops / (t["path_eval"]["median"] * 1e-3) / F32_MFMA_PEAK,
           "speedup_vs_torch": t["torch_f32_composition"]["median"] / t["path_eval"]["median"],
           "normwise_vs_torch": diff,
           "predict_f_samples_full_cov_dense_grid": {"largest_N_that_ran": good, "first_N_that_failed": bad}}
    if a.test_log:
        worst = {}
        for name, val in re.findall(r"\bSCOREERR (\S+) (\S+)$", open(a.test_log).read(), flags=re.M):
            pick = min if name.endswith("_min") else max
            worst[name] = pick(worst.get(name, float(val)), float(val))
        res["worst_errors"] = worst
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    assert res["speedup_vs_torch"] > 1.0, "the fused call must be faster than the composition"


if __name__ == "__main__":
    main()
