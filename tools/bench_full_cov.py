"""Timing of the full-covariance conditional (csrc/fullcov.hip) against the same formula
composed from PyTorch-ROCm float32 matmul / bmm on the same inputs -- the lines a user
would otherwise write -- and of layer.predict_f(X, full_cov=True) end to end.  HIP events,
3 warm-up calls, median of 10 timed calls.
Usage: python tools/bench_full_cov.py [--N 4096 --M 1024 --K 8 --D 8] [--out profiles/full_cov_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modulatedgps_amd import ops  # noqa: E402
from modulatedgps_amd.kernels import SquaredExponential  # noqa: E402
from modulatedgps_amd.models import SVGPModified  # noqa: E402

F32_MFMA_PEAK = 157.3e12   # v_mfma_f32_32x32x2_f32, MI355X


def timeit(fn, warmup=3, reps=10):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(np.min(ts))


def torch_full_cov(X, A, q_sqrt, var, ls):
    """Knn - A^T A + (L_k^T A)^T (L_k^T A) with torch float32 kernels."""
    Xs = X / ls
    Knn = var * torch.exp(-0.5 * torch.cdist(Xs, Xs).square())
    C = torch.matmul(torch.tril(q_sqrt).transpose(-1, -2), A)           # [K, M, N]
    return (Knn - A.t() @ A)[None] + torch.bmm(C.transpose(-1, -2), C)  # [K, N, N]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=4096)
    ap.add_argument("--M", type=int, default=1024)
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--D", type=int, default=8)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    N, M, K, D = a.N, a.M, a.K, a.D
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn(N, D, device=dev, generator=g)
    kern = SquaredExponential(variance=0.5, lengthscales=float(np.sqrt(D)), device=dev)
    layer = SVGPModified(kern, None, X[:M].clone(), num_latent_gps=K, device=dev)
    layer.set_variational(0.5 * torch.randn(M, K, device=dev, generator=g),
                          0.5 * torch.eye(M, device=dev) + 0.1 * torch.randn(K, M, M, device=dev, generator=g))
    var, ls, q_sqrt = kern.variance, kern.lengthscales, layer.q_sqrt
    A = ops.padded(M, N, dev)
    layer.conditional_kn(X, bufs={"A32": A})                            # K4's f32 A
    out = ops.padded(N, N, dev, batch=K)
    ws = torch.empty(ops.full_cov_workspace_bytes(M, N, K), dtype=torch.uint8, device=dev)

    cov = ops.full_cov_conditional(X, A, q_sqrt, var, ls, out=out, workspace=ws)
    ref = torch_full_cov(X, A, q_sqrt, var, ls)
    diff = float((cov - ref).norm() / ref.norm())
    t_hip = timeit(lambda: ops.full_cov_conditional(X, A, q_sqrt, var, ls, out=out, workspace=ws))
    t_torch = timeit(lambda: torch_full_cov(X, A, q_sqrt, var, ls))
    t_api = timeit(lambda: layer.predict_f(X, full_cov=True))
    flops = 2.0 * M * N * N * (1 + K) / 2 + float(K) * M * M * N
    res = {"N": N, "M": M, "K": K, "D": D, "flops_counted": flops,
           "full_cov_conditional_ms": {"median": t_hip[0], "min": t_hip[1]},
           "torch_f32_matmul_ms": {"median": t_torch[0], "min": t_torch[1]},
           "predict_f_full_cov_ms": {"median": t_api[0], "min": t_api[1]},
           "tflops": flops / (t_hip[0] * 1e-3) / 1e12,
           "fraction_of_f32_mfma_peak": flops / (t_hip[0] * 1e-3) / F32_MFMA_PEAK,
           "speedup_vs_torch": t_torch[0] / t_hip[0], "normwise_vs_torch": diff}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
