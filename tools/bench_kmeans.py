"""Timing of the device k-means (csrc/kmeans.hip) at the benchmark shape N = 65536, k = 1024,
D = 8 and the demo shape N = 1500, k = 25, D = 1:
  one Lloyd iteration (assign + update + finish, mgp_kmeans_iterate with R = 1, B = 1, from
  the same start rows every time) against (1) the same iteration composed from PyTorch-ROCm
  ops on the same device -- torch.cdist, min/argmin over the codes, index_add_ of the
  float64 rows and counts, the division -- which writes and re-reads the N x k distance
  matrix (268 MB at the benchmark shape) that the fused kernel never stores; and
  a whole kmeans(obs, k, seed=0) (20 restarts to convergence, host readbacks included);
  (2) SciPy on the host, for information only (one vq + update pass at the benchmark shape,
  where the whole call takes minutes; the whole call at the demo shape).
HIP events, 3 warm-up calls, median of 10 timed calls, the candidates' calls taken in turn.
Usage: python tools/bench_kmeans.py [--no-scipy] [--out profiles/kmeans_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modulatedgps_amd import cluster, ops  # noqa: E402

SHAPES = {"benchmark": (65536, 1024, 8), "demo": (1500, 25, 1)}


def timeit_all(fns, warmup=3, reps=10):
    """{name: {median, min}} in ms of fns = {name: (prepare, call)}: `prepare` runs outside
    the events; the timed repetitions are taken in turn (a, b, a, b, ...) so that a drift of
    the machine falls on all candidates alike."""
    for prep, fn in fns.values():
        for _ in range(warmup):
            prep()
            fn()
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, (prep, fn) in fns.items():
            prep()
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts[name].append(e0.elapsed_time(e1))
    return {name: {"median": float(np.median(t)), "min": float(np.min(t))} for name, t in ts.items()}


def torch_iteration(obs, obs64, book):
    """One Lloyd iteration with torch kernels -> (new code book float32 [k, D] with zeros for
    the empty codes, counts, mean distance float64).  The compaction over the empty codes is
    left out (it would need a host synchronisation for the shape)."""
    k, D = book.shape
    dist, code = torch.cdist(obs, book).min(dim=1)
    avg = dist.double().mean()
    sums = torch.zeros(k, D, dtype=torch.float64, device=obs.device).index_add_(0, code, obs64)
    counts = torch.zeros(k, dtype=torch.float64, device=obs.device).index_add_(
        0, code, torch.ones_like(dist, dtype=torch.float64))
    return (sums / counts.clamp(min=1.0)[:, None]).float(), counts, avg


def scipy_times(X, k, idx, whole):
    from scipy.cluster.vq import _vq, kmeans, vq
    t0 = time.perf_counter()
    code, _ = vq(X, X[idx])
    _vq.update_cluster_means(X, code, k)
    out = {"scipy_one_iteration_s": time.perf_counter() - t0}
    if whole:
        t0 = time.perf_counter()
        kmeans(X, k, seed=0)
        out["scipy_kmeans_seed0_s"] = time.perf_counter() - t0
    return out


def bench_shape(N, k, D, dev, with_scipy, scipy_whole):
    rng = np.random.default_rng(N + k)
    X = rng.normal(size=(N, D))
    X[: N // 3] += 3.0
    obs = torch.as_tensor(X, device=dev, dtype=torch.float32).contiguous()
    obs64 = obs.double()
    idx_np = cluster.start_indices(N, k, 1, seed=0)
    idx = torch.as_tensor(idx_np, device=dev)
    start = obs[idx[0]].contiguous()
    ws = ops.kmeans_workspace(N, k, D, 1, dev)
    done = torch.zeros(1, dtype=torch.int32, device=dev)

    # the fused iteration against the torch composition on the same start rows
    ops.kmeans_init(obs, k, ws, idx=idx)
    ops.kmeans_iterate(obs, k, 1, 1, -1.0, ws, done)          # thresh < 0: never done
    result = torch.empty(32 + k * D * 4, dtype=torch.uint8, device=dev)
    ops.kmeans_select(N, k, D, 1, ws, result)
    fused_book = result[32:].view(torch.float32).reshape(k, D)
    tb, tc, tavg = torch_iteration(obs, obs64, start)
    keep = tc > 0
    ka = int(keep.sum())
    res = {"N": N, "k": k, "D": D,
           "distance_matrix_MB": N * k * 4 / 1e6,
           "iteration_max_abs_diff_vs_torch": float((fused_book[:ka] - tb[keep]).abs().max()),
           "iteration_avg_rel_diff_vs_torch":
               abs(float(np.frombuffer(bytes(result[:8].cpu().numpy()), np.float64)[0]) - float(tavg)) / float(tavg)}
    res.update(timeit_all({
        "fused_iteration_ms": (lambda: ops.kmeans_init(obs, k, ws, idx=idx),
                               lambda: ops.kmeans_iterate(obs, k, 1, 1, -1.0, ws, done)),
        "torch_iteration_ms": (lambda: None, lambda: torch_iteration(obs, obs64, start)),
        "vq_ms": (lambda: None, lambda: ops.vq(obs, start)),
        "kmeans_seed0_20_restarts_ms": (lambda: None, lambda: cluster.kmeans(obs, k, seed=0))}))
    res["iteration_speedup_vs_torch"] = res["torch_iteration_ms"]["median"] / res["fused_iteration_ms"]["median"]
    if with_scipy:
        res.update(scipy_times(X.astype(np.float32).astype(np.float64), k, idx_np[0], scipy_whole))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-scipy", action="store_true", help="skip the host comparator")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"method": "HIP events, 3 warm-ups, median of 10, candidates in turn",
           "device": torch.cuda.get_device_name(0)}
    for name, (N, k, D) in SHAPES.items():
        res[name] = bench_shape(N, k, D, dev, not a.no_scipy, scipy_whole=(name == "demo"))
    res["acceptance"] = {"fused_iteration_not_slower_than_torch_at_benchmark_shape":
                         res["benchmark"]["iteration_speedup_vs_torch"] >= 1.0}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
