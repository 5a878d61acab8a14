"""Timing and accuracy of the greedy conditional-variance selection (csrc/greedy.hip).

Timing, at the benchmark shape N = 65536, M = 1024, D = 8 (uniform inputs, a lengthscale at
which all 1024 steps run; m is reported): the whole selection enqueued in one call (init, M
step launches, result; no readback in between) against the same algorithm composed from
PyTorch-ROCm ops on the same device -- a device-side pivot index (no host synchronisation
per step), float64 d and kernel values, a float32 factor, and the dot product as a float32
matrix-vector product over the factor (the cheapest form; the HIP kernel accumulates it in
float64).  The composition has no threshold test.  Effective bytes/s is the factor traffic
the algorithm needs, 4 N m^2 / 2, over the time.  HIP events, 1 warm-up, median of 5, the
candidates taken in turn.

Accuracy, on the inputs of tests/greedy_ref.py: the gate of tests/test_gpu_greedy.py and
what the device measures against it, and the threshold floor: every input run at threshold
1e-6, the float64 reference recomputed along the device's pivots, and for each level of a
ladder of thresholds the worst relative shortfall (max d_ref - d_ref[pivot]) / max d_ref over
the steps taken above it.  The floor is the smallest level down to which every pivot is the
float64 maximum.
Usage: python tools/bench_greedy.py [--out profiles/greedy_init_bench.json] [--no-torch]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modulatedgps_amd import inducing, ops  # noqa: E402
from modulatedgps_amd.kernels import SquaredExponential  # noqa: E402
from tests import greedy_ref as GR  # noqa: E402

SHAPE = (65536, 1024, 8)
LENGTHSCALE, VARIANCE = 1.0, 1.0
HBM_MEASURED_TBS, HBM_SPEC_TBS = 6.29, 8.0      # float4 copy / data sheet
LADDER = (1e-4, 3e-5, 1e-5, 3e-6, 1e-6)


def timeit_all(fns, warmup=1, reps=5):
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
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


def torch_selection(X, M, variance, ls, L):
    """The loop with torch kernels -> (indices int64 [M], d).  L: float32 [M, N] storage."""
    N = X.shape[0]
    Xs = X.double() / ls.double()
    var = variance.double()
    d = var.expand(N).clone()
    piv = torch.empty(M, dtype=torch.int64, device=X.device)
    for i in range(M):
        j = torch.argmax(d).reshape(1)
        piv[i:i + 1] = j
        diff = Xs - Xs.index_select(0, j)
        c = var * torch.exp(-0.5 * (diff * diff).sum(dim=1))
        if i:
            Li = L[:i]
            c = c - torch.mv(Li.t(), Li.index_select(1, j).reshape(i)).double()
        l = (c / torch.sqrt(d.index_select(0, j))).float()
        L[i] = l
        d = torch.clamp(d - l.double() ** 2, min=0.0)
    return piv, d


def bench(dev, with_torch):
    N, M, D = SHAPE
    X = torch.as_tensor(GR.f32(np.random.default_rng(N + M).uniform(-1.0, 1.0, size=(N, D))), device=dev)
    kern = SquaredExponential(VARIANCE, LENGTHSCALE, device=dev)
    ws = ops.greedy_workspace(N, M, D, dev)
    factor = ops.greedy_factor(N, M, dev)
    state = torch.zeros(2, dtype=torch.int32, device=dev)
    out = {}

    def fused():
        ops.greedy_init(N, D, kern.variance, 1e-4, ws)
        ops.greedy_steps(X, kern.variance, kern.lengthscales, M, M, factor, ws, state)
        out["fused"] = ops.greedy_result(X, M, ws)

    fns = {"fused_selection_ms": fused}
    if with_torch:
        Lt = torch.zeros(M, N, device=dev)

        def composed():
            out["torch"] = torch_selection(X, M, kern.variance, kern.lengthscales, Lt)
        fns["torch_selection_ms"] = composed
    res = {"N": N, "M": M, "D": D, "lengthscale": LENGTHSCALE, "variance": VARIANCE}
    res.update(timeit_all(fns))
    indices, _, dmax, trace, _, info = out["fused"]
    m, stopped = (int(v) for v in info.cpu())
    t = res["fused_selection_ms"]["median"] * 1e-3
    res.update({"m": m, "stopped": bool(stopped), "dmax_last": float(dmax[m - 1].cpu()),
                "trace_last_over_N": float(trace[m - 1].cpu()) / N,
                "fused_step_us": 1e6 * t / m,
                "factor_bytes_needed": 4 * N * m * m // 2,
                "fused_effective_TBs": 4 * N * m * m / 2 / t / 1e12})
    res["fused_share_of_measured_hbm"] = res["fused_effective_TBs"] / HBM_MEASURED_TBS
    res["hbm_TBs"] = {"measured_float4_copy": HBM_MEASURED_TBS, "spec": HBM_SPEC_TBS}
    if with_torch:
        tp = out["torch"][0][:m]
        same = int((tp == indices[:m]).sum().cpu())
        first = int((tp != indices[:m]).int().argmax().cpu()) if same < m else None
        res.update({"torch_step_us": 1e3 * res["torch_selection_ms"]["median"] / M,
                    "speedup_vs_torch": res["torch_selection_ms"]["median"] / res["fused_selection_ms"]["median"],
                    "torch_pivots_equal": same, "torch_first_different_step": first})
    return res


def accuracy(dev):
    gate = GR.gate()
    res = {"emulation_max_d_error_over_variance": GR.emulation_d_error(), "gate": gate, "cases": {}}
    ladder = {f"{thr:g}": {"steps": 0, "worst_relative_shortfall": 0.0} for thr in LADDER}
    for c in GR.CASES:
        X, M, variance, ls = c.args()
        var = GR.hyper(variance, 1.0)[0]
        kern = SquaredExponential(variance, np.asarray(ls), device=dev)
        r = inducing.greedy_variance_device(X, M, kern)
        p = r.indices.cpu().numpy()
        ref = GR.reference(X, len(p), variance, ls, path=p)
        res["cases"][c.name] = {
            "m": len(p), "stopped": r.stopped,
            "pivots_equal_float64": bool(np.array_equal(p, GR.case_reference(c.name).indices)),
            "shortfall_over_variance": float(((ref.top - ref.dmax) / var).max()),
            "residual_error_over_variance": float(np.abs(r.residual.cpu().numpy() - ref.residual).max() / var)}
        low = inducing.greedy_variance_device(X, min(c.N, 256), kern, threshold=LADDER[-1])
        p = low.indices.cpu().numpy()
        ref = GR.reference(X, len(p), variance, ls, path=p)
        sub = GR.suboptimality(ref)
        for thr in LADDER:
            k = int((ref.top > thr * var).sum())
            e = ladder[f"{thr:g}"]
            e["steps"] += k
            e["worst_relative_shortfall"] = max(e["worst_relative_shortfall"], float(sub[:k].max()) if k else 0.0)
    res["measured_max_shortfall_over_variance"] = max(v["shortfall_over_variance"] for v in res["cases"].values())
    res["measured_max_residual_error_over_variance"] = max(
        v["residual_error_over_variance"] for v in res["cases"].values())
    res["threshold_ladder"] = ladder
    exact = [thr for thr in LADDER if ladder[f"{thr:g}"]["worst_relative_shortfall"] == 0.0]
    res["threshold_floor"] = min(exact) if exact else None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-torch", action="store_true", help="skip the composed comparator")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"method": "HIP events, 1 warm-up, median of 5, candidates in turn",
           "device": torch.cuda.get_device_name(0)}
    res["accuracy"] = accuracy(dev)
    res["benchmark"] = bench(dev, not a.no_torch)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
