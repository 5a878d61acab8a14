"""Timing of the Matern kernels (csrc/matern.hip) at BASELINE config 3's sizes, N = 65536,
M = 1024, K = 8, D = 8, each beside its SquaredExponential counterpart:
  (1) K1: mgp_matern_kuf_image (nu2 = 5) in both image formats beside mgp_rbf_kuf_f16, and beside
      the same Matern formula composed from PyTorch-ROCm float32 ops (per-dimension differences
      of the scaled inputs, polynomial, exp) writing an f32 Kuf;
  (2) mgp_matern_kuu_potrf_trtri beside mgp_kuu_potrf_trtri (one layer, L and L^-T);
  (3) mgp_matern_backward beside mgp_rbf_backward (the Kuf cotangent [M, N]);
  (4) the ELBO step and the training step (elbo_and_grad) of a Matern52 model beside the
      SquaredExponential model of the same shape (the Matern model runs per-layer launches: no
      K1 inside K3, no two-layer K3 / RBF backward batch).
Image kernel bounds, from shapes: the image is 6 B per padded element (two of three planes for
split-f16: 4 B) and the kernel does 3 D + ~10 VALU operations per element.
HIP events, 3 warm-up calls, median of 10 timed calls, the candidates' calls taken in turn.
Usage: python tools/bench_matern.py [--no-steps] [--out profiles/matern_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from modulatedgps_amd import ops  # noqa: E402

NU2 = 5


def timeit_all(fns, warmup=3, reps=10):
    """{name: {median, min}} in ms of fns = {name: call}; the timed repetitions are taken in turn."""
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


def torch_matern52(X, Z, variance, lengthscales):
    Zs, Xs = Z / lengthscales, X / lengthscales
    r2 = torch.zeros(Z.shape[0], X.shape[0], dtype=torch.float32, device=Z.device)
    for d in range(Z.shape[1]):   # direct differences, one [M, N] pass per dimension
        diff = Zs[:, d, None] - Xs[None, :, d]
        r2.addcmul_(diff, diff)
    s = torch.sqrt(5.0 * r2)
    return variance * (1.0 + s + s * s * (1.0 / 3.0)) * torch.exp(-s)


def bench_kernels(cfg, dev, res):
    N, M, K, D, ls, _ = cfg
    X, _, layers = bench.synthetic(cfg, 0, dev)
    Xd, Zd = torch.as_tensor(X, device=dev), torch.as_tensor(layers[0][0], device=dev)
    var = torch.tensor([0.5], device=dev)
    lsd = torch.full((1,), float(ls), device=dev)
    img = torch.empty(ops.x6_cols_bytes(M, N), dtype=torch.uint8, device=dev)
    k1 = timeit_all({
        "matern_kuf_image_f16_ms": lambda: ops.matern_kuf_image(Xd, Zd, var, lsd, NU2, out=img, fmt="f16"),
        "matern_kuf_image_x6_ms": lambda: ops.matern_kuf_image(Xd, Zd, var, lsd, NU2, out=img, fmt="x6"),
        "rbf_kuf_f16_ms": lambda: ops.rbf_kuf_x6(Xd, Zd, var, lsd, out=img, fmt="f16"),
        "rbf_kuf_x6_ms": lambda: ops.rbf_kuf_x6(Xd, Zd, var, lsd, out=img, fmt="x6"),
        "torch_float32_matern52_kuf_ms": lambda: torch_matern52(Xd, Zd, var, lsd),
    })
    Mp, Np = -(-M // 128) * 128, -(-N // 256) * 256
    for fmt, planes in (("f16", 2), ("x6", 3)):
        t = k1[f"matern_kuf_image_{fmt}_ms"]["median"] * 1e-3
        k1[f"matern_kuf_image_{fmt}_bounds"] = {
            "image_bytes_written": Mp * Np * 2 * planes, "write_GBps": Mp * Np * 2 * planes / t / 1e9,
            "valu_ops_counted": Mp * Np * (3 * D + 10), "valu_Gops": Mp * Np * (3 * D + 10) / t / 1e9,
            "share_of_hbm_peak": Mp * Np * 2 * planes / bench.PEAK_HBM / t}
    res["k1"] = k1

    L = ops.padded(M, M, dev, batch=1)
    LinvT = ops.padded(M, M, dev, batch=1)
    info = torch.empty(1, dtype=torch.int32, device=dev)
    ws_m = ops._new_workspace("mgp_matern_chol_workspace_bytes", (M,), dev)
    ws_r = ops._new_workspace("mgp_chol_workspace_bytes", (M, 1), dev)
    res["kuu_potrf_trtri"] = timeit_all({
        "matern_kuu_potrf_trtri_ms": lambda: ops.matern_kuu_potrf_trtri(Zd, var, lsd, NU2, 1e-6, LinvT=LinvT, L=L,
                                                                      info=info, workspace=ws_m),
        "rbf_kuu_potrf_trtri_ms": lambda: ops.kuu_potrf_trtri([Zd], [var], [lsd], 1e-6, LinvT=LinvT, L=L, info=info,
                                                             workspace=ws_r),
    })
    assert int(info.cpu()[0]) == 0

    gK = ops.padded(M, N, dev)
    gK.copy_(torch.randn(M, N, device=dev, generator=torch.Generator(device=dev).manual_seed(1)))
    gZ = torch.zeros(M, D, device=dev)
    gv = torch.zeros(1, dtype=torch.float64, device=dev)
    gl = torch.zeros(1, dtype=torch.float64, device=dev)
    wb_m = ops._new_workspace("mgp_matern_backward_workspace_bytes", (N, M, D), dev)
    wb_r = ops._new_workspace("mgp_rbf_backward_workspace_bytes", (N, M, D), dev)
    res["backward"] = timeit_all({
        "matern_backward_ms": lambda: ops.matern_backward(Xd, Zd, var, lsd, NU2, gK, gZ=gZ, g_var=gv, g_ls=gl,
                                                          workspace=wb_m),
        "rbf_backward_ms": lambda: ops.rbf_backward(Xd, Zd, var, lsd, gK, gZ=gZ, g_var=gv, g_ls=gl, workspace=wb_r),
    })


def build(cfg, layers, dev, family):
    from modulatedgps_amd import kernels
    from modulatedgps_amd.likelihoods import GaussianModified
    from modulatedgps_amd.models import SMGP, SVGPModified
    N, M, K, D, ls, S = cfg
    lik = GaussianModified(variance=0.5, D=K, device=dev)
    svgp = []
    for Z, var, q_mu, q_sqrt in layers:
        layer = SVGPModified(kernel=getattr(kernels, family)(variance=var, lengthscales=ls, device=dev),
                             likelihood=lik, inducing_variable=Z, num_latent_gps=K, device=dev)
        layer.set_variational(torch.from_numpy(q_mu), torch.from_numpy(q_sqrt))
        svgp.append(layer)
    return SMGP(likelihood=lik, pred_layer=svgp[0], assign_layer=svgp[1], K=K, num_samples=S, num_data=N, seed=1234)


def bench_steps(cfg, dev, res):
    X, Y, layers = bench.synthetic(cfg, 0, dev)
    Xd, Yd = torch.as_tensor(X, device=dev), torch.as_tensor(Y, device=dev)
    models = {name: build(cfg, layers, dev, name) for name in ("SquaredExponential", "Matern52")}
    res["elbo_step"] = timeit_all({name + "_ms": (lambda m=m: m._build_likelihood(Xd, Yd)) for name, m in models.items()})
    res["training_step"] = timeit_all({name + "_ms": (lambda m=m: m.elbo_and_grad(Xd, Yd))
                                       for name, m in models.items()})
    for m in models.values():
        m.check_linalg()
    for key in ("elbo_step", "training_step"):
        res[key]["matern52_over_squared_exponential"] = (res[key]["Matern52_ms"]["median"]
                                                         / res[key]["SquaredExponential_ms"]["median"])
    res["layers_per_launch"] = {name: m.layers_per_launch for name, m in models.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-steps", action="store_true", help="skip the ELBO and training steps")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = bench.CONFIGS["c3"]
    res = {"method": "HIP events, 3 warm-ups, median of 10, candidates in turn", "device": torch.cuda.get_device_name(0),
           "N": cfg[0], "M": cfg[1], "K": cfg[2], "D": cfg[3], "nu2": NU2}
    bench_kernels(cfg, dev, res)
    if not a.no_steps:
        bench_steps(cfg, dev, res)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
