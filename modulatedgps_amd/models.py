"""SGP / SMGP / SMGPModified / SVGPModified on the MI355X kernels.

Drop-in counterparts of MixtureGPs/models.py (same class names, constructor
arguments and method names).  The SMGP ELBO hot path
(SMGP._build_likelihood, models.py:69-79) runs as:

  both layers (pred, assign) at once, default split-f16 format:   reference call site
    K2+K3 mgp_kuu_potrf_trtri_kuf   Kuu + jitter I built in     models.py:135, 141 (cholesky)
                                    float64, L and L^-1; the
                                    step launches also write
    K1                              both layers' Kuf images     models.py:139
          mgp_split_upper_f16_bounded_batch   L^-T images
          mgp_qsqrt_images_kl_f16_batch       tril(q_sqrt) images + K7 KL   models.py:79, 141-143
    K4 mgp_trsm_stats_f16_batch     A image + stats             models.py:141-143 (triangular_solve, A^T q_mu)
    K5 mgp_expert_conditional_f16_batch  fmean, fvar [K, N]     models.py:141-143 (LTA, fvar)
    (config expert_format "x6": the same chain on exact split-bf16 images, six bf16
     products per f32 product -- mgp_rbf_kuf_x6, mgp_split_upper_x6 / _lower_x6,
     mgp_trsm_stats_x6, mgp_expert_conditional_x6 -- csrc/images.hip, csrc/trsm_stats.hip, csrc/expert_cond.hip;
     config.set_conditional_mode("f32"): mgp_rbf_kuf + mgp_trsm_stats +
     mgp_expert_conditional_f32 on the exact-f32 MFMA)
    (a layer on a Matern32 / Matern52 kernel: mgp_matern_kuu_potrf_trtri and
     mgp_matern_kuf_image per layer, through the kernel's factorise / kuf_image / backward
     methods, then the same split, K4 and K5 launches; the two-layer and fused launches above
     run only where both kernels are SquaredExponential)
  K6 mgp_elbo_terms         sum_n lse_s(...)        models.py:55-67,73-76
  mgp_elbo_combine          ELBO scalar             models.py:76,79

The reference evaluates every conditional on S tiled copies of X
(SGP.integrate, models.py:35-36); the copies are identical, so the conditional
is computed once per data point and S only enters the Monte-Carlo term.
Outputs that the reference returns with a leading S axis (predict_f on tiled
inputs, predict_y) are returned as broadcast views of that single result.

Compute dtype is float32 on the device; the parity tolerances against the
float64 reference semantics are stated in tests/.
"""
from typing import NamedTuple

import numpy as np
import torch

from . import ops
from .broadcasting_lik import BroadcastingLikelihood
from .config import (conditional_mode, default_device, default_jitter, expert_cross, expert_planes,
                     forward_image_format, step_schedule)

# both layers' K4, and both layers' K5, in one launch each in the step (False: one launch
# per layer and kernel, the reference of tests/test_gpu_properties.py's bit-for-bit test)
_K4_BATCHED = True
# split-f16: both layers' tril(q_sqrt) images and KL terms by mgp_qsqrt_images_kl_f16_batch
# (False: mgp_split_lower_f16 + mgp_gauss_kl_white per layer, the same test's reference)
_QS_BATCH = True
# k1_in_k3 carries K1's image blocks on the step launches' idle CUs at one 512-thread
# workgroup per CU; past this image size (N * M) the blocks outlast the chain's steps
# (BASELINE c5, N * M = 2^29: K3 2.15 -> 5.78 ms) and K1 runs on the side stream instead
# (schedule overlap, bit-identical)
_K1_IN_K3_MAX_NM = 1 << 27

# The training step keeps each layer's C_k = L_k^T A images for the backward
# (mgp_conditional_backward_f16c) while both layers' sets fit in this fraction of the
# device's HBM (config 5: 2 x 51.5 GB of 288 GB); beyond it the backward rebuilds
# S_k = L_k L_k^T.  C_IMAGES_MAX_BYTES (per layer), when set, overrides it.
C_IMAGES_HBM_FRACTION = 0.4
C_IMAGES_MAX_BYTES = None
from .kernels import Matern32, Matern52, SquaredExponential
from .likelihoods import MultiClass

TAU = 1e-2  # RelaxedOneHotCategorical temperature, models.py:60


def _is_se(kernel):
    return isinstance(kernel, SquaredExponential)


def _matern_unsupported(kernel, what):
    """Surfaces that are SquaredExponential-only (spectral features, the Knn of the full
    covariance) refuse a Matern kernel before anything is launched."""
    if not _is_se(kernel):
        raise NotImplementedError(f"{what} is not implemented for a {type(kernel).__name__} kernel "
                                  "(SquaredExponential only)")


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return x ^ (x >> 31)


class _Stage:
    """Optional HIP-event bracket around a stage, recorded on torch's current
    stream (the stream every libmgp_hip call of the model is launched on)."""

    def __init__(self, timing, name):
        self.timing, self.name = timing, name

    def __enter__(self):
        if self.timing is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if self.timing is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            self.timing.setdefault(self.name, []).append((self.e0, e1))
        return False


class HostArray(np.ndarray):
    """Host float64 array returned by the public predict_* methods: what the
    reference's EagerTensors give the demos (numpy consumes it directly,
    demos/demo_tf2.py:63-72,86-87,98-99, and `.numpy()` works as on a TF tensor)."""

    def numpy(self):
        return np.asarray(self)


def _host(t):
    """Device result -> HostArray (float64, the reference's default_float)."""
    return t.detach().to(torch.float64).cpu().numpy().view(HostArray)


def _to_dev(x, device, dtype=torch.float32):
    t = torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x)
    return t.to(device=device, dtype=dtype)


class SVGPModified:
    """Whitened SVGP layer with K latent GPs sharing one kernel and one Z
    (GPflow SVGP(kernel, likelihood, Z, num_latent_gps=K, whiten=True) with the
    posterior plugin IndependentPosteriorSingleOutputModified, models.py:126-160).

    Variational state: q_mu [M, K] (init zeros) and q_sqrt [K, M, M] lower
    triangular (init identity), as GPflow's SVGP initialises them."""

    def __init__(self, kernel, likelihood, inducing_variable, num_latent_gps=1, whiten=True,
                 q_mu=None, q_sqrt=None, q_diag=False, mean_function=None, device=None):
        if not whiten:
            raise NotImplementedError("only the whitened SVGP (whiten=True) is on the hot path")
        if q_diag:
            raise NotImplementedError("q_diag=True is not used by the reference models")
        if mean_function is not None:
            raise NotImplementedError("the reference layers use the Zero mean function")
        if not isinstance(kernel, (SquaredExponential, Matern32, Matern52)):
            raise TypeError("kernel must be a modulatedgps_amd.kernels SquaredExponential, Matern32 or Matern52")
        self.device = torch.device(device or kernel.device or default_device())
        self.kernel = kernel
        self.likelihood = likelihood
        self.whiten = True
        Z = _to_dev(inducing_variable, self.device)
        if Z.dim() == 1:
            Z = Z[:, None]
        self.Z = Z.contiguous()
        self._last_info = None
        self.seed, self._draws = 0, 0   # Philox key stream of predict_f_samples
        M = self.Z.shape[0]
        self.num_latent_gps = int(num_latent_gps)
        K = self.num_latent_gps
        self.q_mu = torch.zeros(M, K, dtype=torch.float32, device=self.device)
        self.q_sqrt = ops.padded(M, M, self.device, batch=K, zero=True)
        self.q_sqrt.copy_(torch.eye(M, device=self.device).expand(K, M, M))
        if q_mu is not None or q_sqrt is not None:
            self.set_variational(q_mu if q_mu is not None else self.q_mu,
                                 q_sqrt if q_sqrt is not None else self.q_sqrt)

    # ------------------------------------------------------------------ state
    @property
    def inducing_variable(self):
        return self.Z

    @property
    def num_inducing(self):
        return self.Z.shape[0]

    def set_variational(self, q_mu, q_sqrt):
        """Set q_mu [M, K] and q_sqrt [K, M, M] (band_part(-1, 0) is applied)."""
        q_mu = _to_dev(q_mu, self.device)
        q_sqrt = _to_dev(q_sqrt, self.device)
        M, K = self.num_inducing, self.num_latent_gps
        if tuple(q_mu.shape) != (M, K) or tuple(q_sqrt.shape) != (K, M, M):
            raise ValueError(f"expected q_mu [{M},{K}] and q_sqrt [{K},{M},{M}]")
        self.q_mu.copy_(q_mu)
        self.q_sqrt.copy_(torch.tril(q_sqrt))

    def parameters(self):
        return {"Z": self.Z, "q_mu": self.q_mu, "q_sqrt": self.q_sqrt, **self.kernel.parameters()}

    # ------------------------------------------------------------------ ops
    def Kuu(self, out=None):
        if not _is_se(self.kernel):
            return ops.matern_kuu(self.Z, self.kernel.variance, self.kernel.lengthscales, self.kernel.nu2,
                                  default_jitter(), out=out)
        return ops.rbf_kuu(self.Z, self.kernel.variance, self.kernel.lengthscales, default_jitter(),
                           out=out)

    def factorise(self, want_L=False):
        """Kuu (float64) -> L, (L^-1)^T (float32 [1, M, M]) and info (models.py:135,141)."""
        return self.kernel.factorise(self.Z, want_L=want_L)

    def prior_kl(self, out=None):
        """GPflow SVGP.prior_kl -> gauss_kl(q_mu, q_sqrt) whitened (models.py:79); float64 [1]."""
        return ops.gauss_kl_white(self.q_mu, self.q_sqrt, out=out)

    def operand_images(self, X, bufs=None, timing=None, fmt="x6"):
        """x6 mode: the split-bf16 images that do not depend on the Cholesky --
        Kuf (K1) and tril(q_sqrt) (split-f16 when fmt == "f16") -- so a caller
        can build them on a side stream while K3 runs.  Returns (Kfr, Lfr)."""
        bufs = bufs or {}
        X = self.kernel._x(X)
        with _Stage(timing, "rbf_kuf"):
            Kfr = self.kernel.kuf_image(X, self.Z, out=bufs.get("Kfr"), fmt=fmt)
        with _Stage(timing, "split_tri"):
            Lfr = ops.split_lower_x6(self.q_sqrt, out=bufs.get("Lfr"), fmt=fmt)
        return Kfr, Lfr

    def conditional_kn(self, X, LinvT=None, bufs=None, timing=None, images=None, fmt=None):
        """Whitened conditional for X [N, D]: fmean, fvar as expert-major [K, N] views.

        LinvT: (L^-1)^T of this layer's Kuu if already factorised (the SMGP
        factorises both layers in one batched sweep).  images: (Kfr, Lfr) from
        operand_images (x6 mode), if already built."""
        ops.check_conditional_experts(self.num_latent_gps)
        X = self.kernel._x(X)
        if LinvT is None:
            _, LinvT, info = self.factorise()
            self._last_info = info
            LinvT = LinvT[0]
        bufs = bufs or {}
        fmt = fmt or forward_image_format()
        if conditional_mode() == "x6":
            Kfr, Lfr = images if images is not None else self.operand_images(X, bufs, timing, fmt)
        else:
            with _Stage(timing, "rbf_kuf"):
                if _is_se(self.kernel):
                    Kuf = ops.rbf_kuf(X, self.Z, self.kernel.variance, self.kernel.lengthscales,
                                      out=bufs.get("Kuf"))
                else:
                    Kuf = ops.matern_kuf(X, self.Z, self.kernel.variance, self.kernel.lengthscales,
                                         self.kernel.nu2, out=bufs.get("Kuf"))
        if conditional_mode() == "f32":
            with _Stage(timing, "trsm_stats"):
                A, stats = ops.trsm_stats(LinvT, Kuf, self.q_mu, A=bufs.get("A"),
                                          stats=bufs.get("stats"))
            with _Stage(timing, "expert_cond"):
                return ops.expert_conditional(A, self.q_sqrt, stats, self.kernel.variance,
                                              fmean=bufs.get("fmean"), fvar=bufs.get("fvar"),
                                              workspace=bufs.get("ws_expert"))
        Afr, stats = self.x6_trsm(X.shape[0], LinvT, Kfr, bufs, timing, fmt)
        return self.x6_expert(X.shape[0], Afr, Lfr, stats, bufs, timing, fmt)

    def x6_trsm(self, N, LinvT, Kfr, bufs, timing=None, fmt="x6", Tfr=None):
        """K4 on images: A's image (split-f16 when fmt == "f16") and the column
        statistics (x6 mode).  Tfr: L^-T's image if already split."""
        if Tfr is None:
            with _Stage(timing, "split_tri"):
                Tfr = ops.split_upper_x6(LinvT, out=bufs.get("Tfr"), fmt=fmt)
        with _Stage(timing, "trsm_stats"):
            return ops.trsm_stats_x6(Tfr, Kfr, self.q_mu, self.num_inducing, N, Afr=bufs.get("Afr"),
                                     stats=bufs.get("stats"), A=bufs.get("A32"),
                                     f16_variance=self.kernel.variance if fmt == "f16" else None, in_fmt=fmt)

    def x6_expert(self, N, Afr, Lfr, stats, bufs, timing=None, fmt="x6", colmax_ready=False):
        """K5 on images: fmean, fvar [K, N] (x6 mode).  colmax_ready: the C_k images'
        column bound (colnorm_max of q_sqrt) is already in bufs["c_out"][1]."""
        with _Stage(timing, "expert_cond"):
            c_out = bufs.get("c_out")  # training (split-f16): C_k images for the backward
            if c_out is not None and not colmax_ready:
                ops.colnorm_max(self.q_sqrt, out=c_out[1])
            return ops.expert_conditional_x6(Afr, Lfr, stats, self.kernel.variance, self.num_inducing, N,
                                             self.num_latent_gps, fmean=bufs.get("fmean"),
                                             fvar=bufs.get("fvar"), workspace=bufs.get("ws_expert"),
                                             planes=expert_planes(), fmt=fmt, c_out=c_out)

    def conditional_experts(self, X, k0, k1, LinvT=None):
        """fmean, fvar [k1 - k0, N] of experts k0 .. k1 - 1 only (the expert-parallel
        layout: each rank owns a range of the K experts).  Kuf, the
        Cholesky and A are shared by all experts and computed in full; K4's
        statistics and K5 run on the expert range (q_mu columns, q_sqrt batch)."""
        X = self.kernel._x(X)
        M, N = self.num_inducing, X.shape[0]
        if not (0 <= k0 <= k1 <= self.num_latent_gps):
            raise ValueError("invalid expert range")
        if LinvT is None:
            _, LinvT, info = self.factorise()
            self._last_info = info
            LinvT = LinvT[0]
        fmt = forward_image_format()
        Kfr = self.kernel.kuf_image(X, self.Z, fmt=fmt)
        Tfr = ops.split_upper_x6(LinvT, fmt=fmt)
        Afr, stats = ops.trsm_stats_x6(Tfr, Kfr, self.q_mu[:, k0:k1], M, N,
                                       f16_variance=self.kernel.variance if fmt == "f16" else None, in_fmt=fmt)
        Lfr = ops.split_lower_x6(self.q_sqrt[k0:k1], fmt=fmt)
        return ops.expert_conditional_x6(Afr, Lfr, stats, self.kernel.variance, M, N, k1 - k0,
                                         planes=expert_planes(), fmt=fmt)

    def _marginals_kn(self, Xnew, tiled=None):
        """Xnew [..., N, D] -> (fmean, fvar, S, N, stride_s, lead): expert-major [K, cols]
        marginals where sample s of point n is column s * stride_s + n.  S tiled copies
        of one input (SGP.integrate, models.py:35-36) are computed once (stride_s = 0).
        tiled=None recognises tiling without a device sync: a device tensor whose sample
        axis has stride 0 (what integrate() returns, an expand() view), or a host array
        whose copies compare equal on the host; a materialised device copy of tiled
        rows (X[None].repeat(S, 1, 1), tf.tile's result) is then computed row by row (the
        same values, S times the work and buffers).  tiled=True: the caller asserts the
        S copies are equal and copy 0 is computed once (no check, no sync); tiled=False:
        every row is computed."""
        host_tiled = False
        if tiled is not None:
            if not isinstance(Xnew, torch.Tensor):
                Xnew = torch.as_tensor(np.asarray(Xnew))
            host_tiled = bool(tiled) and Xnew.dim() >= 3
        elif not isinstance(Xnew, torch.Tensor):
            Xh = np.asarray(Xnew)
            if Xh.ndim >= 3:
                Xh2 = Xh.reshape(-1, *Xh.shape[-2:])
                host_tiled = Xh2.shape[0] > 1 and bool((Xh2 == Xh2[:1]).all())
        elif Xnew.dim() >= 3:
            lead_t = Xnew.shape[:-2]
            if Xnew.device.type == "cpu":
                X2 = Xnew.reshape(-1, *Xnew.shape[-2:])
                host_tiled = X2.shape[0] > 1 and bool(torch.equal(X2, X2[:1].expand_as(X2)))
            else:
                host_tiled = all(st == 0 for st, n in zip(Xnew.stride()[:len(lead_t)], lead_t) if n > 1)
        X = self.kernel._x(Xnew) if not host_tiled else None
        if host_tiled:
            Xsrc = Xnew if isinstance(Xnew, torch.Tensor) else torch.as_tensor(np.asarray(Xnew))
            lead, N = Xsrc.shape[:-2], Xsrc.shape[-2]
            S = int(np.prod(lead)) if len(lead) else 1
            fm, fv = self.conditional_kn(Xsrc[(0,) * len(lead)])
            return fm, fv, S, N, 0, lead
        if X.dim() == 2:
            fm, fv = self.conditional_kn(X)
            return fm, fv, 1, X.shape[0], 0, ()
        lead, N = X.shape[:-2], X.shape[-2]
        S = X.reshape(-1, N, X.shape[-1]).shape[0]
        fm, fv = self.conditional_kn(X.reshape(-1, X.shape[-1]))
        return fm, fv, S, N, N, lead

    def posterior(self, precompute_cache=None):
        """SVGPModified.posterior (models.py:148-160): the posterior plugin object whose
        _conditional_fused runs K1-K5 on this layer's current state (a NOCACHE-style
        view: the variational parameters are read at call time, whatever the cache type)."""
        return IndependentPosteriorSingleOutputModified(
            self.kernel, self.inducing_variable, self.q_mu, self.q_sqrt, whiten=self.whiten,
            mean_function=None, precompute_cache=precompute_cache, layer=self)

    @property
    def trainable_variables(self):
        """GPflow Module.trainable_variables of the layer: Z, q_mu, q_sqrt, kernel variance
        and lengthscales (device tensors holding the constrained values)."""
        return (self.Z, self.q_mu, self.q_sqrt, self.kernel.variance, self.kernel.lengthscales)

    def predict_f(self, Xnew, full_cov=False, full_output_cov=False, tiled=None):
        """GPflow SVGP.predict_f(Xnew): posterior(NOCACHE).fused_predict_f, i.e. the
        Modified posterior's _conditional_fused (models.py:129-144).
        Xnew [..., N, D] -> mean, var [..., N, K]; full_cov=True: mean [..., N, K] and
        cov [..., K, N, N] (see _full_cov).  tiled: see _marginals_kn."""
        return self.posterior(PrecomputeCacheType.NOCACHE).fused_predict_f(Xnew, full_cov, full_output_cov,
                                                                          tiled=tiled)

    # ------------------------------------------------------------------ full covariance
    def next_seed(self):
        """Fresh Philox key per sampling call of the layer (as SMGP.next_seed)."""
        self._draws += 1
        return _splitmix64(self.seed * 0x100000001B3 + self._draws)

    def conditional_full_cov_kn(self, X):
        """X [N, D] -> fmean [K, N] (conditional_kn's) and cov [K, N, N]: the chain
        K1 -> K3 -> K4 -> K5 as conditional_kn runs it, with K4 also writing the f32 A,
        then mgp_full_cov_conditional on that A (base_conditional, full_cov=True)."""
        X = self.kernel._x(X)
        A = ops.padded(self.num_inducing, X.shape[0], self.device)
        fm, _ = self.conditional_kn(X, bufs={"A" if conditional_mode() == "f32" else "A32": A})
        cov = ops.full_cov_conditional(X, A, self.q_sqrt, self.kernel.variance, self.kernel.lengthscales)
        return fm, cov

    def _full_cov(self, Xnew, tiled=None):
        """Xnew [..., N, D] -> mean [..., N, K], cov [..., K, N, N] (GPflow's [..., P, N, N]).
        Leading dimensions are batch: each leading index has its own N x N blocks.  Tiled
        copies of one input (recognised as in _marginals_kn, or tiled=True) are computed
        once and returned as expand() views; distinct leading slices are computed in turn."""
        _matern_unsupported(self.kernel, "predict_f(full_cov=True)")
        if not isinstance(Xnew, torch.Tensor):
            Xnew = torch.as_tensor(np.asarray(Xnew))
        if Xnew.dim() <= 2:
            fm, cov = self.conditional_full_cov_kn(Xnew)
            return fm.t(), cov
        lead, N = Xnew.shape[:-2], Xnew.shape[-2]
        K = self.num_latent_gps
        if tiled is None:
            if Xnew.device.type == "cpu":
                X2 = Xnew.reshape(-1, *Xnew.shape[-2:])
                tiled = X2.shape[0] > 1 and bool(torch.equal(X2, X2[:1].expand_as(X2)))
            else:
                tiled = all(st == 0 for st, n in zip(Xnew.stride()[:len(lead)], lead) if n > 1)
        if tiled:
            fm, cov = self.conditional_full_cov_kn(Xnew[(0,) * len(lead)])
            return fm.t().expand(*lead, N, K), cov.expand(*lead, K, N, N)
        outs = [self.conditional_full_cov_kn(x) for x in Xnew.reshape(-1, *Xnew.shape[-2:])]
        mean = torch.stack([fm.t() for fm, _ in outs]).reshape(*lead, N, K)
        return mean, torch.stack([cov for _, cov in outs]).reshape(*lead, K, N, N)

    def _chol_full_cov(self, cov, jitter):
        """chol(cov[..., k] + jitter I) [..., K, N, N] (lower, zeros above) by the float64
        K3 (mgp_potrf_trtri, at most 8 matrices per call); MGPLinAlgError on a non-positive
        pivot.  Expanded (tiled) leading dimensions are factorised once."""
        lead = cov.shape[:-3]
        if len(lead) and all(st == 0 for st, n in zip(cov.stride(), lead) if n > 1):
            return self._chol_full_cov(cov[(0,) * len(lead)], jitter).expand(cov.shape)
        N = cov.shape[-1]
        mats = cov.reshape(-1, N, N)
        B = mats.shape[0]
        Aj = ops.padded(N, N, self.device, batch=B)
        Aj.copy_(mats)
        Aj.diagonal(dim1=-2, dim2=-1).add_(jitter)
        L = ops.padded(N, N, self.device, batch=B)
        info = torch.empty(B, dtype=torch.int32, device=self.device)
        for b0 in range(0, B, 8):
            b1 = min(b0 + 8, B)
            ops.potrf_trtri(Aj[b0:b1], L=L[b0:b1], info=info[b0:b1])
        ops.check_info(info)
        return L.unflatten(0, tuple(cov.shape[:-2]))

    def predict_f_samples(self, Xnew, num_samples=None, full_cov=True, full_output_cov=False, noise=None,
                          seed=None, jitter=None, tiled=None):
        """GPflow GPModel.predict_f_samples (sample_mvn): joint samples of the K latent
        functions at Xnew [..., N, D] -> [..., S, N, K] ([..., N, K] for num_samples=None):
            samples[..., s, :, k] = mean[..., :, k] + chol(cov[..., k] + jitter I) noise[..., s, :, k]
        with predict_f(Xnew, full_cov=True)'s mean and cov; full_cov=False draws from the
        marginals, mean + sqrt(var + jitter) noise.  noise: explicit standard normals of the
        samples' shape; else Philox normals (ops.philox_normal2) keyed by `seed`, or by a
        fresh key of the layer per call.  jitter defaults to default_jitter().

        Float32 limit: a float32 covariance of densely spaced points is positive definite
        only down to about sqrt(N) * 6e-8 * variance, so the default jitter of 1e-6 holds
        for N in the hundreds (minimum eigenvalues of -7e-8 .. -3.5e-7 at N = 100 .. 200) but
        not for N in the thousands.  The default is not raised silently: a failed
        factorisation raises MGPLinAlgError, and the caller passes a larger jitter."""
        if full_output_cov:
            raise NotImplementedError("full_output_cov predictions are not implemented")
        if full_cov:
            _matern_unsupported(self.kernel, "predict_f_samples(full_cov=True)")
        jitter = default_jitter() if jitter is None else float(jitter)
        mean, var = self.predict_f(Xnew, full_cov=full_cov, tiled=tiled)
        lead, (N, K) = tuple(mean.shape[:-2]), mean.shape[-2:]
        S = 1 if num_samples is None else int(num_samples)
        shape = (*lead, S, N, K)
        if noise is None:
            B = int(np.prod(lead)) if lead else 1
            key = self.next_seed() if seed is None else int(seed)
            z = ops.philox_normal2(key, 0, N, K, B * S, self.device).reshape(shape)
        else:
            z = _to_dev(noise, self.device)
            if num_samples is None and z.dim() == mean.dim():
                z = z.unsqueeze(-3)
            if tuple(z.shape) != shape:
                raise ValueError(f"noise must have the samples' shape {shape}, got {tuple(z.shape)}")
        if not full_cov:
            samples = mean.unsqueeze(-3) + torch.sqrt(var.unsqueeze(-3) + jitter) * z
        else:
            L = self._chol_full_cov(var, jitter)                       # [..., K, N, N]
            Lz = torch.matmul(L, z.permute(*range(len(lead)), -1, -2, -3))   # [..., K, N, S]
            samples = mean.unsqueeze(-3) + Lz.permute(*range(len(lead)), -1, -2, -3)
        return samples if num_samples is not None else samples.squeeze(-3)

    # ------------------------------------------------------------------ pathwise samples
    def sample_paths(self, num_samples, num_features=1024, seed=None, basis=None, noise=None):
        """num_samples joint samples of the K latent functions as functions (paths.LayerPaths;
        pathwise conditioning on num_features random Fourier features): the returned object
        is a snapshot of the layer, paths(X) -> [S, N, K] for any X [N, D] at a cost linear in
        N, and the same seed gives the same functions on every rank.  basis = (zeta [R, D],
        phase [R] in turns) and noise = (w [S, K, R], eps [S, K, M]) are explicit draws; else
        Philox draws keyed by `seed`, or by a fresh key of the layer.  1024 features is a
        convention, not a measured optimum.  ValueError on bad arguments before anything is
        uploaded."""
        _matern_unsupported(self.kernel, "sample_paths")
        from .paths import LayerPaths
        return LayerPaths(self, num_samples, num_features, seed=seed, basis=basis, noise=noise)


class PrecomputeCacheType:
    """gpflow.posteriors.PrecomputeCacheType (TENSOR / VARIABLE / NOCACHE)."""
    TENSOR = "tensor"
    VARIABLE = "variable"
    NOCACHE = "nocache"


class IndependentPosteriorSingleOutputModified:
    """The reference's posterior plugin (models.py:126-144): GPflow's IndependentPosterior
    with _conditional_fused overridden to Knn = K_diag, Kmm = Kuu + jitter,
    Kmn = K(Z, Xnew), base_conditional(white=True).  Here _conditional_fused is the
    K1 -> K3 -> K4 -> K5 chain of the layer it was made from (SVGPModified.posterior)."""

    def __init__(self, kernel, inducing_variable, q_mu, q_sqrt, whiten=True, mean_function=None,
                 precompute_cache=None, layer=None):
        if not whiten:
            raise NotImplementedError("only the whitened posterior is on the hot path")
        if mean_function is not None:
            raise NotImplementedError("the reference layers use the Zero mean function")
        if layer is None:
            raise ValueError("the posterior runs on an SVGPModified layer's kernels (layer=...)")
        self.kernel, self.X_data, self.q_mu, self.q_sqrt = kernel, inducing_variable, q_mu, q_sqrt
        self.whiten, self.mean_function = whiten, mean_function
        self.cache_type = precompute_cache
        self._layer = layer

    def _conditional_fused(self, Xnew, full_cov=False, full_output_cov=False, tiled=None):
        """(fmean, fvar) [..., N, K] of the whitened SVGP marginals (models.py:129-144).
        tiled (extension): True when the caller's [S, N, D] input holds S equal copies
        (computed once without a check), False to compute every row, None to detect
        (SVGPModified._marginals_kn).  full_cov=True: (fmean [..., N, K], cov [..., K, N, N])
        of base_conditional(..., full_cov=True, white=True) (SVGPModified._full_cov)."""
        if full_output_cov:
            raise NotImplementedError("full_output_cov predictions are not implemented")
        if full_cov:
            return self._layer._full_cov(Xnew, tiled=tiled)
        fm, fv, S, N, stride, lead = self._layer._marginals_kn(Xnew, tiled=tiled)
        K = fm.shape[0]
        shape = (*lead, N, K)
        if stride == 0 and len(lead):
            return fm.t().expand(shape), fv.t().expand(shape)
        return fm.t().reshape(shape), fv.t().reshape(shape)

    def fused_predict_f(self, Xnew, full_cov=False, full_output_cov=False, tiled=None):
        """GPflow BasePosterior.fused_predict_f: _conditional_fused + the (Zero) mean function."""
        return self._conditional_fused(Xnew, full_cov, full_output_cov, tiled=tiled)

    def predict_f(self, Xnew, full_cov=False, full_output_cov=False, tiled=None):
        return self.fused_predict_f(Xnew, full_cov, full_output_cov, tiled=tiled)


class RelaxedOneHotCategorical:
    """tfp.distributions.RelaxedOneHotCategorical(temperature, logits) as SMGP.W_dist
    returns it (models.py:60): logits [S * N, K] on the device; sample() runs the
    Gumbel-softmax kernel.  The first sample uses the key the logits were drawn with,
    so W_dist(Xt) -> sample(1) -> E_log_p_Y reproduces _build_likelihood with that key."""

    def __init__(self, temperature, logits, rows, seed=None, n_offset=0, model=None):
        self.temperature = float(temperature)
        self.logits = logits
        self._S, self._N = rows
        self._seed = seed
        self._model = model
        self._n_offset = int(n_offset)
        self._draws = 0

    def sample(self, sample_shape=(), noise_u=None, seed=None):
        """TFP sample semantics: sample() -> [S * N, K], sample(n) / sample((n,)) ->
        [n, S * N, K] relaxed one-hot samples (the reference draws sample(1)[0],
        models.py:73).  noise_u: explicit uniforms [n?, S, N, K].  Without noise and
        seed, the first draw uses the key the logits were drawn with (W_dist's, so
        W_dist -> sample(1) -> E_log_p_Y reproduces _build_likelihood with that key)
        and every later draw a fresh key from the model (TF's stateful RNG advances
        per call); with W_dist(noise_z=...) and no seed every draw is fresh."""
        shape = tuple(sample_shape) if isinstance(sample_shape, (tuple, list)) else (int(sample_shape),)
        n = int(np.prod(shape)) if shape else 1
        if n == 0:   # TFP: an empty sample, no draw (the RNG stream does not advance)
            return self.logits.new_empty((*shape, *self.logits.shape))
        outs = []
        for i in range(n):
            u = None
            if noise_u is not None:
                u = noise_u[i] if noise_u.dim() == 4 else noise_u
            if seed is not None:
                key = _splitmix64(int(seed) + i) if i else int(seed)
            elif self._draws == 0 and self._seed is not None:
                key = self._seed
            elif self._model is not None:
                key = self._model.next_seed()
            else:
                key = _splitmix64((self._seed or 0) * 0x100000001B3 + 0x5EED + self._draws)
            self._draws += 1
            outs.append(ops.relaxed_onehot_sample(self.logits, self._S, self._N, self.temperature, noise_u=u,
                                                  seed=key, n_offset=self._n_offset))
        if not shape:
            return outs[0]
        return torch.stack(outs).reshape(*shape, *outs[0].shape)


class SGP:
    """Scalable GP: X -> Xt = integrate(X) -> GP -> Y (models.py:23-41)."""

    def __init__(self, likelihood, pred_layer, num_samples=1, num_data=None):
        self.num_samples = int(num_samples)
        self.num_data = num_data
        self.likelihood = BroadcastingLikelihood(likelihood)
        self.pred_layer = pred_layer

    def integrate(self, X, S=1):
        """models.py:35-36 (kept for API parity; the hot path never tiles)."""
        X = torch.as_tensor(X)
        return X[None].expand(S, *X.shape), None

    def _mc_eps(self):
        """RobustMax epsilon when the pred likelihood is MultiClass, else None."""
        lik = self.likelihood.likelihood
        return lik.invlink.epsilon if isinstance(lik, MultiClass) else None

    def predict_y(self, Xnew, S=1):
        """models.py:38-41 -> (mean, var) [S, N, K] host arrays (HostArray, float64; S
        copies); the likelihood's _predict_mean_and_var through BroadcastingLikelihood
        (broadcasting_lik.py:44-46): Gaussian (mu, var + sigma^2) or MultiClass (ps, ps - ps^2).
        predict_y_device returns the same as float32 device views."""
        ym, yv = self.predict_y_device(Xnew, S)
        self.check_linalg(self.pred_layer._last_info)
        return _host(ym), _host(yv)

    def check_linalg(self, info=None):
        """Raise MGPLinAlgError if the last Cholesky of Kuu (both layers' for an SMGP
        evaluation) found a non-positive pivot -- the reference's InvalidArgumentError
        from base_conditional (models.py:141).  Reads K3's device `info` back (one host
        sync): run_adam does it at its ELBO readback, predict_* before returning."""
        info = getattr(self, "last_info", None) if info is None else info
        if info is not None:
            ops.check_info(info)

    def predict_y_device(self, Xnew, S=1):
        """predict_y as float32 device tensors [S, N, K] (broadcast views, no host copy)."""
        lik = self.likelihood.likelihood
        X = self.pred_layer.kernel._x(Xnew)
        fm, fv = self.pred_layer.conditional_kn(X)
        if self._mc_eps() is not None:
            ym, yv = ops.multiclass_predict(fm, fv, self._mc_eps())
        else:
            ym, yv, _ = ops.predict_epilogue(fm, fv, None, lik.variance.reshape(-1), want_y=True)
        return ym[None].expand(S, *ym.shape), yv[None].expand(S, *yv.shape)


class _Buffers(dict):
    """One cached buffer set of SMGP._buffers: name -> tensor.  Beside the tensors it names what
    the set was sized for -- every launch decision that follows from the layers' shapes and
    kernels, the config and `train` alone -- so that SMGP._plan reads booleans and nothing asks
    whether a key exists.  layer: per layer ("f" pred, "a" assign) the `bufs` mapping that the
    SVGPModified stage methods take (absent buffers are None)."""
    __slots__ = ("train", "x6", "fmt", "batched_k3", "pairable", "q_batchable", "c_images", "layer")


class _StepPlan(NamedTuple):
    """What one SMGP step launches and where: every decision, resolved once at the top of the
    step by SMGP._plan (rebuilt each call: the config and the module flags may change between
    calls on one model).  The stage methods read these and decide nothing themselves."""
    train: bool       # the training forward: K3 keeps L, K4 the f32 A
    x6: bool          # the chain runs on fragment images (conditional mode "x6"), else on the exact-f32 MFMA
    fmt: str          # the images' format, "f16" or "x6" (config.forward_image_format)
    sched: str        # the schedule that runs: config.step_schedule(), or "overlap" where it cannot
    batched_k3: bool  # one K3 sweep factorises both layers
    bounded: bool     # K3 writes max |LinvT| into the L^-T images' trailers; the split and the backward read it
    tfr_pair: bool    # both layers' L^-T images in one launch (bit-identical to two)
    q_batch: bool     # both layers' tril(q_sqrt) images and KL terms in one batch entry
    paired: bool      # both layers' K4 in one launch, and both layers' K5 in one
    c_images: bool    # K5 keeps the C_k images for the backward, whose q_sqrt-only prep runs beside K3
    tail_paired: bool  # both layers' Cholesky backward in one launch, and their RBF backward in one


class _StepState(NamedTuple):
    """What a step's forward hands to its backward: the plan it ran under, its buffer set and
    input, and per layer ("f", "a") K3's factors (L only in training)."""
    plan: _StepPlan
    b: _Buffers
    X: torch.Tensor
    L: dict
    LinvT: dict


class SMGP(SGP):
    """Mixture of Gaussian processes (models.py:44-103)."""

    def __init__(self, likelihood, pred_layer, assign_layer, K=3, num_samples=1, num_data=None,
                 seed=0):
        SGP.__init__(self, likelihood, pred_layer, num_samples, num_data)
        self.assign_layer = assign_layer
        self.K = int(K)
        if pred_layer.num_latent_gps != self.K or assign_layer.num_latent_gps != self.K:
            raise ValueError("both layers must have num_latent_gps == K")
        if isinstance(likelihood, MultiClass) and likelihood.num_classes != self.K:
            raise ValueError("a MultiClass pred likelihood needs num_classes == K (one latent GP per class)")
        self.device = pred_layer.device
        self.seed = int(seed)
        self._draws = 0
        self._bufs = {}
        self.last_info = None

    # ------------------------------------------------------------------ internals
    def _buffers(self, N, train=False):
        # the image formats decide which buffers exist (e.g. the C_k images of the
        # split-f16 training step), so a format switch between calls gets its own set
        key = (N, conditional_mode(), bool(train), forward_image_format(train), expert_cross())
        b = self._bufs.get(key)
        if b is not None:
            return b
        dev = self.device
        Mf, Ma, K = self.pred_layer.num_inducing, self.assign_layer.num_inducing, self.K
        Mx = max(Mf, Ma)
        T = ops.stats_tiles(Mx)
        x6 = conditional_mode() == "x6"
        kuf = None if x6 else ops.padded(Mx, N, dev)
        a = None if x6 else ops.padded(Mx, N, dev)
        st = ops.padded(2 * T * (K + 1), N, dev)  # per layer (the layers' K4 may run concurrently)
        cond = ops.padded(4 * K, N, dev)          # mu_f, var_f, mu_a, var_a
        fmt = forward_image_format(train)
        b = _Buffers({
            "Kuf_f": None if x6 else kuf[:Mf], "Kuf_a": None if x6 else kuf[:Ma],
            "A_f": None if x6 else a[:Mf], "A_a": None if x6 else a[:Ma],
            "stats_f": st[:ops.stats_tiles(Mf) * (K + 1)].unflatten(0, (-1, K + 1)),
            "stats_a": st[T * (K + 1):(T + ops.stats_tiles(Ma)) * (K + 1)].unflatten(0, (-1, K + 1)),
            "mu_f": cond[0:K], "var_f": cond[K:2 * K], "mu_a": cond[2 * K:3 * K],
            "var_a": cond[3 * K:4 * K],
            "kl": torch.empty(2, dtype=torch.float64, device=dev),
            "data_sum": torch.empty(1, dtype=torch.float64, device=dev),
            "elbo64": torch.empty((), dtype=torch.float64, device=dev),
            "ws_expert": torch.empty(max(ops.expert_workspace_bytes(Mx, N, K),
                                         ops.expert_x6_workspace_bytes(Mx, N, K)), dtype=torch.uint8,
                                     device=dev),
        })
        b.train, b.x6, b.fmt = bool(train), x6, fmt
        # both layers' K4, and both layers' K5, can run as one launch each: split-f16 images
        # with f16 cross terms, equal M (mgp_trsm_stats_f16_batch, mgp_expert_conditional_f16_batch)
        b.pairable = x6 and Mf == Ma and fmt == "f16" and expert_cross() == "f16"
        if b.pairable:
            b["ws_expert2"] = torch.empty_like(b["ws_expert"])   # the second layer's K5 workspace
        # both layers' tril(q_sqrt) images and KL terms can come from the batch entry
        # (mgp_qsqrt_images_kl_f16_batch): split-f16 images, equal q_mu shapes
        b.q_batchable = x6 and fmt == "f16" and Mf == Ma
        if b.q_batchable:
            b["qs_ws"] = torch.empty(2 * ops._lib.load().mgp_qsqrt_workspace_bytes(Mf, K), dtype=torch.uint8,
                                     device=dev)
            # prediction: the images are wanted, the KL values are not
            b["kl_scratch"] = torch.empty(2, dtype=torch.float64, device=dev)
        if x6:  # split-bf16 images: Kuf / tril(q_sqrt) per layer (built on the side
            # stream while K3 runs), A and L^-T shared by the layers (processed in turn)
            for L in ("f", "a"):
                b["Kfr_" + L] = torch.empty(ops.x6_cols_bytes(Mx, N), dtype=torch.uint8, device=dev)
                b["Lfr_" + L] = torch.empty(ops.x6_lower_bytes(Mx, K), dtype=torch.uint8, device=dev)
            for L in ("f", "a"):  # per layer: the two layers' K4 run concurrently
                b["Afr_" + L] = torch.empty(ops.x6_cols_bytes(Mx, N), dtype=torch.uint8, device=dev)
                b["Tfr_" + L] = torch.empty(ops.x6_lower_bytes(Mx, 1), dtype=torch.uint8, device=dev)
        # one K3 sweep for both layers: equal M and D (the two-layer K3 builds
        # SquaredExponential Kuu; a Matern layer factorises on its own)
        b.batched_k3 = (Mf == Ma and self.pred_layer.Z.shape[1] == self.assign_layer.Z.shape[1]
                        and self._both_se())
        if b.batched_k3:
            b["LinvT2"] = ops.padded(Mf, Mf, dev, batch=2)
        b.c_images = False
        if train:
            if not x6:
                raise NotImplementedError("the training step runs on the x6 conditional path")
            if b.batched_k3:
                b["L2"] = ops.padded(Mf, Mf, dev, batch=2)
            for L, M in (("f", Mf), ("a", Ma)):  # kept for the backward pass
                b["A32_" + L] = ops.padded(M, N, dev)
            b["G"] = ops.padded(4 * K, N, dev).unflatten(0, (4, K))
            cb = ops.c_images_bytes(Mx, N, K)
            limit = (C_IMAGES_MAX_BYTES if C_IMAGES_MAX_BYTES is not None else
                     C_IMAGES_HBM_FRACTION * torch.cuda.get_device_properties(dev).total_memory / 2)
            b.c_images = fmt == "f16" and expert_cross() == "f16" and cb <= limit
            if b.c_images:
                for L in ("f", "a"):  # K5 writes C_k per expert; the backward reads them
                    b["Cfr_" + L] = torch.empty(cb, dtype=torch.uint8, device=dev)
                    b["colmax_" + L] = torch.empty(1, dtype=torch.float32, device=dev)
                    b["cprep_" + L] = torch.empty(ops._lib.load().mgp_conditional_backward_prep_bytes(Mx, K),
                                                  dtype=torch.uint8, device=dev)
            b["ws_cbwd"] = torch.empty(ops.conditional_backward_workspace_bytes(Mx, N, K), dtype=torch.uint8,
                                       device=dev)
        b.layer = {L: {"Kuf": b["Kuf_" + L], "A": b["A_" + L], "stats": b["stats_" + L], "fmean": b["mu_" + L],
                       "fvar": b["var_" + L], "ws_expert": b["ws_expert"],
                       "Afr": b["Afr_" + L] if x6 else None, "Tfr": b["Tfr_" + L] if x6 else None,
                       "A32": b["A32_" + L] if train else None,
                       "c_out": (b["Cfr_" + L], b["colmax_" + L]) if b.c_images else None} for L in ("f", "a")}
        self._bufs[key] = b
        return b

    def _layers(self):
        return (("f", self.pred_layer), ("a", self.assign_layer))

    def _plan(self, b, X):
        """The launch plan of a step on buffer set b and input X (already through kernel._x)."""
        pf, pa = self.pred_layer, self.assign_layer
        # the schedules order the image chain's work; the exact-f32 mode has one order
        sched = step_schedule() if b.x6 else "overlap"
        # k1_in_k3: both layers' K1 as a side job of the batched K3's step launches, which read
        # X as given (neither kernel converts it) and carry K1 only up to _K1_IN_K3_MAX_NM;
        # else K1 runs on the side stream as in overlap (bit-identical)
        if sched == "k1_in_k3" and not (b.batched_k3 and pf.kernel._x(X) is X and pa.kernel._x(X) is X
                                        and X.shape[0] * pf.num_inducing <= _K1_IN_K3_MAX_NM):
            sched = "overlap"
        # split-f16 L^-T images: K3 folds their scale bound (max |LinvT|) into its
        # writes of the inverse, so the split needs no reduction launches
        bounded = b.x6 and b.batched_k3 and b.fmt == "f16"
        return _StepPlan(
            train=b.train, x6=b.x6, fmt=b.fmt, sched=sched, batched_k3=b.batched_k3,
            bounded=bounded, tfr_pair=bounded and _K4_BATCHED,
            # three launches (mgp_qsqrt_images_kl_f16_batch) instead of five per layer, beside
            # K3's chain; the batch entry also needs equal q_mu leading dimensions and q_sqrt
            # ld / stride(0), else the per-layer launches run
            q_batch=(_QS_BATCH and b.q_batchable and pf.q_mu.stride() == pa.q_mu.stride()
                     and pf.q_sqrt.stride() == pa.q_sqrt.stride()),
            # bit-identical to two launches: one kernel tail and dispatch-round boundary fewer
            # (~25 us, measured).  K5 pairs whenever K4 does: its second workspace exists under
            # the same condition, and both layers keep or drop their C_k images together
            paired=_K4_BATCHED and b.pairable,
            c_images=b.c_images,
            # with matching shapes (mgp_chol_backward_batch, mgp_rbf_backward_batch)
            tail_paired=b.train and self._tail_batchable())

    def _factorise(self, plan, b, X, prep_event):
        """Kuu of both layers and their Cholesky + inverse: per layer ("f", "a") L (training
        only: kept for the backward pass, else None) and (L^-1)^T, as two dicts.
        Batched K3 (one sweep for both layers): prep_event is recorded once Kuu is built (else
        after K3); plan.bounded: K3 also writes max |LinvT| into the L^-T split-f16 images'
        trailers (b["Tfr_f"], b["Tfr_a"]), for bounded splits; schedule k1_in_k3: its step
        launches also write both layers' Kuf images (b["Kfr_f"], b["Kfr_a"])."""
        pf, pa = self.pred_layer, self.assign_layer
        if plan.batched_k3:
            if pf.Z.stride(0) != pa.Z.stride(0):
                pa.Z = pa.Z.contiguous()
                pf.Z = pf.Z.contiguous()
            Lo, LinvT, info = ops.kuu_potrf_trtri(
                [pf.Z, pa.Z], [pf.kernel.variance, pa.kernel.variance],
                [pf.kernel.lengthscales, pa.kernel.lengthscales], default_jitter(), LinvT=b["LinvT2"],
                L=b["L2"] if plan.train else None, want_L=plan.train, prep_event=prep_event,
                tfr_bound_images=[b["Tfr_f"], b["Tfr_a"]] if plan.bounded else None,
                kuf=(X, [b["Kfr_f"], b["Kfr_a"]], plan.fmt) if plan.sched == "k1_in_k3" else None)
            self.last_info = info
            return dict(zip("fa", Lo if plan.train else (None, None))), dict(zip("fa", LinvT))
        outs = [layer.factorise(want_L=plan.train) for _, layer in self._layers()]
        self.last_info = torch.cat([info for *_, info in outs])
        if prep_event is not None:
            prep_event.record()
        return ({n: Lo[0] if plan.train else None for n, (Lo, _, _) in zip("fa", outs)},
                {n: LinvT[0] for n, (_, LinvT, _) in zip("fa", outs)})

    def _both_se(self):
        """Both layers on SquaredExponential kernels: what the two-layer and fused launches
        (batched K3 with K1 as its side job, bounded L^-T split, mgp_rbf_backward_batch) compute."""
        return _is_se(self.pred_layer.kernel) and _is_se(self.assign_layer.kernel)

    def _prep_event(self):
        """The K3 prep-done event (created once: its handle is passed to the C-ABI)."""
        if getattr(self, "_prep_ev", None) is None:
            self._prep_ev = torch.cuda.Event()
            self._prep_ev.record()   # creates the underlying hipEvent_t
        return self._prep_ev

    def _side_stream(self):
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream(device=self.device)
        return self._side

    def conditionals(self, X, timing=None, kl_out=None, train=False):
        """(mu_f, var_f, mu_a, var_a), each an expert-major [K, N] device view.

        x6 mode: K1 and the tril(q_sqrt) images of both layers (and, when kl_out
        is given, both KL terms) run on a side stream concurrently with the
        latency-bound K3 sweep, which occupies only a few CUs.  They start once
        K3 has built Kuu (its prep event): launched beside the build, K1's 4096
        workgroups starve it (101 us instead of ~20)."""
        b = self._conditionals(X, timing, kl_out, train).b
        return b["mu_f"], b["var_f"], b["mu_a"], b["var_a"]

    def _conditionals(self, X, timing, kl_out, train):
        """conditionals' work; the results are in the buffer set of the returned _StepState."""
        ops.check_conditional_experts(self.K)
        X = self.pred_layer.kernel._x(X)
        b = self._buffers(X.shape[0], train)
        plan = self._plan(b, X)
        self.layers_per_launch = 2 if plan.paired else 1   # K4 / K5 launches cover this many layers
        prep = self._prep_event() if plan.x6 else None
        with _Stage(timing, "kuu_chol"):
            L, LinvT = self._factorise(plan, b, X, prep)
        st = _StepState(plan, b, X, L, LinvT)
        if not plan.x6:
            self._chain_f32(st, timing, kl_out)
            return st
        # L^-T images straight after K3 on its stream (no cross-stream wait in front)
        self._linvt_images(st, timing)
        if plan.sched == "serial":   # everything on the main stream, K1 kept off K3's window
            self._side_work(st, timing, kl_out)
            for L, layer in self._layers():
                self._kuf_image(st, L, layer, timing)
        else:
            main, side = torch.cuda.current_stream(self.device), self._side_stream()
            side.wait_event(prep)   # after Kuu's build (and so after everything before K3 on main)
            with torch.cuda.stream(side):
                self._side_work(st, timing, kl_out)
            main.wait_stream(side)
        self._k4_k5(st, timing)
        return st

    def _kuf_image(self, st, L, layer, timing):
        """K1 of one layer on the current stream: its Kuf image."""
        with _Stage(timing, "rbf_kuf"):
            layer.kernel.kuf_image(layer.kernel._x(st.X), layer.Z, out=st.b["Kfr_" + L], fmt=st.plan.fmt)

    def _linvt_images(self, st, timing):
        """Both layers' L^-T images for K4 (x6 mode), on K3's stream."""
        plan, b = st.plan, st.b
        with _Stage(timing, "split_tri"):
            if plan.tfr_pair:
                ops.split_upper_f16_bounded_batch(b["LinvT2"], [b["Tfr_f"], b["Tfr_a"]])
            else:
                for L, _ in self._layers():
                    ops.split_upper_x6(st.LinvT[L], out=b["Tfr_" + L], fmt=plan.fmt, bounded=plan.bounded)

    def _side_work(self, st, timing, kl_out):
        """The Cholesky-independent work of an x6 step, on the current stream (the side stream
        beside K3; schedule serial: the main stream): K1 (schedule overlap), the tril(q_sqrt)
        images, both KL terms when kl_out is given, and in training the C_k images' bound and
        the backward's q_sqrt-only launches."""
        plan, b = st.plan, st.b
        pf, pa = self.pred_layer, self.assign_layer
        for L, layer in self._layers():
            if plan.sched == "overlap":
                self._kuf_image(st, L, layer, timing)
            with _Stage(timing, "split_tri"):
                if not plan.q_batch:
                    ops.split_lower_x6(layer.q_sqrt, out=b["Lfr_" + L], fmt=plan.fmt)
                if plan.c_images:   # colnorm_max of q_sqrt, off the K3 -> K5 path
                    ops.colnorm_max(layer.q_sqrt, out=b["colmax_" + L])
        if plan.q_batch:
            kl = kl_out if kl_out is not None else b["kl_scratch"]
            with _Stage(timing, "split_tri"):
                ops.qsqrt_images_kl_f16_batch([pf.q_mu, pa.q_mu], [pf.q_sqrt, pa.q_sqrt],
                                              [b["Lfr_f"], b["Lfr_a"]], [kl[0:1], kl[1:2]], workspace=b["qs_ws"])
        elif kl_out is not None:
            with _Stage(timing, "gauss_kl"):
                pf.prior_kl(out=kl_out[0:1])
                pa.prior_kl(out=kl_out[1:2])
        if plan.c_images:
            # the backward's q_sqrt-only launches, on the forward's L_k image bounds
            with _Stage(timing, "split_tri"):
                for L, layer in self._layers():
                    ops.conditional_backward_prep(
                        layer.q_sqrt, ops.image_bound(b["Lfr_" + L], layer.num_inducing,
                                                      K=layer.num_latent_gps), out=b["cprep_" + L])

    def _k4_k5(self, st, timing):
        """Both layers' K4 then both K5 in stream order on the main stream (x6 mode): the
        matrix-core kernels fill the chip alone, and a cross-stream hand-off costs 10-25 us
        of idle GPU per wait (measured).  plan.paired: one launch for both layers' K4 and one
        for their K5; else one per layer and kernel."""
        plan, b, N = st.plan, st.b, st.X.shape[0]
        pf, pa = self.pred_layer, self.assign_layer
        bf, ba = b.layer["f"], b.layer["a"]
        if not plan.paired:
            k4 = [layer.x6_trsm(N, st.LinvT[L], b["Kfr_" + L], b.layer[L], timing, plan.fmt, Tfr=b["Tfr_" + L])
                  for L, layer in self._layers()]
            for (L, layer), (Afr, stats) in zip(self._layers(), k4):   # (the C_k bounds: _side_work's)
                layer.x6_expert(N, Afr, b["Lfr_" + L], stats, b.layer[L], timing, plan.fmt, colmax_ready=True)
            return
        variances = [pf.kernel.variance, pa.kernel.variance]
        with _Stage(timing, "trsm_stats"):
            ops.trsm_stats_f16_batch(
                [b["Tfr_f"], b["Tfr_a"]], [b["Kfr_f"], b["Kfr_a"]], [pf.q_mu, pa.q_mu], pf.num_inducing, N,
                [bf["Afr"], ba["Afr"]], [bf["stats"], ba["stats"]], variances,
                As=[bf["A32"], ba["A32"]] if plan.train else None)
        with _Stage(timing, "expert_cond"):
            ops.expert_conditional_f16_batch(
                [bf["Afr"], ba["Afr"]], [b["Lfr_f"], b["Lfr_a"]], [bf["stats"], ba["stats"]], variances,
                pf.num_inducing, N, self.K, [bf["fmean"], ba["fmean"]], [bf["fvar"], ba["fvar"]],
                [b["ws_expert"], b["ws_expert2"]],
                # bounds from _side_work's colnorm_max
                c_outs=[bf["c_out"], ba["c_out"]] if plan.c_images else None)

    def _chain_f32(self, st, timing, kl_out):
        """The exact-f32 mode's chain: K1, K4 and K5 per layer on the main stream, then the KL."""
        for L, layer in self._layers():
            layer.conditional_kn(st.X, st.LinvT[L], bufs=st.b.layer[L], timing=timing, fmt=st.plan.fmt)
        if kl_out is not None:
            with _Stage(timing, "gauss_kl"):
                self.pred_layer.prior_kl(out=kl_out[0:1])
                self.assign_layer.prior_kl(out=kl_out[1:2])

    def _assign_lik_var(self):
        return None  # SMGPModified: the assignment likelihood's variances

    def next_seed(self):
        """Fresh Philox key per evaluation (TF's stateful RNG advances per call)."""
        self._draws += 1
        return _splitmix64(self.seed * 0x100000001B3 + self._draws)

    # ------------------------------------------------------------------ reference methods
    def W_dist(self, Xt, noise_z=None, seed=None, n_offset=0, tiled=None):
        """SMGP.W_dist (models.py:55-61): the assign layer's marginals, reparameterised
        with z ~ N(0, 1) [S, N, K] (utils.py:26-27) into logits [S * N, K], as a
        RelaxedOneHotCategorical(1e-2).  noise_z: explicit normals [S, N, K]; else
        Philox with `seed` (a fresh key per call when None), K6's z stream.  tiled:
        SVGPModified._marginals_kn's switch for materialised S-tiled inputs."""
        fm, fv, S, N, stride, _ = self.assign_layer._marginals_kn(Xt, tiled=tiled)
        if seed is None and noise_z is None:
            seed = self.next_seed()
        logits = ops.assign_logits(fm, fv, S, N, stride, noise_z=noise_z, seed=seed or 0, n_offset=n_offset)
        return RelaxedOneHotCategorical(TAU, logits.reshape(S * N, self.K), (S, N), seed=seed, n_offset=n_offset,
                                        model=self)

    def E_log_p_Y(self, Xt, Y, W_SND, tiled=None):
        """SMGP.E_log_p_Y (models.py:63-67): logsumexp_S(sum_K W ve) - log S -> [N]
        (device float32), ve the pred likelihood's variational expectation."""
        fm, fv, S, N, stride, _ = self.pred_layer._marginals_kn(Xt, tiled=tiled)
        Yd = _to_dev(Y, self.device).reshape(-1).contiguous()
        W = _to_dev(W_SND, self.device)
        mc = self._mc_eps()
        lik_var = None if mc is not None else self.likelihood.likelihood.variance.reshape(-1)
        extra = {}
        if self._assign_lik_var() is not None:   # SMGPModified.E_log_p_Y (models.py:112-123)
            fa, va, Sa, Na, stride_a, _ = self.assign_layer._marginals_kn(Xt, tiled=tiled)
            if (Sa, Na, stride_a) != (S, N, stride):
                raise ValueError("the two layers' marginals disagree in shape")
            extra = dict(mu_a=fa, var_a=va, assign_lik_var=self._assign_lik_var())
        return ops.e_log_p_y(fm, fv, Yd, lik_var, W, S, N, stride, multiclass_eps=mc, **extra)

    @property
    def trainable_variables(self):
        """GPflow Module.trainable_variables (utils/training_utils.py:10): the device
        tensors of trainable_parameters(), in its order.  These hold the CONSTRAINED
        values (what every kernel reads); GPflow's tf.Variables hold the unconstrained
        ones (softplus^-1 for positive parameters).  run_adam / AdamTF keep the
        unconstrained shadows themselves; a custom loop gets GPflow's semantics from
        unconstrained_variables(), elbo_and_grad(..., unconstrained=True) and
        assign_unconstrained() (tests/test_gpu_api.py)."""
        return tuple(t for _, t, _ in self.trainable_parameters())

    # ------------------------------------------------------------------ ELBO
    def _data_term(self, X, Y, train, noise, seed, n_offset, n_total, timing):
        """What _build_likelihood and elbo_and_grad share up to the data term: the inputs, both
        layers' conditionals with the KL terms (b["kl"]) and sum_n of the data term
        (b["data_sum"]).  Returns the step state, the (args, kwargs) that ops.elbo_terms took
        (ops.elbo_terms_backward takes the same) and (n_batch, num_data)."""
        X = self.pred_layer.kernel._x(X)
        N = X.shape[0]
        Yd = _to_dev(Y, self.device).reshape(-1).contiguous()
        if Yd.numel() != N:
            raise ValueError("X and Y must have the same number of rows")
        st = self._conditionals(X, timing, self._buffers(N, train)["kl"], train)
        b = st.b
        mc = self._mc_eps()
        lik_var = None if mc is not None else self.likelihood.likelihood.variance.reshape(-1)
        if seed is None and noise is None:
            seed = self.next_seed()
        args = (b["mu_f"], b["var_f"], b["mu_a"], b["var_a"], Yd, lik_var, self.num_samples, TAU)
        kw = dict(noise=noise, seed=seed or 0, n_offset=n_offset, assign_lik_var=self._assign_lik_var(),
                  multiclass_eps=mc)
        with _Stage(timing, "elbo_terms"):
            ops.elbo_terms(*args, out=b["data_sum"], **kw)
        n_batch = n_total if n_total is not None else N
        return st, (args, kw), (n_batch, self.num_data if self.num_data is not None else n_batch)

    def _combine(self, b, n_batch, num_data, out64):
        """The ELBO from the data-term sum and the KL terms: a fresh float32 tensor per call
        (the reference returns a new value each time), written by the combine kernel itself
        (no copy launch behind it); out64 receives the float64 value."""
        e32 = torch.empty((), dtype=torch.float32, device=self.device)
        ops.elbo_combine(b["data_sum"], b["kl"][0:1], b["kl"][1:2], n_batch, num_data, out=e32, out64=out64)
        return e32

    def _build_likelihood(self, X, Y, noise=None, seed=None, n_offset=0, n_total=None,
                          process_group=None, return64=False, timing=None):
        """ELBO (models.py:69-79) as a 0-d float32 device tensor.

        noise: optional explicit (z, u) [S, N, K] device tensors (parity mode);
        otherwise in-kernel Philox keyed by (seed, global n, s, k).
        n_offset / n_total / process_group: data-parallel sharding over N (each
        rank passes its shard; one all-reduce of the data-term sum)."""
        st, _, (n_batch, num_data) = self._data_term(X, Y, False, noise, seed, n_offset, n_total, timing)
        if process_group is not None:
            import torch.distributed as dist
            with _Stage(timing, "allreduce"):
                dist.all_reduce(st.b["data_sum"], op=dist.ReduceOp.SUM, group=process_group)
        e64 = torch.empty((), dtype=torch.float64, device=self.device)
        e32 = self._combine(st.b, n_batch, num_data, e64)
        return e64 if return64 else e32

    # ------------------------------------------------------------------ training
    def trainable_parameters(self):
        """[(name, tensor, transform)] of every trainable variable (Z, q_mu,
        q_sqrt (lower triangle), kernel variance / lengthscales (softplus) of both layers,
        and the shared Gaussian likelihood variance (softplus))."""
        ps = []
        for name, layer in (("pred", self.pred_layer), ("assign", self.assign_layer)):
            ps += [(name + ".Z", layer.Z, "free"), (name + ".q_mu", layer.q_mu, "free"),
                   (name + ".q_sqrt", layer.q_sqrt, "free"),
                   (name + ".variance", layer.kernel.variance, "positive"),
                   (name + ".lengthscales", layer.kernel.lengthscales, "positive")]
        if self._mc_eps() is None:  # MultiClass / RobustMax: no trainable likelihood parameter
            ps.append(("lik_variance", self.likelihood.likelihood.variance, "positive"))
        if self._assign_lik_var() is not None:
            ps.append(("assign_lik_variance", self.assign_likelihood.likelihood.variance, "positive"))
        return ps

    def unconstrained_variables(self):
        """{name: device tensor} of the unconstrained values GPflow's trainable_variables
        hold (utils/training_utils.py:10 differentiates w.r.t. these): free parameters as
        they are, positive ones as u = softplus^-1(theta) (gpflow.utilities.positive(),
        float64 inverse, then float32; the value theta = softplus(u) reproduces theta)."""
        out = {}
        for name, t, kind in self.trainable_parameters():
            if kind == "positive":
                th = t.detach().double()
                out[name] = torch.where(th > 20, th, torch.log(torch.expm1(th))).float()
            else:
                out[name] = t.detach().clone()
        return out

    def assign_unconstrained(self, values):
        """Set parameters from unconstrained values (dict name -> tensor, e.g. after a
        custom optimiser step on unconstrained_variables()): theta = softplus(u) for
        positive parameters, in place, so every kernel reads the new state."""
        for name, t, kind in self.trainable_parameters():
            if name not in values:
                continue
            v = values[name].to(device=t.device, dtype=torch.float32).reshape(t.shape)
            t.copy_(torch.nn.functional.softplus(v.double()).float() if kind == "positive" else v)

    def _tail_batchable(self):
        """Both layers' Cholesky / RBF backward can share launches: same M, D and
        lengthscale count (mgp_chol_backward_batch, mgp_rbf_backward_batch)."""
        f, a = self.pred_layer, self.assign_layer
        return (self._both_se() and f.Z.shape == a.Z.shape
                and f.kernel.lengthscales.numel() == a.kernel.lengthscales.numel()
                and f.Z.stride() == a.Z.stride())

    def _cond_backward(self, st, L, layer, g_mean, g_var, timing):
        """One layer's conditional backward (x6) from the gradients of its fmean and fvar."""
        plan, b = st.plan, st.b
        M = layer.num_inducing
        with _Stage(timing, "conditional_bwd"):
            cimg = prep = t_bound = None
            if plan.c_images:
                # the forward's C_k images (mgp_conditional_backward_f16c) and, from its side
                # stream, the q_sqrt-only prep; max |LinvT| from K3's bounded L^-T images
                cimg = (b["Cfr_" + L], b["colmax_" + L], ops.image_bound(b["Lfr_" + L], M, K=layer.num_latent_gps))
                prep = b["cprep_" + L]
                if plan.bounded:
                    t_bound = ops.image_bound(b["Tfr_" + L], M, K=1)
            return ops.conditional_backward_x6(b["Afr_" + L], b["A32_" + L], layer.q_sqrt, layer.q_mu,
                                               st.LinvT[L], g_mean, g_var, M, st.X.shape[0],
                                               workspace=b["ws_cbwd"], fmt=plan.fmt, c_images=cimg, prep=prep,
                                               t_bound=t_bound)

    def _tail_backward(self, st, L, name, layer, g, timing):
        """One layer's Cholesky and kernel backward (Kuf and Kuu): its gradient blocks."""
        with _Stage(timing, "chol_bwd"):
            gKuu = ops.chol_backward(st.L[L], st.LinvT[L], g["g_Lm"])
        with _Stage(timing, "rbf_bwd"):
            k = layer.kernel
            gZ, gvar, gls = k.backward(st.X, layer.Z, g["g_Kuf"], accumulate=True, g_var=g["g_var"],
                                       gZ=torch.zeros_like(layer.Z),
                                       g_ls=torch.zeros(k.lengthscales.numel(), dtype=torch.float64,
                                                        device=self.device))
            k.backward(layer.Z, layer.Z, gKuu, symmetric=True, accumulate=True, gZ=gZ, g_var=gvar, g_ls=gls)
        return {name + ".Z": gZ, name + ".variance": gvar, name + ".lengthscales": gls,
                name + ".q_mu": g["g_q_mu"], name + ".q_sqrt": g["g_q_sqrt"]}

    def _tail_backward_pair(self, st, order, gs, timing):
        """_tail_backward of both layers with one Cholesky and one RBF backward launch."""
        with _Stage(timing, "chol_bwd"):
            gKuus = ops.chol_backward_batch([st.L[L] for L, *_ in order], [st.LinvT[L] for L, *_ in order],
                                            [g["g_Lm"] for g in gs])
        with _Stage(timing, "rbf_bwd"):
            layers = [layer for _, _, layer, _ in order]
            # gZ / g_ls written by the finish (accumulate 2: no zero fills), g_var added
            # to the conditional backward's part
            gZs = [torch.empty(layer.Z.shape, dtype=layer.Z.dtype, device=self.device) for layer in layers]
            glss = [torch.empty(layer.kernel.lengthscales.numel(), dtype=torch.float64, device=self.device)
                    for layer in layers]
            ops.rbf_backward_batch(st.X, [layer.Z for layer in layers], [layer.kernel.variance for layer in layers],
                                   [layer.kernel.lengthscales for layer in layers], [g["g_Kuf"] for g in gs],
                                   gKuus, gZs, [g["g_var"] for g in gs], glss, accumulate=2)
        return [{name + ".Z": gZ, name + ".variance": g["g_var"], name + ".lengthscales": gls,
                 name + ".q_mu": g["g_q_mu"], name + ".q_sqrt": g["g_q_sqrt"]}
                for (_, name, _, _), g, gZ, gls in zip(order, gs, gZs, glss)]

    def elbo_and_grad(self, X, Y, noise=None, seed=None, n_offset=0, n_total=None, process_group=None,
                      timing=None, unconstrained=False):
        """ELBO (0-d float32) and its gradient w.r.t. every constrained parameter of
        trainable_parameters() (dict name -> device tensor; unconstrained=True: w.r.t.
        the unconstrained values of unconstrained_variables(), GPflow's
        trainable_variables, by the softplus chain rule), i.e. the GradientTape pass
        of run_adam's optimisation step (training_utils.py:10) on the HIP kernels:
        K6 backward -> per layer conditional backward (x6) -> Cholesky backward -> RBF
        backward (Kuf and Kuu) -> + KL.  Data-parallel: one all-reduce of the
        data-term gradients per step (the KL part is added after it)."""
        st, (args, kw), (n_batch, num_data) = self._data_term(X, Y, True, noise, seed, n_offset, n_total, timing)
        b = st.b
        with _Stage(timing, "elbo_terms_bwd"):
            G, glv, glva = ops.elbo_terms_backward(*args, scale=1.0 / n_batch, G=b["G"], **kw)
        grads = {"lik_variance": glv} if kw["multiclass_eps"] is None else {}
        if kw["assign_lik_var"] is not None:
            grads["assign_lik_variance"] = glva
        head = [b["data_sum"]] + list(grads.values())   # reduced with the first layer's bucket
        pending = []
        # the two layers in order on this stream (a side stream for one layer's Cholesky /
        # RBF backward beside the other's conditional backward measured slower: the
        # matrix-core kernel starves the small ones, DESIGN.md round-4 results); with
        # matching shapes both layers' Cholesky and RBF backward run as one batch each
        order = (("f", "pred", self.pred_layer, 0), ("a", "assign", self.assign_layer, 2))
        if st.plan.tail_paired:
            gs = [self._cond_backward(st, L, layer, G[gi], G[gi + 1], timing) for L, _, layer, gi in order]
            layer_grads = self._tail_backward_pair(st, order, gs, timing)
        else:
            layer_grads = (self._tail_backward(st, L, name, layer,
                                               self._cond_backward(st, L, layer, G[gi], G[gi + 1], timing), timing)
                           for L, name, layer, gi in order)
        for lg in layer_grads:   # (unpaired: computed here, layer by layer)
            if process_group is not None:
                # one bucket per layer (the first also carries the data-term sum and the
                # likelihood gradients); the pred layer's is in flight while the assign
                # layer's backward still runs
                from .distributed import allreduce_gradients_async
                bucket = list(lg.values())
                pending.append(allreduce_gradients_async(bucket if pending else head + bucket, group=process_group))
            grads.update(lg)
        if process_group is not None:
            with _Stage(timing, "allreduce"):
                for pb in pending:
                    pb.wait()
        for name, layer in (("pred", self.pred_layer), ("assign", self.assign_layer)):
            ops.kl_grad(layer.q_mu, layer.q_sqrt, num_data, grads[name + ".q_mu"], grads[name + ".q_sqrt"])
        e32 = self._combine(b, n_batch, num_data, b["elbo64"])
        if unconstrained:   # d/du = d/dtheta * softplus'(u) = d/dtheta * (1 - exp(-theta)) for positive ones
            for name, t, kind in self.trainable_parameters():
                if kind == "positive":
                    grads[name] = grads[name] * (-torch.expm1(-t.double())).float()
        return e32, grads

    def training_loss_closure(self, data_iter, compile=True):
        """GPflow ExternalDataTrainingLossMixin.training_loss_closure: () -> -ELBO on the next batch."""
        def closure():
            X, Y = next(data_iter)
            return self.training_loss((X, Y))
        return closure

    def elbo(self, data, **kw):
        X, Y = data
        return self._build_likelihood(X, Y, **kw)

    def _training_loss(self, data):
        """models.py:81-83."""
        X, Y = data
        return -self._build_likelihood(X, Y)

    def training_loss(self, data):
        return self._training_loss(data)

    # ------------------------------------------------------------------ predictions
    def predict_assign(self, Xnew, S=1):
        """models.py:85-89: softmax_K(mean_S mu_a) -> [N, K] host array (HostArray, float64)."""
        asg = self.predict_assign_device(Xnew, S)
        self.check_linalg(self.assign_layer._last_info)
        return _host(asg)

    def predict_assign_device(self, Xnew, S=1):
        """predict_assign as a float32 device tensor [N, K]."""
        X = self.assign_layer.kernel._x(Xnew)
        am, _ = self.assign_layer.conditional_kn(X)
        _, _, asg = ops.predict_epilogue(None, None, am, None, want_y=False, want_assign=True)
        return asg

    def predict_samples(self, Xnew, S=1, noise=None, seed=None):
        """models.py:91-103 -> samples_y, samples_f [S, N, 1] host arrays (HostArray, float64)."""
        sy, sf = self.predict_samples_device(Xnew, S, noise=noise, seed=seed)
        self.check_linalg()
        return _host(sy), _host(sf)

    def predict_samples_device(self, Xnew, S=1, noise=None, seed=None):
        """predict_samples as float32 device tensors [S, N, 1]."""
        X = self.pred_layer.kernel._x(Xnew)
        mu_f, var_f, mu_a, var_a = self.conditionals(X)
        if seed is None and noise is None:
            seed = self.next_seed()
        mc = self._mc_eps()
        sy, sf = ops.predict_samples(mu_f, var_f, mu_a, var_a,
                                     None if mc is not None else self.likelihood.likelihood.variance.reshape(-1),
                                     S, TAU, noise=noise, seed=seed or 0, multiclass_eps=mc)
        return sy[..., None], sf[..., None]

    # ------------------------------------------------------------------ mixture predictive
    # p(y* | x*) = sum_k w_k N(y* | mu_f,k, var_f,k + sigma_k^2) with w = mean_s softmax_k(mu_a +
    # z_s sqrt(var_a + jitter)) -- the Gumbel noise of RelaxedOneHotCategorical integrated out
    # (its argmax has class probabilities softmax(logits)); S = 0: the plug-in weights of
    # predict_assign.  The reference has no counterpart (DESIGN "Mixture predictive").  Each
    # method runs one conditionals(X) and one mgp_mixture_predict.  noise_z: explicit normals
    # [S, N, K]; else Philox with `seed` (K6's z stream; a fresh key per call when None).
    def _mixture(self, Xnew, S, want, Y=None, noise_z=None, seed=None, n_offset=0):
        if self._mc_eps() is not None:
            raise NotImplementedError(
                "a MultiClass pred likelihood has no expert mixture: W multiplies one value per point, "
                "and predict_y already returns the class probabilities")
        S = int(S)
        if S < 0:
            raise ValueError("S must be >= 0")
        X = self.pred_layer.kernel._x(Xnew)
        Yd = None
        if Y is not None:
            Yd = _to_dev(Y, self.device).reshape(-1).contiguous()
            if Yd.numel() != X.shape[0]:
                raise ValueError("X and Y must have the same number of rows")
        if noise_z is not None:
            noise_z = _to_dev(noise_z, self.device)
        elif S >= 1 and seed is None:
            seed = self.next_seed()
        mu_f, var_f, mu_a, var_a = self.conditionals(X)
        lik_var = self.likelihood.likelihood.variance.reshape(-1)
        out = ops.mixture_predict(mu_f, var_f, mu_a, var_a, lik_var, S, Y=Yd, noise_z=noise_z, seed=seed or 0,
                                  n_offset=n_offset, want=want)
        return out, (mu_f, var_f, lik_var)

    def predict_mixture_weights_device(self, Xnew, S=0, noise_z=None, seed=None):
        """predict_mixture_weights as a float32 device tensor [N, K]."""
        return self._mixture(Xnew, S, ("weights",), noise_z=noise_z, seed=seed)[0]["weights"]

    def predict_mixture_weights(self, Xnew, S=0, noise_z=None, seed=None):
        """The mixture weights w [N, K] (HostArray, float64): S = 0 is predict_assign; S >= 1
        averages the softmax over S draws of the assignment GP's logits, so its variance counts."""
        w = self.predict_mixture_weights_device(Xnew, S, noise_z=noise_z, seed=seed)
        self.check_linalg()
        return _host(w)

    def predict_mixture_mean_and_var_device(self, Xnew, S=0, noise_z=None, seed=None):
        """predict_mixture_mean_and_var as float32 device tensors ([N, 1], [N, 1])."""
        out, _ = self._mixture(Xnew, S, ("mix_mean", "mix_var"), noise_z=noise_z, seed=seed)
        return out["mix_mean"][:, None], out["mix_var"][:, None]

    def predict_mixture_mean_and_var(self, Xnew, S=0, noise_z=None, seed=None):
        """Mean and variance of the mixture predictive, ([N, 1], [N, 1]) (HostArray, float64):
        sum_k w mu_f and sum_k w (var_f + sigma_k^2 + (mu_f - mean)^2)."""
        m, v = self.predict_mixture_mean_and_var_device(Xnew, S, noise_z=noise_z, seed=seed)
        self.check_linalg()
        return _host(m), _host(v)

    def predict_log_density_device(self, Xnew, Ynew, S=0, noise_z=None, seed=None):
        """predict_log_density as a float32 device tensor [N]."""
        return self._mixture(Xnew, S, ("log_density",), Y=Ynew, noise_z=noise_z, seed=seed)[0]["log_density"]

    def predict_log_density(self, Xnew, Ynew, S=0, noise_z=None, seed=None):
        """log p(Ynew | Xnew) of the mixture predictive per point, [N] (HostArray, float64; GPflow's
        predict_log_density shape), a max-subtracted log-sum-exp that stays finite in the tails."""
        ld = self.predict_log_density_device(Xnew, Ynew, S, noise_z=noise_z, seed=seed)
        self.check_linalg()
        return _host(ld)

    def predict_density_device(self, Xnew, y_grid, S=0, noise_z=None, seed=None):
        """predict_density as a float32 device tensor [N, G]."""
        g = _to_dev(y_grid, self.device)
        if g.dim() != 1:
            raise ValueError("y_grid must be 1-D")
        out, (mu_f, var_f, lik_var) = self._mixture(Xnew, S, ("weights",), noise_z=noise_z, seed=seed)
        return ops.mixture_density_grid(mu_f, var_f, lik_var, out["weights"], g.contiguous())

    def predict_density(self, Xnew, y_grid, S=0, noise_z=None, seed=None):
        """The mixture predictive density p(y_grid[g] | Xnew[n]), [N, G] (HostArray, float64), on a
        1-D grid of targets shared by all points."""
        d = self.predict_density_device(Xnew, y_grid, S, noise_z=noise_z, seed=seed)
        self.check_linalg()
        return _host(d)

    def log_predictive_density_device(self, X, Y, S=0, noise_z=None, seed=None, n_offset=0, n_total=None,
                                      process_group=None):
        """log_predictive_density as a 0-d float64 device tensor (no host sync)."""
        out, (mu_f, _, _) = self._mixture(X, S, ("log_density_sum",), Y=Y, noise_z=noise_z, seed=seed,
                                          n_offset=n_offset)
        total, N = out["log_density_sum"], mu_f.shape[1]
        f64 = dict(dtype=torch.float64, device=self.device)
        sc = torch.cat([total, torch.full((1,), float(N), **f64)])
        if process_group is not None:
            import torch.distributed as dist
            dist.all_reduce(sc, op=dist.ReduceOp.SUM, group=process_group)
        # a tensor divisor in every case (a Python one is multiplied by as its reciprocal),
        # so that a one-rank group gives the plain call's bits
        return sc[0] / (sc[1] if n_total is None else torch.full((), float(n_total), **f64))

    def log_predictive_density(self, X, Y, S=0, noise_z=None, seed=None, n_offset=0, n_total=None,
                               process_group=None):
        """Mean over all points of log p(Y | X) (the held-out log-likelihood; its negative is
        the NLPD), a Python float from the float64 sum of the per-point values.  n_offset /
        n_total / process_group: sharding over N as in _build_likelihood (each rank passes its
        shard; one all-reduce of [sum, count]; without a group the local sum is divided by
        n_total, so the shards' values add up to the one-call value)."""
        v = self.log_predictive_density_device(X, Y, S, noise_z=noise_z, seed=seed, n_offset=n_offset,
                                               n_total=n_total, process_group=process_group)
        self.check_linalg()
        return float(v.cpu())

    # ------------------------------------------------------------------ mixture scores
    # CDF / PIT values, quantiles and CRPS of the mixture predictive above (DESIGN "Mixture
    # scores"): one conditionals(X), one mgp_mixture_predict for the weights (S, noise_z and seed
    # as in the methods above) and one mgp_mixture_score or mgp_mixture_quantiles on them.
    def _score(self, Xnew, Ynew, S, want, noise_z=None, seed=None, n_offset=0):
        if Ynew is None:
            raise ValueError("Ynew is required")
        out, (mu_f, var_f, lik_var) = self._mixture(Xnew, S, ("weights",), Y=Ynew, noise_z=noise_z, seed=seed,
                                                    n_offset=n_offset)
        Yd = _to_dev(Ynew, self.device).reshape(-1).contiguous()
        return ops.mixture_score(mu_f, var_f, lik_var, out["weights"], Yd, want=want), mu_f.shape[1]

    def predict_cdf_device(self, Xnew, Ynew, S=0, noise_z=None, seed=None, tail="lower"):
        """predict_cdf as a float32 device tensor [N]."""
        if tail not in ("lower", "upper"):
            raise ValueError("tail must be 'lower' or 'upper'")
        name = "cdf" if tail == "lower" else "sf"
        return self._score(Xnew, Ynew, S, (name,), noise_z=noise_z, seed=seed)[0][name]

    def predict_cdf(self, Xnew, Ynew, S=0, noise_z=None, seed=None, tail="lower"):
        """F(Ynew | Xnew) of the mixture predictive per point, [N] (HostArray, float64): the
        probability integral transform values of a calibration histogram.  tail="upper": the
        survival function 1 - F as its own sum, accurate relative to the upper tail."""
        c = self.predict_cdf_device(Xnew, Ynew, S, noise_z=noise_z, seed=seed, tail=tail)
        self.check_linalg()
        return _host(c)

    def predict_quantiles_device(self, Xnew, levels, S=0, noise_z=None, seed=None):
        """predict_quantiles as a float32 device tensor [N, Q]."""
        lv = ops.quantile_levels(levels)   # ValueError before anything runs
        out, (mu_f, var_f, lik_var) = self._mixture(Xnew, S, ("weights",), noise_z=noise_z, seed=seed)
        return ops.mixture_quantiles(mu_f, var_f, lik_var, out["weights"], lv)

    def predict_quantiles(self, Xnew, levels, S=0, noise_z=None, seed=None):
        """Quantiles of the mixture predictive, [N, Q] (HostArray, float64), e.g. levels
        [0.025, 0.5, 0.975] for a credible band that follows a multimodal predictive where
        mean +- 2 sd cannot.  Levels lie strictly inside (0, 1) (ValueError otherwise)."""
        q = self.predict_quantiles_device(Xnew, levels, S, noise_z=noise_z, seed=seed)
        self.check_linalg()
        return _host(q)

    def predict_crps_device(self, Xnew, Ynew, S=0, noise_z=None, seed=None):
        """predict_crps as a float32 device tensor [N]."""
        return self._score(Xnew, Ynew, S, ("crps",), noise_z=noise_z, seed=seed)[0]["crps"]

    def predict_crps(self, Xnew, Ynew, S=0, noise_z=None, seed=None):
        """The continuous ranked probability score of the mixture predictive at Ynew per point,
        [N] (HostArray, float64), in closed form (lower is better; the units of y)."""
        c = self.predict_crps_device(Xnew, Ynew, S, noise_z=noise_z, seed=seed)
        self.check_linalg()
        return _host(c)

    def crps_device(self, X, Y, S=0, noise_z=None, seed=None, n_offset=0, n_total=None, process_group=None):
        """crps as a 0-d float64 device tensor (no host sync)."""
        out, N = self._score(X, Y, S, ("crps_sum",), noise_z=noise_z, seed=seed, n_offset=n_offset)
        f64 = dict(dtype=torch.float64, device=self.device)
        sc = torch.cat([out["crps_sum"], torch.full((1,), float(N), **f64)])
        if process_group is not None:
            import torch.distributed as dist
            dist.all_reduce(sc, op=dist.ReduceOp.SUM, group=process_group)
        # a tensor divisor in every case, as in log_predictive_density_device
        return sc[0] / (sc[1] if n_total is None else torch.full((), float(n_total), **f64))

    def crps(self, X, Y, S=0, noise_z=None, seed=None, n_offset=0, n_total=None, process_group=None):
        """Mean CRPS over all points, a Python float from the float64 sum of the per-point
        values; sharded over N exactly as log_predictive_density (n_offset / n_total /
        process_group: one all-reduce of [sum, count])."""
        v = self.crps_device(X, Y, S, noise_z=noise_z, seed=seed, n_offset=n_offset, n_total=n_total,
                             process_group=process_group)
        self.check_linalg()
        return float(v.cpu())

    # ------------------------------------------------------------------ data association and modes
    # Which expert produced an observation -- the posterior p(z = k | x, y) ~ w_k(x) N(y | mu_k,
    # s_k^2), where predict_assign and predict_mixture_weights give the prior w_k(x) -- and the
    # point predictions of the mixture predictive, its modes (DESIGN "Data association and
    # modes").  One conditionals(X), one mgp_mixture_predict for the weights (S, noise_z and seed
    # as above) and one mgp_mixture_responsibilities or mgp_mixture_modes on them.
    def _responsibilities(self, Xnew, Ynew, S, want, noise_z=None, seed=None, n_offset=0):
        if Ynew is None:
            raise ValueError("Ynew is required")
        out, (mu_f, var_f, lik_var) = self._mixture(Xnew, S, ("weights",), Y=Ynew, noise_z=noise_z, seed=seed,
                                                    n_offset=n_offset)
        Yd = _to_dev(Ynew, self.device).reshape(-1).contiguous()
        return ops.mixture_responsibilities(mu_f, var_f, lik_var, out["weights"], Yd, want=want)

    def predict_responsibilities_device(self, Xnew, Ynew, S=0, noise_z=None, seed=None):
        """predict_responsibilities as a float32 device tensor [N, K]."""
        return self._responsibilities(Xnew, Ynew, S, ("resp",), noise_z=noise_z, seed=seed)["resp"]

    def predict_responsibilities(self, Xnew, Ynew, S=0, noise_z=None, seed=None):
        """The posterior responsibilities p(z = k | Xnew, Ynew), [N, K] (HostArray, float64):
        w_k N(Ynew | mu_k, s_k^2) normalised over k in the log domain, so a target far from every
        expert still gets finite values that sum to 1."""
        r = self.predict_responsibilities_device(Xnew, Ynew, S, noise_z=noise_z, seed=seed)
        self.check_linalg()
        return _host(r)

    def predict_labels_device(self, Xnew, Ynew, S=0, noise_z=None, seed=None):
        """predict_labels as an int32 device tensor [N]."""
        return self._responsibilities(Xnew, Ynew, S, ("labels",), noise_z=noise_z, seed=seed)["labels"]

    def predict_labels(self, Xnew, Ynew, S=0, noise_z=None, seed=None):
        """The expert that most probably produced each observation, int [N] (HostArray): the
        argmax of the responsibilities, decided on their logarithms, ties to the lowest k."""
        lab = self.predict_labels_device(Xnew, Ynew, S, noise_z=noise_z, seed=seed)
        self.check_linalg()
        return lab.cpu().numpy().astype(np.int64).view(HostArray)

    def predict_assignment_entropy_device(self, Xnew, Ynew, S=0, noise_z=None, seed=None):
        """predict_assignment_entropy as a float32 device tensor [N]."""
        return self._responsibilities(Xnew, Ynew, S, ("entropy",), noise_z=noise_z, seed=seed)["entropy"]

    def predict_assignment_entropy(self, Xnew, Ynew, S=0, noise_z=None, seed=None):
        """The entropy of the responsibilities per point in nats, [N] (HostArray, float64): 0
        where one expert explains the observation, log K where all do equally."""
        e = self.predict_assignment_entropy_device(Xnew, Ynew, S, noise_z=noise_z, seed=seed)
        self.check_linalg()
        return _host(e)

    def expert_usage_device(self, X, Y, S=0, noise_z=None, seed=None, n_offset=0, process_group=None):
        """expert_usage as a float64 device tensor [K] (no host sync)."""
        usage = self._responsibilities(X, Y, S, ("usage",), noise_z=noise_z, seed=seed, n_offset=n_offset)["usage"]
        if process_group is not None:
            import torch.distributed as dist
            dist.all_reduce(usage, op=dist.ReduceOp.SUM, group=process_group)
        return usage

    def expert_usage(self, X, Y, S=0, noise_z=None, seed=None, n_offset=0, process_group=None):
        """The effective number of points each expert explains, float64 [K] (HostArray): the
        responsibilities summed over the points (the values add up to N).  An expert whose
        count stays near 0 is dead.  n_offset / process_group: sharding over N as in crps (each
        rank passes its shard; one all-reduce of the K sums; without a group the shards' values
        add up to the one-call value)."""
        u = self.expert_usage_device(X, Y, S, noise_z=noise_z, seed=seed, n_offset=n_offset,
                                     process_group=process_group)
        self.check_linalg()
        return _host(u)

    def predict_modes_device(self, Xnew, S=0, noise_z=None, seed=None):
        """predict_modes as device tensors (float32 [N, K], float32 [N, K], int32 [N])."""
        out, (mu_f, var_f, lik_var) = self._mixture(Xnew, S, ("weights",), noise_z=noise_z, seed=seed)
        return ops.mixture_modes(mu_f, var_f, lik_var, out["weights"])

    def predict_modes(self, Xnew, S=0, noise_z=None, seed=None):
        """The modes of the mixture predictive per point -- its branches, where mean +- 2 sd
        points between them: (modes [N, K], density [N, K], count [N]) (HostArray; float64,
        float64, int).  Row n holds its count[n] modes in order of decreasing density, then NaN."""
        m, d, c = self.predict_modes_device(Xnew, S, noise_z=noise_z, seed=seed)
        self.check_linalg()
        return _host(m), _host(d), c.cpu().numpy().astype(np.int64).view(HostArray)

    def predict_map_device(self, Xnew, S=0, noise_z=None, seed=None):
        """predict_map as a float32 device tensor [N]."""
        return self.predict_modes_device(Xnew, S, noise_z=noise_z, seed=seed)[0][:, 0]

    def predict_map(self, Xnew, S=0, noise_z=None, seed=None):
        """The highest mode of the mixture predictive per point, [N] (HostArray, float64):
        column 0 of predict_modes."""
        m = self.predict_map_device(Xnew, S, noise_z=noise_z, seed=seed)
        self.check_linalg()
        return _host(m)

    def sample_paths(self, num_samples, num_features=1024, seed=None):
        """Coherent function samples of the trained mixture (paths.MixturePaths): `.pred` and
        `.assign` are SVGPModified.sample_paths of the two layers, and predict_f(X),
        predict_logits(X), predict_weights(X) = softmax_k of the logit curves [S, N, K] and
        predict_mean(X) = sum_k weights f [S, N] evaluate them at any X.  The relaxed-one-hot
        sampling of W at tau = 1e-2 is left out: it is discontinuous in the logits.  A
        MultiClass pred likelihood raises NotImplementedError from predict_mean."""
        for layer in (self.pred_layer, self.assign_layer):
            _matern_unsupported(layer.kernel, "sample_paths")
        from .paths import MixturePaths
        return MixturePaths(self, num_samples, num_features, seed=seed)


class SMGPModified(SMGP):
    """SMGP with a second (assignment) Gaussian likelihood on the assign layer
    (models.py:106-123): E_log_p_Y = lse_S(sum_k W ve_a) + lse_S(sum_k W ve_f) - 2 log S,
    both weighted by the same W.  The assign-layer conditional feeds both W and
    ve_a (the reference computes it twice, :113 and in W_dist); the data term is
    the MOD variant of K6 (mgp_elbo_terms_modified)."""

    def __init__(self, likelihood, assign_likelihood, pred_layer, assign_layer, K=3, num_samples=1,
                 num_data=None, seed=0):
        SMGP.__init__(self, likelihood, pred_layer, assign_layer, K, num_samples, num_data, seed)
        self.assign_likelihood = BroadcastingLikelihood(assign_likelihood)

    def _assign_lik_var(self):
        return self.assign_likelihood.likelihood.variance.reshape(-1)
