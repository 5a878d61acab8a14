"""Torch-tensor wrappers over the libmgp_hip C-ABI (device memory + streams only).

PyTorch is used here as plumbing: it allocates device buffers and supplies the
current HIP stream.  Every arithmetic op runs in a hand-written gfx950 kernel
of libmgp_hip.so; nothing here computes on the CPU or with torch kernels.

Layout conventions (see include/mgp_hip.h): float32, row-major, leading
dimensions padded to a multiple of 4 elements so rows can be read as float4.
``padded(rows, cols)`` returns such a view; the expert-major conditional
outputs are [K][N] views.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .config import default_jitter

F32 = torch.float32


def _round4(x):
    return (int(x) + 3) // 4 * 4


def _stream():
    return ctypes_stream(torch.cuda.current_stream())


def ctypes_stream(s):
    return s.cuda_stream


def padded(rows, cols, device, batch=None, dtype=F32, zero=False):
    """[batch?][rows][cols] view over storage whose rows are padded to a multiple of 4."""
    ld = _round4(max(cols, 1))
    shape = (rows, ld) if batch is None else (batch, rows, ld)
    fn = torch.zeros if zero else torch.empty
    buf = fn(shape, dtype=dtype, device=device)
    return buf[..., :cols]


def as_padded(t, device=None, dtype=F32):
    """Copy a 2-D/3-D tensor (or array) into padded storage (unless it already is)."""
    t = torch.as_tensor(t)
    device = device or t.device
    if (t.device == torch.device(device) and t.dtype == dtype and t.stride(-1) == 1
            and t.stride(-2) % 4 == 0 and t.data_ptr() % 16 == 0
            and (t.dim() == 2 or t.stride(0) % 4 == 0)):
        return t
    out = padded(t.shape[-2], t.shape[-1], device, batch=t.shape[0] if t.dim() == 3 else None,
                 dtype=dtype)
    out.copy_(t.to(device=device, dtype=dtype))
    return out


def _ld(t):
    if t.stride(-1) != 1:
        raise ValueError("innermost dimension must be contiguous")
    return t.stride(-2) if t.dim() >= 2 else t.shape[-1]


def _check(t, name, ndim=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"{name} must be a CUDA (HIP) tensor")
    if t.dtype != F32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"{name} must be {ndim}-D, got shape {tuple(t.shape)}")


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def _workspace(entry, dims, workspace, device, count=1):
    """`workspace` if it holds count * entry(*dims) bytes (entry: a *_bytes function of the
    library), else a new buffer that does."""
    nbytes = getattr(_lib.load(), entry)(*dims) * count
    if workspace is None or workspace.numel() < nbytes:
        workspace = _ws(nbytes, device)
    return workspace


def _ptrs(ts):
    """The c_void_p array of the tensors' pointers (None -> NULL) for _lib.call_raw: the
    wrappers of the ELBO step (kuu_potrf_trtri, split_upper_f16_bounded_batch,
    qsqrt_images_kl_f16_batch, trsm_stats_f16_batch, expert_conditional_f16_batch,
    elbo_terms, elbo_combine) convert their own pointers, because at small sizes the
    step's time is the host's and a generic pass over every argument shows in it."""
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _new_workspace(entry, dims, device):
    """A new workspace of entry(*dims) bytes; 0 bytes is the library refusing the sizes."""
    nbytes = getattr(_lib.load(), entry)(*dims)
    if nbytes == 0:
        _lib.check(entry, 3)
    return _ws(nbytes, device)


# --------------------------------------------------------------------------- K1 / K2
def rbf_kuf(X, Z, variance, lengthscales, out=None):
    """Kuf = K(Z, X) [M, N] (models.py:139)."""
    _check(X, "X", 2), _check(Z, "Z", 2), _check(variance, "variance"), _check(lengthscales, "lengthscales")
    N, D = X.shape
    M = Z.shape[0]
    if Z.shape[1] != D:
        raise ValueError("X and Z must have the same number of columns")
    if out is None:
        out = padded(M, N, X.device)
    _lib.call("mgp_rbf_kuf", X, _ld(X), Z, _ld(Z), N, M, D, variance, lengthscales, lengthscales.numel(), out,
              _ld(out), _stream())
    return out


def rbf_kuu(Z, variance, lengthscales, jitter, out=None):
    """Kuu = K(Z, Z) + jitter I [M, M] (models.py:135)."""
    _check(Z, "Z", 2)
    M, D = Z.shape
    if out is None:
        out = padded(M, M, Z.device)
    _lib.call("mgp_rbf_kuu", Z, _ld(Z), M, D, variance, lengthscales, lengthscales.numel(), float(jitter), out,
              _ld(out), _stream())
    return out


# --------------------------------------------------------------------------- K3
def potrf_trtri(A, L=None, LinvT=None, info=None, workspace=None):
    """Batched Cholesky + inverse of A [B, M, M] (lower part read).
    Returns L [B,M,M], LinvT [B,M,M] and info int32 [B] (device; 0 = success)."""
    _check(A, "A", 3)
    Bt, M, _ = A.shape
    dev = A.device
    if L is None:
        L = padded(M, M, dev, batch=Bt)
    if LinvT is None:
        LinvT = padded(M, M, dev, batch=Bt)
    if info is None:
        info = torch.empty(Bt, dtype=torch.int32, device=dev)
    workspace = _workspace("mgp_chol_workspace_bytes", (M, Bt), workspace, dev)
    if L.stride(0) != LinvT.stride(0) or _ld(L) != _ld(LinvT):
        raise ValueError("L and LinvT must share a layout")
    _lib.call("mgp_potrf_trtri", A, _ld(A), A.stride(0), M, Bt, L, LinvT, _ld(L), L.stride(0), info, workspace,
              workspace.numel(), _stream())
    return L, LinvT, info


def kuu_potrf_trtri(Zs, variances, lengthscales, jitter, LinvT=None, L=None, info=None,
                    workspace=None, want_L=False, prep_event=None, tfr_bound_images=None, kuf=None):
    """Kuu (float64, from Z) + Cholesky + inverse for a batch of layers sharing M, D.
    Zs / variances / lengthscales: lists of device tensors.  Returns L (or None),
    LinvT [B, M, M] and info int32 [B].  prep_event: a torch.cuda.Event (already
    created) recorded once Kuu is built (mgp_kuu_potrf_trtri_ev).
    tfr_bound_images: per layer, the L^-T split-f16 image buffer whose trailer
    receives max |LinvT| (mgp_kuu_potrf_trtri_ex; then split_upper_x6(...,
    bounded=True) skips its reduction).
    kuf: (X [N, D], [image per layer], fmt "f16" | "x6"): the factorisation's step
    launches also write each layer's Kuf image K(Z_b, X), bit-identical to
    rbf_kuf_x6(X, Z_b, ..., fmt=fmt) (mgp_kuu_potrf_trtri_kuf)."""
    Bt = len(Zs)
    M, D = Zs[0].shape
    ldz = _ld(Zs[0])
    for Z in Zs:
        _check(Z, "Z", 2)
        if tuple(Z.shape) != (M, D) or _ld(Z) != ldz:
            raise ValueError("all Z must share shape and leading dimension")
    dev = Zs[0].device
    if LinvT is None:
        LinvT = padded(M, M, dev, batch=Bt)
    if want_L and L is None:
        L = padded(M, M, dev, batch=Bt)
    if info is None:
        info = torch.empty(Bt, dtype=torch.int32, device=dev)
    workspace = _workspace("mgp_chol_workspace_bytes", (M, Bt), workspace, dev)
    nl = (ctypes.c_int32 * Bt)(*[l.numel() for l in lengthscales])
    args = [_ptrs(Zs), ldz, M, D, _ptrs(variances), _ptrs(lengthscales), nl, float(jitter), Bt,
            L.data_ptr() if L is not None else None, LinvT.data_ptr(), _ld(LinvT), LinvT.stride(0), info.data_ptr(),
            workspace.data_ptr(), workspace.numel()]
    # each variant's tail extends the one before it: _ev the event, _ex the bound pointers, _kuf the Kuf images
    variant = ("_kuf" if kuf is not None else "_ex" if tfr_bound_images is not None
               else "_ev" if prep_event is not None else "")
    if variant:
        args.append(prep_event.cuda_event if prep_event is not None else None)
    if variant in ("_ex", "_kuf"):
        bp = None
        if tfr_bound_images is not None:
            bound_ptr = _lib.load().mgp_x6_bound_ptr
            bp = (ctypes.c_void_p * Bt)(*[bound_ptr(t.data_ptr(), M, 0, 1) for t in tfr_bound_images])
        args.append(bp)
    if variant == "_kuf":
        X, imgs, fmt = kuf
        _check(X, "X", 2)
        if X.shape[1] != D or len(imgs) != Bt:
            raise ValueError("kuf: X must have Z's D columns and one image per layer")
        if min(t.numel() for t in imgs) < _lib.load().mgp_x6_cols_bytes(M, X.shape[0]):
            raise ValueError("kuf: an image buffer is smaller than mgp_x6_cols_bytes(M, N)")
        args += [X.data_ptr(), _ld(X), X.shape[0], _ptrs(imgs), min(t.numel() for t in imgs),
                 {"x6": 0, "f16": 1}[fmt]]
    _lib.call_raw("mgp_kuu_potrf_trtri" + variant, *args, _stream())
    return L, LinvT, info


def check_info(info):
    """Raise MGPLinAlgError if any factorisation reported a bad pivot (host sync)."""
    bad = info.cpu()
    if bool((bad != 0).any()):
        raise _lib.MGPLinAlgError("mgp_potrf_trtri", int(bad.max()),
                                  "Cholesky decomposition was not successful: the input might "
                                  "not be valid (non-positive pivot at column %s); a float32 "
                                  "covariance of densely spaced points may need a larger jitter"
                                  % bad.tolist())


# --------------------------------------------------------------------------- K4 / K5
MAX_EXPERTS_K4 = 16   # mgp_trsm_stats* and the conditional backward (MGP_ERR_UNSUPPORTED beyond)


def check_conditional_experts(K):
    """The layer conditional and its backward go through K4, which stops at K <= 16 (K5, K6
    and the SURVEY §8(b) front take K <= 32): refuse before anything is launched."""
    if K > MAX_EXPERTS_K4:
        raise ValueError(f"K = {K} experts: the conditional path (K4, mgp_trsm_stats*, and the conditional "
                         f"backward) supports K <= {MAX_EXPERTS_K4}")


def stats_tiles(M):
    return _lib.load().mgp_stats_tiles(M)


def trsm_stats(LinvT, Kuf, q_mu, A=None, stats=None):
    """A = L^-1 Kuf and per-row-tile column stats [T, K+1, N]."""
    _check(LinvT, "LinvT", 2), _check(Kuf, "Kuf", 2), _check(q_mu, "q_mu", 2)
    M, N = Kuf.shape
    K = q_mu.shape[1]
    dev = Kuf.device
    if A is None:
        A = padded(M, N, dev)
    if stats is None:
        T = stats_tiles(M)
        stats = padded(T * (K + 1), N, dev).unflatten(0, (T, K + 1))
    _lib.call("mgp_trsm_stats", LinvT, _ld(LinvT), Kuf, _ld(Kuf), M, N, q_mu, _ld(q_mu), K, A, _ld(A), stats,
              _ld(stats), _stream())
    return A, stats


def rbf_kuf_x6(X, Z, variance, lengthscales, out=None, fmt="x6"):
    """K1 writing the split-bf16 image of Kuf = K(Z, X) (uint8 device tensor);
    fmt "f16": the split-f16 image (mgp_rbf_kuf_f16) for trsm_stats_x6(..., in_fmt="f16")."""
    _check(X, "X", 2), _check(Z, "Z", 2)
    N, D = X.shape
    M = Z.shape[0]
    out = _workspace("mgp_x6_cols_bytes", (M, N), out, X.device)
    _lib.call("mgp_rbf_kuf_" + _fmt(fmt), X, _ld(X), Z, _ld(Z), N, M, D, variance, lengthscales, lengthscales.numel(),
              out, out.numel(), _stream())
    return out


def split_upper_x6(LinvT, out=None, fmt="x6", bounded=False):
    """Split-bf16 image of (L^-1)^T [M, M] (upper triangle) as K4's T operand
    (fmt "f16": the split-f16 image, mgp_split_upper_f16; bounded: `out`'s trailer
    already holds max |LinvT| from kuu_potrf_trtri(..., tfr_bound_images=...),
    mgp_split_upper_f16_bounded)."""
    _check(LinvT, "LinvT", 2)
    M = LinvT.shape[0]
    if bounded and (fmt != "f16" or out is None):
        raise ValueError("bounded splits are split-f16 into the image that received the bound")
    out = _workspace("mgp_x6_lower_bytes", (M, 1), out, LinvT.device)
    name = "mgp_split_upper_f16_bounded" if bounded else "mgp_split_upper_" + _fmt(fmt)
    _lib.call(name, LinvT, _ld(LinvT), M, out, out.numel(), _stream())
    return out


def split_upper_f16_bounded_batch(LinvT, outs):
    """split_upper_x6(LinvT[b], out=outs[b], fmt="f16", bounded=True) for every matrix of
    LinvT [B, M, M] (B = len(outs) <= 2) in one launch (mgp_split_upper_f16_bounded_batch)."""
    _check(LinvT, "LinvT", 3)
    n, M = len(outs), LinvT.shape[1]
    if LinvT.shape[0] < n:
        raise ValueError("one LinvT matrix per image")
    _lib.call_raw("mgp_split_upper_f16_bounded_batch", n, LinvT.data_ptr(), _ld(LinvT), LinvT.stride(0), M,
                  _ptrs(outs), min(o.numel() for o in outs), _stream())
    return list(outs)


def trsm_stats_x6(Tfr, Kfr, q_mu, M, N, Afr=None, stats=None, A=None, f16_variance=None, in_fmt="x6", cross=None):
    """K4 on images: A's image (for expert_conditional_x6) and the stats [T, K+1, N];
    also the f32 A when a buffer `A` [M, N] is given (training).  f16_variance
    (the layer's kernel variance): A's image is split-f16 instead
    (mgp_trsm_stats_x6_f16, for expert_conditional_x6(..., fmt="f16")).
    in_fmt "f16": Tfr and Kfr are split-f16 images (split_upper_x6 / rbf_kuf_x6 with
    fmt "f16"; mgp_trsm_stats_f16, needs f16_variance).
    cross "f8" (default: config.expert_cross()) with split-f16 inputs: A's image also
    carries the e4m3 cross-term plane of expert_conditional_x6(..., cross="f8")
    (mgp_trsm_stats_f16x8)."""
    _check(q_mu, "q_mu", 2)
    K = q_mu.shape[1]
    dev = q_mu.device
    Afr = _workspace("mgp_x6_cols_bytes", (M, N), Afr, dev)
    if stats is None:
        T = stats_tiles(M)
        stats = padded(T * (K + 1), N, dev).unflatten(0, (T, K + 1))
    args = [Tfr, Tfr.numel(), Kfr, Kfr.numel(), M, N, q_mu, _ld(q_mu), K]
    out_args = [Afr, Afr.numel(), stats, _ld(stats)]
    a_args = [A, _ld(A) if A is not None else N]
    if f16_variance is None:
        if _fmt(in_fmt) != "x6":
            raise ValueError("split-f16 K4 inputs need the split-f16 output (f16_variance)")
        _lib.call("mgp_trsm_stats_x6", *args, *out_args, *a_args, _stream())
    elif _fmt(in_fmt) == "x6":
        if A is not None:
            raise ValueError("the split-bf16 -> split-f16 K4 does not write the f32 A")
        _lib.call("mgp_trsm_stats_x6_f16", *args, f16_variance, *out_args, _stream())
    else:
        from .config import expert_cross
        entry = "mgp_trsm_stats_f16x8" if (cross or expert_cross()) == "f8" else "mgp_trsm_stats_f16"
        _lib.call(entry, *args, f16_variance, *out_args, *a_args, _stream())
    return Afr, stats


def trsm_stats_f16_batch(Tfrs, Kfrs, q_mus, M, N, Afrs, statss, variances, As=None):
    """K4 of several layers (1 or 2, equal M, N, K) in one launch (mgp_trsm_stats_f16_batch):
    trsm_stats_x6(Tfr, Kfr, q_mu, M, N, Afr=Afr, stats=stats, A=A, f16_variance=variance,
    in_fmt="f16", cross="f16") for each layer, bit-identical.  Afrs / statss: the output
    buffers (required); As: f32 A buffers or None."""
    n = len(Tfrs)
    for seq in (Kfrs, q_mus, Afrs, statss, variances) + ((As,) if As is not None else ()):
        if len(seq) != n:
            raise ValueError("one entry per layer in every operand list")
    K = q_mus[0].shape[1]
    ldq, lds = _ld(q_mus[0]), _ld(statss[0])
    for q, st in zip(q_mus, statss):
        _check(q, "q_mu", 2)
        if q.shape[1] != K or _ld(q) != ldq or _ld(st) != lds:
            raise ValueError("the layers' q_mu / stats must share K and leading dimensions")
    lda = N
    if As is not None:
        lda = _ld(As[0])
        if any(_ld(a) != lda for a in As):
            raise ValueError("the f32 A buffers must share a leading dimension")
    _lib.call_raw("mgp_trsm_stats_f16_batch", n, _ptrs(Tfrs), min(t.numel() for t in Tfrs), _ptrs(Kfrs),
                  min(t.numel() for t in Kfrs), M, N, _ptrs(q_mus), ldq, K, _ptrs(variances), _ptrs(Afrs),
                  min(t.numel() for t in Afrs), _ptrs(statss), lds, _ptrs(As) if As is not None else None, lda,
                  _stream())
    return list(zip(Afrs, statss))


def expert_workspace_bytes(M, N, K):
    return max(int(_lib.load().mgp_expert_workspace_bytes(M, N, K)), 16)


def expert_x6_workspace_bytes(M, N, K):
    return max(int(_lib.load().mgp_expert_x6_workspace_bytes(M, N, K)), 16)


def x6_cols_bytes(M, N):
    return int(_lib.load().mgp_x6_cols_bytes(M, N))


def x6_lower_bytes(M, K):
    return int(_lib.load().mgp_x6_lower_bytes(M, K))


def expert_conditional(A, q_sqrt, stats, variance, fmean=None, fvar=None, workspace=None):
    """fmean, fvar [K, N] of the whitened K-expert conditional."""
    _check(A, "A", 2), _check(q_sqrt, "q_sqrt", 3), _check(stats, "stats", 3)
    M, N = A.shape
    K = q_sqrt.shape[0]
    dev = A.device
    if fmean is None:
        fmean = padded(K, N, dev)
    if fvar is None:
        fvar = padded(K, N, dev)
    if _ld(fmean) != _ld(fvar):
        raise ValueError("fmean and fvar must share a leading dimension")
    workspace = _workspace("mgp_expert_workspace_bytes", (M, N, K), workspace, dev)
    _lib.call("mgp_expert_conditional_f32", A, _ld(A), q_sqrt, _ld(q_sqrt), q_sqrt.stride(0), stats, _ld(stats),
              variance, M, N, K, fmean, fvar, _ld(fmean), workspace, workspace.numel(), _stream())
    return fmean, fvar


def full_cov_workspace_bytes(M, N, K):
    return max(int(_lib.load().mgp_full_cov_workspace_bytes(M, N, K)), 16)


def full_cov_conditional(X, A, q_sqrt, variance, lengthscales, out=None, workspace=None):
    """cov [K, N, N] of the whitened conditional with full_cov=True (base_conditional,
    models.py:133-143): K(X, X) - A^T A + (L_k^T A)^T (L_k^T A) per expert, from the f32
    A = L^-1 Kuf [M, N] that K4 writes (trsm_stats, or trsm_stats_x6 with an A buffer).
    The result is a view of padded storage (leading dimension % 4 == 0), each cov[k]
    bitwise symmetric; `out`, if given, must be such a view."""
    _check(X, "X", 2), _check(A, "A", 2), _check(q_sqrt, "q_sqrt", 3)
    _check(variance, "variance"), _check(lengthscales, "lengthscales")
    N, D = X.shape
    M = A.shape[0]
    K = q_sqrt.shape[0]
    if A.shape[1] != N or tuple(q_sqrt.shape[1:]) != (M, M):
        raise ValueError(f"expected A [M, {N}] and q_sqrt [K, M, M], got {tuple(A.shape)} and {tuple(q_sqrt.shape)}")
    dev = X.device
    if out is None:
        out = padded(N, N, dev, batch=K)
    elif tuple(out.shape) != (K, N, N):
        raise ValueError(f"out must be [{K}, {N}, {N}]")
    workspace = _workspace("mgp_full_cov_workspace_bytes", (M, N, K), workspace, dev)
    _lib.call("mgp_full_cov_conditional", X, _ld(X), N, D, variance, lengthscales, lengthscales.numel(), A, _ld(A),
              q_sqrt, _ld(q_sqrt), q_sqrt.stride(0), M, K, out, _ld(out), out.stride(0), workspace, workspace.numel(),
              _stream())
    return out


# ------------------------------------------------------------ K5, split-bf16 (x6)
def _fmt(fmt):
    if fmt not in ("x6", "f16"):
        raise ValueError("image format must be 'x6' (split-bf16) or 'f16' (split-f16)")
    return fmt


def split_lower_x6(q_sqrt, out=None, fmt="x6"):
    """Fragment image (uint8 device tensor) of L_k = tril(q_sqrt[k]) for the split-bf16
    K5 (fmt "f16": the split-f16 image, mgp_split_lower_f16)."""
    _check(q_sqrt, "q_sqrt", 3)
    K, M = q_sqrt.shape[0], q_sqrt.shape[1]
    out = _workspace("mgp_x6_lower_bytes", (M, K), out, q_sqrt.device)
    _lib.call("mgp_split_lower_" + _fmt(fmt), q_sqrt, _ld(q_sqrt), q_sqrt.stride(0), M, K, out, out.numel(), _stream())
    return out


def qsqrt_images_kl_f16_batch(q_mus, q_sqrts, Lfrs, kl_outs, workspace=None):
    """Both layers' split-f16 tril(q_sqrt) images (split_lower_x6(q_sqrt, fmt="f16")) and
    whitened KL terms (gauss_kl_white(q_mu, q_sqrt), float64 [1] each) in three launches
    (mgp_qsqrt_images_kl_f16_batch; bit-identical).  Layers share q_mu / q_sqrt shapes."""
    n = len(q_mus)
    q_sqrts = [as_padded(t) for t in q_sqrts]   # float4 rows (no copy for the layers' storage)
    M, K = q_mus[0].shape
    for qm, qs, lf, kl in zip(q_mus, q_sqrts, Lfrs, kl_outs):
        _check(qm, "q_mu", 2), _check(qs, "q_sqrt", 3)
        if (tuple(qm.shape) != (M, K) or tuple(qs.shape) != (K, M, M) or _ld(qm) != _ld(q_mus[0])
                or _ld(qs) != _ld(q_sqrts[0]) or qs.stride(0) != q_sqrts[0].stride(0)):
            raise ValueError("every layer's q_mu [M, K] / q_sqrt [K, M, M] must share shape and strides")
        if kl.dtype != torch.float64 or kl.numel() < 1:
            raise ValueError("kl_out: float64 tensors of at least one element")
    workspace = _workspace("mgp_qsqrt_workspace_bytes", (M, K), workspace, q_mus[0].device, count=n)
    _lib.call_raw("mgp_qsqrt_images_kl_f16_batch", n, _ptrs(q_mus), _ld(q_mus[0]), _ptrs(q_sqrts), _ld(q_sqrts[0]),
                  q_sqrts[0].stride(0), M, K, _ptrs(Lfrs), min(t.numel() for t in Lfrs), _ptrs(kl_outs),
                  workspace.data_ptr(), workspace.numel(), _stream())
    return Lfrs, kl_outs


def split_cols_x6(A, out=None, fmt="x6"):
    """Fragment image (uint8 device tensor) of A [M, N] for the split-bf16 K5
    (fmt "f16": the split-f16 image, mgp_split_cols_f16)."""
    _check(A, "A", 2)
    M, N = A.shape
    out = _workspace("mgp_x6_cols_bytes", (M, N), out, A.device)
    _lib.call("mgp_split_cols_" + _fmt(fmt), A, _ld(A), M, N, out, out.numel(), _stream())
    return out


def expert_conditional_x6(Afr, Lfr, stats, variance, M, N, K, fmean=None, fvar=None, workspace=None, planes=3,
                          fmt="x6", cross=None, c_out=None):
    """fmean, fvar [K, N] of the whitened K-expert conditional from split-bf16 images
    (planes < 3: K5 on the leading bf16 planes only, mgp_expert_conditional_planes;
    fmt "f16": from split-f16 images, mgp_expert_conditional_f16, or with cross "f8"
    (default: config.expert_cross()) mgp_expert_conditional_f16x8, the cross terms
    on the e4m3 MFMA).  c_out = (Cfr, colmax) (f16, cross "f16"; colmax from colnorm_max):
    also write C_k = L_k^T A as images for the backward (mgp_expert_conditional_f16c)."""
    _check(stats, "stats", 3)
    dev = stats.device
    if fmean is None:
        fmean = padded(K, N, dev)
    if fvar is None:
        fvar = padded(K, N, dev)
    if _ld(fmean) != _ld(fvar):
        raise ValueError("fmean and fvar must share a leading dimension")
    workspace = _workspace("mgp_expert_x6_workspace_bytes", (M, N, K), workspace, dev)
    args = [Afr, Afr.numel(), Lfr, Lfr.numel(), stats, _ld(stats), variance, M, N, K]
    out_args = [fmean, fvar, _ld(fmean), workspace, workspace.numel()]
    if _fmt(fmt) == "f16":
        from .config import expert_cross
        entry = "mgp_expert_conditional_f16x8" if (cross or expert_cross()) == "f8" else "mgp_expert_conditional_f16"
        if c_out is not None:
            if entry != "mgp_expert_conditional_f16":
                raise ValueError("c_out needs f16 cross terms")
            Cfr, colmax = c_out
            entry = "mgp_expert_conditional_f16c"
            out_args += [Cfr, Cfr.numel(), colmax]
        _lib.call(entry, *args, *out_args, _stream())
    elif planes == 3:
        _lib.call("mgp_expert_conditional_x6", *args, *out_args, _stream())
    else:
        _lib.call("mgp_expert_conditional_planes", *args, int(planes), *out_args, _stream())
    return fmean, fvar


def expert_conditional_f16_batch(Afrs, Lfrs, statss, variances, M, N, K, fmeans, fvars, workspaces, c_outs=None):
    """K5 of several layers (1 or 2, equal M, N, K) in one launch
    (mgp_expert_conditional_f16_batch): expert_conditional_x6(Afr, Lfr, stats, variance, M, N, K,
    fmean=..., fvar=..., workspace=..., fmt="f16", cross="f16", c_out=...) for each layer,
    bit-identical.  Outputs and one workspace per layer are required; c_outs: a
    (Cfr, colmax) per layer (training) or None."""
    n = len(Afrs)
    lists = (Lfrs, statss, variances, fmeans, fvars, workspaces) + ((c_outs,) if c_outs is not None else ())
    if any(len(x) != n for x in lists):
        raise ValueError("one entry per layer in every operand list")
    lds, ldf = _ld(statss[0]), _ld(fmeans[0])
    if any(_ld(t) != lds for t in statss) or any(_ld(t) != ldf for t in list(fmeans) + list(fvars)):
        raise ValueError("the layers' stats / fmean / fvar must share leading dimensions")
    cf = cm = None
    cb = 0
    if c_outs is not None:
        cf, cm = _ptrs([c[0] for c in c_outs]), _ptrs([c[1] for c in c_outs])
        cb = min(c[0].numel() for c in c_outs)
    _lib.call_raw("mgp_expert_conditional_f16_batch", n, _ptrs(Afrs), min(t.numel() for t in Afrs), _ptrs(Lfrs),
                  min(t.numel() for t in Lfrs), _ptrs(statss), lds, _ptrs(variances), M, N, K, _ptrs(fmeans),
                  _ptrs(fvars), ldf, _ptrs(workspaces), min(t.numel() for t in workspaces), cf, cb, cm, _stream())
    return list(zip(fmeans, fvars))


def elbo_terms_backward(mu_f, var_f, mu_a, var_a, Y, lik_var, S, tau=1e-2, noise=None, seed=0,
                        n_offset=0, scale=1.0, assign_lik_var=None, G=None, workspace=None, multiclass_eps=None,
                        jitter=None):
    """Gradient of the data term: G [4, K, N] = scale * d/d(mu_f, var_f, mu_a, var_a) and the
    likelihood-variance gradients (float64 [K]; second one for SMGPModified, else None).
    multiclass_eps: MultiClass / RobustMax pred likelihood (no likelihood-variance gradient: None)."""
    jitter = default_jitter() if jitter is None else jitter
    for t, n in ((mu_f, "mu_f"), (var_f, "var_f"), (mu_a, "mu_a"), (var_a, "var_a")):
        _check(t, n, 2)
    ldf = _ld(mu_f)
    if not (_ld(var_f) == _ld(mu_a) == _ld(var_a) == ldf):
        raise ValueError("conditional outputs must share a leading dimension")
    K, N = mu_f.shape
    dev = mu_f.device
    Y = Y.reshape(-1)
    _check(Y, "Y")
    if multiclass_eps is None:
        _check(lik_var, "lik_var")
    if G is None:
        G = padded(4 * K, N, dev).unflatten(0, (4, K))
    # the kernel addresses G's 4K rows as one [4K][ldg] block: the row stride from
    # G's outer dimension (a K = 1 view's stride(1) is torch's contiguous placeholder,
    # N, not the padded row length)
    if G.dim() != 3 or tuple(G.shape) != (4, K, N) or G.stride(2) != 1 or G.stride(0) % K:
        raise ValueError("G must be a [4, K, N] view of [4K][ldg] rows")
    ldg = G.stride(0) // K
    if K > 1 and G.stride(1) != ldg:
        raise ValueError("G must be a [4, K, N] view of [4K][ldg] rows")
    glv = torch.empty(K, dtype=torch.float64, device=dev) if multiclass_eps is None else None
    glva = torch.empty(K, dtype=torch.float64, device=dev) if assign_lik_var is not None else None
    workspace = _workspace("mgp_elbo_backward_workspace_bytes", (N, K), workspace, dev)
    z = u = None
    if noise is not None:
        z, u = noise
        z, u = z.contiguous(), u.contiguous()
    # the multiclass entry takes epsilon in lik_var's place and has no lik_var gradient
    entry, lik, g_lik = "mgp_elbo_terms_backward", lik_var, [glv, glva]
    if multiclass_eps is not None:
        entry, lik, g_lik = "mgp_elbo_terms_multiclass_backward", float(multiclass_eps), [glva]
    _lib.call(entry, mu_f, var_f, mu_a, var_a, ldf, Y, lik, assign_lik_var, N, K, S, float(tau), float(jitter), z, u,
              int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_offset), float(scale), G, ldg, *g_lik, workspace, workspace.numel(),
              _stream())
    return G, glv, glva


def rbf_backward(X, Z, variance, lengthscales, gK, symmetric=False, accumulate=False, gZ=None, g_var=None,
                 g_ls=None, workspace=None):
    """Reverse mode of K(Z, X): (gZ [M, D] float32, g_var float64 [1], g_ls float64 [n_ls])."""
    _check(X, "X", 2), _check(Z, "Z", 2), _check(gK, "gK", 2)
    N, D = X.shape
    M = Z.shape[0]
    dev = X.device
    n_ls = lengthscales.numel()
    if gZ is None:
        gZ = torch.zeros(M, D, dtype=torch.float32, device=dev)
    if g_var is None:
        g_var = torch.zeros(1, dtype=torch.float64, device=dev)
    if g_ls is None:
        g_ls = torch.zeros(n_ls, dtype=torch.float64, device=dev)
    workspace = _workspace("mgp_rbf_backward_workspace_bytes", (N, M, D), workspace, dev)
    _lib.call("mgp_rbf_backward", X, _ld(X), Z, _ld(Z), N, M, D, variance, lengthscales, n_ls, gK, _ld(gK),
              int(symmetric), int(accumulate), gZ, _ld(gZ), g_var, g_ls, workspace, workspace.numel(), _stream())
    return gZ, g_var, g_ls


# --------------------------------------------------------------------------- Matern kernels
def _nu2(nu2):
    if nu2 not in (3, 5):
        raise ValueError("nu2 (twice the Matern smoothness) must be 3 or 5")
    return int(nu2)


def matern_kuf(X, Z, variance, lengthscales, nu2, out=None):
    """Matern Kuf = K(Z, X) [M, N] float32 (mgp_matern_kuf)."""
    _check(X, "X", 2), _check(Z, "Z", 2), _check(variance, "variance"), _check(lengthscales, "lengthscales")
    N, D = X.shape
    M = Z.shape[0]
    if Z.shape[1] != D:
        raise ValueError("X and Z must have the same number of columns")
    if out is None:
        out = padded(M, N, X.device)
    _lib.call("mgp_matern_kuf", X, _ld(X), Z, _ld(Z), N, M, D, variance, lengthscales, lengthscales.numel(),
              _nu2(nu2), out, _ld(out), _stream())
    return out


def matern_kuu(Z, variance, lengthscales, nu2, jitter, out=None):
    """Matern Kuu = K(Z, Z) + jitter I [M, M] float32 (mgp_matern_kuu)."""
    _check(Z, "Z", 2)
    M, D = Z.shape
    if out is None:
        out = padded(M, M, Z.device)
    _lib.call("mgp_matern_kuu", Z, _ld(Z), M, D, variance, lengthscales, lengthscales.numel(), _nu2(nu2),
              float(jitter), out, _ld(out), _stream())
    return out


def matern_kuf_image(X, Z, variance, lengthscales, nu2, out=None, fmt="x6"):
    """K1 for Matern: the fragment image of Kuf = K(Z, X) (uint8 device tensor), split-bf16
    (fmt "x6") or split-f16 ("f16"), as rbf_kuf_x6 writes it (mgp_matern_kuf_image)."""
    _check(X, "X", 2), _check(Z, "Z", 2)
    N, D = X.shape
    M = Z.shape[0]
    out = _workspace("mgp_x6_cols_bytes", (M, N), out, X.device)
    _lib.call("mgp_matern_kuf_image", X, _ld(X), Z, _ld(Z), N, M, D, variance, lengthscales, lengthscales.numel(),
              _nu2(nu2), out, out.numel(), {"x6": 0, "f16": 1}[_fmt(fmt)], _stream())
    return out


def matern_kuu_potrf_trtri(Z, variance, lengthscales, nu2, jitter, LinvT=None, L=None, info=None, workspace=None,
                           want_L=False):
    """One layer's Matern Kuu (float64, from Z) + Cholesky + inverse (mgp_matern_kuu_potrf_trtri):
    L (or None), LinvT [1, M, M] and info int32 [1], as kuu_potrf_trtri returns them."""
    _check(Z, "Z", 2)
    M, D = Z.shape
    dev = Z.device
    if LinvT is None:
        LinvT = padded(M, M, dev, batch=1)
    if want_L and L is None:
        L = padded(M, M, dev, batch=1)
    if L is not None and _ld(L) != _ld(LinvT):
        raise ValueError("L and LinvT must share a layout")
    if info is None:
        info = torch.empty(1, dtype=torch.int32, device=dev)
    workspace = _workspace("mgp_matern_chol_workspace_bytes", (M,), workspace, dev)
    _lib.call("mgp_matern_kuu_potrf_trtri", Z, _ld(Z), M, D, variance, lengthscales, lengthscales.numel(), _nu2(nu2),
              float(jitter), L, LinvT, _ld(LinvT), info, workspace, workspace.numel(), _stream())
    return L, LinvT, info


def matern_backward(X, Z, variance, lengthscales, nu2, gK, symmetric=False, accumulate=False, gZ=None, g_var=None,
                    g_ls=None, workspace=None):
    """Reverse mode of the Matern K(Z, X), as rbf_backward (mgp_matern_backward)."""
    _check(X, "X", 2), _check(Z, "Z", 2), _check(gK, "gK", 2)
    N, D = X.shape
    M = Z.shape[0]
    dev = X.device
    n_ls = lengthscales.numel()
    if gZ is None:
        gZ = torch.zeros(M, D, dtype=torch.float32, device=dev)
    if g_var is None:
        g_var = torch.zeros(1, dtype=torch.float64, device=dev)
    if g_ls is None:
        g_ls = torch.zeros(n_ls, dtype=torch.float64, device=dev)
    workspace = _workspace("mgp_matern_backward_workspace_bytes", (N, M, D), workspace, dev)
    _lib.call("mgp_matern_backward", X, _ld(X), Z, _ld(Z), N, M, D, variance, lengthscales, n_ls, _nu2(nu2), gK,
              _ld(gK), int(symmetric), int(accumulate), gZ, _ld(gZ), g_var, g_ls, workspace, workspace.numel(),
              _stream())
    return gZ, g_var, g_ls


def _same_ld(ts, what):
    if any(_ld(t) != _ld(ts[0]) for t in ts):
        raise ValueError(f"every layer's {what} must share its leading dimension")
    return _ld(ts[0])


def rbf_backward_batch(X, Zs, variances, lengthscales, gKufs, gKuus, gZs, g_vars, g_lss, accumulate=True,
                       workspace=None):
    """Per layer b: rbf_backward(X, Z[b], .., gKuf[b], accumulate) then
    rbf_backward(Z[b], Z[b], .., gKuu[b], symmetric=True, accumulate=True) into
    gZ[b], g_var[b], g_ls[b], for all layers in three launches (mgp_rbf_backward_batch;
    bit-identical).  accumulate 2: gZ / g_ls overwritten, g_var added to."""
    _check(X, "X", 2)
    N, D = X.shape
    Zs, variances, lengthscales, gKufs, gKuus, gZs, g_vars, g_lss = map(
        list, (Zs, variances, lengthscales, gKufs, gKuus, gZs, g_vars, g_lss))   # any sequence of tensors
    n = len(Zs)
    M = Zs[0].shape[0]
    n_ls = lengthscales[0].numel()
    for z, gf, gu in zip(Zs, gKufs, gKuus):
        _check(z, "Z", 2), _check(gf, "gKuf", 2), _check(gu, "gKuu", 2)
        if tuple(z.shape) != (M, D):
            raise ValueError("every layer's Z must be [M, D]")
    if any(t.numel() != n_ls for t in lengthscales):
        raise ValueError("every layer's lengthscales must have the same size")
    workspace = _workspace("mgp_rbf_backward_batch_workspace_bytes", (N, M, D), workspace, X.device, count=n)
    _lib.call("mgp_rbf_backward_batch", n, X, _ld(X), N, Zs, _same_ld(Zs, "Z"), M, D, variances, lengthscales, n_ls,
              gKufs, _same_ld(gKufs, "gKuf"), gKuus, _same_ld(gKuus, "gKuu"), int(accumulate), gZs,
              _same_ld(gZs, "gZ"), g_vars, g_lss, workspace, workspace.numel(), _stream())
    return gZs, g_vars, g_lss


def chol_backward_batch(Ls, LinvTs, gLs, outs=None, workspace=None):
    """chol_backward for every layer (same M) in five launches (mgp_chol_backward_batch;
    bit-identical): list of gKuu [M, M]."""
    Ls, LinvTs, gLs = list(Ls), list(LinvTs), list(gLs)   # any sequence of tensors
    n = len(Ls)
    M = Ls[0].shape[0]
    for t in Ls + LinvTs + gLs:
        _check(t, "L / LinvT / gL", 2)
        if tuple(t.shape) != (M, M):
            raise ValueError("every layer's L, LinvT and gL must be [M, M]")
    if outs is None:
        outs = [padded(M, M, Ls[0].device) for _ in range(n)]
    workspace = _workspace("mgp_chol_backward_workspace_bytes", (M,), workspace, Ls[0].device, count=n)
    _lib.call("mgp_chol_backward_batch", n, Ls, _same_ld(Ls, "L"), LinvTs, _same_ld(LinvTs, "LinvT"), gLs,
              _same_ld(gLs, "gL"), M, list(outs), _same_ld(outs, "gKuu"), workspace, workspace.numel(), _stream())
    return outs


def chol_backward(L, LinvT, gL, out=None, workspace=None):
    """gKuu [M, M] (float32, symmetric) from the gradient w.r.t. Lm = chol(Kuu)."""
    _check(L, "L", 2), _check(LinvT, "LinvT", 2), _check(gL, "gL", 2)
    M = L.shape[0]
    if out is None:
        out = padded(M, M, L.device)
    workspace = _workspace("mgp_chol_backward_workspace_bytes", (M,), workspace, L.device)
    _lib.call("mgp_chol_backward", L, _ld(L), LinvT, _ld(LinvT), gL, _ld(gL), M, out, _ld(out), workspace,
              workspace.numel(), _stream())
    return out


def kl_grad(q_mu, q_sqrt, num_data, g_q_mu, g_q_sqrt):
    """Fold -KL / num_data into the ELBO gradients (in place)."""
    M, K = q_mu.shape
    _lib.call("mgp_kl_grad", q_mu, _ld(q_mu), q_sqrt, _ld(q_sqrt), q_sqrt.stride(0), M, K, float(num_data), g_q_mu,
              _ld(g_q_mu), g_q_sqrt, _ld(g_q_sqrt), g_q_sqrt.stride(0), _stream())


def adam_step(theta, grad, m1, m2, t, lr, u=None, beta1=0.9, beta2=0.999, eps=1e-7, grad_sign=-1.0):
    """One TF-legacy Adam step on theta (2-D view [rows, cols] with leading dimension),
    gradient of the ELBO (grad_sign -1 minimises -ELBO); u: unconstrained softplus shadow."""
    rows, cols = theta.shape
    if grad.shape[-1] != cols:
        raise ValueError("gradient / parameter shape mismatch")
    _lib.call("mgp_adam_step", theta, u, grad, int(grad.dtype == torch.float64), _ld(grad), m1, m2, rows, cols,
              _ld(theta), float(lr), float(beta1), float(beta2), float(eps), int(t), float(grad_sign), _stream())


class AdamSet:
    """adam_step over a fixed list of parameter blocks in one launch (mgp_adam_step_set;
    bit-identical to one adam_step per block).  blocks: (theta 2-D view, m1, m2, u or
    None); the pointer arrays of the fixed state are built once."""

    def __init__(self, blocks):
        n = len(blocks)
        if not 1 <= n <= 16:
            raise ValueError("AdamSet takes 1 .. 16 parameter blocks")
        I64 = ctypes.c_int64 * n
        self.n = n
        self.shapes = [tuple(th.shape) for th, *_ in blocks]
        self.theta, self.m1, self.m2, self.u = (_lib.marshal(list(ts)) for ts in zip(*blocks))
        self.rows = I64(*[s[0] for s in self.shapes])
        self.cols = I64(*[s[1] for s in self.shapes])
        self.ld = I64(*[_ld(th) for th, *_ in blocks])
        self._keep = blocks
        self._I64, self._I32 = I64, ctypes.c_int32 * n

    def step(self, grads, t, lr, beta1=0.9, beta2=0.999, eps=1e-7, grad_sign=-1.0):
        """grads: one 2-D gradient per block, in order (float32 or float64)."""
        if len(grads) != self.n:
            raise ValueError(f"AdamSet.step takes {self.n} gradients, got {len(grads)}")
        dev = self._keep[0][0].device
        for j, (gr, s) in enumerate(zip(grads, self.shapes)):
            # the kernel reads rows x cols at the gradient's leading dimension: every block must
            # match its parameter's shape exactly, be float32 / float64, row-contiguous and on
            # the parameters' device
            if tuple(gr.shape) != s:
                raise ValueError(f"gradient {j}: shape {tuple(gr.shape)} != parameter shape {s}")
            if gr.dtype not in (torch.float32, torch.float64):
                raise ValueError(f"gradient {j}: dtype {gr.dtype} (float32 or float64 expected)")
            if gr.numel() and (gr.stride(-1) != 1 or gr.device != dev):
                raise ValueError(f"gradient {j}: must be row-contiguous on {dev}")
        _lib.call("mgp_adam_step_set", self.n, self.theta, self.u, list(grads),
                  self._I32(*[int(gr.dtype == torch.float64) for gr in grads]), self._I64(*[_ld(gr) for gr in grads]),
                  self.m1, self.m2, self.rows, self.cols, self.ld, float(lr), float(beta1), float(beta2), float(eps),
                  int(t), float(grad_sign), _stream())


def natgrad_workspace(M, K, device):
    return _new_workspace("mgp_natgrad_workspace_bytes", (M, K), device)


def natgrad_step(q_mu, q_sqrt, g_q_mu, g_q_sqrt, step, grad_sign=-1.0, info=None, workspace=None):
    """One natural-gradient step (mgp_natgrad_step; gpflow.optimizers.NaturalGradient with
    XiSqrtMeanVar) on q_mu [M, K] and q_sqrt [K, M, M], in place, from the gradients
    g_q_mu [M, K] / g_q_sqrt [K, M, M] (both float32 or both float64; grad_sign -1: they are
    the ELBO's, as elbo_and_grad returns them).  Returns info, device int32 [K]: 0, or the
    pivot column where the step does not exist (that expert is left unchanged).  No
    synchronisation with the host."""
    _check(q_mu, "q_mu", 2), _check(q_sqrt, "q_sqrt", 3)
    M, K = q_mu.shape
    if tuple(q_sqrt.shape) != (K, M, M):
        raise ValueError(f"q_sqrt must be [{K}, {M}, {M}], got {tuple(q_sqrt.shape)}")
    if tuple(g_q_mu.shape) != (M, K) or tuple(g_q_sqrt.shape) != (K, M, M):
        raise ValueError("gradient / parameter shape mismatch")
    if g_q_mu.dtype != g_q_sqrt.dtype or g_q_mu.dtype not in (torch.float32, torch.float64):
        raise ValueError("g_q_mu and g_q_sqrt must both be float32 or both float64")
    for t, name in ((g_q_mu, "g_q_mu"), (g_q_sqrt, "g_q_sqrt")):
        if not t.is_cuda or t.device != q_mu.device:
            raise ValueError(f"{name} must be on {q_mu.device}")
    if info is None:
        info = torch.empty(K, dtype=torch.int32, device=q_mu.device)
    nbytes = _lib.load().mgp_natgrad_workspace_bytes(M, K)
    if workspace is None or workspace.numel() < nbytes:
        workspace = natgrad_workspace(M, K, q_mu.device)
    _lib.call("mgp_natgrad_step", q_mu, _ld(q_mu), q_sqrt, _ld(q_sqrt), q_sqrt.stride(0), g_q_mu, _ld(g_q_mu),
              g_q_sqrt, _ld(g_q_sqrt), g_q_sqrt.stride(0), int(g_q_mu.dtype == torch.float64), M, K, float(step),
              float(grad_sign), info, workspace, workspace.numel(), _stream())
    return info


def gram(X, Y, N=None, alpha=1.0, tri=False, out=None, workspace=None):
    """out[i][j] = alpha * sum_n X[i][n] Y[j][n] (tri: lower triangle, zeros above)."""
    _check(X, "X", 2), _check(Y, "Y", 2)
    MI, MJ = X.shape[0], Y.shape[0]
    N = X.shape[1] if N is None else N
    dev = X.device
    if out is None:
        out = padded(MI, MJ, dev)
    workspace = _workspace("mgp_gram_workspace_bytes", (MI, MJ, N, int(tri)), workspace, dev)
    _lib.call("mgp_gram", X, _ld(X), MI, Y, _ld(Y), MJ, N, float(alpha), int(tri), out, _ld(out), workspace,
              workspace.numel(), _stream())
    return out


def split_rows_f16(X, bound, N=None, out=None):
    """X's row image for gram_x6(x_rows=...) (mgp_split_rows_f16): X [MI, >=N] f32, bound a float32
    device tensor >= max |X| (the scale mgp_gram_f16 would use)."""
    _check(X, "X", 2)
    M = X.shape[0]
    N = X.shape[1] if N is None else N
    out = _workspace("mgp_rows_f16_bytes", (M, N), out, X.device)
    _lib.call("mgp_split_rows_f16", X, _ld(X), M, N, bound, out, out.numel(), _stream())
    return out


def gram_x6(X, Y, W=None, alpha=1.0, mode=0, N=None, out=None, workspace=None, bounds=None, x_rows=None):
    """out[b][i][j] = alpha * sum_n X[b][i][n] W[b][n] Y[b][j][n] at f32 accuracy on the bf16 MFMA.
    X [B, MI, >=N] / [MI, >=N] (Y likewise; a 2-D operand is shared by the batch); W [B, >=N] or None;
    mode 0 full, 1 lower triangle, 2 symmetric.  bounds = (x_bound, y_bound, w_bound) float32
    device tensors of max |X|, |Y|, |W| (w_bound None without W): the split-f16 variant
    (mgp_gram_f16).  x_rows: split_rows_f16(X, x_bound) of a 2-D X (with bounds, W and a 2-D Y):
    the same products with X's split done once (mgp_gram_f16_rows)."""
    X3 = X if X.dim() == 3 else X.unsqueeze(0)
    Y3 = Y if Y.dim() == 3 else Y.unsqueeze(0)
    B = max(X3.shape[0], Y3.shape[0], W.shape[0] if W is not None and W.dim() == 2 else 1)
    MI, MJ = X3.shape[1], Y3.shape[1]
    N = X3.shape[2] if N is None else N
    dev = X.device
    if out is None:
        out = padded(MI, MJ, dev, batch=B)
    sx = X3.stride(0) if X3.shape[0] > 1 else 0
    sy = Y3.stride(0) if Y3.shape[0] > 1 else 0
    sw = (W.stride(0) if W.dim() == 2 and W.shape[0] > 1 else 0) if W is not None else 0
    workspace = _workspace("mgp_gram_x6_workspace_bytes", (MI, MJ, N, B, int(mode)), workspace, dev)
    so = out.stride(0) if out.dim() == 3 else MI * _ld(out)
    entry, xy_args, bound_args = "mgp_gram_x6", [X3, X3.stride(1), sx, MI, Y3, Y3.stride(1), sy, MJ], ()
    if x_rows is not None:
        if W is None or any(b is None for b in bounds):
            raise ValueError("x_rows needs W and all three bounds")
        entry, xy_args, bound_args = "mgp_gram_f16_rows", [x_rows, x_rows.numel(), MI, Y3, Y3.stride(1), MJ], bounds
    elif bounds is not None:
        entry, bound_args = "mgp_gram_f16", bounds
    _lib.call(entry, *xy_args, W, sw, N, B, float(alpha), int(mode), out, out.stride(-2), so, *bound_args, workspace,
              workspace.numel(), _stream())
    return out


def conditional_backward_workspace_bytes(M, N, K):
    return int(_lib.load().mgp_conditional_backward_workspace_bytes(M, N, K))


def conditional_backward_prep(q_sqrt, l_bound, out=None):
    """The q_sqrt-only part of the C-images backward (L_k's image at scale l_bound, the
    transposed triangles) as a uint8 device buffer for conditional_backward_x6(...,
    prep=...) (mgp_conditional_backward_prep_f16c)."""
    _check(q_sqrt, "q_sqrt", 3)
    K, M, _ = q_sqrt.shape
    out = _workspace("mgp_conditional_backward_prep_bytes", (M, K), out, q_sqrt.device)
    _lib.call("mgp_conditional_backward_prep_f16c", q_sqrt, _ld(q_sqrt), q_sqrt.stride(0), M, K, l_bound, out,
              out.numel(), _stream())
    return out


def conditional_backward_x6(Afr, A, q_sqrt, q_mu, LinvT, Gmu, Gv, M, N, out=None, workspace=None, fmt="x6",
                            cross=None, c_images=None, prep=None, t_bound=None):
    """Backward of one layer's conditional (see include/mgp_hip.h): returns dict of
    g_q_mu [M, K], g_q_sqrt [K, M, M], g_Kuf [M, N], g_Lm [M, M], g_var (float64 [1]).
    fmt: format of A's image Afr ("f16": mgp_conditional_backward_f16; with cross "f8",
    default config.expert_cross(), mgp_conditional_backward_f16x8 -- Afr then comes
    from trsm_stats_x6(..., A=..., cross="f8")).  c_images = (Cfr, colmax, l_bound) from
    expert_conditional_x6(..., c_out=...) (f16, cross "f16"): mgp_conditional_backward_f16c."""
    K = q_mu.shape[1]
    dev = q_mu.device
    if out is None:
        out = {"g_q_mu": padded(M, K, dev), "g_q_sqrt": padded(M, M, dev, batch=K),
               "g_Kuf": padded(M, N, dev), "g_Lm": padded(M, M, dev),
               "g_var": torch.empty(1, dtype=torch.float64, device=dev)}
    workspace = _workspace("mgp_conditional_backward_workspace_bytes", (M, N, K), workspace, dev)
    if _ld(Gmu) != _ld(Gv):
        raise ValueError("Gmu and Gv must share a leading dimension")
    o = out
    from .config import expert_cross
    entry = "mgp_conditional_backward_" + _fmt(fmt)
    if entry.endswith("f16") and (cross or expert_cross()) == "f8":
        entry += "x8"
    args = [Afr, Afr.numel(), A, _ld(A), q_sqrt, _ld(q_sqrt), q_sqrt.stride(0), q_mu, _ld(q_mu), LinvT, _ld(LinvT),
            Gmu, Gv, _ld(Gmu), M, N, K, o["g_q_mu"], _ld(o["g_q_mu"]), o["g_q_sqrt"], _ld(o["g_q_sqrt"]),
            o["g_q_sqrt"].stride(0), o["g_Kuf"], _ld(o["g_Kuf"]), o["g_Lm"], _ld(o["g_Lm"]), o["g_var"], workspace,
            workspace.numel()]
    if c_images is not None:
        if entry != "mgp_conditional_backward_f16":
            raise ValueError("c_images need the split-f16 format with f16 cross terms")
        Cfr, colmax, l_bound = c_images
        entry = "mgp_conditional_backward_f16c"
        args += [Cfr, Cfr.numel(), colmax, l_bound]
        if prep is not None:   # from conditional_backward_prep(q_sqrt, l_bound) of the same q_sqrt
            entry += "_prepped"   # t_bound: max |LinvT| (e.g. image_bound of K3's bounded L^-T image)
            args += [prep, prep.numel(), t_bound]
    elif prep is not None:
        raise ValueError("prep needs c_images (the C-images backward)")
    _lib.call(entry, *args, _stream())
    return out


def c_images_bytes(M, N, K):
    """Bytes of the C_k = L_k^T A images of expert_conditional_x6(..., c_out=...)."""
    return _lib.load().mgp_c_images_bytes(M, N, K)


def colnorm_max(q_sqrt, out=None):
    """max over experts and columns of ||tril(q_sqrt[k])[:, j]||_2 (float32 device [1])."""
    _check(q_sqrt, "q_sqrt", 3)
    if out is None:
        out = torch.empty(1, dtype=torch.float32, device=q_sqrt.device)
    K, M = q_sqrt.shape[0], q_sqrt.shape[1]
    _lib.call("mgp_colnorm_max", q_sqrt, _ld(q_sqrt), q_sqrt.stride(0), M, K, out, _stream())
    return out


def image_bound(img, M, K=None, N=None):
    """The device bound in a split image's trailer (float32 view [1]): lower images
    (K given) or column images (N given)."""
    lib = _lib.load()
    size = lib.mgp_x6_lower_bytes(M, K) if K is not None else lib.mgp_x6_cols_bytes(M, N)
    return img.view(torch.uint8)[size - 256:size - 252].view(torch.float32)


# --------------------------------------------------------------------------- K7
def gauss_kl_white(q_mu, q_sqrt, out=None, workspace=None):
    """Whitened KL (models.py:79) as a float64 device tensor of shape [1]."""
    _check(q_mu, "q_mu", 2), _check(q_sqrt, "q_sqrt", 3)
    q_sqrt = as_padded(q_sqrt)  # float4 rows (no copy for the layers' padded storage)
    M, K = q_mu.shape
    dev = q_mu.device
    if out is None:
        out = torch.empty(1, dtype=torch.float64, device=dev)
    workspace = _workspace("mgp_kl_workspace_bytes", (M, K), workspace, dev)
    _lib.call("mgp_gauss_kl_white", q_mu, _ld(q_mu), q_sqrt, _ld(q_sqrt), q_sqrt.stride(0), M, K, out, workspace,
              workspace.numel(), _stream())
    return out


# --------------------------------------------------------------------------- K6
def elbo_terms(mu_f, var_f, mu_a, var_a, Y, lik_var, S, tau=1e-2, noise=None, seed=0, n_offset=0,
               out=None, workspace=None, assign_lik_var=None, multiclass_eps=None, jitter=None):
    """Sum over local points of logsumexp_s(sum_k W ve) - log S (float64 [1]).
    With assign_lik_var: the SMGPModified data term (models.py:112-123).
    multiclass_eps: the pred likelihood is MultiClass(K) / RobustMax(eps) (lik_var unused)."""
    jitter = default_jitter() if jitter is None else jitter
    for t, n in ((mu_f, "mu_f"), (var_f, "var_f"), (mu_a, "mu_a"), (var_a, "var_a")):
        _check(t, n, 2)
    ldf = _ld(mu_f)
    if not (_ld(var_f) == _ld(mu_a) == _ld(var_a) == ldf):
        raise ValueError("conditional outputs must share a leading dimension")
    K, N = mu_f.shape
    dev = mu_f.device
    Y = Y.reshape(-1)
    _check(Y, "Y")
    if multiclass_eps is None:
        _check(lik_var, "lik_var")
    if Y.numel() != N or not Y.is_contiguous():
        raise ValueError("Y must be contiguous with N elements")
    if out is None:
        out = torch.empty(1, dtype=torch.float64, device=dev)
    workspace = _workspace("mgp_elbo_workspace_bytes", (N,), workspace, dev)
    z = u = None
    if noise is not None:
        z, u = noise
        _check(z, "noise_z", 3), _check(u, "noise_u", 3)
        if tuple(z.shape) != (S, N, K) or tuple(u.shape) != (S, N, K):
            raise ValueError("explicit noise must be [S, N, K]")
        z, u = z.contiguous(), u.contiguous()
    if assign_lik_var is not None:
        _check(assign_lik_var, "assign_lik_var")
    # the entries differ in the likelihood arguments after Y only
    alv = assign_lik_var.data_ptr() if assign_lik_var is not None else None
    if multiclass_eps is not None:
        entry, lik_args = "mgp_elbo_terms_multiclass", [float(multiclass_eps), alv]
    elif assign_lik_var is not None:
        entry, lik_args = "mgp_elbo_terms_modified", [lik_var.data_ptr(), alv]
    else:
        entry, lik_args = "mgp_elbo_terms", [lik_var.data_ptr()]
    _lib.call_raw(entry, mu_f.data_ptr(), var_f.data_ptr(), mu_a.data_ptr(), var_a.data_ptr(), ldf, Y.data_ptr(),
                  *lik_args, N, K, S, float(tau), float(jitter), z.data_ptr() if z is not None else None,
                  u.data_ptr() if u is not None else None, int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_offset),
                  out.data_ptr(), workspace.data_ptr(), workspace.numel(), _stream())
    return out


def elbo_combine(data_sum, kl_f, kl_a, n_batch, num_data, out=None, out64=None):
    dev = data_sum.device
    if out is None:
        out = torch.empty((), dtype=F32, device=dev)
    if out64 is None:
        out64 = torch.empty((), dtype=torch.float64, device=dev)
    _lib.call_raw("mgp_elbo_combine", data_sum.data_ptr(), kl_f.data_ptr(), kl_a.data_ptr(), float(n_batch),
                  float(num_data), out.data_ptr(), out64.data_ptr(), _stream())
    return out, out64


def predict_epilogue(fmean, fvar, amean, lik_var, want_y=True, want_assign=False):
    """[N, K] outputs: y mean/var (likelihoods.py:31-32) and softmax assignment."""
    ref = fmean if fmean is not None else amean
    K, N = ref.shape
    dev = ref.device
    ym = torch.empty(N, K, dtype=F32, device=dev) if want_y else None
    yv = torch.empty(N, K, dtype=F32, device=dev) if want_y else None
    asg = torch.empty(N, K, dtype=F32, device=dev) if want_assign else None
    _lib.call("mgp_predict_epilogue", fmean, fvar, amean, _ld(ref), lik_var, N, K, ym, yv, asg, _stream())
    return ym, yv, asg


def philox_noise(seed, n_offset, N, K, S, device, want_z=True, want_u=True):
    z = torch.empty(S, N, K, dtype=F32, device=device) if want_z else None
    u = torch.empty(S, N, K, dtype=F32, device=device) if want_u else None
    _lib.call("mgp_philox_noise", int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_offset), N, K, S, z, u, _stream())
    return z, u


def philox_normal2(seed, n_offset, N, K, S, device):
    z = torch.empty(S, N, K, dtype=F32, device=device)
    _lib.call("mgp_philox_normal2", int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_offset), N, K, S, z, _stream())
    return z


def predict_samples(mu_f, var_f, mu_a, var_a, lik_var, S, tau=1e-2, noise=None, seed=0,
                    n_offset=0, multiclass_eps=None, jitter=None):
    """samples_y, samples_f [S, N] (models.py:91-103); multiclass_eps: MultiClass / RobustMax
    predictive mean / variance for samples_y (lik_var unused)."""
    jitter = default_jitter() if jitter is None else jitter
    K, N = mu_f.shape
    dev = mu_f.device
    sy = torch.empty(S, N, dtype=F32, device=dev)
    sf = torch.empty(S, N, dtype=F32, device=dev)
    if noise is None:
        noise = [None, None, None]
    else:
        noise = [t.contiguous() for t in noise]
        for t in noise:
            _check(t, "noise", 3)
            if tuple(t.shape) != (S, N, K):
                raise ValueError("explicit noise must be [S, N, K]")
    entry, lik = "mgp_predict_samples", lik_var
    if multiclass_eps is not None:
        entry, lik = "mgp_predict_samples_multiclass", float(multiclass_eps)
    _lib.call(entry, mu_f, var_f, mu_a, var_a, _ld(mu_f), lik, N, K, S, float(tau), float(jitter), *noise,
              int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_offset), sy, sf, _stream())
    return sy, sf


def multiclass_predict(fmean, fvar, epsilon):
    """MultiClass._predict_mean_and_var (GPflow 2.7): (ps, ps - ps^2), each [N, K]."""
    _check(fmean, "fmean", 2), _check(fvar, "fvar", 2)
    K, N = fmean.shape
    if _ld(fvar) != _ld(fmean):
        raise ValueError("fmean and fvar must share a leading dimension")
    ym = torch.empty(N, K, dtype=F32, device=fmean.device)
    yv = torch.empty(N, K, dtype=F32, device=fmean.device)
    _lib.call("mgp_multiclass_predict", fmean, fvar, _ld(fmean), N, K, float(epsilon), ym, yv, _stream())
    return ym, yv


# --------------------------------------------------------------------------- method-level API
def _latents_check(mu, var, name):
    _check(mu, "mu_" + name, 2), _check(var, "var_" + name, 2)
    if _ld(var) != _ld(mu) or var.shape != mu.shape:
        raise ValueError(f"mu_{name} and var_{name} must share shape and leading dimension")


def assign_logits(mu_a, var_a, S, N, stride_s=0, noise_z=None, seed=0, n_offset=0, jitter=None):
    """SMGP.W_dist's logits (models.py:56-59, utils.py:26-27): [S, N, K] =
    mu_a + z sqrt(var_a + jitter); mu_a / var_a expert-major [K, >= (S-1) stride_s + N]."""
    jitter = default_jitter() if jitter is None else jitter
    _latents_check(mu_a, var_a, "a")
    K = mu_a.shape[0]
    out = torch.empty(S, N, K, dtype=F32, device=mu_a.device)
    if noise_z is not None:
        _check(noise_z, "noise_z", 3)
        if tuple(noise_z.shape) != (S, N, K):
            raise ValueError("explicit noise must be [S, N, K]")
        noise_z = noise_z.contiguous()
    _lib.call("mgp_assign_logits", mu_a, var_a, _ld(mu_a), int(stride_s), N, K, S, float(jitter), noise_z,
              int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_offset), out, _stream())
    return out


def relaxed_onehot_sample(logits, S, N, tau=1e-2, noise_u=None, seed=0, n_offset=0):
    """RelaxedOneHotCategorical(tau, logits).sample() on logits [S * N, K] (rows s * N + n)."""
    _check(logits, "logits")
    K = logits.shape[-1]
    if logits.numel() != S * N * K:
        raise ValueError("logits must hold S * N rows of K")
    logits = logits.contiguous()
    W = torch.empty(S * N, K, dtype=F32, device=logits.device)
    if noise_u is not None:
        _check(noise_u, "noise_u")
        if noise_u.numel() != S * N * K:
            raise ValueError("explicit noise must be [S, N, K]")
        noise_u = noise_u.contiguous()
    _lib.call("mgp_relaxed_onehot_sample", logits, N, K, S, float(tau), noise_u, int(seed) & 0xFFFFFFFFFFFFFFFF,
              int(n_offset), W, _stream())
    return W


def e_log_p_y(mu_f, var_f, Y, lik_var, W, S, N, stride_s=0, mu_a=None, var_a=None, assign_lik_var=None,
              multiclass_eps=None):
    """SMGP.E_log_p_Y (models.py:63-67; SMGPModified :112-123 with assign_lik_var) -> [N]."""
    _latents_check(mu_f, var_f, "f")
    K = mu_f.shape[0]
    Y = Y.reshape(-1)
    _check(Y, "Y"), _check(W, "W")
    if Y.numel() != N or not Y.is_contiguous():
        raise ValueError("Y must be contiguous with N elements")
    if W.numel() != S * N * K:
        raise ValueError("W must be [S, N, K]")
    W = W.contiguous()
    if multiclass_eps is None:
        _check(lik_var, "lik_var")
    if assign_lik_var is not None:
        _check(assign_lik_var, "assign_lik_var")
        _latents_check(mu_a, var_a, "a")
        if _ld(mu_a) != _ld(mu_f):
            raise ValueError("the two layers' latents must share a leading dimension")
    out = torch.empty(N, dtype=F32, device=mu_f.device)
    _lib.call("mgp_e_log_p_y", mu_f, var_f, mu_a, var_a, _ld(mu_f), int(stride_s), Y,
              None if multiclass_eps is not None else lik_var, assign_lik_var, float(multiclass_eps or 0.0), W, N, K, S,
              out, _stream())
    return out


# --------------------------------------------------------------------------- mixture predictive
MIXTURE_OUTPUTS = ("weights", "mix_mean", "mix_var", "log_density", "log_density_sum")


def mixture_predict(mu_f, var_f, mu_a, var_a, lik_var, S=0, Y=None, noise_z=None, seed=0, n_offset=0,
                    jitter=None, want=None, workspace=None, out=None):
    """The mixture predictive p(y | x) = sum_k w_k N(y | mu_f,k, var_f,k + lik_var_k)
    (mgp_mixture_predict, csrc/mixture.hip) -> dict of the outputs named in `want`:
    weights [N, K], mix_mean [N], mix_var [N], log_density [N] (float32) and
    log_density_sum [1] (float64).  w = mean_s softmax_k(mu_a + z_s sqrt(var_a + jitter));
    S = 0: the plug-in softmax_k(mu_a).  noise_z: explicit normals [S, N, K], else K6's
    Philox z stream of (seed, n_offset).  want defaults to every output Y allows; out: a
    dict of an earlier call at the same shapes, whose tensors are written again."""
    jitter = default_jitter() if jitter is None else jitter
    for t, n in ((mu_f, "mu_f"), (var_f, "var_f"), (mu_a, "mu_a"), (var_a, "var_a")):
        _check(t, n, 2)
    ldf = _ld(mu_f)
    if not (_ld(var_f) == _ld(mu_a) == _ld(var_a) == ldf):
        raise ValueError("conditional outputs must share a leading dimension")
    K, N = mu_f.shape
    dev = mu_f.device
    _check(lik_var, "lik_var")
    if want is None:
        want = MIXTURE_OUTPUTS if Y is not None else MIXTURE_OUTPUTS[:3]
    unknown = [w for w in want if w not in MIXTURE_OUTPUTS]
    if unknown:
        raise ValueError(f"unknown outputs {unknown}; choose from {MIXTURE_OUTPUTS}")
    if Y is not None:
        Y = Y.reshape(-1)
        _check(Y, "Y")
        if Y.numel() != N or not Y.is_contiguous():
            raise ValueError("Y must be contiguous with N elements")
    elif "log_density" in want or "log_density_sum" in want:
        raise ValueError("log_density needs Y")
    if noise_z is not None:
        _check(noise_z, "noise_z", 3)
        if tuple(noise_z.shape) != (S, N, K):
            raise ValueError("explicit noise must be [S, N, K]")
        noise_z = noise_z.contiguous()
    have, out = out or {}, {}
    for name in want:
        shape, dtype = ((N, K) if name == "weights" else (1,) if name == "log_density_sum" else (N,),
                        torch.float64 if name == "log_density_sum" else F32)
        t = have.get(name)
        if t is not None:
            if tuple(t.shape) != shape or t.dtype != dtype or t.device != dev or not t.is_contiguous():
                raise ValueError(f"out[{name!r}] must be a contiguous {dtype} tensor of shape {shape}")
        elif name == "log_density_sum" and N == 0:
            t = torch.zeros(shape, dtype=dtype, device=dev)   # the entry does nothing for N = 0
        else:
            t = torch.empty(shape, dtype=dtype, device=dev)
        out[name] = t
    ws_args = [None, 0]   # only the sum needs a workspace
    if "log_density_sum" in out:
        workspace = _workspace("mgp_mixture_predict_workspace_bytes", (N, K), workspace, dev)
        ws_args = [workspace, workspace.numel()]
    _lib.call("mgp_mixture_predict", mu_f, var_f, mu_a, var_a, ldf, lik_var, Y, N, K, int(S), float(jitter), noise_z,
              int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_offset), *[out.get(n) for n in MIXTURE_OUTPUTS], *ws_args,
              _stream())
    return out


def mixture_density_grid(mu_f, var_f, lik_var, weights, y_grid):
    """density [N, G] = sum_k weights[n, k] N(y_grid[g] | mu_f,k[n], var_f,k[n] + lik_var_k)
    (mgp_mixture_density_grid), from mixture_predict's weights [N, K]."""
    _latents_check(mu_f, var_f, "f")
    K, N = mu_f.shape
    _check(lik_var, "lik_var"), _check(weights, "weights", 2), _check(y_grid, "y_grid", 1)
    if tuple(weights.shape) != (N, K):
        raise ValueError("weights must be [N, K]")
    weights, y_grid = weights.contiguous(), y_grid.contiguous()
    G = y_grid.numel()
    out = torch.empty(N, G, dtype=F32, device=mu_f.device)
    _lib.call("mgp_mixture_density_grid", mu_f, var_f, _ld(mu_f), lik_var, weights, N, K, y_grid, G, out, max(G, 1),
              _stream())
    return out


# --------------------------------------------------------------------------- mixture scores
SCORE_OUTPUTS = ("cdf", "sf", "crps", "crps_sum")
MAX_LEVELS = 256


def mixture_score(mu_f, var_f, lik_var, weights, Y, want=None, workspace=None, out=None):
    """CDF, survival function and CRPS of the mixture predictive at the targets Y
    (mgp_mixture_score, csrc/mixture_score.hip), from mixture_predict's weights [N, K] -> dict
    of the outputs named in `want` (default: all): cdf [N] (the PIT values), sf [N] (its own
    erfc sum, accurate in the upper tail), crps [N] (float32) and crps_sum [1] (float64).
    out: a dict of an earlier call at the same shapes, whose tensors are written again."""
    _latents_check(mu_f, var_f, "f")
    K, N = mu_f.shape
    dev = mu_f.device
    _check(lik_var, "lik_var"), _check(weights, "weights", 2)
    if tuple(weights.shape) != (N, K):
        raise ValueError("weights must be [N, K]")
    weights = weights.contiguous()
    Y = Y.reshape(-1)
    _check(Y, "Y")
    if Y.numel() != N or not Y.is_contiguous():
        raise ValueError("Y must be contiguous with N elements")
    want = SCORE_OUTPUTS if want is None else want
    unknown = [w for w in want if w not in SCORE_OUTPUTS]
    if unknown:
        raise ValueError(f"unknown outputs {unknown}; choose from {SCORE_OUTPUTS}")
    have, out = out or {}, {}
    for name in want:
        shape, dtype = ((1,), torch.float64) if name == "crps_sum" else ((N,), F32)
        t = have.get(name)
        if t is not None:
            if tuple(t.shape) != shape or t.dtype != dtype or t.device != dev or not t.is_contiguous():
                raise ValueError(f"out[{name!r}] must be a contiguous {dtype} tensor of shape {shape}")
        elif name == "crps_sum" and N == 0:
            t = torch.zeros(shape, dtype=dtype, device=dev)   # the entry does nothing for N = 0
        else:
            t = torch.empty(shape, dtype=dtype, device=dev)
        out[name] = t
    ws_args = [None, 0]   # only the sum needs a workspace
    if "crps_sum" in out:
        workspace = _workspace("mgp_mixture_score_workspace_bytes", (N, K), workspace, dev)
        ws_args = [workspace, workspace.numel()]
    _lib.call("mgp_mixture_score", mu_f, var_f, _ld(mu_f), lik_var, weights, Y, N, K,
              *[out.get(n) for n in SCORE_OUTPUTS], *ws_args, _stream())
    return out


def quantile_levels(levels):
    """The levels as a float32 host array [Q], each inside (0, 1) after the rounding to
    float32 (ValueError otherwise, before anything is uploaded)."""
    if isinstance(levels, torch.Tensor):
        levels = levels.detach().cpu().numpy()
    lv = np.asarray(levels, dtype=np.float32)
    if lv.ndim > 1:
        raise ValueError("levels must be a scalar or 1-D")
    lv = np.ascontiguousarray(lv.reshape(-1))
    if not bool(np.all((lv > 0) & (lv < 1))):
        raise ValueError("quantile levels must lie strictly inside (0, 1) as float32 values")
    if lv.size > MAX_LEVELS:
        raise ValueError(f"at most {MAX_LEVELS} levels per call")
    return lv


def mixture_quantiles(mu_f, var_f, lik_var, weights, levels, out=None):
    """Quantiles [N, Q] of the mixture predictive (mgp_mixture_quantiles): the y with
    cdf(y) = p for a level p <= 1/2 and with sf(y) = 1 - p above, by a bracketed Newton
    iteration per (point, level).  levels: host values in (0, 1) (checked here), rounded to
    float32 once.  out: a float32 [N, Q] view with a contiguous last dimension."""
    _latents_check(mu_f, var_f, "f")
    K, N = mu_f.shape
    _check(lik_var, "lik_var"), _check(weights, "weights", 2)
    if tuple(weights.shape) != (N, K):
        raise ValueError("weights must be [N, K]")
    weights = weights.contiguous()
    lv = quantile_levels(levels)
    Q = lv.size
    if out is None:
        out = torch.empty(N, Q, dtype=F32, device=mu_f.device)
    else:
        _check(out, "out", 2)
        if tuple(out.shape) != (N, Q):
            raise ValueError("out must be [N, Q]")
    if Q == 0:
        return out
    ldq = _ld(out) if N > 1 else Q
    lvd = torch.from_numpy(lv).to(mu_f.device)
    _lib.call("mgp_mixture_quantiles", mu_f, var_f, _ld(mu_f), lik_var, weights, N, K, lvd, Q, out, ldq, _stream())
    return out


# --------------------------------------------------------------------------- mixture assignment and modes
RESP_OUTPUTS = ("resp", "labels", "entropy", "usage")


def _mixture_args(mu_f, var_f, lik_var, weights):
    """The checks shared by the entries that read mixture_predict's weights -> (K, N, weights)."""
    _latents_check(mu_f, var_f, "f")
    K, N = mu_f.shape
    _check(lik_var, "lik_var"), _check(weights, "weights", 2)
    if tuple(weights.shape) != (N, K):
        raise ValueError("weights must be [N, K]")
    return K, N, weights.contiguous()


def mixture_responsibilities(mu_f, var_f, lik_var, weights, Y, want=("resp",), workspace=None, out=None):
    """The posterior responsibilities p(z = k | x, y) of the mixture predictive at the targets Y
    (mgp_mixture_responsibilities, csrc/mixture_assign.hip), from mixture_predict's weights
    [N, K] -> dict of the outputs named in `want`: resp [N, K] (float32; a view of a padded
    buffer), labels [N] (int32; argmax of the log responsibilities, -1 for a row with no positive
    weight), entropy [N] (float32, nats) and usage [K] (float64: sum_n resp, the points each
    expert explains).  out: a dict of an earlier call at the same shapes, written again."""
    K, N, weights = _mixture_args(mu_f, var_f, lik_var, weights)
    dev = mu_f.device
    Y = Y.reshape(-1)
    _check(Y, "Y")
    if Y.numel() != N or not Y.is_contiguous():
        raise ValueError("Y must be contiguous with N elements")
    unknown = [w for w in want if w not in RESP_OUTPUTS]
    if unknown:
        raise ValueError(f"unknown outputs {unknown}; choose from {RESP_OUTPUTS}")
    spec = {"resp": ((N, K), F32), "labels": ((N,), torch.int32), "entropy": ((N,), F32),
            "usage": ((K,), torch.float64)}
    have, out = out or {}, {}
    for name in want:
        shape, dtype = spec[name]
        t = have.get(name)
        if t is not None:
            if tuple(t.shape) != shape or t.dtype != dtype or t.device != dev or (t.dim() and t.stride(-1) != 1):
                raise ValueError(f"out[{name!r}] must be a {dtype} tensor of shape {shape} with contiguous rows")
        elif name == "resp":
            t = padded(N, K, dev)
        elif name == "usage" and N == 0:
            t = torch.zeros(shape, dtype=dtype, device=dev)   # the entry does nothing for N = 0
        else:
            t = torch.empty(shape, dtype=dtype, device=dev)
        out[name] = t
    ldr = _ld(out["resp"]) if "resp" in out and N > 1 else K
    ws_args = [None, 0]   # only the usage sums need a workspace
    if "usage" in out:
        workspace = _workspace("mgp_mixture_responsibilities_workspace_bytes", (N, K), workspace, dev)
        ws_args = [workspace, workspace.numel()]
    _lib.call("mgp_mixture_responsibilities", mu_f, var_f, _ld(mu_f), lik_var, weights, Y, N, K, out.get("resp"), ldr,
              out.get("labels"), out.get("entropy"), out.get("usage"), *ws_args, _stream())
    return out


def mixture_modes(mu_f, var_f, lik_var, weights):
    """The modes of the mixture predictive per point (mgp_mixture_modes): the distinct limits of
    hill-climbing from the expert means with a positive weight -> (modes [N, K], density [N, K],
    count [N] int32).  Row n holds its count[n] modes in order of decreasing density and NaN
    after them; modes and density are views of padded buffers."""
    K, N, weights = _mixture_args(mu_f, var_f, lik_var, weights)
    dev = mu_f.device
    modes, density = padded(N, K, dev), padded(N, K, dev)
    count = torch.empty(N, dtype=torch.int32, device=dev)
    ldm = _ld(modes) if N > 1 else K
    _lib.call("mgp_mixture_modes", mu_f, var_f, _ld(mu_f), lik_var, weights, N, K, modes, density, ldm, count, _stream())
    return modes, density, count


# --------------------------------------------------------------------------- k-means
I32 = torch.int32


def _rows(t, name):
    """A float32 device matrix whose rows are contiguous (any row stride >= D)."""
    _check(t, name, 2)
    if t.shape[1] > 1 and t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t, (t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1))


def vq(obs, code_book, code=None, dist=None):
    """scipy.cluster.vq.vq on the device (mgp_vq): code int32 [N] (first minimum of the
    squared distances on float32 differences), dist float32 [N]."""
    obs, ldo = _rows(obs, "obs")
    code_book, ldc = _rows(code_book, "code_book")
    N, D = obs.shape
    k = code_book.shape[0]
    if code_book.shape[1] != D:
        raise ValueError("obs and code_book must have the same number of features")
    code = torch.empty(N, dtype=I32, device=obs.device) if code is None else code
    dist = torch.empty(N, dtype=F32, device=obs.device) if dist is None else dist
    _lib.call("mgp_vq", obs, ldo, code_book, ldc, N, k, D, code, dist, _stream())
    return code, dist


def kmeans_workspace(N, k, D, R, device):
    return _new_workspace("mgp_kmeans_workspace_bytes", (N, k, D, R), device)


def kmeans_init(obs, k, workspace, idx=None, guess=None):
    """Start R runs from the rows obs[idx[r]] (idx: device int64 [R, k]) or one run from
    guess [k, D] (mgp_kmeans_init)."""
    obs, ldo = _rows(obs, "obs")
    N, D = obs.shape
    R, ldg = 1, 0
    if guess is not None:
        guess, ldg = _rows(guess, "guess")
    if idx is not None:
        if idx.dtype != torch.int64 or not idx.is_cuda or idx.dim() != 2 or idx.shape[1] != k:
            raise ValueError("idx must be a device int64 tensor [R, k]")
        idx = idx.contiguous()
        R = idx.shape[0]
    _lib.call("mgp_kmeans_init", obs, ldo, N, D, idx, guess, ldg, k, R, workspace, workspace.numel(), _stream())
    return R


def kmeans_iterate(obs, k, R, B, thresh, workspace, done):
    """B Lloyd iterations of the R runs of the workspace (mgp_kmeans_iterate); done: device
    int32 [R]."""
    obs, ldo = _rows(obs, "obs")
    N, D = obs.shape
    _lib.call("mgp_kmeans_iterate", obs, ldo, N, D, k, R, int(B), float(thresh), workspace, workspace.numel(), done,
              _stream())


def kmeans_select(N, k, D, R, workspace, result):
    """The winning run into `result`, a device uint8 buffer laid out as
    [float64 distortion | int32 info[4] | pad to 32 B | float32 code_book [k, D]]
    (mgp_kmeans_select), so that one copy brings everything to the host."""
    base = result.data_ptr()
    _lib.call("mgp_kmeans_select", N, k, D, R, workspace, workspace.numel(), base + 32, D, base, base + 8, _stream())


def kmeans_update(obs, code, k, workspace=None):
    """One update from given labels (mgp_kmeans_update): means float32 [k, D] (zeros for a
    code without members), counts int32 [k]."""
    obs, ldo = _rows(obs, "obs")
    N, D = obs.shape
    if code.dtype != I32 or not code.is_cuda or code.numel() != N:
        raise ValueError("code must be a device int32 tensor [N]")
    code = code.contiguous()
    if workspace is None:
        workspace = kmeans_workspace(N, k, D, 1, obs.device)
    means = torch.empty(k, D, dtype=F32, device=obs.device)
    counts = torch.empty(k, dtype=I32, device=obs.device)
    _lib.call("mgp_kmeans_update", obs, ldo, N, D, code, k, means, D, counts, workspace, workspace.numel(), _stream())
    return means, counts


# --------------------------------------------------------------------------- greedy variance selection
def greedy_workspace(N, M, D, device):
    return _new_workspace("mgp_greedy_workspace_bytes", (N, M, D), device)


def greedy_factor(N, M, device):
    """The float32 factor storage [M, N] of a selection, rows padded to a multiple of 4."""
    return padded(M, N, device)


def greedy_init(N, D, variance, threshold, workspace):
    """Start a selection on N points (mgp_greedy_init): d = variance, nothing chosen."""
    _check(variance, "variance")
    _lib.call("mgp_greedy_init", N, D, variance, float(threshold), workspace, workspace.numel(), _stream())


def greedy_steps(X, variance, lengthscales, M, B, factor, workspace, state):
    """The next min(B, M) steps of the selection (mgp_greedy_steps); factor: float32 [M, N]
    view of greedy_factor; state: device int32 [2] = points chosen so far, stopped."""
    X, ldx = _rows(X, "X")
    _check(variance, "variance"), _check(lengthscales, "lengthscales"), _check(factor, "factor", 2)
    N, D = X.shape
    if factor.shape != (M, N):
        raise ValueError(f"factor must be [M, N] = [{M}, {N}], got {tuple(factor.shape)}")
    if state.dtype != I32 or not state.is_cuda or state.numel() < 2:
        raise ValueError("state must be a device int32 tensor [2]")
    _lib.call("mgp_greedy_steps", X, ldx, N, D, variance, lengthscales, lengthscales.numel(), M, int(B), factor,
              _ld(factor), workspace, workspace.numel(), state, _stream())


def greedy_result(X, M, workspace, residual=True):
    """The selection so far (mgp_greedy_result) -> (indices int64 [M], Z float32 [M, D], dmax
    and trace float64 [M], residual float64 [N] or None, info int32 [2] = m, stopped); the
    first m entries of the [M] arrays are written."""
    X, ldx = _rows(X, "X")
    N, D = X.shape
    dev = X.device
    indices = torch.empty(M, dtype=torch.int64, device=dev)
    Z = torch.empty(M, D, dtype=F32, device=dev)
    dmax = torch.empty(M, dtype=torch.float64, device=dev)
    trace = torch.empty(M, dtype=torch.float64, device=dev)
    res = torch.empty(N, dtype=torch.float64, device=dev) if residual else None
    info = torch.empty(2, dtype=I32, device=dev)
    _lib.call("mgp_greedy_result", X, ldx, N, D, M, workspace, workspace.numel(), indices, Z, D, dmax, trace,
              res, info, _stream())
    return indices, Z, dmax, trace, res, info


# --------------------------------------------------------------------------- pathwise samples
def path_eval(X, Omega, phase, W, A=None, out=None):
    """C frozen pathwise posterior samples at the N points of X (mgp_path_eval):
        out[c, n] = sum_{j < R} W[j, c] cos(2 pi (Omega[j] . X[n] + phase[j])) + sum_m W[R + m, c] A[m, n]
    X [N, D]; Omega [R, D] and phase [R] in turns (zeta / lengthscale / 2 pi); W [R + M, C]
    with the prior rows scaled by sqrt(2 variance / R); A [M, N] = L^-1 Kuf in f32 as K4
    writes it (None: the prior features only, W [R, C]).  Returns out [C, N], a view of
    padded storage.  A call on X[a:b] returns out[:, a:b] of the full call bit for bit."""
    X, ldx = _rows(X, "X")
    Omega, ldo = _rows(Omega, "Omega")
    _check(phase, "phase", 1), _check(W, "W", 2)
    N, D = X.shape
    R = Omega.shape[0]
    if Omega.shape[1] != D:
        raise ValueError(f"Omega must have X's {D} columns, got {tuple(Omega.shape)}")
    if phase.numel() != R:
        raise ValueError(f"phase must be [{R}], got {tuple(phase.shape)}")
    M = 0
    if A is not None:
        _check(A, "A", 2)
        M = A.shape[0]
        if A.shape[1] != N:
            raise ValueError(f"A must be [M, {N}], got {tuple(A.shape)}")
        A = as_padded(A)
    if W.shape[0] != R + M:
        raise ValueError(f"W must have R + M = {R + M} rows, got {tuple(W.shape)}")
    C = W.shape[1]
    W = as_padded(W)
    phase = phase.contiguous()
    if out is None:
        out = padded(C, N, X.device)
    elif tuple(out.shape) != (C, N):
        raise ValueError(f"out must be [{C}, {N}]")
    _lib.call("mgp_path_eval", X, ldx, N, D, Omega, ldo, phase, R, A, _ld(A) if A is not None else 0, M, W, _ld(W), C,
              out, _ld(out), _stream())
    return out
