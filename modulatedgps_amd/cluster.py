"""scipy.cluster.vq.kmeans / vq on the device (csrc/kmeans.hip): the inducing-point
initialisation of the reference demos, ``kmeans(Xtrain, num_ind, seed=0)[0]``
(demos/demo_tf2.py:39), with SciPy's arguments, return values and algorithm.

``kmeans`` and ``vq`` return host float64 arrays as SciPy does; ``kmeans_device`` and
``vq_device`` return device tensors (the ``predict_*_device`` convention).  The start
indices of the restarts are drawn on the host with SciPy's NumPy calls
(``rng.choice(N, size=k, replace=False)``, in order from one generator), so an integer
``seed`` reproduces SciPy's starts; everything else runs on the device.
"""
import numpy as np
import torch

from . import ops

MAX_RUNS = 64          # runs that advance in the same launches (mgp_hip.h)
DEFAULT_BLOCK = 8      # iterations enqueued between two readbacks of the done flags


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("modulatedgps_amd.cluster needs a HIP device (there is no CPU fallback)")
    return torch.device("cuda")


def _checked(a, check_finite):
    """np.asarray_chkfinite's test (ValueError for NaN or inf), made before anything is
    moved to the device."""
    if isinstance(a, torch.Tensor):
        if check_finite and not bool(torch.isfinite(a).all()):
            raise ValueError("array must not contain infs or NaNs")
        return a.detach()
    return np.asarray_chkfinite(a) if check_finite else np.asarray(a)


def _as_obs(a, name, device=None):
    """A float32 device matrix [N, D] (inputs are rounded to float32 once); a 1-D input is
    [N, 1].  Returns (tensor, was_1d)."""
    if isinstance(a, torch.Tensor):
        t = a.to(device=device or (a.device if a.is_cuda else _device()), dtype=torch.float32)
    else:
        t = torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=device or _device())
    one_d = t.dim() == 1
    if one_d:
        t = t.reshape(-1, 1)
    if t.dim() != 2:
        raise ValueError(f"{name} must be 1-D or 2-D, got shape {tuple(t.shape)}")
    return t, one_d


def _generator(seed, rng):
    """SciPy 1.15's seed / rng keywords: an integer seed is np.random.RandomState(seed), an
    integer rng is np.random.default_rng(rng), generator objects are used as given."""
    if seed is not None and rng is not None:
        raise TypeError("kmeans() got both 'seed' and 'rng'; give one")
    if rng is not None:
        if isinstance(rng, (np.random.RandomState, np.random.Generator)):
            return rng
        return np.random.default_rng(rng)
    if seed is None:
        return np.random.mtrand._rand
    if isinstance(seed, (np.random.RandomState, np.random.Generator)):
        return seed
    return np.random.RandomState(seed)


def start_indices(N, k, iter, seed=None, rng=None):
    """The [iter, k] start rows SciPy's kmeans draws: one rng.choice(N, size=k,
    replace=False) per restart, in order from one generator."""
    gen = _generator(seed, rng)
    return np.stack([np.asarray(gen.choice(N, size=int(k), replace=False), dtype=np.int64)
                     for _ in range(iter)])


def _run(obs, k, idx=None, guess=None, thresh=1e-5, block=DEFAULT_BLOCK):
    """R runs to convergence -> the device result buffer of ops.kmeans_select."""
    N, D = obs.shape
    R = 1 if idx is None else idx.shape[0]
    ws = ops.kmeans_workspace(N, k, D, R, obs.device)
    ops.kmeans_init(obs, k, ws, idx=idx, guess=guess)
    done = torch.zeros(R, dtype=torch.int32, device=obs.device)
    while True:
        ops.kmeans_iterate(obs, k, R, block, thresh, ws, done)
        if bool(done.cpu().all()):       # the one readback per block: R flags
            break
    result = torch.empty(32 + k * D * 4, dtype=torch.uint8, device=obs.device)
    ops.kmeans_select(N, k, D, R, ws, result)
    return result


def _is_scalar(x):
    """SciPy takes a k_or_guess of size 1 as the number of codes."""
    return (x.numel() if isinstance(x, torch.Tensor) else np.size(x)) == 1


def _header(buf):
    """(distortion, k_active, winner, iterations) of a result buffer's first 32 bytes."""
    raw = bytes(buf[:32].cpu().numpy())
    info = np.frombuffer(raw, dtype=np.int32, count=4, offset=8)
    return float(np.frombuffer(raw, dtype=np.float64, count=1)[0]), int(info[0]), int(info[1]), int(info[2])


def _kmeans(obs, k_or_guess, iter, thresh, check_finite, seed, rng, block, runs_per_launch):
    """-> (obs_was_1d, D, [(result buffer, k)] of the candidates in order)."""
    obs, k_or_guess = _checked(obs, check_finite), _checked(k_or_guess, check_finite)
    obs, one_d = _as_obs(obs, "obs")
    N, D = obs.shape
    if iter < 1:
        raise ValueError(f"iter must be at least 1, got {iter}")
    if int(block) < 1:
        raise ValueError("block must be at least 1")
    if not _is_scalar(k_or_guess):
        guess, _ = _as_obs(k_or_guess, "k_or_guess", obs.device)
        if guess.numel() < 1:
            raise ValueError(f"Asked for 0 clusters. Initial book was {k_or_guess}")
        if guess.shape[1] != D:
            raise ValueError("obs and the initial code book must have the same number of features")
        return one_d, D, [(_run(obs, guess.shape[0], guess=guess, thresh=thresh, block=block), guess.shape[0])]
    kf = float(k_or_guess)
    k = int(kf)
    if k != kf:
        raise ValueError("If k_or_guess is a scalar, it must be an integer.")
    if k < 1:
        raise ValueError("Asked for %d clusters." % k)
    idx = start_indices(N, k, iter, seed=seed, rng=rng)     # k > N: choice raises ValueError
    step = min(MAX_RUNS, int(runs_per_launch or MAX_RUNS))
    if step < 1:
        raise ValueError("runs_per_launch must be at least 1")
    out = []
    for r0 in range(0, iter, step):
        dev_idx = torch.as_tensor(idx[r0:r0 + step], device=obs.device)
        out.append((_run(obs, k, idx=dev_idx, thresh=thresh, block=block), k))
    return one_d, D, out


def _best(cands):
    """The first candidate with the strictly smallest distortion (SciPy's dist < best_dist)
    -> (buffer, k).  Restarts beyond one launch's 64 runs are compared here."""
    if len(cands) == 1:
        return cands[0]
    best = None
    for buf, k in cands:
        d = _header(buf)[0]
        if best is None or d < best[0]:
            best = (d, buf, k)
    return best[1], best[2]


def kmeans_device(obs, k_or_guess, iter=20, thresh=1e-5, check_finite=True, *, seed=None, rng=None,
                  block=DEFAULT_BLOCK, runs_per_launch=None):
    """kmeans with device results: (code_book float32 tensor [k_active, D], distortion
    float).  block: Lloyd iterations enqueued between two readbacks of the done flags;
    runs_per_launch: restarts that advance in the same launches (<= 64).  Neither changes a
    bit of the result."""
    one_d, D, cands = _kmeans(obs, k_or_guess, iter, thresh, check_finite, seed, rng, block, runs_per_launch)
    buf, k = _best(cands)
    dist, k_active, _, _ = _header(buf)
    book = buf[32:].view(torch.float32).reshape(k, D)[:k_active]
    return (book.reshape(-1) if one_d else book), dist


def kmeans(obs, k_or_guess, iter=20, thresh=1e-5, check_finite=True, *, seed=None, rng=None,
           block=DEFAULT_BLOCK, runs_per_launch=None):
    """scipy.cluster.vq.kmeans on the device -> (code_book float64 ndarray, distortion).

    obs [N, D] (1-D: [N, 1]); k_or_guess: an integer k (`iter` restarts from rows drawn
    with seed / rng, the first with the strictly smallest distortion wins) or an initial
    code book [k, D] (one run, `iter` ignored).  A run repeats assignment and update while
    the change of the mean distance exceeds `thresh`; codes that lose all members are
    dropped.  The distortion is the mean distance under the code book before the last
    update, as in SciPy."""
    one_d, D, cands = _kmeans(obs, k_or_guess, iter, thresh, check_finite, seed, rng, block, runs_per_launch)
    buf, k = _best(cands)
    raw = buf.cpu().numpy()              # the one final readback: header and code book
    k_active = int(raw[8:12].view(np.int32)[0])
    dist = float(raw[:8].view(np.float64)[0])
    book = raw[32:].view(np.float32).reshape(k, D)[:k_active].astype(np.float64)
    return (book.reshape(-1) if one_d else book), dist


def vq_device(obs, code_book, check_finite=True):
    """vq with device results: (code int32 tensor [N], dist float32 tensor [N])."""
    obs, code_book = _checked(obs, check_finite), _checked(code_book, check_finite)
    obs, _ = _as_obs(obs, "obs")
    code_book, _ = _as_obs(code_book, "code_book", obs.device)
    if obs.shape[1] != code_book.shape[1]:
        raise ValueError("obs and code_book must have the same number of features")
    return ops.vq(obs, code_book)


def vq(obs, code_book, check_finite=True):
    """scipy.cluster.vq.vq on the device -> (code int32 ndarray [N], dist float64 ndarray
    [N]): the nearest code of every observation (ties to the lowest index) and its
    distance."""
    code, dist = vq_device(obs, code_book, check_finite)
    return code.cpu().numpy(), dist.cpu().numpy().astype(np.float64)
