"""float64 statement of scipy.cluster.vq.kmeans / vq (SciPy 1.15 semantics), the oracle of
modulatedgps_amd.cluster and csrc/kmeans.hip, and a float32 emulation of the device
arithmetic of one run.

kmeans(obs, k_or_guess, iter=20, thresh=1e-5, check_finite=True, *, seed=None, rng=None):
  obs [N, D] (1-D: [N, 1]).  An array k_or_guess [k, D]: one run from it.  An integer k:
  `iter` restarts, restart r from obs[idx_r], idx_r = rng.choice(N, size=k, replace=False)
  drawn in order from one generator (integer seed: np.random.RandomState(seed); integer
  rng: np.random.default_rng(rng)); the winner is the first run with the strictly smallest
  distortion.
One run, while diff > thresh (diff = inf at the start):
  assign every point to its nearest code by squared Euclidean distance (first minimum),
  avg = mean_n sqrt(min d^2), replace each code by the mean of its members, drop the codes
  without members (rows keep their order), diff = |avg_prev - avg|.
  It returns the code book after the last update and the last avg (the distortion under
  the code book BEFORE the last update).
"""
import numpy as np


def _as2d(a):
    a = np.asarray(a, dtype=np.float64)
    return a.reshape(-1, 1) if a.ndim == 1 else a


def sq_dists(obs, book):
    """d2[n, j] = sum_d (obs[n, d] - book[j, d])^2, the features added in order."""
    d2 = np.zeros((obs.shape[0], book.shape[0]), dtype=obs.dtype)
    for d in range(obs.shape[1]):
        t = obs[:, d:d + 1] - book[None, :, d]
        d2 += t * t
    return d2


def vq_ref(obs, code_book):
    """-> (code int32 [N], dist float64 [N]); argmin takes the first minimum."""
    obs, book = _as2d(obs), _as2d(code_book)
    d2 = sq_dists(obs, book)
    code = np.argmin(d2, axis=1)
    return code.astype(np.int32), np.sqrt(d2[np.arange(obs.shape[0]), code])


def update_ref(obs, code, k):
    """update_cluster_means: float64 member sums in point order / counts -> (means [k, D]
    with zeros for a code without members, counts [k])."""
    obs = _as2d(obs)
    sums = np.zeros((k, obs.shape[1]))
    np.add.at(sums, code, obs)
    counts = np.bincount(code, minlength=k)
    means = sums / np.maximum(counts, 1)[:, None]
    return means, counts


def run_ref(obs, guess, thresh=1e-5, trace=None):
    """One run (scipy.cluster.vq._kmeans) -> (code_book, distortion).  trace: a list that
    receives the labels of every iteration."""
    obs, book = _as2d(obs), _as2d(guess)
    diff, prev = np.inf, np.inf
    while diff > thresh:
        code, dist = vq_ref(obs, book)
        avg = np.mean(dist)
        if trace is not None:
            trace.append(code)
        means, counts = update_ref(obs, code, book.shape[0])
        book = means[counts > 0]
        diff = np.abs(prev - avg)
        prev = avg
    return book, prev


def generator(seed=None, rng=None):
    if rng is not None:
        return rng if isinstance(rng, (np.random.RandomState, np.random.Generator)) else np.random.default_rng(rng)
    if seed is None:
        return np.random.mtrand._rand
    return seed if isinstance(seed, (np.random.RandomState, np.random.Generator)) else np.random.RandomState(seed)


def start_indices_ref(N, k, iter, seed=None, rng=None):
    gen = generator(seed, rng)
    return [np.asarray(gen.choice(N, size=int(k), replace=False)) for _ in range(iter)]


def kmeans_ref(obs, k_or_guess, iter=20, thresh=1e-5, check_finite=True, *, seed=None, rng=None, all_runs=None):
    """-> (code_book, distortion).  all_runs: a list that receives every restart's
    (code_book, distortion)."""
    one_d = np.ndim(obs) == 1
    obs = np.asarray_chkfinite(obs, dtype=np.float64) if check_finite else np.asarray(obs, dtype=np.float64)
    guess = np.asarray_chkfinite(k_or_guess) if check_finite else np.asarray(k_or_guess)
    if iter < 1:
        raise ValueError(f"iter must be at least 1, got {iter}")
    shape = (lambda b: b.reshape(-1)) if one_d else (lambda b: b)
    if guess.size != 1:
        if guess.size < 1:
            raise ValueError(f"Asked for 0 clusters. Initial book was {guess}")
        book, dist = run_ref(obs, guess, thresh)
        return shape(book), dist
    k = int(guess)
    if k != guess:
        raise ValueError("If k_or_guess is a scalar, it must be an integer.")
    if k < 1:
        raise ValueError("Asked for %d clusters." % k)
    o2 = _as2d(obs)
    gen = generator(seed, rng)
    best_book, best_dist = None, np.inf
    for _ in range(iter):
        idx = gen.choice(o2.shape[0], size=k, replace=False)
        book, dist = run_ref(o2, o2[idx], thresh)
        if all_runs is not None:
            all_runs.append((book, dist))
        if dist < best_dist:
            best_book, best_dist = book, dist
    return shape(best_book), best_dist


def kmeans_f32_emulation(obs, guess, thresh=1e-5, trace=None):
    """One run in the device's arithmetic: inputs rounded to float32 once, squared
    distances from the float32 differences accumulated in float32, first minimum, float32
    square root, float64 mean of the distances, float64 member sums, code book rounded to
    float32 after every update.  -> (code_book float32, distortion, iterations)."""
    obs = np.ascontiguousarray(_as2d(obs), dtype=np.float32)
    book = np.ascontiguousarray(_as2d(guess), dtype=np.float32)
    diff, prev, iters = np.inf, np.inf, 0
    while diff > thresh:
        d2 = sq_dists(obs, book)
        assert d2.dtype == np.float32
        code = np.argmin(d2, axis=1)
        dist = np.sqrt(d2[np.arange(obs.shape[0]), code])
        avg = np.mean(dist.astype(np.float64))
        if trace is not None:
            trace.append(code.astype(np.int32))
        means, counts = update_ref(obs.astype(np.float64), code, book.shape[0])
        book = means[counts > 0].astype(np.float32)
        diff = np.abs(prev - avg)
        prev = avg
        iters += 1
    return book, prev, iters


def shifted_gaussian(N, D, seed):
    """The free-running test input: standard normal rows, a third of them shifted by 3."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(N, D))
    X[: N // 3] += 3.0
    return X


def sort_rows(a):
    a = _as2d(a)
    return a[np.lexsort(a.T[::-1])]


# The free-running inputs of tests/test_gpu_kmeans.py beside the fixture's Xtrain:
# (N, D, k), run with seed 0 and GAUSSIAN_RESTARTS restarts.  tests/test_kmeans_host.py checks
# that the float32 emulation follows the float64 reference on each of them (same iteration
# count, surviving codes and labels in every iteration), so that a comparison of the
# device result with the float64 reference is meaningful.
GAUSSIAN_CASES = ((1500, 8, 64), (1000, 32, 48), (777, 3, 130))
GAUSSIAN_RESTARTS = 4


def gaussian_case(N, D, k):
    return shifted_gaussian(N, D, 1000 * D + k)


# The tie inputs: n distinct 2-D points (float32 values), each `reps` times.  The k start
# rows hold duplicates, which tie exactly: the lower index takes every member and the higher
# one is dropped.  Run with one restart per seed.  (n, reps, k, seeds); the second has more
# than 1024 codes, so the device's scans over the codes carry across their 1024-code steps
# and codes are dropped on both sides of a step.
TIE_CASES = ((40, 10, 60, (1, 2, 3)), (1000, 3, 1500, (0,)))


def duplicates_case(n=40, reps=10):
    rng = np.random.default_rng(n)
    return np.repeat(rng.normal(size=(n, 2)).astype(np.float32).astype(np.float64), reps, axis=0)


# One lane per point (the assignment kernel's layout from N = 131072): (N, D, k), one run
# from the first start rows of seed 0.
LARGE_N_CASE = (131075, 2, 4)
