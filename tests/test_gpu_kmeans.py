"""GPU tests of the device k-means (csrc/kmeans.hip; modulatedgps_amd.cluster) against the
float64 statement tests/kmeans_ref.py.

Tolerances (none taken from the code under test):
  labels    equal at every point whose float64 gap (d2_2 - d2_1) / d2_2 between the two
            nearest codes exceeds 1e-5: the float32 rounding of a D = 32 sum of squares is
            (D + 2) 2^-24 ~ 2e-6, so 1e-5 leaves 5x.  At most 0.5 % of the points may fall
            under the gap and be excused (the reference alone excuses <= 0.05 % here).
  dist      1e-6 relative (half the rounding of d2, plus the float32 square root).
  means     2^-22 max|obs|: four roundings of one input; the float64 sums add nothing.
  distortion 1e-6 relative.
Every measured figure is printed (`KMERR <quantity> <value>`) before it is asserted."""
import functools

import numpy as np
import pytest
import torch

from modulatedgps_amd import _lib, cluster, ops
from tests import kmeans_ref as KR
from tests.helpers import load_golden

pytestmark = pytest.mark.gpu

GAP = 1e-5
EXCUSED = 0.005
DIST_RTOL = 1e-6
MEAN_EPS = 2.0 ** -22

# 4099 and 257 are ragged against every tile; (20000, 8, 1024) covers several codebook tiles
# and the 4-lanes-per-point kernel (N >= 8192), the others the 16-lane one
VQ_SHAPES = [(1, 1, 1), (257, 1, 3), (777, 3, 130), (1500, 8, 64), (1000, 32, 48), (4099, 5, 257),
             (20000, 8, 1024)]


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def dev(a, device, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), device=device).to(dtype)


@functools.lru_cache(maxsize=None)
def _vq_case(N, D, k, offset):
    """float32 obs and code book of one shape and their float64 reference (computed once).
    offset: the copy on a 2^-10 grid shifted by 1024 -- exactly representable in float32,
    far from the origin."""
    rng = np.random.default_rng(100 * N + 10 * D + k)
    obs, book = rng.normal(size=(N, D)), rng.normal(size=(k, D))
    if offset:
        obs, book = np.round(obs * 1024) / 1024 + 1024, np.round(book * 1024) / 1024 + 1024
        assert np.array_equal(f32(obs), obs) and np.array_equal(f32(book), book)
    obs, book = f32(obs), f32(book)
    d2 = KR.sq_dists(obs.astype(np.float64), book.astype(np.float64))
    code = np.argmin(d2, axis=1)
    part = np.partition(d2, 1, axis=1)[:, :2] if k > 1 else None
    gap = (part[:, 1] - part[:, 0]) / part[:, 1] if k > 1 else np.full(N, np.inf)
    return obs, book, code.astype(np.int32), np.sqrt(d2[np.arange(N), code]), gap


@pytest.mark.parametrize("offset", [False, True], ids=["origin", "offset1024"])
@pytest.mark.parametrize("N,D,k", VQ_SHAPES)
def test_assignment_matches_the_reference(device, N, D, k, offset):
    obs, book, code_ref, dist_ref, gap = _vq_case(N, D, k, offset)
    code, dist = cluster.vq_device(dev(obs, device), dev(book, device))
    assert code.dtype == torch.int32 and dist.dtype == torch.float32
    code, dist = code.cpu().numpy(), dist.cpu().numpy().astype(np.float64)
    decided = gap > GAP
    excused = 1.0 - decided.mean()
    mism = int((code[decided] != code_ref[decided]).sum())
    derr = float(np.max(np.abs(dist - dist_ref) / np.maximum(dist_ref, 1e-300)))
    print(f"KMERR excused_fraction {excused:.3e}")
    print(f"KMERR label_mismatches {mism}")
    print(f"KMERR dist_rel {derr:.3e}")
    assert code.min() >= 0 and code.max() < k
    assert excused <= EXCUSED
    assert mism == 0
    assert derr <= DIST_RTOL
    # the host form returns SciPy's types
    if N <= 1500:
        c2, d2 = cluster.vq(obs, book)
        assert c2.dtype == np.int32 and d2.dtype == np.float64 and np.array_equal(c2, code)


def test_assignment_with_one_lane_per_point(device):
    """From N = 131072 a point has one lane (below: 4 or 16 that split the codes)."""
    test_assignment_matches_the_reference(device, 131075, 3, 37, True)


# ------------------------------------------------------------------ ties and empty codes
TIES = [(n, reps, k, seed) for n, reps, k, seeds in KR.TIE_CASES for seed in seeds]


@pytest.mark.parametrize("n,reps,k,seed", TIES)
def test_ties_go_to_the_lowest_index_and_empty_codes_are_dropped(device, n, reps, k, seed):
    obs = KR.duplicates_case(n, reps)
    ref_book, ref_dist = KR.kmeans_ref(obs, k, iter=1, seed=seed)
    idx = KR.start_indices_ref(n * reps, k, 1, seed=seed)[0]
    assert len(np.unique(obs[idx], axis=0)) < k           # the start really holds duplicates
    assert ref_book.shape[0] < k
    # the first assignment: a duplicate code never wins
    code, _ = cluster.vq(obs, obs[idx])
    assert np.array_equal(code, KR.vq_ref(obs, obs[idx])[0])
    book, dist = cluster.kmeans(obs, k, iter=1, seed=seed)
    print(f"KMERR survivors {book.shape[0]} (oracle {ref_book.shape[0]})")
    assert book.shape == ref_book.shape
    err = float(np.abs(book - ref_book).max())          # rows keep their order: no sorting
    print(f"KMERR tie_codebook_abs {err:.3e}")
    assert err <= MEAN_EPS * np.abs(obs).max()
    assert abs(dist - ref_dist) <= DIST_RTOL * ref_dist


# ------------------------------------------------------------------ one update
@pytest.mark.parametrize("N,D,k,kind", [(65536, 8, 2, "all_in_one"), (4099, 5, 257, "random"),
                                         (1000, 32, 48, "random"), (1500, 1, 25, "random"),
                                         (20000, 3, 2500, "random")])   # > 1024 codes: the scans carry
def test_update_from_given_labels(device, N, D, k, kind):
    rng = np.random.default_rng(N + k)
    obs = f32(rng.normal(size=(N, D)) * 3 + 5)
    if kind == "all_in_one":
        code = np.ones(N, dtype=np.int32)                 # code 0 is empty, code 1 owns all
    else:
        code = rng.integers(0, k, N).astype(np.int32)
        code[code == k // 2] = 0                          # an empty code in the middle
    means_ref, counts_ref = KR.update_ref(obs.astype(np.float64), code, k)
    means, counts = ops.kmeans_update(dev(obs, device), dev(code, device, torch.int32), k)
    means, counts = means.cpu().numpy().astype(np.float64), counts.cpu().numpy()
    assert np.array_equal(counts, counts_ref)
    assert (counts_ref == 0).any() and np.all(means[counts_ref == 0] == 0)
    err = float(np.abs(means - means_ref).max())
    print(f"KMERR update_mean_abs {err:.3e} (bound {MEAN_EPS * np.abs(obs).max():.3e})")
    assert err <= MEAN_EPS * np.abs(obs).max()


# ------------------------------------------------------------------ free-running kmeans
@functools.lru_cache(maxsize=None)
def _demo():
    return load_golden("demo_tf2_data.npz")


def _check_book(book, dist, ref_book, ref_dist, obs):
    assert book.dtype == np.float64 and book.shape == ref_book.shape
    err = float(np.abs(KR.sort_rows(book) - KR.sort_rows(ref_book)).max())
    derr = abs(dist - ref_dist) / ref_dist
    print(f"KMERR codebook_abs {err:.3e} (bound {MEAN_EPS * np.abs(obs).max():.3e})")
    print(f"KMERR distortion_rel {derr:.3e}")
    assert err <= MEAN_EPS * np.abs(obs).max()
    assert derr <= DIST_RTOL


@pytest.mark.parametrize("seed,field", [(0, "Z"), (1, "Z_assign")])
def test_kmeans_reproduces_the_demo_inducing_points(device, seed, field):
    d = _demo()
    X = d["Xtrain"]
    book, dist = cluster.kmeans(X, 25, seed=seed)
    _, ref_dist = KR.kmeans_ref(X, 25, seed=seed)
    _check_book(book, dist, d[field], ref_dist, X)


@pytest.mark.parametrize("N,D,k", KR.GAUSSIAN_CASES)
def test_kmeans_free_running_gaussian(device, N, D, k):
    obs = KR.gaussian_case(N, D, k)
    ref_book, ref_dist = KR.kmeans_ref(obs, k, iter=KR.GAUSSIAN_RESTARTS, seed=0)
    book, dist = cluster.kmeans(obs, k, iter=KR.GAUSSIAN_RESTARTS, seed=0)
    _check_book(book, dist, ref_book, ref_dist, obs)
    # the same through an array guess: the first restart's start rows
    guess = obs[KR.start_indices_ref(N, k, 1, seed=0)[0]]
    ref_book, ref_dist = KR.kmeans_ref(obs, guess)
    book, dist = cluster.kmeans(obs, guess)
    _check_book(book, dist, ref_book, ref_dist, obs)


def test_kmeans_with_one_lane_per_point(device):
    N, D, k = KR.LARGE_N_CASE
    obs = KR.gaussian_case(N, D, k)
    guess = obs[KR.start_indices_ref(N, k, 1, seed=0)[0]]
    ref_book, ref_dist = KR.kmeans_ref(obs, guess)
    book, dist = cluster.kmeans(obs, guess)
    _check_book(book, dist, ref_book, ref_dist, obs)


def test_kmeans_array_guess_on_the_demo_data(device):
    X = _demo()["Xtrain"]
    guess = X[KR.start_indices_ref(X.shape[0], 25, 1, seed=0)[0]]
    ref_book, ref_dist = KR.kmeans_ref(X, guess)
    book, dist = cluster.kmeans(X, guess, iter=3)          # iter is ignored with a guess
    _check_book(book, dist, ref_book, ref_dist, X)
    # 1-D observations give a 1-D code book, as in SciPy
    b1, d1 = cluster.kmeans(X[:, 0], guess[:, 0])
    assert b1.shape == (book.shape[0],) and np.array_equal(b1, book[:, 0]) and d1 == dist


# ------------------------------------------------------------------ invariances
def _bits(res):
    book, dist = res
    return book.cpu().numpy().tobytes(), np.float64(dist).tobytes()


def test_result_bits_do_not_depend_on_block_batching_or_the_call(device):
    N, D, k = KR.GAUSSIAN_CASES[0]
    obs = dev(f32(KR.gaussian_case(N, D, k)), device)
    R = KR.GAUSSIAN_RESTARTS
    base = _bits(cluster.kmeans_device(obs, k, iter=R, seed=0))
    assert _bits(cluster.kmeans_device(obs, k, iter=R, seed=0)) == base                # two calls
    assert _bits(cluster.kmeans_device(obs, k, iter=R, seed=0, block=1)) == base       # B = 1 vs 8
    assert _bits(cluster.kmeans_device(obs, k, iter=R, seed=0, runs_per_launch=1)) == base
    # the same runs one at a time through the array guess, compared on the host
    best = None
    for idx in cluster.start_indices(N, k, R, seed=0):
        res = cluster.kmeans_device(obs, obs[torch.as_tensor(idx, device=device)])
        if best is None or res[1] < best[1]:
            best = res
    assert _bits(best) == base


def test_vq_device_on_a_row_view_equals_the_contiguous_call(device):
    rng = np.random.default_rng(9)
    wide = dev(f32(rng.normal(size=(777, 8))), device)
    book = dev(f32(rng.normal(size=(130, 8))), device)
    view, bview = wide[:, :3], book[:, :3]
    assert not view.is_contiguous()
    c1, d1 = cluster.vq_device(view, bview)
    c2, d2 = cluster.vq_device(view.contiguous(), bview.contiguous())
    assert torch.equal(c1, c2) and torch.equal(d1, d2)
    c3, d3 = cluster.vq_device(wide[::2], book)            # every other row
    c4, d4 = cluster.vq_device(wide[::2].contiguous(), book)
    assert torch.equal(c3, c4) and torch.equal(d3, d4)


# ------------------------------------------------------------------ interface
def test_interface_errors(device):
    X = _demo()["Xtrain"]
    bad = X.copy()
    bad[3, 0] = np.nan
    with pytest.raises(ValueError):
        cluster.kmeans(bad, 25, seed=0)
    with pytest.raises(ValueError):
        cluster.kmeans(X, np.array([[np.inf]]) * np.ones((2, 1)))
    with pytest.raises(ValueError):
        cluster.vq(dev(bad, device), X[:5])
    with pytest.raises(ValueError):
        cluster.kmeans(X, X.shape[0] + 1, seed=0)          # k > N: the ValueError of choice
    with pytest.raises(ValueError):
        cluster.kmeans(X, 0)
    # D = 33: refused before anything is launched or written
    obs = torch.zeros(100, 33, device=device)
    code = torch.full((100,), -7, dtype=torch.int32, device=device)
    dist = torch.full((100,), -7.0, device=device)
    with pytest.raises(_lib.MGPError) as e:
        ops.vq(obs, obs[:10], code=code, dist=dist)
    assert e.value.status == 3
    torch.cuda.synchronize()
    assert bool((code == -7).all()) and bool((dist == -7.0).all())
    with pytest.raises(_lib.MGPError) as e:
        cluster.kmeans(obs, 5, seed=0)
    assert e.value.status == 3


def test_drop_in_import_feeds_the_svgp_layer(device):
    from MixtureGPs.cluster import kmeans
    from modulatedgps_amd.kernels import SquaredExponential
    from modulatedgps_amd.likelihoods import GaussianModified
    from modulatedgps_amd.models import SVGPModified
    d = _demo()
    Z = kmeans(d["Xtrain"], 25, seed=0)[0]                  # the demo's line, import changed
    assert isinstance(Z, np.ndarray) and Z.dtype == np.float64 and Z.shape == (25, 1)
    lik = GaussianModified(variance=np.full((1, 3), 0.1), device=device)
    kern = SquaredExponential(variance=1.0, lengthscales=1.0, device=device)
    layer = SVGPModified(kern, lik, inducing_variable=Z, num_latent_gps=3, whiten=True, device=device)
    assert tuple(layer.inducing_variable.shape) == (25, 1)
    np.testing.assert_allclose(layer.inducing_variable.cpu().numpy()[:, 0], Z[:, 0], rtol=1e-6)
