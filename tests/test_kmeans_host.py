"""CPU tests of the device k-means: the float64 statement tests/kmeans_ref.py against SciPy
and the stored SciPy results, the start indices, the C-ABI entries' argument checks and
size limits (all made before any HIP call, so they run without a GPU), and the suitability
of the free-running GPU test inputs."""
import ctypes

import numpy as np
import pytest

from modulatedgps_amd import _lib, cluster
from tests import kmeans_ref as KR
from tests.helpers import load_golden

ENTRIES = ("mgp_vq", "mgp_kmeans_workspace_bytes", "mgp_kmeans_init", "mgp_kmeans_iterate", "mgp_kmeans_select",
           "mgp_kmeans_update")
MGP_ERR_WORKSPACE, MGP_ERR_ALIGN, MGP_ERR_UNSUPPORTED = 1, 2, 3
NMAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def demo():
    return load_golden("demo_tf2_data.npz")


def test_entries_are_bound_declared_and_exported():
    syms = _lib.header_symbols()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and name in syms and hasattr(raw, name), name


# ------------------------------------------------------------------ the reference
def test_reference_is_scipy_bit_for_bit(demo):
    """Integer k with seed 0 and 1 and an array guess (below SciPy's five-feature switch to
    a BLAS distance, so the arithmetic is the same operation for operation)."""
    sp = pytest.importorskip("scipy.cluster.vq")
    X = demo["Xtrain"]
    G = KR.gaussian_case(777, 3, 130)
    for obs, k in ((X, 25), (X[:, 0], 7), (G, 130)):
        for seed in (0, 1):
            a, b = sp.kmeans(obs, k, seed=seed), KR.kmeans_ref(obs, k, seed=seed)
            assert a[0].shape == b[0].shape and np.array_equal(a[0], b[0]) and a[1] == b[1]
    a, b = sp.kmeans(G, 12, iter=5, rng=3), KR.kmeans_ref(G, 12, iter=5, rng=3)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    for obs, guess in ((G, G[:40]), (X, X[::100]), (G, np.repeat(G[:5], 3, axis=0))):
        a, b = sp.kmeans(obs, guess), KR.kmeans_ref(obs, guess)
        assert a[0].shape == b[0].shape and np.array_equal(a[0], b[0]) and a[1] == b[1]
    code, dist = sp.vq(G, G[:40])
    rc, rd = KR.vq_ref(G, G[:40])
    assert np.array_equal(code, rc) and np.array_equal(dist, rd)


def test_reference_reproduces_the_stored_scipy_results(demo):
    X = demo["Xtrain"]
    for name, obs, k, seed in (("Z", X, 25, 0), ("Z_assign", X, 25, 1), ("Z20", X[:600], 20, 0),
                               ("Z20_assign", X[:600], 20, 1)):
        book, _ = KR.kmeans_ref(obs, k, seed=seed)
        assert book.shape == demo[name].shape
        np.testing.assert_allclose(KR.sort_rows(book), KR.sort_rows(demo[name]), rtol=0, atol=1e-12)


def test_start_indices_are_scipys():
    """cluster.start_indices draws what scipy.cluster.vq._kpoints draws, restart by restart."""
    for kw in (dict(seed=0), dict(seed=1), dict(rng=5)):
        ours = cluster.start_indices(1500, 25, 20, **kw)
        ref = KR.start_indices_ref(1500, 25, 20, **kw)
        assert ours.shape == (20, 25) and ours.dtype == np.int64
        assert all(np.array_equal(a, b) for a, b in zip(ours, ref))
    spv = pytest.importorskip("scipy.cluster.vq")
    drawn = []

    class Spy(np.random.RandomState):
        def choice(self, *a, **kw):
            drawn.append(super().choice(*a, **kw))
            return drawn[-1]
    obs = KR.gaussian_case(777, 3, 130)
    spv.kmeans(obs, 9, iter=3, seed=Spy(7))
    assert all(np.array_equal(a, b) for a, b in zip(cluster.start_indices(777, 9, 3, seed=7), drawn))
    with pytest.raises(ValueError):
        cluster.start_indices(10, 11, 1, seed=0)         # k > N: choice raises
    with pytest.raises(TypeError):
        cluster.start_indices(10, 2, 1, seed=0, rng=0)


# ------------------------------------------------------------------ the C-ABI
def _call(name, base, **kw):
    assert len(base) == len(_lib.SIGNATURES[name][1]), name
    return getattr(_lib.load(), name)(*{**base, **kw}.values())


def _ws(N, k, D, R):
    return _lib.load().mgp_kmeans_workspace_bytes(N, k, D, R)


def test_workspace_query_and_limits():
    assert _ws(1500, 25, 1, 20) > 0 and _ws(1500, 25, 1, 20) % 256 == 0
    assert _ws(65536, 1024, 8, 20) > _ws(65536, 1024, 8, 1)
    assert _ws(100, 100, 32, 64) > 0 and _ws(NMAX, 1, 1, 1) > 0
    # one past each limit, and nonsense sizes: 0
    assert _ws(100, 10, 33, 1) == 0 and _ws(100, 10, 8, 65) == 0 and _ws(100, 101, 8, 1) == 0
    assert _ws(NMAX + 1, 10, 8, 1) == 0 and _ws(0, 1, 1, 1) == 0 and _ws(10, 0, 1, 1) == 0


def test_vq_rejects_bad_arguments_before_any_hip_call():
    c = ctypes.c_void_p(256)
    base = dict(obs=c, ldo=8, code_book=c, ldc=8, N=100, k=10, D=8, code=c, dist=c, stream=None)
    call = lambda **kw: _call("mgp_vq", base, **kw)
    assert call(obs=None) == -1 and call(ldo=7) == -2 and call(code_book=None) == -3 and call(ldc=7) == -4
    assert call(N=-1) == -5 and call(k=0) == -6 and call(D=0) == -7 and call(code=None) == -8
    assert call(dist=None) == -9
    assert call(D=33, ldo=33, ldc=33) == MGP_ERR_UNSUPPORTED
    assert call(N=NMAX + 1) == MGP_ERR_UNSUPPORTED and call(k=NMAX + 1) == MGP_ERR_UNSUPPORTED
    assert call(N=0) == 0


def test_kmeans_entries_reject_bad_arguments_before_any_hip_call():
    c = ctypes.c_void_p(256)
    N, k, D, R = 100, 10, 8, 4
    wsb = _ws(N, k, D, R)
    init = dict(obs=c, ldo=D, N=N, D=D, idx=c, guess=None, ldg=0, k=k, R=R, ws=c, wsb=wsb, stream=None)
    call = lambda **kw: _call("mgp_kmeans_init", init, **kw)
    assert call(obs=None) == -1 and call(ldo=D - 1) == -2 and call(N=0) == -3 and call(D=0) == -4
    assert call(idx=None) == -5 and call(guess=c, ldg=D) == -6
    assert call(idx=None, guess=c, ldg=D - 1, R=1) == -7
    assert call(k=0) == -8 and call(R=0) == -9 and call(idx=None, guess=c, ldg=D) == -9
    assert call(D=33, ldo=33) == call(R=65) == call(k=N + 1) == call(N=NMAX + 1) == MGP_ERR_UNSUPPORTED
    assert call(wsb=wsb - 1) == call(ws=None) == MGP_ERR_WORKSPACE
    assert call(ws=ctypes.c_void_p(264)) == MGP_ERR_ALIGN

    it = dict(obs=c, ldo=D, N=N, D=D, k=k, R=R, B=8, thresh=1e-5, ws=c, wsb=wsb, done=c, stream=None)
    call = lambda **kw: _call("mgp_kmeans_iterate", it, **kw)
    assert call(obs=None) == -1 and call(ldo=D - 1) == -2 and call(N=0) == -3 and call(D=0) == -4
    assert call(k=0) == -5 and call(R=0) == -6 and call(B=0) == -7 and call(thresh=float("nan")) == -8
    assert call(done=None) == -11
    assert call(D=33, ldo=33) == call(R=65) == call(k=N + 1) == call(N=NMAX + 1) == MGP_ERR_UNSUPPORTED
    assert call(wsb=wsb - 1) == call(ws=None) == MGP_ERR_WORKSPACE

    sel = dict(N=N, k=k, D=D, R=R, ws=c, wsb=wsb, code_book=c, ldcb=D, distortion=c, info=c, stream=None)
    call = lambda **kw: _call("mgp_kmeans_select", sel, **kw)
    assert call(N=0) == -1 and call(k=0) == -2 and call(D=0) == -3 and call(R=0) == -4
    assert call(code_book=None) == -7 and call(ldcb=D - 1) == -8 and call(distortion=None) == -9
    assert call(info=None) == -10
    assert call(D=33, ldcb=33) == call(R=65) == call(k=N + 1) == call(N=NMAX + 1) == MGP_ERR_UNSUPPORTED
    assert call(wsb=wsb - 1) == call(ws=None) == MGP_ERR_WORKSPACE

    wsb1 = _ws(N, k, D, 1)
    upd = dict(obs=c, ldo=D, N=N, D=D, code=c, k=k, means=c, ldm=D, counts=c, ws=c, wsb=wsb1, stream=None)
    call = lambda **kw: _call("mgp_kmeans_update", upd, **kw)
    assert call(obs=None) == -1 and call(ldo=D - 1) == -2 and call(N=0) == -3 and call(D=0) == -4
    assert call(code=None) == -5 and call(k=0) == -6 and call(means=None) == -7 and call(ldm=D - 1) == -8
    assert call(counts=None) == -9
    assert call(D=33, ldo=33, ldm=33) == call(k=N + 1) == call(N=NMAX + 1) == MGP_ERR_UNSUPPORTED
    assert call(wsb=wsb1 - 1) == call(ws=None) == MGP_ERR_WORKSPACE


def test_python_argument_checks_need_no_device():
    with pytest.raises(ValueError):
        cluster.kmeans(np.array([[0.0], [np.nan]]), 1)
    with pytest.raises(ValueError):
        cluster.kmeans(np.array([[0.0], [np.inf]]), np.array([[0.0]]))
    with pytest.raises(ValueError):
        cluster.vq(np.array([[0.0], [1.0]]), np.array([[np.nan]]))


# ------------------------------------------------------------------ input suitability
def _follows(obs, idx):
    """The float32 emulation of the device arithmetic takes the float64 reference's path
    from the start rows obs[idx]: same iterations, surviving codes and labels."""
    t64, t32 = [], []
    b64, d64 = KR.run_ref(obs, obs[idx], trace=t64)
    b32, d32, iters = KR.kmeans_f32_emulation(obs, obs[idx], trace=t32)
    return (iters == len(t64) and b32.shape == b64.shape and all(np.array_equal(p, q) for p, q in zip(t64, t32))
            and abs(d32 - d64) <= 1e-6 * d64)


def test_free_running_inputs_are_suitable(demo):
    X = demo["Xtrain"]
    for seed in (0, 1):
        for idx in KR.start_indices_ref(X.shape[0], 25, 20, seed=seed):
            assert _follows(X, idx), seed
    for n, reps, k, seeds in KR.TIE_CASES:
        dup = KR.duplicates_case(n, reps)
        for seed in seeds:
            assert _follows(dup, KR.start_indices_ref(dup.shape[0], k, 1, seed=seed)[0]), (n, seed)
    N, D, k = KR.LARGE_N_CASE
    big = KR.gaussian_case(N, D, k)
    assert _follows(big, KR.start_indices_ref(N, k, 1, seed=0)[0])
    for N, D, k in KR.GAUSSIAN_CASES:
        obs = KR.gaussian_case(N, D, k)
        for idx in KR.start_indices_ref(N, k, KR.GAUSSIAN_RESTARTS, seed=0):
            assert _follows(obs, idx), (N, D, k)
