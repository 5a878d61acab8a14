"""Cases for the translation invariance of the RBF kernels (tests/test_translation_host.py,
tests/test_gpu_translation.py).

A case is *grid-exact* when every coordinate of X and Z is a multiple of 2^-10 in [-4, 4]
and the per-axis offset c is a multiple of 2^-10 with |c| <= 4096.  Then x + c needs at most
13 integer and 10 fraction bits: X + c and Z + c are exact in float32, and every difference
of two shifted coordinates, (x + c) - (z + c) = x - z, is exact in float32 too.  A kernel that
takes differences of raw coordinates before any scaling, squaring or product therefore
returns the same bits for (X, Z) and (X + c, Z + c): the assertion needs no tolerance.

The float64 reference is oracle.cpu_ref.rbf_K / rbf_Kuu on the float32-rounded inputs."""
import numpy as np

from oracle import cpu_ref as R

GRID = 2.0 ** -10
LIMIT = 4.0
MAX_OFFSET = 4096.0
# the mixed offset's cycle over the axes: a large positive one, the largest negative one, a
# small one, and two with every fraction bit of the grid in use
MIXED = (1024.0, -4096.0, 0.5, -333.0009765625, 4095.9990234375)
OFFSETS = ("zero", "plus1024", "mixed")
KUF_CENTRE_ROWS = 32   # kuf_image.hpp kKufCentre


def snap(A):
    """A clipped to [-4, 4] and rounded to the 2^-10 grid (float32, exact)."""
    out = (np.round(np.clip(np.asarray(A, np.float64), -LIMIT, LIMIT) / GRID) * GRID).astype(np.float32)
    assert np.array_equal(out.astype(np.float64) / GRID, np.round(out.astype(np.float64) / GRID))
    return out


def offset_vector(kind, D):
    """The per-axis offset [D] (float64) of one of OFFSETS."""
    if kind == "zero":
        c = np.zeros(D)
    elif kind == "plus1024":
        c = np.full(D, 1024.0)
    elif kind == "mixed":
        c = np.array([MIXED[d % len(MIXED)] for d in range(D)])
    else:
        raise ValueError(kind)
    assert np.all(np.abs(c) <= MAX_OFFSET) and np.array_equal(c / GRID, np.round(c / GRID))
    return c


def shift(A, c):
    """A + c in float32 for a grid-exact A [.., D] and offset c [D]; asserts the shift is exact."""
    A = np.asarray(A)
    assert A.dtype == np.float32
    exact = A.astype(np.float64) + np.asarray(c, np.float64)
    As = exact.astype(np.float32)
    assert np.array_equal(As.astype(np.float64), exact), "the shifted coordinates are not exact in float32"
    assert np.array_equal((As - np.asarray(c, np.float64)).astype(np.float32), A)
    return As


def grid_case(N, M, D, ard, seed=0):
    """Grid-exact X [N, D], Z [M, D] (float32), variance, lengthscales ([1] or [D], float32).
    The lengthscales grow with sqrt(D) so that Kuf keeps entries of every size."""
    rng = np.random.default_rng(1000 * D + 10 * seed + int(ard))
    X = snap(rng.standard_normal((N, D)))
    Z = snap(rng.standard_normal((M, D)))
    ls = (rng.uniform(0.5, 2.0, D) if ard else np.array([0.7])) * np.sqrt(D)
    return X, Z, 0.7, ls.astype(np.float32)


def f64(A):
    return np.asarray(A, np.float32).astype(np.float64)


def rbf_K_ref(Z, X, variance, ls, centred=True):
    """float64 K(Z, X) of the float32-rounded inputs and hyperparameters.  The oracle evaluates
    GPflow's expanded square distance, whose float64 cancellation error grows with the squared
    offset (4e-9 of the variance at an offset of 4096 and lengthscale 0.7,
    tests/test_translation_host.py), so it is given the inputs minus Z[0]: a difference of two
    float32 numbers, exact in float64.  centred=False: the oracle on the inputs as they are."""
    Z, X = f64(Z), f64(X)
    z0 = Z[0] if centred else 0.0
    return R.rbf_K(Z - z0, X - z0, float(np.float32(variance)), f64(ls))


def rbf_Kuu_ref(Z, variance, ls, jitter, centred=True):
    Z = f64(Z)
    return R.rbf_Kuu(Z - (Z[0] if centred else 0.0), float(np.float32(variance)), f64(ls), jitter)


def kuf_reference_point(Z):
    """The point K1's image kernel subtracts from Z and X (kuf_image.hpp), in float64:
    Z[0] + the mean over the rows i M / 32, i < 32, of (Z[i M / 32] - Z[0])."""
    Z = f64(Z)
    M = Z.shape[0]
    rows = (np.arange(KUF_CENTRE_ROWS) * M) // KUF_CENTRE_ROWS
    return Z[0] + np.mean(Z[rows] - Z[0], axis=0)


def image_bound(Z, X, variance, ls, k64):
    """The elementwise bound of tests/test_gpu_kernels.py::test_kuf_and_trsm_images on a decoded
    Kuf image, its `norms` term taken about the reference point the kernel subtracts:
    2e-6 variance + k ln2 8 2^-24 (|z'|^2 + |x'|^2), z' = (z - ref) sqrt(0.5 log2 e) / l."""
    ref = kuf_reference_point(Z)
    c2 = 0.5 * np.log2(np.e) / np.broadcast_to(f64(ls), (Z.shape[1],)) ** 2
    norms = np.sum(c2 * (f64(Z) - ref) ** 2, 1)[:, None] + np.sum(c2 * (f64(X) - ref) ** 2, 1)[None, :]
    return 2e-6 * variance + k64 * np.log(2.0) * 8 * 2.0 ** -24 * norms


def shifted_params(p, c):
    """A copy of an oracle SMGPParams with both layers' (grid-exact, float32) Z moved by c."""
    def layer(L):
        out = dict(L)
        out["Z"] = shift(L["Z"], c).astype(np.float64)
        return out
    return R.SMGPParams(layer(p.pred), layer(p.assign), p.lik_variance, p.num_data, p.S)


def snapped_problem(N, M, K, D, ls, S, state="perturbed"):
    """oracle.cpu_ref.synthetic_problem with X and both layers' Z snapped to the grid."""
    X, Y, p = R.synthetic_problem(N, M, K, D, ls, state=state, S=S)
    X = snap(X)
    for L in (p.pred, p.assign):
        L["Z"] = snap(L["Z"])
    return X, Y, p
