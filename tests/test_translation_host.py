"""The translation cases of tests/translation_ref.py are sound (no GPU): the shifts are exact
in float32 and the float64 reference itself does not care where the data sits.

The oracle's rbf_K evaluates GPflow's expanded square distance |a|^2 + |b|^2 - 2 a.b in
float64.  At the largest offset used (4096 on an axis, lengthscale 0.7 sqrt(D)) its three
terms are ~1e8 and cancel to r2 = O(10): an absolute error of a few eps64 1e8 on r2, measured
below as up to 4e-9 of the variance on K (printed, asserted below 1e-7) -- not the 1e-10 one
would like under the GPU tests' tightest bounds (5e-7 normwise, 2e-6 variance elementwise).
translation_ref therefore hands the oracle the inputs minus Z[0], an exact float64 difference
of float32 numbers, and that reference of the shifted case equals the unshifted one to 1e-9
relative to the variance (on the grid-exact cases, to the bit): the assertion here.  So the
reference alone stays inside every bound the GPU tests use."""
import numpy as np
import pytest

from tests import translation_ref as T

DIMS = (1, 3, 8, 32)


@pytest.mark.parametrize("kind", T.OFFSETS)
@pytest.mark.parametrize("D", DIMS)
def test_shift_is_exact(D, kind):
    X, Z, _, _ = T.grid_case(301, 130, D, ard=True)
    c = T.offset_vector(kind, D)
    for A in (X, Z):
        assert A.dtype == np.float32 and np.abs(A).max() <= T.LIMIT
        As = T.shift(A, c)                      # asserts exactness itself
        assert As.dtype == np.float32
        assert np.array_equal((As - c).astype(np.float32), A)
        # every difference of two shifted coordinates is the unshifted difference, in float32
        d0 = A[:, None, :] - Z[None, :7, :]
        d1 = As[:, None, :] - T.shift(Z, c)[None, :7, :]
        assert d0.dtype == np.float32 and np.array_equal(d0, d1)
    if kind == "mixed":
        assert c[0] == 1024.0 and (D < 2 or c[1] == -4096.0) and (D < 3 or c[2] == 0.5)


def test_shift_refuses_inexact_input():
    X = np.array([[0.1]], np.float32)           # not on the grid
    with pytest.raises(AssertionError):
        T.shift(X, np.array([4096.0]))


@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("D", DIMS)
def test_float64_reference_is_translation_invariant(D, ard):
    X, Z, var, ls = T.grid_case(301, 130, D, ard)
    k0 = T.rbf_K_ref(Z, X, var, ls)
    u0 = T.rbf_Kuu_ref(Z, var, ls, 1e-6)
    for kind in T.OFFSETS:
        c = T.offset_vector(kind, D)
        k1 = T.rbf_K_ref(T.shift(Z, c), T.shift(X, c), var, ls)
        u1 = T.rbf_Kuu_ref(T.shift(Z, c), var, ls, 1e-6)
        ek, eu = np.abs(k1 - k0).max() / var, np.abs(u1 - u0).max() / var
        raw = np.abs(T.rbf_K_ref(T.shift(Z, c), T.shift(X, c), var, ls, centred=False) - k0).max() / var
        print(f"D {D} ard {ard} {kind}: Kuf {ek:.2e} Kuu {eu:.2e}; the oracle on the raw shifted inputs {raw:.2e} "
              "(relative to the variance)")
        assert ek <= 1e-9 and eu <= 1e-9
        assert raw <= 1e-7


def test_model_problem_snaps_and_shifts():
    """The model-level case: snapped synthetic problem, X and both layers' Z moved by the mixed
    offset, everything else shared."""
    X, Y, p = T.snapped_problem(1000, 64, 3, 2, 0.7, S=3)
    c = T.offset_vector("mixed", 2)
    ps = T.shifted_params(p, c)
    Xs = T.shift(X, c)
    assert Xs.dtype == np.float32
    for L, Ls in ((p.pred, ps.pred), (p.assign, ps.assign)):
        assert np.array_equal(Ls["Z"] - c, L["Z"].astype(np.float64))
        assert Ls["q_mu"] is L["q_mu"] and Ls["q_sqrt"] is L["q_sqrt"]
    k0 = T.rbf_K_ref(p.pred["Z"], X, 0.5, 0.7)
    k1 = T.rbf_K_ref(ps.pred["Z"], Xs, 0.5, 0.7)
    assert np.abs(k1 - k0).max() <= 1e-9 * 0.5


def test_kuf_reference_point_moves_with_the_data():
    """The point the image bound is centred on is Z[0] plus a mean of differences: it moves by
    exactly c on a grid-exact case."""
    _, Z, _, _ = T.grid_case(301, 130, 3, False)
    c = T.offset_vector("mixed", 3)
    assert np.array_equal(T.kuf_reference_point(T.shift(Z, c)), T.kuf_reference_point(Z) + c)
