"""Float64 statement of the greedy conditional-variance selection (csrc/greedy.hip,
modulatedgps_amd.inducing), an emulation of the device's number formats, and the inputs of
tests/test_greedy_host.py and tests/test_gpu_greedy.py.

    d[n] = variance
    step i:  j = argmax_n d[n] (ties: the lowest n);  stop if d[j] <= threshold * variance
             c[n] = k(x_n, x_j) - sum_{t < i} L[t][n] L[t][j];  L[i][n] = c[n] / sqrt(d[j])
             d[n] = max(d[n] - L[i][n]^2, 0);  dmax[i] = d[j] before,  trace[i] = sum d after

`greedy` runs it in float64 (factor_dtype = float64: the reference) or with the factor
rounded to float32 on storage and float64 everywhere else (the device scheme).  Kernel
hyper-parameters are the float32 values the device holds, inputs are float32.
"""
import functools
from dataclasses import dataclass

import numpy as np


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def hyper(variance, lengthscales):
    """The float32-rounded hyper-parameters as float64: what the device kernel reads."""
    return float(np.float32(variance)), f32(np.atleast_1d(lengthscales)).astype(np.float64)


def kernel_column(X, j, variance, ls):
    """K[:, j] of the SquaredExponential kernel in float64 from float32 inputs."""
    X = X.astype(np.float64)
    s = (X - X[j]) / ls
    return variance * np.exp(-0.5 * (s * s).sum(axis=1))


def kernel_matrix(A, B, variance, ls):
    A, B = A.astype(np.float64) / ls, B.astype(np.float64) / ls
    d2 = ((A[:, None, :] - B[None, :, :]) ** 2).sum(axis=2)
    return variance * np.exp(-0.5 * d2)


@dataclass
class Selection:
    indices: np.ndarray    # int64 [m]
    dmax: np.ndarray       # [m] d[j] when j was chosen
    trace: np.ndarray      # [m] sum d after each step
    residual: np.ndarray   # [N] d at the end
    factor: np.ndarray     # [m, N]
    stopped: bool
    top: np.ndarray        # [m] max_n d[n] before each step (= dmax unless a path was forced)
    d_steps: list          # d after each step (keep_d) or []


def greedy(X, M, variance, lengthscales, threshold=1e-4, factor_dtype=np.float64, path=None, keep_d=False,
           blas=False):
    """The loop above.  path: follow these indices instead of the argmax (and never stop):
    the reference recomputed along another selection's pivots.  blas: the dot product as one
    float64 matrix-vector product (for thousands of steps; the order of its sum is BLAS's)."""
    X = f32(X).reshape(len(X), -1)
    var, ls = hyper(variance, lengthscales)
    N = X.shape[0]
    steps = M if path is None else len(path)
    d = np.full(N, var, np.float64)
    L = np.zeros((steps, N), np.float64)       # the stored (rounded) factor, as float64
    piv, dmax, trace, top, ds = [], [], [], [], []
    stopped = False
    for i in range(steps):
        jmax = int(np.argmax(d))               # the first maximum: ties to the lowest n
        j = jmax if path is None else int(path[i])
        if path is None and d[j] <= threshold * var:
            stopped = True
            break
        piv.append(j), dmax.append(d[j]), top.append(d[jmax])
        c = kernel_column(X, j, var, ls)
        if blas:
            c = c - L[:i, j] @ L[:i]
        else:
            for t in range(i):                 # sequentially in t, as the device's float64 dot
                c = c - L[t] * L[t, j]
        L[i] = (c / np.sqrt(d[j])).astype(factor_dtype)    # rounded to factor_dtype on storage
        d = np.maximum(d - L[i] * L[i], 0.0)
        trace.append(d.sum())
        if keep_d:
            ds.append(d.copy())
    m = len(piv)
    return Selection(np.asarray(piv, np.int64), np.asarray(dmax), np.asarray(trace), d, L[:m].astype(factor_dtype),
                     stopped, np.asarray(top), ds)


def reference(X, M, variance, lengthscales, threshold=1e-4, **kw):
    return greedy(X, M, variance, lengthscales, threshold, np.float64, **kw)


def emulation(X, M, variance, lengthscales, threshold=1e-4, **kw):
    """The device scheme: float64 kernel values, dot, d; the factor rounded to float32."""
    return greedy(X, M, variance, lengthscales, threshold, np.float32, **kw)


def suboptimality(sel):
    """(max_n d[n] - d[p_i]) / max_n d[n] per step of a selection made along a forced path."""
    return (sel.top - sel.dmax) / sel.top


# ------------------------------------------------------------------ inputs
@dataclass(frozen=True)
class Case:
    name: str
    N: int
    D: int
    M: int
    variance: float
    lengthscales: tuple
    m: int                 # points the float64 reference chooses at threshold 1e-4
    stopped: bool
    repeat: int = 1        # every row this many times in a row

    def X(self):
        return case_inputs()[self.name]

    def args(self):
        return self.X(), self.M, self.variance, np.asarray(self.lengthscales)


# the exact-sequence cases (threshold 1e-4), uniform in [-1, 1]^D.
#   tie         after the first pivot (row 0: all d are equal) 66 rows in all six 256-row tiles
#               still have d == variance exactly, so the second pivot is a true tie that the
#               lowest index decides across workgroups
#   stops       the threshold ends it at 17 of 32
#   ard32       the top of the D range, ARD lengthscales 2 .. 6
#   f64kernel   M = N, ends at 115; with float32 kernel values the sequence leaves the float64 one
#   duplicates  300 rows, each twice in a row: no pair of equal rows may both be chosen
CASES = (
    Case("tie", 1500, 2, 128, 1.0, (0.3,), m=128, stopped=False),
    Case("stops", 777, 1, 32, 0.5, (0.2,), m=17, stopped=True),
    Case("ard32", 1024, 32, 96, 1.7, tuple(np.linspace(2.0, 6.0, 32)), m=96, stopped=False),
    Case("f64kernel", 257, 3, 257, 1.0, (0.8,), m=115, stopped=True),
    Case("duplicates", 600, 2, 64, 1.0, (0.3,), m=64, stopped=False, repeat=2),
)


@functools.lru_cache(maxsize=None)
def case_inputs():
    """The five inputs, drawn in order from one generator."""
    rng = np.random.default_rng(7)
    out = {}
    for c in CASES:
        X = f32(rng.uniform(-1.0, 1.0, size=(c.N, c.D)))
        out[c.name] = np.repeat(X[:c.N // c.repeat], c.repeat, axis=0) if c.repeat > 1 else X
    return out


# sizes around a wave (64) and a workgroup tile (256), M = min(N, 8); and a smooth 1-D input on
# which M = N ends early
EDGE_SIZES = (1, 63, 64, 65, 255, 257)
EDGE_KERNEL = (1.3, (0.5,))
SMOOTH_N = 300


@functools.lru_cache(maxsize=None)
def edge_input(N):
    return f32(np.random.default_rng(1000 + N).uniform(-1.0, 1.0, size=(N, 2)))


@functools.lru_cache(maxsize=None)
def smooth_input():
    return f32(np.sort(np.random.default_rng(99).uniform(-1.0, 1.0, size=SMOOTH_N)))


# the two other paths of the step kernel: more 256-row tiles than workgroups (1024), so that a
# workgroup sweeps two tiles; and more steps than one LDS chunk of the pivot row (1024).  On
# the first the rows are so dense that neighbours tie to 1e-9 and no exact sequence exists:
# both are checked along the device's own pivots.  (name, N, D, M, variance, lengthscales, seed)
PATH_CASES = (("two_tiles", 1024 * 256 + 257, 1, 6, 1.0, (0.3,), 22),
              ("two_chunks", 1280, 2, 1100, 1.0, (0.04,), 21))


@functools.lru_cache(maxsize=None)
def path_case(name):
    """-> (X, M, variance, lengthscales) of a PATH_CASES entry."""
    _, N, D, M, variance, ls, seed = {c[0]: c for c in PATH_CASES}[name]
    return f32(np.random.default_rng(seed).uniform(-1.0, 1.0, size=(N, D))), M, variance, np.asarray(ls)


def along(X, indices, variance, lengthscales, **kw):
    """The float64 reference recomputed along given pivots."""
    return reference(X, len(indices), variance, lengthscales, path=indices, blas=len(indices) > 300, **kw)


@functools.lru_cache(maxsize=None)
def path_case_emulation_error(name):
    """The emulation on a PATH_CASES input against the reference along its pivots ->
    (max |d - d_ref| / variance over the steps, worst shortfall / variance, m)."""
    X, M, variance, ls = path_case(name)
    e = emulation(X, M, variance, ls, keep_d=True, blas=M > 300)
    r = along(X, e.indices, variance, ls, keep_d=True)
    var = hyper(variance, 1.0)[0]
    err = max(float(np.abs(a - b).max()) for a, b in zip(e.d_steps, r.d_steps)) / var
    return err, float((r.top - r.dmax).max()) / var, len(e.indices)


LOW_THRESHOLD = 1e-6       # test 4: below the default, on the first input
LOW_M = 200


@functools.lru_cache(maxsize=None)
def case_reference(name):
    c = {c.name: c for c in CASES}[name]
    return reference(*c.args(), keep_d=True)


@functools.lru_cache(maxsize=None)
def case_emulation(name):
    c = {c.name: c for c in CASES}[name]
    return emulation(*c.args(), keep_d=True)


@functools.lru_cache(maxsize=None)
def emulation_d_error():
    """max over the cases, steps and rows of |d_emulation - d_reference| / variance (both
    along their own, equal, pivot sequences)."""
    worst = 0.0
    for c in CASES:
        r, e = case_reference(c.name), case_emulation(c.name)
        var = hyper(c.variance, 1.0)[0]
        for dr, de in zip(r.d_steps, e.d_steps):
            worst = max(worst, float(np.abs(de - dr).max()) / var)
    return worst


def gate():
    """The GPU tests' bound on |d - d_ref| / variance: 4 x the emulation's worst value; the
    4 x covers the device's exp and fused multiply-adds differing from NumPy's."""
    return 4.0 * emulation_d_error()


@functools.lru_cache(maxsize=None)
def low_threshold_emulation():
    """The emulation at LOW_THRESHOLD on the first input and the float64 reference along its
    pivots -> (emulation, reference along it, worst relative suboptimality)."""
    c = CASES[0]
    X, _, var, ls = c.args()
    e = emulation(X, LOW_M, var, ls, LOW_THRESHOLD)
    r = reference(X, LOW_M, var, ls, path=e.indices)
    return e, r, float(suboptimality(r).max())
