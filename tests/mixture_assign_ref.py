"""Float64 statement of the data-association outputs and the modes of the mixture predictive
(DESIGN "Data association and modes"; include/mgp_hip.h, mgp_mixture_responsibilities /
mgp_mixture_modes) for p(y | x) = sum_k w_k N(y | mu_k, s_k^2), s_k^2 = var_f,k + lik_var_k.  The
reference project has no counterpart, so this file is the specification the tests hold the
kernels to.  Latents and weights are point-major [N, K] here.  Nothing of the package is imported.

    a_k = log w_k - log s_k - (Y - mu_k)^2 / (2 s_k^2)           (-inf for w_k <= 0)
    resp_k = exp(a_k - logsumexp_j a_j),  label = argmax_k a_k (ties: lowest k)
    entropy = logsumexp(a) - sum_k resp_k a_k (resp_k == 0 skipped),  usage_k = sum_n resp[n, k]
    modes: the distinct limits of hill-climbing p from the means mu_k with w_k > 0; limits within
           1e-3 min_k s_k are one mode, the denser one stands for it; decreasing density, ties in
           ascending y

Two independent routes to the modes: modes_climb (the climb of the header, run to a float64
fixed point) and modes_grid (sign changes of p' on a grid, refined by bisection).  climb_f32 runs
the climb in float32 arithmetic under the device's iteration bound.
"""
import functools

import numpy as np

MERGE_TOL = 1e-3
RELEVANT = 2.0 ** -10   # an expert counts at y with at least this fraction of the largest term
SQRT2PI = np.sqrt(2.0 * np.pi)


def _f64(*a):
    return [np.asarray(x, np.float64) for x in a]


def scales(var_f, lik_var):
    """s [N, K] = sqrt(var_f + lik_var)."""
    var_f, lik_var = _f64(var_f, lik_var)
    return np.sqrt(var_f + lik_var.reshape(1, -1))


def log_terms(mu_f, var_f, lik_var, w, Y):
    """a [N, K]; -inf where w <= 0."""
    mu_f, w = _f64(mu_f, w)
    s = scales(var_f, lik_var)
    t = (np.asarray(Y, np.float64).reshape(-1, 1) - mu_f) / s
    with np.errstate(divide="ignore"):
        return np.where(w > 0, np.log(np.where(w > 0, w, 1.0)) - np.log(s) - 0.5 * t * t, -np.inf)


def _lse(a):
    m = a.max(-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        return (m + np.log(np.exp(a - m).sum(-1, keepdims=True)))[:, 0]


def responsibilities(mu_f, var_f, lik_var, w, Y):
    """[N, K]; a row with no positive weight is NaN."""
    a = log_terms(mu_f, var_f, lik_var, w, Y)
    with np.errstate(invalid="ignore"):
        return np.exp(a - _lse(a)[:, None])


def labels(mu_f, var_f, lik_var, w, Y):
    """argmax_k a_k, the first maximum; -1 for a row with no positive weight."""
    a = log_terms(mu_f, var_f, lik_var, w, Y)
    return np.where(np.isfinite(a.max(-1)), a.argmax(-1), -1)


def label_gap(mu_f, var_f, lik_var, w, Y):
    """[N]: the gap between the two largest a_k (inf for K = 1)."""
    a = np.sort(log_terms(mu_f, var_f, lik_var, w, Y), -1)
    return a[:, -1] - a[:, -2] if a.shape[1] > 1 else np.full(a.shape[0], np.inf)


def entropy(mu_f, var_f, lik_var, w, Y):
    """[N], nats."""
    a = log_terms(mu_f, var_f, lik_var, w, Y)
    r = responsibilities(mu_f, var_f, lik_var, w, Y)
    with np.errstate(invalid="ignore"):
        return _lse(a) - np.where(r == 0, 0.0, r * np.where(np.isfinite(a), a, 0.0)).sum(-1)


def usage(mu_f, var_f, lik_var, w, Y):
    """[K] = sum_n resp[n, k]."""
    return responsibilities(mu_f, var_f, lik_var, w, Y).sum(0)


# --------------------------------------------------------------------------- density and p'
def _params(mu_f, var_f, lik_var, w, dtype=np.float64):
    """(log w - log s, mu, 1 / (2 s^2)) [N, K] in `dtype`, and min_k s_k [N] (float64)."""
    mu_f, w = _f64(mu_f, w)
    s = scales(var_f, lik_var)
    with np.errstate(divide="ignore"):
        lc = np.where(w > 0, np.log(np.where(w > 0, w, 1.0)) - np.log(s), -np.inf)
    return lc.astype(dtype), mu_f.astype(dtype), (0.5 / (s * s)).astype(dtype), s.min(-1)


def _sums(y, lc, mu, h):
    """y [T], parameters [T, K] -> (S0, A, G, H, mx, max 1 / s_k^2 over the experts that count at
    y) of the header's climb, in the inputs' dtype."""
    d = mu - y[:, None]
    c = lc - h * d * d
    mx = c.max(-1)
    u = np.exp(c - mx[:, None])
    i2 = h + h
    ui = u * i2
    return u.sum(-1), ui.sum(-1), (ui * d).sum(-1), (ui * (i2 * d * d - 1)).sum(-1), mx, np.where(u >= RELEVANT, i2, 0).max(-1)


def density(mu_f, var_f, lik_var, w, y):
    """p(y[n, j]) of point n, y [N, J] -> [N, J]."""
    lc, mu, h, _ = _params(mu_f, var_f, lik_var, w)
    y = np.asarray(y, np.float64)
    N, J = y.shape
    rep = lambda a: np.repeat(a, J, 0)
    S0, _, _, _, mx, _ = _sums(y.reshape(-1), rep(lc), rep(mu), rep(h))
    return (np.exp(mx) * S0 / SQRT2PI).reshape(N, J)


def dp(mu_f, var_f, lik_var, w, y):
    """p'(y[n, j]) of point n, y [N, J] -> [N, J]."""
    lc, mu, h, _ = _params(mu_f, var_f, lik_var, w)
    y = np.asarray(y, np.float64)
    N, J = y.shape
    rep = lambda a: np.repeat(a, J, 0)
    _, _, G, _, mx, _ = _sums(y.reshape(-1), rep(lc), rep(mu), rep(h))
    return (np.exp(mx) * G / SQRT2PI).reshape(N, J)


# --------------------------------------------------------------------------- the climb
def climb(mu_f, var_f, lik_var, w, dtype=np.float64, max_iter=1000, stop_tol=1e-14):
    """Hill-climbing from every mean with w > 0, all starts at once, in `dtype` arithmetic: uphill
    by the mean-shift step or by half the bandwidth of the narrowest expert that counts at y
    (a term of at least RELEVANT times the largest) where that is longer, by the Newton step on
    p' where p'' < 0 and it is shorter; the bisection point of the last iterates with p' > 0 and
    p' < 0 replaces an iterate outside them.  It stops at a step of at most stop_tol min_k s_k
    (or below the resolution of y).  -> (point index [T], limit [T] float64, converged [T])."""
    lc, mu, h, smin = _params(mu_f, var_f, lik_var, w, dtype)
    pidx, kidx = np.nonzero(np.isfinite(lc))
    T = pidx.size
    y = mu[pidx, kidx].copy()
    inf = dtype(np.inf)
    lo, hi = np.full(T, -inf, dtype), np.full(T, inf, dtype)
    tol = (stop_tol * smin[pidx]).astype(dtype)
    active = np.ones(T, bool)
    half = dtype(0.5)
    for _ in range(max_iter):
        ix = np.nonzero(active)[0]
        if ix.size == 0:
            break
        p = pidx[ix]
        with np.errstate(all="ignore"):
            S0, A, G, H, _, imax = _sums(y[ix], lc[p], mu[p], h[p])
            flat = ~((G > 0) | (G < 0))
            lo[ix] = np.where(G > 0, y[ix], lo[ix])
            hi[ix] = np.where(G < 0, y[ix], hi[ix])
            step = G / A
            cap = np.maximum(np.abs(step), half / np.sqrt(imax))
            newton = np.copysign(np.minimum(np.abs(-G / H), cap), G)
            step = np.where(H < 0, newton, np.copysign(cap, G))
            yn = y[ix] + step
            small = (np.abs(step) <= tol[ix]) | (yn == y[ix])
            l, u = lo[ix], hi[ix]
            mid = l + half * (u - l)
            bisect = np.isfinite(l) & np.isfinite(u) & ~small & ~((yn > l) & (yn < u))
            shut = bisect & ((mid == l) | (mid == u))
            yn = np.where(bisect, mid, yn)
            moved = ~(flat | shut)
            done = small | (np.abs(yn - y[ix]) <= tol[ix])
        y[ix] = np.where(moved, yn, y[ix])
        active[ix] = moved & ~done
    return pidx, y.astype(np.float64), ~active


def merge(y, dens, tol):
    """The merge rule on one point's limits -> (modes, densities), decreasing density with ties
    in ascending y; a limit within tol of a mode already taken is dropped."""
    order = np.lexsort((y, -dens))
    keep = []
    for i in order:
        if all(abs(y[i] - y[j]) > tol for j in keep):
            keep.append(i)
    return y[keep], dens[keep]


def _merge_all(mu_f, var_f, lik_var, w, pidx, y):
    """Per point: (modes, densities) of the limits y of the starts pidx, densities in float64."""
    lc, mu, h, smin = _params(mu_f, var_f, lik_var, w)
    S0, _, _, _, mx, _ = _sums(y, lc[pidx], mu[pidx], h[pidx])
    dens = np.exp(mx) * S0 / SQRT2PI
    out = []
    bounds = np.searchsorted(pidx, np.arange(lc.shape[0] + 1))
    for n in range(lc.shape[0]):
        sl = slice(bounds[n], bounds[n + 1])
        out.append(merge(y[sl], dens[sl], MERGE_TOL * smin[n]))
    return out


def modes_climb(mu_f, var_f, lik_var, w):
    """Per point (modes, densities): the climb run to a float64 fixed point, then the merge rule.
    Raises if a start has not converged."""
    pidx, y, ok = climb(mu_f, var_f, lik_var, w)
    if not ok.all():
        raise RuntimeError(f"{(~ok).sum()} starts did not reach a fixed point")
    return _merge_all(mu_f, var_f, lik_var, w, pidx, y)


def climb_f32(mu_f, var_f, lik_var, w, max_iter=100, stop_tol=1e-9):
    """The climb in float32 arithmetic under the device's bound of 100 evaluations per start and
    its stopping step, then the merge rule (densities in float64 at the float32 limits)."""
    pidx, y, _ = climb(mu_f, var_f, lik_var, w, dtype=np.float32, max_iter=max_iter, stop_tol=stop_tol)
    return _merge_all(mu_f, var_f, lik_var, w, pidx, y)


# --------------------------------------------------------------------------- the grid
GRID_HALF_WIDTH, GRID_PER_EXPERT = 6.0, 193


def modes_grid(mu_f, var_f, lik_var, w):
    """Per point (modes, densities): the + to - sign changes of p' over [min mu, max mu] (means
    with w > 0; outside it p' has one sign) on the union of the experts' own grids mu_k + s_k
    linspace(-6, 6, 193), each refined by bisection to adjacent float64 numbers.  Decreasing
    density, ties in ascending y."""
    lc, mu, h, _ = _params(mu_f, var_f, lik_var, w)
    s = scales(var_f, lik_var)
    N = lc.shape[0]
    u = np.linspace(-GRID_HALF_WIDTH, GRID_HALF_WIDTH, GRID_PER_EXPERT)
    bp, bl, bh = [], [], []       # brackets: point, lower end (p' > 0), upper end (p' < 0)
    exact = [[] for _ in range(N)]
    for n in range(N):
        on = np.isfinite(lc[n])
        if not on.any():
            continue
        a, b = mu[n, on].min(), mu[n, on].max()
        nodes = np.unique(np.clip((mu[n, on, None] + s[n, on, None] * u[None]).reshape(-1), a, b))
        rep = lambda x: np.broadcast_to(x[n], (nodes.size, x.shape[1]))
        g = _sums(nodes, rep(lc), rep(mu), rep(h))[2]
        for i in np.nonzero(g == 0)[0]:
            if (i == 0 or g[i - 1] > 0) and (i == nodes.size - 1 or g[i + 1] < 0):
                exact[n].append(nodes[i])
        for i in np.nonzero((g[:-1] > 0) & (g[1:] < 0))[0]:
            bp.append(n), bl.append(nodes[i]), bh.append(nodes[i + 1])
    bp, bl, bh = np.asarray(bp, int), np.asarray(bl, np.float64), np.asarray(bh, np.float64)
    for _ in range(200):
        mid = bl + 0.5 * (bh - bl)
        if not ((mid > bl) & (mid < bh)).any():
            break
        g = _sums(mid, lc[bp], mu[bp], h[bp])[2]
        inside = (mid > bl) & (mid < bh)
        bl = np.where(inside & (g > 0), mid, bl)
        bh = np.where(inside & (g <= 0), mid, bh)
    roots = np.where(np.abs(_sums(bl, lc[bp], mu[bp], h[bp])[2]) <= np.abs(_sums(bh, lc[bp], mu[bp], h[bp])[2]), bl, bh)
    out = []
    for n in range(N):
        y = np.asarray(list(roots[bp == n]) + exact[n], np.float64)
        rep = lambda x: np.broadcast_to(x[n], (y.size, x.shape[1]))
        S0, _, _, _, mx, _ = _sums(y, rep(lc), rep(mu), rep(h))
        dens = np.exp(mx) * S0 / SQRT2PI
        order = np.lexsort((y, -dens))
        out.append((y[order], dens[order]))
    return out


# --------------------------------------------------------------------------- cases
N_CASE = 1000
KS = (1, 2, 3, 8, 32)
# chosen so that the conditions of test_mixture_assign_host hold: SEEDS draws the mixtures, Y_SEEDS the targets
SEEDS = {1: 1, 2: 2, 3: 3, 8: 106, 32: 252}
Y_SEEDS = {1: 1, 2: 1, 3: 1, 8: 1, 32: 17}


@functools.lru_cache(maxsize=None)
def case(K, N=N_CASE):
    """Float32 inputs, point-major [N, K]: mu ~ N(0, 2^2), log s ~ N(-1, 0.7^2), Dirichlet(1)
    weights, Y = mu_k + t s_k of a random expert with t ~ U(-12, 12)."""
    rng = np.random.default_rng(SEEDS[K])
    f32 = lambda a: np.asarray(a, np.float32)
    s = np.exp(rng.normal(-1.0, 0.7, (N, K)))
    lik_var = f32(rng.uniform(0.2, 0.6, K) * (s * s).min(0))
    d = dict(mu_f=f32(rng.normal(0.0, 2.0, (N, K))), lik_var=lik_var,
             var_f=f32(s * s - lik_var[None].astype(np.float64)), w=f32(rng.dirichlet(np.ones(K), N)))
    rng = np.random.default_rng(Y_SEEDS[K])
    k = rng.integers(0, K, N)
    s32 = scales(d["var_f"], lik_var)
    rows = np.arange(N)
    d["Y"] = f32(d["mu_f"][rows, k] + rng.uniform(-12, 12, N) * s32[rows, k])
    return d


@functools.lru_cache(maxsize=None)
def far_case(K, N=200):
    """The first N rows of case(K) with Y 25.01 sigma (25 after the rounding to float32) beyond
    every expert: above all of them at even rows, below at odd ones."""
    d = {key: (val[:N] if key != "lik_var" else val) for key, val in case(K).items()}
    s = scales(d["var_f"], d["lik_var"])
    mu = d["mu_f"].astype(np.float64)
    up, down = (mu + 25.01 * s).max(-1), (mu - 25.01 * s).min(-1)
    d["Y"] = np.where(np.arange(N) % 2 == 0, up, down).astype(np.float32)
    return d


@functools.lru_cache(maxsize=None)
def case_climb(K):
    """modes_climb of case(K): a list of (modes, densities) per point."""
    d = case(K)
    return modes_climb(d["mu_f"], d["var_f"], d["lik_var"], d["w"])


@functools.lru_cache(maxsize=None)
def case_modes(K):
    """(climb, grid, float32 climb) of case(K), each a list of (modes, densities) per point."""
    d = case(K)
    args = (d["mu_f"], d["var_f"], d["lik_var"], d["w"])
    return case_climb(K), modes_grid(*args), climb_f32(*args)


# The worst f32_position_error over KS, measured on the CPU (K = 32; 1.7e-6, 2.7e-6 and 5.3e-6 at
# K = 2, 3, 8): the source of the position gate of tests/test_gpu_mixture_assign.py, which is
# four times this.  test_mixture_assign_host.py measures it again.
F32_POSITION_ERROR = 8.22e-6


def f32_position_error(K):
    """The worst |y32 - y64| / min_k s_k over the points of case(K) whose float32 climb finds the
    reference's number of modes (the host test asserts that all do), modes paired by position."""
    d = case(K)
    smin = scales(d["var_f"], d["lik_var"]).min(-1)
    ref, _, emu = case_modes(K)
    worst = 0.0
    for n, ((y64, _), (y32, _)) in enumerate(zip(ref, emu)):
        if y64.size == y32.size:
            worst = max(worst, float(np.abs(np.sort(y32) - np.sort(y64)).max() / smin[n]))
    return worst
