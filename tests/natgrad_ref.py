"""Float64 restatement of the natural-gradient step on (q_mu, q_sqrt) of a whitened SVGP
layer (mgp_natgrad_step, csrc/natgrad.hip; gpflow.optimizers.NaturalGradient with
XiSqrtMeanVar), by the DIRECT route -- deliberately not the closed form the kernel uses:

    theta = (S^-1 mu, -S^-1 / 2),  eta = (mu, S + mu mu^T),  S = L L^T   (explicit inverses)
    d loss / d eta_2 = Sbar = L^-T (P + P^T) L^-1 / 2,  P = Phi(L^T g_L)
    d loss / d eta_1 = g_mu - 2 Sbar mu
    theta' = theta - step d loss / d eta
    S' = (-2 theta_2')^-1,  mu' = S' theta_1',  L' = chol(S') with column j carrying sign(L_jj)

The step does not exist where -2 theta_2' is not positive definite (ok[k] = False).
Also the shared input draws of tests/test_natgrad_host.py and tests/test_gpu_natgrad.py."""
import numpy as np

SHAPES_M = (1, 25, 64, 70, 130)
SHAPES_K = (1, 3, 9)
STEPS = (0.1, 1.0, 1000.0)
KINDS = ("plain", "negdiag", "illcond")


def f32(a):
    """Round to float32, keep float64 storage (what the device holds)."""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def phi(A):
    """Lower triangle with the diagonal halved."""
    return np.tril(A, -1) + 0.5 * np.diag(np.diag(A))


def is_pd(A):
    try:
        np.linalg.cholesky(0.5 * (A + A.T))
        return True
    except np.linalg.LinAlgError:
        return False


def step_direct(q_mu, q_sqrt, g_mu, g_sqrt, step):
    """q_mu, g_mu [M, K]; q_sqrt, g_sqrt [K, M, M] (gradients of the loss being minimised).
    Returns mu' [M, K], L' [K, M, M], ok [K]; a failed expert keeps its input."""
    q_mu, q_sqrt = np.asarray(q_mu, np.float64), np.asarray(q_sqrt, np.float64)
    g_mu, g_sqrt = np.asarray(g_mu, np.float64), np.asarray(g_sqrt, np.float64)
    M, K = q_mu.shape
    mu_new, L_new, ok = q_mu.copy(), np.tril(q_sqrt).copy(), np.ones(K, bool)
    for k in range(K):
        L, mu = np.tril(q_sqrt[k]), q_mu[:, k]
        Linv = np.linalg.inv(L)
        Sinv = Linv.T @ Linv
        P = phi(L.T @ np.tril(g_sqrt[k]))
        Sbar = 0.5 * Linv.T @ (P + P.T) @ Linv
        th1, th2 = Sinv @ mu, -0.5 * Sinv
        th1n = th1 - step * (g_mu[:, k] - 2.0 * Sbar @ mu)
        th2n = th2 - step * Sbar
        prec = -2.0 * th2n
        if not is_pd(prec):
            ok[k] = False
            continue
        Sn = np.linalg.inv(prec)
        Sn = 0.5 * (Sn + Sn.T)
        sgn = np.where(np.diag(L) < 0, -1.0, 1.0)
        L_new[k] = np.linalg.cholesky(Sn) * sgn[None, :]
        mu_new[:, k] = Sn @ th1n
    return mu_new, L_new, ok


def min_eig_B(q_sqrt_k, g_sqrt_k, step):
    """Smallest eigenvalue of B = I + step (P + P^T) of one expert."""
    L = np.tril(q_sqrt_k)
    P = phi(L.T @ np.tril(g_sqrt_k))
    return float(np.linalg.eigvalsh(np.eye(L.shape[0]) + step * (P + P.T)).min())


def draw_case(M, K, step, kind, seed=0):
    """Random float32-rounded inputs (q_mu, q_sqrt, g_mu, g_sqrt; loss gradients) for which
    the step exists for every expert: g_L = tril(2 g_S L) with g_S a positive semi-definite
    part plus a smaller indefinite one, scaled down per expert until
    step * lambda_min(P + P^T) >= -0.5 (so lambda_min(B) >= 0.5 before the float32 rounding)."""
    rng = np.random.default_rng([seed, M, K, int(step * 10), KINDS.index(kind)])
    q_mu = 0.5 * rng.standard_normal((M, K))
    g_mu = rng.standard_normal((M, K))
    q_sqrt = np.zeros((K, M, M))
    g_sqrt = np.zeros((K, M, M))
    for k in range(K):
        if kind == "illcond":     # diag(L) log-uniform in [1e-3, 1]: unit lower T times diag(d)
            d = 10.0 ** rng.uniform(-3.0, 0.0, M)
            L = (np.eye(M) + np.tril(0.2 * rng.standard_normal((M, M)), -1)) * d[None, :]
        else:
            L = 0.5 * np.eye(M) + np.tril(0.1 * rng.standard_normal((M, M)))
            if kind == "negdiag":  # every other column (at least one) with a negative diagonal
                sgn = np.where(rng.uniform(size=M) < 0.5, -1.0, 1.0)
                sgn[0] = -1.0
                L = L * sgn[None, :]
        L = f32(L)
        G = rng.standard_normal((M, M + 5)) / np.sqrt(M + 5)
        R = rng.standard_normal((M, M)) / np.sqrt(M)
        g_S = G @ G.T + 0.05 * (R + R.T)
        gL = np.tril(2.0 * g_S @ L)
        P = phi(L.T @ gL)
        lam = float(np.linalg.eigvalsh(P + P.T).min())
        if step * lam < -0.5:
            gL *= 0.5 / (step * -lam)
        q_sqrt[k], g_sqrt[k] = L, f32(gL)
    return f32(q_mu), q_sqrt, f32(g_mu), g_sqrt


def conjugate_case(M=70, N=200, seed=11):
    """A conjugate Gaussian model in whitened form, f = A^T v with v ~ N(0, I), y = f + noise:
    loss(mu, S) = KL(N(mu, S) || N(0, I)) - E_q log N(y | A^T v, sigma2), whose gradients at
    a perturbed start (mu, L) are
        g_mu = mu - A (y - A^T mu) / sigma2,   g_S = I/2 - S^-1/2 + A A^T / (2 sigma2),
        g_L = tril(2 g_S L),
    and whose optimum, reached by ONE natural-gradient step at step = 1 from any start, is
    S* = (I + A A^T / sigma2)^-1, mu* = S* A y / sigma2.  Returns a dict; g_mu / g_L are the
    float64 gradients rounded to float32 (what the device is given)."""
    rng = np.random.default_rng(seed)
    A = f32(rng.standard_normal((M, N)) / np.sqrt(M))
    y = f32(rng.standard_normal(N))
    sigma2 = float(f32(0.3))
    mu = f32(0.5 * rng.standard_normal(M))
    L = f32(0.5 * np.eye(M) + np.tril(0.1 * rng.standard_normal((M, M))))
    S = L @ L.T
    g_mu = mu - A @ (y - A.T @ mu) / sigma2
    g_S = 0.5 * np.eye(M) - 0.5 * np.linalg.inv(S) + 0.5 * A @ A.T / sigma2
    g_L = np.tril(2.0 * g_S @ L)
    S_star = np.linalg.inv(np.eye(M) + A @ A.T / sigma2)
    S_star = 0.5 * (S_star + S_star.T)
    mu_star = S_star @ A @ y / sigma2
    return dict(A=A, y=y, sigma2=sigma2, mu=mu, L=L, g_mu=f32(g_mu), g_L=f32(g_L), g_mu64=g_mu, g_L64=g_L,
                S_star=S_star, mu_star=mu_star)


def normwise(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)
