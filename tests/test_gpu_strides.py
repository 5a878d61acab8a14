"""Every core-chain entry with each operand on its own leading dimension and stride, over
storage whose padding is poisoned.

ops.padded always allocates ld = round4(cols), so in the other tests every N-wide leading
dimension of a call is one number (lda = ldk = ldg = lds = ldf), every M-wide one another
(ldl = ldli = ldgl = ldqs = ldgs = ldo), every K-wide one a third (ldq = ldgq), and each
batch stride is rows x ld: an entry that indexes one operand with another's ld, or derives
a stride as M x ld, passes them all.  The production buffers come from torch.empty, so
their padding columns hold whatever was there before; the other tests mostly see zeros.

Here (tests/helpers.py wide / padding_intact) every operand of a call is a view over
storage of its own row length -- round4(cols) + 4, + 8, + 12, ... within a family (N-, M-
or K-wide), in the order the operands are made -- and batch entries sit rows x ld + 8 apart.
All of these stay multiples of 4 floats on 16-byte aligned bases, so the same kernels run
as in the tight call.  Input padding (and the gaps between batch entries) holds NaN in one
run and +-3e38 in the other (a bound or absmax pass that reads padding then shows as lost
precision, not as NaN); output padding holds a NaN sentinel.  The strict upper triangle of
q_sqrt is poisoned too (band_part(q_sqrt, -1, 0): it is ignored).

Every entry must (a) give, bit for bit, what the same entry gives on tight ops.padded
buffers of the same values, with the output padding and batch gaps untouched, and (b) agree
with the float64 reference of its operation, evaluated at the same float32 inputs, at the
tolerance of its sibling test: Kuf / Kuu 2e-6 x variance elementwise; L, L^-1 normwise
max(1e-5, 10 sqrt(cond) 1.2e-7); A, stats, fmean, fvar normwise 1e-4 (test_gpu_kernels);
the data term 1e-4 relative / 1e-3 absolute and its gradients 1e-4 normwise
(test_gpu_range_edges); every backward block 1e-4 normwise, g_var 1e-5 relative
(test_gpu_backward); KL 1e-5 relative; grams 2e-6 (x6, f32) and 4e-6 (split-f16) normwise.

Alignment contract (include/mgp_hip.h; refusals in the style of test_gpu_range_edges._refused):
  checked, refused with MGP_ERR_ALIGN: ldk of mgp_rbf_kuf / _kuu; ldl, strideL of
    mgp_potrf_trtri; ldl, ldk, lda, lds of mgp_trsm_stats; lda, ldqs, strideq, lds of
    mgp_expert_conditional_f32; ldqs, strideq of mgp_gauss_kl_white and
    mgp_qsqrt_images_kl_f16_batch;
  checked, refused with the argument's own number: ldx (-2), sx (-3), ldy (-6), sw (-10) of
    mgp_gram_x6 / mgp_gram_f16, ldy (-5) of mgp_gram_f16_rows;
  not checked and not needed (element stores and loads), one odd case each here: lda of
    mgp_potrf_trtri (the header asked for lda % 4); lds, lda of the image K4 entries; lds,
    ldf of the image K5 entries; ldq of the conditional backward (odd ldq = 5 at K = 4: the
    scalar q_mu path of grad_a_prep_kernel at a full KMAX); ldx, ldy of mgp_gram where
    MJ <= 16 (the narrow path);
  not checked but needed, host check added: lda, ldk (and ldg, K > 1) of every
    mgp_conditional_backward_* entry (operands and weights of the grams over N: an odd
    value was refused only by an inner gram, under that gram's argument number, after g_Kuf
    had been written); ldx, ldy of mgp_gram's 128 x 128 tile path (float4 loads).
K6, its backward, mgp_chol_backward / _batch and mgp_kl_grad read and write by elements:
no leading dimension of theirs is constrained."""
import ctypes
import functools
import types

import numpy as np
import pytest
import scipy.linalg as sla
import torch

from oracle import cpu_ref as R
from oracle import grad_ref as GR
from tests.helpers import normwise, padding_intact, poison_like, round4, to_np, wide

pytestmark = pytest.mark.gpu

POISONS = ["nan", "big"]
SHAPES = [(301, 37, 3), (515, 130, 4), (301, 130, 5)]   # (N, M, K)
D = 2
LS = 0.2            # cond(Kuu + 1e-6 I) <= 2.4e4 at these shapes (float64)
ALIGN = 2           # MGP_ERR_ALIGN
NAN = float("nan")


def _r(a):
    """float64 array of the float32-rounded values (what the device sees)."""
    return np.asarray(a, np.float32).astype(np.float64)


def _t(x, dev):
    return torch.as_tensor(np.array(x, dtype=np.float32), device=dev)


# =========================================================================== layouts
class Lay:
    """The operands of one call.  Tight (poison None): ops.padded storage.  Wide: every
    operand on its own leading dimension -- round4(cols) + 4, + 8, ... per family, in the
    order the operands are made -- batch entries rows x ld + 8 apart, padding poisoned."""

    def __init__(self, device, poison=None, odd=()):
        self.dev, self.poison, self.count, self.outs, self.odd = device, poison, {}, [], set(odd)

    @property
    def is_wide(self):
        return self.poison is not None

    def ld(self, fam, cols, name=None):
        if not self.is_wide:
            return round4(cols)
        self.count[fam] = self.count.get(fam, 0) + 1
        return round4(cols) + 4 * self.count[fam] + (1 if name in self.odd else 0)

    def _make(self, v, fam, ld, poison, name):
        from modulatedgps_amd import ops
        v = np.asarray(v, np.float32)
        if v.ndim == 1:
            v = v[None]
        if ld is None:
            ld = self.ld(fam, v.shape[-1], name)
        if not self.is_wide:
            assert ld == round4(v.shape[-1])
            t = ops.padded(v.shape[-2], v.shape[-1], self.dev, batch=v.shape[0] if v.ndim == 3 else None)
            t.copy_(torch.as_tensor(v))
            return t
        bs = v.shape[-2] * ld + 8 if v.ndim == 3 else None
        return wide(v, ld, poison, self.dev, batch_stride=bs)

    def inp(self, v, fam, ld=None, upper=False, name=None):
        """An input.  upper: the strict upper triangle of each matrix is poisoned too (wide)."""
        t = self._make(v, fam, ld, self.poison, name)
        if upper and self.is_wide:
            mask = torch.triu(torch.ones(t.shape[-2:], dtype=torch.bool, device=self.dev), 1).expand(t.shape)
            t.copy_(torch.where(mask, poison_like(self.poison, tuple(t.shape), self.dev), t))
        return t

    def inout(self, v, fam, ld=None, name=None):
        """An operand updated in place: its padding must come back as it was."""
        t = self._make(v, fam, ld, self.poison, name)
        if self.is_wide:
            self.outs.append((t, self.poison))
        return t

    def out(self, shape, fam, ld=None, name=None):
        """An output, sentinel-filled; its padding (wide) holds the NaN sentinel as well."""
        t = self._make(np.zeros(shape, np.float32), fam, ld, "nan", name)
        t.fill_(NAN)
        if self.is_wide:
            self.outs.append((t, "nan"))
        return t


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.is_floating_point:
        a, b = a.view(torch.int32 if a.dtype == torch.float32 else torch.int64), b.view(
            torch.int32 if b.dtype == torch.float32 else torch.int64)
    return bool(torch.equal(a, b))


def both(device, poison, run, odd=(), bit_identical=True):
    """run(lay) -> {name: output tensor}, once on tight and once on wide operands: the same
    bits, the wide call's output padding and batch gaps untouched.  Returns the wide outputs."""
    tight = run(Lay(device))
    lay = Lay(device, poison, odd)
    got = run(lay)
    torch.cuda.synchronize()
    assert sorted(got) == sorted(tight)
    if bit_identical:
        for k in got:
            assert same_bits(got[k], tight[k]), k
    assert lay.outs
    for t, p in lay.outs:
        assert padding_intact(t, p)
    return got


def _zeros_u8(n, device):
    return torch.zeros(int(n), dtype=torch.uint8, device=device)   # split-f16 images never write plane 2


# =========================================================================== shared inputs
def _stats_ref(A, q_mu):
    M, K = q_mu.shape
    T = -(-M // 64)
    st = np.zeros((T, K + 1, A.shape[1]))
    for t in range(T):
        rows = slice(64 * t, min(64 * t + 64, M))
        st[t, 0] = np.sum(A[rows] ** 2, axis=0)
        st[t, 1:] = q_mu[rows].T @ A[rows]
    return st


@functools.lru_cache(maxsize=None)
def chain(N, M, K):
    """One layer's operands along the chain, float64 arrays of float32 values (read-only):
    each entry is tested from these inputs against the float64 formula of its operation
    at the same inputs."""
    X, _, p = R.synthetic_problem(N, M, K, D, LS, state="perturbed", S=2)
    L = p.pred
    c = types.SimpleNamespace(N=N, M=M, K=K, var=float(np.float32(L["variance"])), ls=float(np.float32(LS)))
    c.X, c.Z, c.q_mu, c.q_sqrt = _r(X), _r(L["Z"]), _r(L["q_mu"]), np.tril(_r(L["q_sqrt"]))
    Kuu = R.rbf_Kuu(c.Z, c.var, c.ls)
    c.cond = np.linalg.cond(Kuu)
    assert c.cond < 1e5, c.cond
    Lc = np.linalg.cholesky(Kuu)
    c.Kuu, c.L = Kuu, _r(Lc)
    c.LinvT = _r(sla.solve_triangular(Lc, np.eye(M), lower=True).T)
    c.Kuf = _r(R.rbf_K(c.Z, c.X, c.var, c.ls))
    c.A = _r(c.LinvT.T @ c.Kuf)
    c.stats = _r(_stats_ref(c.A, c.q_mu))
    rng = np.random.default_rng(N + M + K)
    c.Gmu, c.Gv = _r(rng.standard_normal((K, N))), _r(rng.standard_normal((K, N)))
    c.gL = np.tril(_r(rng.standard_normal((M, M))))
    c.gL2 = np.tril(_r(rng.standard_normal((M, M))))
    c.q_mu2 = _r(0.3 * rng.standard_normal((M, K)))
    c.q_sqrt2 = np.tril(_r(0.7 * np.eye(M)[None] + 0.05 * rng.standard_normal((K, M, M))))
    for a in vars(c).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def _k5_ref(A, stats, q_sqrt, var):
    fmean = stats[:, 1:].sum(0)
    LTA = np.einsum("kmi,mn->kin", np.tril(q_sqrt), A)
    return fmean, var - stats[:, 0].sum(0)[None] + (LTA ** 2).sum(1)


# =========================================================================== K1 / K2
@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("N,M,K", SHAPES[:2])
def test_rbf_kuf_kuu(device, N, M, K, poison):
    """mgp_rbf_kuf / mgp_rbf_kuu: X (ldx), Z (ldz) and the output (ldk) each on its own row
    length (X and Z: rows of 8 and 12 floats for D = 2)."""
    from modulatedgps_amd import ops
    from tests.test_gpu_range_edges import _rows_of
    c = chain(N, M, K)
    var, ls = _t([c.var], device), _t([c.ls], device)

    def run(lay):
        if lay.is_wide and poison == "nan":   # the NaN-padded rows of test_gpu_range_edges
            X, Z = _rows_of(c.X, lay.ld("D", D), device), _rows_of(c.Z, lay.ld("D", D), device)
        elif lay.is_wide:
            X, Z = lay.inp(c.X, "D"), lay.inp(c.Z, "D")
        else:
            X, Z = _t(c.X, device), _t(c.Z, device)
        Kuf = ops.rbf_kuf(X, Z, var, ls, out=lay.out((M, N), "N"))
        Kuu = ops.rbf_kuu(Z, var, ls, 1e-6, out=lay.out((M, M), "M"))
        return {"Kuf": Kuf, "Kuu": Kuu}

    got = both(device, poison, run)
    assert np.abs(to_np(got["Kuf"]) - R.rbf_K(c.Z, c.X, c.var, c.ls)).max() <= 2e-6 * c.var
    Kuu = to_np(got["Kuu"])
    assert np.abs(Kuu - c.Kuu).max() <= 2e-6 * c.var
    assert np.array_equal(Kuu, Kuu.T)


# =========================================================================== K3
@functools.lru_cache(maxsize=None)
def _spd(M):
    rng = np.random.default_rng(M)
    return tuple(_r(R.rbf_Kuu(rng.standard_normal((M, 4)), 1.0, 1.5) + 1e-3 * np.eye(M)) for _ in range(2))


def _check_factors(As, L, LinvT):
    M = As[0].shape[0]
    for b, A in enumerate(As):
        tol = max(1e-5, 10 * np.sqrt(np.linalg.cond(A)) * 1.2e-7)
        Lr = np.linalg.cholesky(A)
        Lg, Lt = to_np(L[b]), to_np(LinvT[b])
        assert not np.triu(Lg, 1).any() and not np.tril(Lt, -1).any()
        assert normwise(Lg, Lr) < tol
        assert normwise(Lt.T, sla.solve_triangular(Lr, np.eye(M), lower=True)) < tol


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("M", [37, 130])
@pytest.mark.parametrize("odd", [False, True], ids=["ld4", "odd_lda"])
def test_potrf_trtri(device, M, poison, odd):
    """mgp_potrf_trtri, batch 2: lda != ldl and strideA != strideL.  odd_lda: A is read by
    elements, so an odd lda (and strideA) is legal although ldl is not."""
    from modulatedgps_amd import ops
    As = _spd(M)

    def run(lay):
        if lay.is_wide and odd:
            lda = round4(M) + 5
            A = wide(np.stack(As), lda, poison, device, batch_stride=M * lda + 7)
        else:
            A = lay.inp(np.stack(As), "M")
        ldl = lay.ld("M", M)
        L, LinvT = lay.out((2, M, M), "M", ld=ldl), lay.out((2, M, M), "M", ld=ldl)
        info = torch.full((2,), -1, dtype=torch.int32, device=device)
        ops.potrf_trtri(A, L=L, LinvT=LinvT, info=info)
        if lay.is_wide:
            assert A.stride(1) != L.stride(1) and A.stride(0) != L.stride(0)
        return {"L": L, "LinvT": LinvT, "info": info}

    got = both(device, poison, run)
    assert (got["info"].cpu() == 0).all()
    _check_factors(As, got["L"], got["LinvT"])


# =========================================================================== K4
def _check_k4(c, A, stats, tag=""):
    A_ref = c.LinvT.T @ c.Kuf
    assert normwise(to_np(A), A_ref) < 1e-4, tag
    assert normwise(to_np(stats), _stats_ref(A_ref, c.q_mu)) < 1e-4, tag


def _stats_out(lay, c, name=None):
    from modulatedgps_amd import ops
    T = ops.stats_tiles(c.M)
    assert T == -(-c.M // 64)
    return lay.out((T * (c.K + 1), c.N), "N", name=name).unflatten(0, (T, c.K + 1))


def _stats_in(lay, c, ld=None):
    T = c.stats.shape[0]
    return lay.inp(c.stats.reshape(T * (c.K + 1), c.N), "N", ld=ld).unflatten(0, (T, c.K + 1))


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("N,M,K", SHAPES)
def test_trsm_stats_f32(device, N, M, K, poison):
    """mgp_trsm_stats: ldl (M-wide), ldk, lda, lds (N-wide) and ldq (K-wide) all differ."""
    from modulatedgps_amd import ops
    c = chain(N, M, K)

    def run(lay):
        LinvT, Kuf, q_mu = lay.inp(c.LinvT, "M"), lay.inp(c.Kuf, "N"), lay.inp(c.q_mu, "K")
        A, stats = ops.trsm_stats(LinvT, Kuf, q_mu, A=lay.out((M, N), "N"), stats=_stats_out(lay, c))
        return {"A": A, "stats": stats}

    got = both(device, poison, run)
    _check_k4(c, got["A"], got["stats"])


def _k4_images(ops, lay, c, fmt, device):
    """Tfr and Kfr from the (wide) LinvT and Kuf: the splits take a leading dimension too."""
    LinvT, Kuf = lay.inp(c.LinvT, "M"), lay.inp(c.Kuf, "N")
    Tfr = ops.split_upper_x6(LinvT, out=_zeros_u8(ops.x6_lower_bytes(c.M, 1), device), fmt=fmt)
    Kfr = ops.split_cols_x6(Kuf, out=_zeros_u8(ops.x6_cols_bytes(c.M, c.N), device), fmt=fmt)
    return Tfr, Kfr


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("N,M,K,odd", [s + (False,) for s in SHAPES] + [SHAPES[1] + (True,)])
@pytest.mark.parametrize("fmt", ["x6", "f16"])
def test_trsm_stats_images(device, N, M, K, odd, fmt, poison):
    """mgp_trsm_stats_x6 (x6) and mgp_trsm_stats_f16 (f16) with wide stats (lds), f32 A (lda)
    and q_mu (ldq); the operand images come from the wide LinvT and Kuf (mgp_split_upper_*,
    mgp_split_cols_*: ldl, lda).  odd: lds and lda odd -- the image K4 stores stats and A
    by elements (buffer stores of one dword), so the host does not ask for lds, lda % 4."""
    from modulatedgps_amd import ops
    c = chain(N, M, K)
    var = _t([c.var], device)

    def run(lay):
        Tfr, Kfr = _k4_images(ops, lay, c, fmt, device)
        q_mu = lay.inp(c.q_mu, "K")
        stats, A = _stats_out(lay, c, name="stats"), lay.out((M, N), "N", name="A")
        if lay.is_wide and odd:
            assert stats.stride(1) % 2 == 1 and A.stride(0) % 2 == 1
        Afr = _zeros_u8(ops.x6_cols_bytes(M, N), device)
        kw = dict(f16_variance=var, in_fmt="f16", cross="f16") if fmt == "f16" else {}
        ops.trsm_stats_x6(Tfr, Kfr, q_mu, M, N, Afr=Afr, stats=stats, A=A, **kw)
        return {"Tfr": Tfr, "Kfr": Kfr, "Afr": Afr, "stats": stats, "A": A}

    got = both(device, poison, run, odd=("stats", "A") if odd else ())
    _check_k4(c, got["A"], got["stats"], fmt)


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("N,M,K", SHAPES)
def test_trsm_stats_f16_batch(device, N, M, K, poison):
    """mgp_trsm_stats_f16_batch: two layers share ldq, lds and lda, each a different number."""
    from modulatedgps_amd import ops
    c = chain(N, M, K)
    var = [_t([c.var], device), _t([c.var], device)]
    q_mus = [c.q_mu, c.q_mu2]

    def run(lay):
        Tfr, Kfr = _k4_images(ops, lay, c, "f16", device)
        T = ops.stats_tiles(M)
        ldq, lds, lda = lay.ld("K", K), lay.ld("N", N), lay.ld("N", N)
        qs = [lay.inp(q, "K", ld=ldq) for q in q_mus]
        sts = [lay.out((T * (K + 1), N), "N", ld=lds).unflatten(0, (T, K + 1)) for _ in range(2)]
        As = [lay.out((M, N), "N", ld=lda) for _ in range(2)]
        Afrs = [_zeros_u8(ops.x6_cols_bytes(M, N), device) for _ in range(2)]
        ops.trsm_stats_f16_batch([Tfr, Tfr], [Kfr, Kfr], qs, M, N, Afrs, sts, var, As=As)
        return {"Afr0": Afrs[0], "Afr1": Afrs[1], "st0": sts[0], "st1": sts[1], "A0": As[0], "A1": As[1]}

    got = both(device, poison, run)
    _check_k4(c, got["A0"], got["st0"])
    A_ref = c.LinvT.T @ c.Kuf
    assert normwise(to_np(got["A1"]), A_ref) < 1e-4
    assert normwise(to_np(got["st1"]), _stats_ref(A_ref, c.q_mu2)) < 1e-4


# =========================================================================== K5
def _check_k5(c, fmean, fvar, tag=""):
    fm_ref, fv_ref = _k5_ref(c.A, c.stats, c.q_sqrt, c.var)
    assert normwise(to_np(fmean), fm_ref) < 1e-4, tag
    assert normwise(to_np(fvar), fv_ref) < 1e-4, tag


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("N,M,K", SHAPES)
def test_expert_conditional_f32(device, N, M, K, poison):
    """mgp_expert_conditional_f32: lda, lds, ldf (N-wide) and ldqs / strideq (M-wide) all
    differ; fmean and fvar share ldf (one argument of the C-ABI) on separate storage."""
    from modulatedgps_amd import ops
    c = chain(N, M, K)
    var = _t([c.var], device)

    def run(lay):
        A, q_sqrt, stats = lay.inp(c.A, "N"), lay.inp(c.q_sqrt, "M", upper=True), _stats_in(lay, c)
        ldf = lay.ld("N", N)
        fm, fv = ops.expert_conditional(A, q_sqrt, stats, var, fmean=lay.out((K, N), "N", ld=ldf),
                                        fvar=lay.out((K, N), "N", ld=ldf))
        return {"fmean": fm, "fvar": fv}

    got = both(device, poison, run)
    _check_k5(c, got["fmean"], got["fvar"])


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("N,M,K,odd", [s + (False,) for s in SHAPES] + [SHAPES[1] + (True,)])
@pytest.mark.parametrize("fmt", ["x6", "f16", "f16c"])
def test_expert_conditional_images(device, N, M, K, odd, fmt, poison):
    """mgp_expert_conditional_x6, _f16 and _f16c (c_out: the C_k images): wide stats (lds)
    and fmean / fvar (ldf, shared by the two as the C-ABI has it); the operand images come
    from the wide A (mgp_split_cols_*, lda) and the wide q_sqrt with a poisoned upper triangle
    (mgp_split_lower_*, mgp_colnorm_max: ldqs, strideq).  odd: lds and ldf odd -- K5's
    finalize reads the stats and writes fmean / fvar by elements."""
    from modulatedgps_amd import ops
    c = chain(N, M, K)
    var = _t([c.var], device)
    f = "x6" if fmt == "x6" else "f16"

    def run(lay):
        A, q_sqrt = lay.inp(c.A, "N"), lay.inp(c.q_sqrt, "M", upper=True)
        Afr = ops.split_cols_x6(A, out=_zeros_u8(ops.x6_cols_bytes(M, N), device), fmt=f)
        Lfr = ops.split_lower_x6(q_sqrt, out=_zeros_u8(ops.x6_lower_bytes(M, K), device), fmt=f)
        T = c.stats.shape[0]
        stats = lay.inp(c.stats.reshape(T * (K + 1), N), "N", name="stats").unflatten(0, (T, K + 1))
        ldf = lay.ld("N", N, name="f")
        fm, fv = lay.out((K, N), "N", ld=ldf), lay.out((K, N), "N", ld=ldf)
        if lay.is_wide and odd:
            assert stats.stride(1) % 2 == 1 and fm.stride(0) % 2 == 1
        out = {"Afr": Afr, "Lfr": Lfr, "fmean": fm, "fvar": fv}
        c_out = None
        if fmt == "f16c":
            c_out = (_zeros_u8(ops.c_images_bytes(M, N, K), device), ops.colnorm_max(q_sqrt))
            out["Cfr"], out["colmax"] = c_out
        ops.expert_conditional_x6(Afr, Lfr, stats, var, M, N, K, fmean=fm, fvar=fv, fmt=f, cross="f16", c_out=c_out)
        return out

    got = both(device, poison, run, odd=("stats", "f") if odd else ())
    _check_k5(c, got["fmean"], got["fvar"], fmt)
    if fmt == "f16c":
        ref = np.linalg.norm(np.tril(c.q_sqrt), axis=1).max()
        assert float(got["colmax"].cpu()) == pytest.approx(ref, rel=1e-6)


@pytest.mark.parametrize("train", [False, True], ids=["forward", "c_out"])
@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("N,M,K", SHAPES)
def test_expert_conditional_f16_batch(device, N, M, K, poison, train):
    """mgp_expert_conditional_f16_batch: two layers share lds and ldf."""
    from modulatedgps_amd import ops
    c = chain(N, M, K)
    var = [_t([c.var], device), _t([0.5 * c.var], device)]
    A_t = ops.as_padded(_t(c.A, device))
    Afr = ops.split_cols_x6(A_t, out=_zeros_u8(ops.x6_cols_bytes(M, N), device), fmt="f16")
    q_sqrts = [c.q_sqrt, c.q_sqrt2]

    def run(lay):
        qs = [lay.inp(q, "M", upper=True) for q in q_sqrts]
        Lfrs = [ops.split_lower_x6(q, out=_zeros_u8(ops.x6_lower_bytes(M, K), device), fmt="f16") for q in qs]
        lds, ldf = lay.ld("N", N), lay.ld("N", N)
        sts = [_stats_in(lay, c, ld=lds) for _ in range(2)]
        fms, fvs = [lay.out((K, N), "N", ld=ldf) for _ in range(2)], [lay.out((K, N), "N", ld=ldf) for _ in range(2)]
        wss = [torch.empty(ops.expert_x6_workspace_bytes(M, N, K), dtype=torch.uint8, device=device) for _ in range(2)]
        c_outs = [(_zeros_u8(ops.c_images_bytes(M, N, K), device), ops.colnorm_max(q)) for q in qs] if train else None
        ops.expert_conditional_f16_batch([Afr, Afr], Lfrs, sts, var, M, N, K, fms, fvs, wss, c_outs=c_outs)
        out = {"fm0": fms[0], "fv0": fvs[0], "fm1": fms[1], "fv1": fvs[1]}
        if train:
            out["C0"], out["C1"] = c_outs[0][0], c_outs[1][0]
        return out

    got = both(device, poison, run)
    _check_k5(c, got["fm0"], got["fv0"])
    fm_ref, fv_ref = _k5_ref(c.A, c.stats, c.q_sqrt2, 0.5 * c.var)
    assert normwise(to_np(got["fm1"]), fm_ref) < 1e-4 and normwise(to_np(got["fv1"]), fv_ref) < 1e-4


# =========================================================================== K6
K6_CASES = [(301, 3, "gauss"), (301, 3, "modified"), (301, 3, "multiclass"), (301, 3, "multiclass_modified"),
            (515, 4, "gauss"), (515, 4, "modified"), (301, 5, "gauss"), (301, 5, "modified")]


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("N,K,lik", K6_CASES)
def test_elbo_terms_and_backward(device, N, K, lik, poison):
    """mgp_elbo_terms / _modified / _multiclass and their backward entries with explicit
    noise: the four conditionals share ldf (the wrapper and the C-ABI demand it) on four
    separate storages, G has ldg != ldf."""
    from modulatedgps_amd import ops
    from tests.test_gpu_range_edges import EPS, _data_term_grads_f32, k6_case, k6_data_ref
    c = k6_case(N, K, 3)
    mc, mod = lik.startswith("multiclass"), lik.endswith("modified")
    Y = _t(c.Yc if mc else c.Y, device)
    lv = None if mc else _t(c.lv, device)
    kw = {}
    if mc:
        kw["multiclass_eps"] = EPS
    if mod:
        kw["assign_lik_var"] = _t(c.av, device)
    noise = (_t(c.z, device), _t(c.u, device))

    def run(lay):
        ldf = lay.ld("N", N)
        conds = [lay.inp(a.T, "N", ld=ldf) for a in (c.mu_f, c.var_f, c.mu_a, c.var_a)]
        val = ops.elbo_terms(*conds, Y, lv, c.S, noise=noise, out=torch.full((1,), NAN, dtype=torch.float64,
                                                                             device=device), **kw)
        G = lay.out((4 * K, N), "N").unflatten(0, (4, K))
        if lay.is_wide:
            assert G.stride(1) != conds[0].stride(0)
        G, glv, glva = ops.elbo_terms_backward(*conds, Y, lv, c.S, noise=noise, scale=1.0 / N, G=G, **kw)
        out = {"value": val, "G": G}
        if glv is not None:
            out["glv"] = glv
        if glva is not None:
            out["glva"] = glva
        return out

    got = both(device, poison, run)
    assert float(got["value"].cpu()) == pytest.approx(k6_data_ref(c, c.z, c.u, lik), rel=1e-4, abs=1e-3)
    leaves = [torch.tensor(np.array(a), requires_grad=True) for a in (c.mu_f, c.var_f, c.mu_a, c.var_a)]
    lv64 = None if mc else torch.tensor(np.array(c.lv), requires_grad=True)
    av64 = torch.tensor(np.array(c.av), requires_grad=True) if mod else None
    dt = GR.data_term(*leaves, torch.tensor(np.array(c.Yc if mc else c.Y)), lv64, torch.tensor(np.array(c.z)),
                      torch.tensor(np.array(c.u)), assign_lik_var=av64, multiclass_eps=EPS if mc else None)
    (dt / N).backward()
    scale_ref = np.linalg.norm(leaves[0].grad.numpy())
    for i, name in enumerate(("mu_f", "var_f", "mu_a", "var_a")):
        g, ref = to_np(got["G"][i]).T, leaves[i].grad.numpy()
        if np.linalg.norm(ref) < 1e-12 * scale_ref:   # MultiClass without the assignment term: roundoff
            assert mc and not mod, name                # (test_elbo_terms_backward_edges, the same bound)
            noise32 = np.linalg.norm(_data_term_grads_f32(c, lik)[i])
            assert np.linalg.norm(g) < max(1e-5 * scale_ref, 1.5 * noise32), name
        else:
            assert normwise(g, ref) < 1e-4, name
    for key, leaf in (("glv", lv64), ("glva", av64)):
        assert (key in got) == (leaf is not None)
        if leaf is not None:
            assert normwise(got[key].cpu().numpy(), leaf.grad.numpy()) < 1e-4, key


# =========================================================================== conditional backward
BWD_VARIANTS = ["x6", "f16", "f16c", "prep", "t_bound", "f16x8"]


@functools.lru_cache(maxsize=None)
def _bwd_forward(device, N, M, K, variant):
    """The forward of one layer on tight buffers, as test_conditional_backward(_c_images) runs
    it: A's image and the f32 A from K4, L^-T from K3, and for the C path the C_k images,
    colmax and the L_k image's bound from K5.  Opaque to the leading dimensions under test."""
    from modulatedgps_amd import ops
    c = chain(N, M, K)
    fmt = "x6" if variant == "x6" else "f16"
    cross = "f8" if variant == "f16x8" else "f16"
    Xt, Zt, var, ls = _t(c.X, device), _t(c.Z, device), _t([c.var], device), _t([c.ls], device)
    qmu, qs = _t(c.q_mu, device), ops.as_padded(_t(c.q_sqrt, device))
    _, LinvT, info = ops.kuu_potrf_trtri([Zt], [var], [ls], 1e-6)
    assert int(info.cpu()[0]) == 0
    Kfr = ops.rbf_kuf_x6(Xt, Zt, var, ls, fmt=fmt)
    Tfr = ops.split_upper_x6(LinvT[0], fmt=fmt)
    A = ops.padded(M, N, device)
    f = types.SimpleNamespace(fmt=fmt, cross=cross, c_images=None)
    if fmt == "x6":
        f.Afr, st = ops.trsm_stats_x6(Tfr, Kfr, qmu, M, N, A=A)
    else:
        f.Afr, st = ops.trsm_stats_x6(Tfr, Kfr, qmu, M, N, A=A, f16_variance=var, in_fmt="f16", cross=cross)
    if variant in ("f16c", "prep", "t_bound"):
        Lfr = ops.split_lower_x6(qs, fmt="f16")
        Cfr = torch.empty(ops.c_images_bytes(M, N, K), dtype=torch.uint8, device=device)
        colmax = ops.colnorm_max(qs)
        ops.expert_conditional_x6(f.Afr, Lfr, st, var, M, N, K, fmt="f16", cross="f16", c_out=(Cfr, colmax))
        f.c_images = (Cfr, colmax, ops.image_bound(Lfr, M, K=K).clone())
    f.A, f.LinvT = to_np(A), to_np(LinvT[0])
    f.t_bound = torch.triu(LinvT[0]).abs().max().reshape(1).contiguous()
    return f


def _bwd_reference(c, f):
    """float64 autograd at the device's own A and L^-1 (test_conditional_backward)."""
    A64 = torch.tensor(f.A, requires_grad=True)
    q_mu = torch.tensor(np.array(c.q_mu), requires_grad=True)
    q_sqrt = torch.tensor(np.array(c.q_sqrt), requires_grad=True)
    v = torch.tensor(c.var, dtype=torch.float64, requires_grad=True)
    fmean = (A64.T @ q_mu).T
    LTA = torch.tril(q_sqrt).transpose(1, 2) @ A64
    fvar = v - (A64 ** 2).sum(0)[None, :] + (LTA ** 2).sum(1)
    ((torch.tensor(np.array(c.Gmu)) * fmean).sum() + (torch.tensor(np.array(c.Gv)) * fvar).sum()).backward()
    gKuf = f.LinvT @ A64.grad.numpy()                      # Linv^T gA, Linv = LinvT^T
    return {"g_Kuf": gKuf, "g_Lm": -np.tril(gKuf @ f.A.T), "g_q_mu": q_mu.grad.numpy(),
            "g_q_sqrt": np.tril(q_sqrt.grad.numpy()), "g_var": float(v.grad)}


def _bwd_run(ops, c, f, variant, device, ldq=None):
    def run(lay):
        # N-wide: lda, ldg, ldk; M-wide: ldqs, ldl, ldgs, ldgl; K-wide: ldq, ldgq -- in this order
        A = lay.inp(f.A, "N")
        q_sqrt = lay.inp(c.q_sqrt, "M", upper=True)
        if lay.is_wide and ldq is not None:
            q_mu = wide(np.array(c.q_mu), ldq, lay.poison, device)
        else:
            q_mu = lay.inp(c.q_mu, "K")
        LinvT = lay.inp(f.LinvT, "M")
        G = lay.inp(np.concatenate([c.Gmu, c.Gv]), "N")
        out = {"g_q_mu": lay.out((c.M, c.K), "K"), "g_q_sqrt": lay.out((c.K, c.M, c.M), "M"),
               "g_Kuf": lay.out((c.M, c.N), "N"), "g_Lm": lay.out((c.M, c.M), "M"),
               "g_var": torch.full((1,), NAN, dtype=torch.float64, device=device)}
        if lay.is_wide:
            lds_ = [A.stride(0), q_sqrt.stride(1), q_mu.stride(0), LinvT.stride(0), G.stride(0),
                    out["g_q_mu"].stride(0), out["g_q_sqrt"].stride(1), out["g_Kuf"].stride(0), out["g_Lm"].stride(0)]
            assert len(set(lds_)) == len(lds_), lds_
            assert q_sqrt.stride(0) != c.M * q_sqrt.stride(1) and out["g_q_sqrt"].stride(0) != q_sqrt.stride(0)
        kw, extra = {}, {}
        if f.c_images is not None:
            kw["c_images"] = f.c_images
            if variant in ("prep", "t_bound"):
                nb = ops._lib.load().mgp_conditional_backward_prep_bytes(c.M, c.K)
                kw["prep"] = extra["prep"] = ops.conditional_backward_prep(q_sqrt, f.c_images[2],
                                                                           out=_zeros_u8(nb, device))
            if variant == "t_bound":
                kw["t_bound"] = f.t_bound
        ops.conditional_backward_x6(f.Afr, A, q_sqrt, q_mu, LinvT, G[:c.K], G[c.K:], c.M, c.N, out=out, fmt=f.fmt,
                                    cross=f.cross, **kw)
        return {**out, **extra}
    return run


def _check_bwd(got, ref):
    for key in ("g_Kuf", "g_Lm", "g_q_mu", "g_q_sqrt"):
        assert normwise(to_np(got[key]), ref[key]) < 1e-4, key
    assert float(got["g_var"].cpu()) == pytest.approx(ref["g_var"], rel=1e-5)


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("N,M,K", SHAPES)
@pytest.mark.parametrize("variant", BWD_VARIANTS)
def test_conditional_backward(device, N, M, K, variant, poison):
    """mgp_conditional_backward_x6, _f16 (S form), _f16c (the forward's C_k images),
    _f16c_prepped (prep; prep and t_bound) and _f16x8: lda, ldqs / strideq, ldq, ldl, ldg,
    ldgq, ldgs / strideg, ldk and ldgl are nine different numbers, and the strict upper
    triangle of q_sqrt is poisoned."""
    from modulatedgps_amd import ops
    c, f = chain(N, M, K), _bwd_forward(device, N, M, K, variant)
    got = both(device, poison, _bwd_run(ops, c, f, variant, device))
    _check_bwd(got, _bwd_reference(c, f))


@pytest.mark.parametrize("poison", POISONS)
def test_conditional_backward_scalar_q_mu(device, poison):
    """K = 4 with q_mu in rows of 5 floats: grad_a_prep_kernel reads q_mu by elements
    (qvec == 0) at a full KMAX = 4, where ld % 4 == 0 always took the float4 path.  Both
    paths form sum_k q_mu[m][k] G_mu[k][n] in the same order, so the bits are the tight
    call's."""
    from modulatedgps_amd import ops
    N, M, K = SHAPES[1]
    c, f = chain(N, M, K), _bwd_forward(device, N, M, K, "prep")
    got = both(device, poison, _bwd_run(ops, c, f, "prep", device, ldq=5))
    _check_bwd(got, _bwd_reference(c, f))


# =========================================================================== Cholesky backward
def _chol_bwd_ref(c, gL):
    Kuu = torch.tensor(np.array(c.Kuu), requires_grad=True)
    (torch.linalg.cholesky(Kuu) * torch.tensor(np.array(gL))).sum().backward()
    return 0.5 * (Kuu.grad + Kuu.grad.T).numpy()


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("N,M,K", SHAPES[:2])
def test_chol_backward(device, N, M, K, poison):
    """mgp_chol_backward and mgp_chol_backward_batch (two layers): ldl, ldli, ldg and ldo
    all differ (the batch's layers share each)."""
    from modulatedgps_amd import ops
    c = chain(N, M, K)

    def run(lay):
        L, LinvT, gL = lay.inp(c.L, "M"), lay.inp(c.LinvT, "M"), lay.inp(c.gL, "M")
        one = ops.chol_backward(L, LinvT, gL, out=lay.out((M, M), "M"))
        if lay.is_wide:
            assert len({L.stride(0), LinvT.stride(0), gL.stride(0), one.stride(0)}) == 4
        ldl, ldli, ldg, ldo = (lay.ld("M", M) for _ in range(4))
        Ls, Lis = [lay.inp(c.L, "M", ld=ldl) for _ in range(2)], [lay.inp(c.LinvT, "M", ld=ldli) for _ in range(2)]
        gLs = [lay.inp(g, "M", ld=ldg) for g in (c.gL, c.gL2)]
        two = ops.chol_backward_batch(Ls, Lis, gLs, outs=[lay.out((M, M), "M", ld=ldo) for _ in range(2)])
        return {"one": one, "b0": two[0], "b1": two[1]}

    got = both(device, poison, run)
    assert same_bits(got["b0"], got["one"])
    assert normwise(to_np(got["one"]), _chol_bwd_ref(c, c.gL)) < 1e-4
    assert normwise(to_np(got["b1"]), _chol_bwd_ref(c, c.gL2)) < 1e-4


# =========================================================================== KL and the image batch
@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("N,M,K", SHAPES)
def test_kl_and_qsqrt_images(device, N, M, K, poison):
    """mgp_gauss_kl_white, mgp_kl_grad and mgp_qsqrt_images_kl_f16_batch: wide q_mu (ldq) and
    q_sqrt (ldqs, strideq) with a poisoned upper triangle; kl_grad's g_q_mu (ldgq) and
    g_q_sqrt (ldgs, strideg) are updated in place, their padding must come back as it was."""
    from modulatedgps_amd import ops
    c = chain(N, M, K)
    rng = np.random.default_rng(M + K)
    g_mu0, g_sq0 = _r(rng.standard_normal((M, K))), _r(rng.standard_normal((K, M, M)))
    num_data = 1000.0

    def run(lay):
        q_mu, q_sqrt = lay.inp(c.q_mu, "K"), lay.inp(c.q_sqrt, "M", upper=True)
        kl = ops.gauss_kl_white(q_mu, q_sqrt, out=torch.full((1,), NAN, dtype=torch.float64, device=device))
        g_mu, g_sq = lay.inout(g_mu0, "K"), lay.inout(g_sq0, "M")
        ops.kl_grad(q_mu, q_sqrt, num_data, g_mu, g_sq)
        ldq, ldqs = lay.ld("K", K), lay.ld("M", M)
        q_mus = [lay.inp(q, "K", ld=ldq) for q in (c.q_mu, c.q_mu2)]
        q_sqrts = [lay.inp(q, "M", ld=ldqs, upper=True) for q in (c.q_sqrt, c.q_sqrt2)]
        if lay.is_wide:
            assert q_sqrts[0].data_ptr() % 16 == 0 and q_sqrts[0].stride(0) % 4 == 0   # no copy in the wrapper
        Lfrs = [_zeros_u8(ops.x6_lower_bytes(M, K), device) for _ in range(2)]
        kls = [torch.full((1,), NAN, dtype=torch.float64, device=device) for _ in range(2)]
        ops.qsqrt_images_kl_f16_batch(q_mus, q_sqrts, Lfrs, kls)
        one = ops.split_lower_x6(q_sqrts[1], out=_zeros_u8(ops.x6_lower_bytes(M, K), device), fmt="f16")
        return {"kl": kl, "g_q_mu": g_mu, "g_q_sqrt": g_sq, "Lfr0": Lfrs[0], "Lfr1": Lfrs[1], "kl0": kls[0],
                "kl1": kls[1], "Lfr1_single": one}

    got = both(device, poison, run)
    assert float(got["kl"].cpu()) == pytest.approx(R.gauss_kl_white(c.q_mu, c.q_sqrt), rel=1e-5)
    assert same_bits(got["kl0"], got["kl"])
    assert float(got["kl1"].cpu()) == pytest.approx(R.gauss_kl_white(c.q_mu2, c.q_sqrt2), rel=1e-5)
    # d(-KL / num_data): q_mu / nd off g_q_mu, (L - diag(1 / L_ii)) / nd off the lower triangle
    Linv_d = np.stack([np.diag(1.0 / np.diag(Lk)) for Lk in c.q_sqrt])
    assert normwise(to_np(got["g_q_mu"]), g_mu0 - c.q_mu / num_data) < 1e-4
    ref_sq = g_sq0 - np.tril(c.q_sqrt - Linv_d) / num_data
    assert normwise(to_np(got["g_q_sqrt"]), ref_sq) < 1e-4
    assert np.array_equal(np.triu(to_np(got["g_q_sqrt"]), 1), np.triu(g_sq0, 1))   # above the diagonal: untouched
    Mp = (M + 127) // 128 * 128
    nfb = K * (Mp // 32) * (Mp // 16) * 3 * 1024     # the fragments' bytes; the bound in the trailer
    lb = got["Lfr1"].numel()
    assert torch.equal(got["Lfr1"][:nfb], got["Lfr1_single"][:nfb])
    assert torch.equal(got["Lfr1"][lb - 256:lb - 252], got["Lfr1_single"][lb - 256:lb - 252])


# =========================================================================== grams
def _gram_ref(X, Y, W, alpha, mode):
    Yw = Y * (W[:, None, :] if W is not None else 1.0)
    ref = alpha * np.einsum("bin,bjn->bij", X, Yw)
    if mode == 1:
        ref = np.tril(ref)
    elif mode == 2:
        ref = np.tril(ref) + np.swapaxes(np.tril(ref, -1), 1, 2)
    return ref


@functools.lru_cache(maxsize=None)
def _gram_case(MI, MJ, N, B, same):
    rng = np.random.default_rng(MI + MJ + N)
    X = _r(rng.standard_normal((B, MI, N)))
    Y = _r(X[:, :MJ] + 0.3 * rng.standard_normal((B, MJ, N))) if same else _r(rng.standard_normal((B, MJ, N)))
    W = _r(rng.uniform(0.0, 1.0, (B, N)) - 0.3)
    for a in (X, Y, W):
        a.setflags(write=False)
    return X, Y, W


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("MI,MJ,N,tri", [(130, 37, 301, False), (37, 37, 515, True), (37, 37, 301, False)])
def test_gram_f32(device, MI, MJ, N, tri, poison):
    """mgp_gram (the 128 x 128 tile path, MJ > 16): ldx, ldy (N-wide) and ldo differ."""
    from modulatedgps_amd import ops
    X, Y, _ = _gram_case(MI, MJ, N, 1, tri)

    def run(lay):
        Xd, Yd = lay.inp(X[0], "N"), lay.inp(Y[0], "N")
        out = ops.gram(Xd, Yd, N=N, alpha=-0.5, tri=tri, out=lay.out((MI, MJ), "M"))
        if lay.is_wide:
            assert Xd.stride(0) != Yd.stride(0)
        return {"out": out}

    got = both(device, poison, run)
    assert normwise(to_np(got["out"]), _gram_ref(X, Y, None, -0.5, 1 if tri else 0)[0]) < 2e-6


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("f16", [False, True], ids=["x6", "f16"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("MI,MJ,N,mode", [(130, 37, 301, 0), (37, 37, 515, 1), (37, 37, 301, 2)])
def test_gram_x6(device, MI, MJ, N, mode, weighted, f16, poison):
    """mgp_gram_x6 and mgp_gram_f16 (bounds), batch 2, modes 0 / 1 / 2: ldx, ldy, sw (N-wide),
    ldo, and the batch strides sx, sy, so (rows x ld + 8) all differ."""
    from modulatedgps_amd import ops
    X, Y, W = _gram_case(MI, MJ, N, 2, mode != 0)
    bounds = None
    if f16:   # loose on X (4 x), exact on Y and W, as test_gram_x6
        bounds = (_t([4 * np.abs(X).max()], device), _t([np.abs(Y).max()], device),
                  _t([np.abs(W).max()], device) if weighted else None)

    def run(lay):
        Xd, Yd = lay.inp(X, "N"), lay.inp(Y, "N")
        Wd = lay.inp(W, "N") if weighted else None
        out = lay.out((2, MI, MJ), "M")
        if lay.is_wide:
            assert len({Xd.stride(1), Yd.stride(1)} | ({Wd.stride(0)} if weighted else set())) == 2 + weighted
            assert Xd.stride(0) == MI * Xd.stride(1) + 8 and out.stride(0) == MI * out.stride(1) + 8
        ops.gram_x6(Xd, Yd, Wd, alpha=-0.5, mode=mode, N=N, out=out, bounds=bounds)
        return {"out": out}

    got = both(device, poison, run)
    ref = _gram_ref(X, Y, W if weighted else None, -0.5, mode)
    assert normwise(to_np(got["out"]), ref) < (4e-6 if f16 else 2e-6)


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("MI,MJ,N,mode", [(130, 37, 301, 0), (37, 37, 515, 2), (37, 37, 301, 1)])
def test_gram_f16_rows(device, MI, MJ, N, mode, poison):
    """mgp_split_rows_f16 + mgp_gram_f16_rows: ldx of the split, ldy, sw, ldo and so differ;
    the same bits as mgp_gram_f16 splitting X on the fly (test_gram_f16_rows)."""
    from modulatedgps_amd import ops
    X, Y, W = _gram_case(MI, MJ, N, 2, False)
    X, Y = X[0], (X[0][:MJ] if mode else Y[0])
    bounds = (_t([1.5 * np.abs(X).max()], device), _t([np.abs(Y).max()], device), _t([np.abs(W).max()], device))

    def run(lay):
        Xd, Yd, Wd = lay.inp(X, "N"), lay.inp(Y, "N"), lay.inp(W, "N")
        img = ops.split_rows_f16(Xd, bounds[0], N=N, out=_zeros_u8(ops._lib.load().mgp_rows_f16_bytes(MI, N), device))
        out = ops.gram_x6(Xd, Yd, Wd, alpha=2.0, mode=mode, N=N, bounds=bounds, x_rows=img,
                          out=lay.out((2, MI, MJ), "M"))
        fly = ops.gram_x6(Xd, Yd, Wd, alpha=2.0, mode=mode, N=N, bounds=bounds, out=lay.out((2, MI, MJ), "M"))
        return {"img": img, "out": out, "fly": fly}

    got = both(device, poison, run)
    assert same_bits(got["out"], got["fly"])
    ref = _gram_ref(np.stack([X, X]), np.stack([Y, Y]), W, 2.0, mode)
    assert normwise(to_np(got["out"]), ref) < 4e-6


# =========================================================================== the alignment contract
def _refused(call, outputs, status=ALIGN):
    """`call` raises MGPError(status) and writes none of the sentinel-filled `outputs`."""
    from modulatedgps_amd import _lib
    before = [t.clone() for t in outputs]
    with pytest.raises(_lib.MGPError) as e:
        call()
    assert e.value.status == status, e.value
    torch.cuda.synchronize()
    for t, b in zip(outputs, before):
        assert same_bits(t, b)


def _odd(rows, cols, device, value=-12345.0, batch=None, stride_extra=0):
    """A sentinel-filled [batch?][rows][cols] view whose leading dimension is odd."""
    ld = round4(cols) + 5
    if batch is None:
        return torch.full((rows * ld,), value, device=device).as_strided((rows, cols), (ld, 1))
    bs = rows * ld + stride_extra
    return torch.full((batch * bs,), value, device=device).as_strided((batch, rows, cols), (bs, ld, 1))


def _sent(rows, cols, device, value=-12345.0, batch=None):
    from modulatedgps_amd import ops
    t = ops.padded(rows, cols, device, batch=batch)
    t.fill_(value)
    return t


def _storage_of(t):
    n = t.untyped_storage().nbytes() // 4
    return t.as_strided((n,), (1,), 0)


def test_refuses_misaligned_forward(device):
    """The forward entries' checked leading dimensions, one odd value at a time:
    MGP_ERR_ALIGN, and the sentinel-filled outputs stay as they were."""
    from modulatedgps_amd import ops
    N, M, K = SHAPES[0]
    c = chain(N, M, K)
    var, ls = _t([c.var], device), _t([c.ls], device)
    X, Z = _t(c.X, device), _t(c.Z, device)
    o = _odd(M, N, device)
    _refused(lambda: ops.rbf_kuf(X, Z, var, ls, out=o), [_storage_of(o)])
    o = _odd(M, M, device)
    _refused(lambda: ops.rbf_kuu(Z, var, ls, 1e-6, out=o), [_storage_of(o)])
    # K3: ldl, strideL
    A = ops.as_padded(_t(np.stack(_spd(M)), device))
    info = torch.full((2,), -7, dtype=torch.int32, device=device)
    ld = round4(M)
    odd_stride = lambda: torch.full((2 * (M * ld + 1),), -12345.0, device=device).as_strided(
        (2, M, M), (M * ld + 1, ld, 1))
    for mk in (lambda: _odd(M, M, device, batch=2), odd_stride):
        Lo, Li = mk(), mk()
        _refused(lambda: ops.potrf_trtri(A, L=Lo, LinvT=Li, info=info), [_storage_of(Lo), _storage_of(Li), info])
    # K4 (f32): ldl, ldk, lda, lds
    T = ops.stats_tiles(M)
    good = dict(LinvT=ops.as_padded(_t(c.LinvT, device)), Kuf=ops.as_padded(_t(c.Kuf, device)))
    for bad in ("LinvT", "Kuf", "A", "stats"):
        LinvT = _odd(M, M, device) if bad == "LinvT" else good["LinvT"]
        Kuf = _odd(M, N, device) if bad == "Kuf" else good["Kuf"]
        Ao = _odd(M, N, device) if bad == "A" else _sent(M, N, device)
        st = (_odd(T * (K + 1), N, device) if bad == "stats" else _sent(T * (K + 1), N, device)).unflatten(0, (T, K + 1))
        _refused(lambda: ops.trsm_stats(LinvT, Kuf, _t(c.q_mu, device), A=Ao, stats=st),
                 [_storage_of(Ao), _storage_of(st)])
    # K5 (f32): lda, ldqs, strideq, lds
    good = dict(A=ops.as_padded(_t(c.A, device)), qs=ops.as_padded(_t(c.q_sqrt, device)),
                st=ops.as_padded(_t(c.stats.reshape(T * (K + 1), N), device)))
    for bad in ("A", "qs", "strideq", "st"):
        Ain = _odd(M, N, device) if bad == "A" else good["A"]
        qs = good["qs"]
        if bad == "qs":
            qs = _odd(M, M, device, batch=K)
        elif bad == "strideq":
            ld = round4(M)
            qs = torch.zeros(K * (M * ld + 1), device=device).as_strided((K, M, M), (M * ld + 1, ld, 1))
        st = (_odd(T * (K + 1), N, device) if bad == "st" else good["st"]).unflatten(0, (T, K + 1))
        fm, fv = _sent(K, N, device), _sent(K, N, device)
        _refused(lambda: ops.expert_conditional(Ain, qs, st, var, fmean=fm, fvar=fv), [_storage_of(fm), _storage_of(fv)])
    # K7 (the wrapper copies a view it could not pass on, so the entry itself is called)
    q_mu, out = _t(c.q_mu, device), torch.full((1,), -5.0, dtype=torch.float64, device=device)
    ws = torch.empty(max(ops._lib.load().mgp_kl_workspace_bytes(M, K), 16), dtype=torch.uint8, device=device)
    stream = torch.cuda.current_stream().cuda_stream
    P = ctypes.c_void_p * 1
    Lfr = torch.full((ops.x6_lower_bytes(M, K),), 7, dtype=torch.uint8, device=device)
    ws2 = torch.empty(max(ops._lib.load().mgp_qsqrt_workspace_bytes(M, K), 16), dtype=torch.uint8, device=device)
    for ldqs, strideq in ((round4(M) + 5, M * (round4(M) + 5)), (round4(M), M * round4(M) + 1)):
        qs = torch.zeros(K * strideq, device=device)
        _refused(lambda: ops._lib.call("mgp_gauss_kl_white", q_mu.data_ptr(), K, qs.data_ptr(), ldqs, strideq, M, K,
                                       out.data_ptr(), ws.data_ptr(), ws.numel(), stream), [out])
        _refused(lambda: ops._lib.call("mgp_qsqrt_images_kl_f16_batch", 1, P(q_mu.data_ptr()), K, P(qs.data_ptr()),
                                       ldqs, strideq, M, K, P(Lfr.data_ptr()), Lfr.numel(), P(out.data_ptr()),
                                       ws2.data_ptr(), ws2.numel(), stream), [Lfr, out])


@pytest.mark.parametrize("variant", ["x6", "f16", "f16c"])
def test_conditional_backward_refuses_misaligned(device, variant):
    """lda, ldk and ldg (K > 1) are leading dimensions of gram operands and weights: an odd
    one is refused with MGP_ERR_ALIGN before anything is launched.  (It used to reach an
    inner mgp_gram_x6 / mgp_split_rows_f16 and come back as that call's -2, -6 or -10, for
    ldk after g_Kuf had been written.)"""
    from modulatedgps_amd import ops
    N, M, K = SHAPES[0]
    c, f = chain(N, M, K), _bwd_forward(device, N, M, K, variant)
    qs, q_mu, LinvT = ops.as_padded(_t(c.q_sqrt, device)), _t(c.q_mu, device), ops.as_padded(_t(f.LinvT, device))
    for bad in ("lda", "ldg", "ldk"):
        A = _odd(M, N, device, value=0.0) if bad == "lda" else ops.as_padded(_t(f.A, device))
        G = (_odd(2 * K, N, device, value=0.0) if bad == "ldg" else ops.padded(2 * K, N, device, zero=True))
        out = {"g_q_mu": _sent(M, K, device), "g_q_sqrt": _sent(M, M, device, batch=K),
               "g_Kuf": _odd(M, N, device) if bad == "ldk" else _sent(M, N, device), "g_Lm": _sent(M, M, device),
               "g_var": torch.full((1,), -5.0, dtype=torch.float64, device=device)}
        kw = {"c_images": f.c_images} if f.c_images is not None else {}
        _refused(lambda: ops.conditional_backward_x6(f.Afr, A, qs, q_mu, LinvT, G[:K], G[K:], M, N, out=out, fmt=f.fmt,
                                                     cross=f.cross, **kw),
                 [_storage_of(out[k]) for k in ("g_q_mu", "g_q_sqrt", "g_Kuf", "g_Lm")] + [out["g_var"]])


def test_gram_alignment(device):
    """mgp_gram: the tile path (MJ > 16) refuses an odd ldx / ldy with MGP_ERR_ALIGN (a host
    check this contract found missing); the narrow path (MJ <= 16) reads by elements and takes
    them.  mgp_gram_x6 / _f16 / _f16_rows refuse with the number of the argument."""
    from modulatedgps_amd import ops
    MI, MJ, N = 130, 37, 301
    X, Y, W = _gram_case(MI, MJ, N, 2, False)
    Xt, Yt, Wt = (ops.as_padded(_t(a, device)) for a in (X, Y, W[:, None, :]))
    Wt = Wt[:, 0, :]

    def odd_of(a):
        o = _odd(a.shape[-2], a.shape[-1], device, batch=a.shape[0] if a.ndim == 3 else None)
        o.copy_(_t(a, device))
        return o

    out = _sent(MI, MJ, device)
    _refused(lambda: ops.gram(odd_of(X[0]), Yt[0], N=N, out=out), [_storage_of(out)])
    _refused(lambda: ops.gram(Xt[0], odd_of(Y[0]), N=N, out=out), [_storage_of(out)])
    narrow = ops.gram(odd_of(X[0]), odd_of(Y[0][:5]), N=N, alpha=-0.5)        # MJ = 5: by elements
    assert normwise(to_np(narrow), -0.5 * X[0] @ Y[0][:5].T) < 2e-6
    out = _sent(MI, MJ, device, batch=2)
    odd_stride = lambda a: torch.zeros(2 * (a.shape[1] * round4(N) + 1), device=device).as_strided(
        a.shape, (a.shape[1] * round4(N) + 1, round4(N), 1))
    Wodd = torch.zeros(2 * (round4(N) + 1), device=device).as_strided((2, N), (round4(N) + 1, 1))
    bounds = (_t([4.0], device), _t([4.0], device), _t([1.0], device))
    for kw in ({}, {"bounds": bounds}):
        _refused(lambda: ops.gram_x6(odd_of(X), Yt, Wt, N=N, out=out, **kw), [_storage_of(out)], status=-2)
        _refused(lambda: ops.gram_x6(odd_stride(X), Yt, Wt, N=N, out=out, **kw), [_storage_of(out)], status=-3)
        _refused(lambda: ops.gram_x6(Xt, odd_of(Y), Wt, N=N, out=out, **kw), [_storage_of(out)], status=-6)
        _refused(lambda: ops.gram_x6(Xt, Yt, Wodd, N=N, out=out, **kw), [_storage_of(out)], status=-10)
    img = ops.split_rows_f16(Xt[0], bounds[0], N=N)
    _refused(lambda: ops.gram_x6(Xt[0], odd_of(Y[0]), Wt, N=N, out=out, bounds=bounds, x_rows=img),
             [_storage_of(out)], status=-5)
    _refused(lambda: ops.gram_x6(Xt[0], Yt[0], Wodd, N=N, out=out, bounds=bounds, x_rows=img),
             [_storage_of(out)], status=-10)
