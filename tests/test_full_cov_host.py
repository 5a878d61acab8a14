"""CPU tests of the full-covariance C-ABI entries (include/mgp_hip.h): workspace sizing and
argument validation, all before any HIP call (no GPU needed)."""
import ctypes

from modulatedgps_amd import _lib

MGP_OP_FULL_COV_CONDITIONAL = 12


def test_full_cov_workspace_bytes():
    lib = _lib.load()
    assert lib.mgp_full_cov_workspace_bytes(64, 100, 3) >= 3 * 64 * 100 * 4
    for M, N, K in ((64, 100, 3), (1024, 4096, 8), (25, 33, 1), (130, 257, 32)):
        assert lib.mgp_workspace_bytes(MGP_OP_FULL_COV_CONDITIONAL, M, N, K) == \
            lib.mgp_full_cov_workspace_bytes(M, N, K) >= K * M * N * 4
    assert lib.mgp_full_cov_workspace_bytes(0, 100, 3) == 0
    assert lib.mgp_full_cov_workspace_bytes(64, 0, 3) == 0
    assert lib.mgp_full_cov_workspace_bytes(64, 100, 0) == 0


def test_full_cov_conditional_checks_arguments():
    """Every bad argument is rejected with the code documented in mgp_hip.h before any
    pointer is read or HIP call made; empty sizes are a no-op."""
    lib = _lib.load()
    c = ctypes.c_void_p(256)
    M, N, K, D = 64, 100, 3, 2
    wsb = lib.mgp_full_cov_workspace_bytes(M, N, K)
    names = ("X", "ldx", "N", "D", "var", "ls", "n_ls", "A", "lda", "q", "ldqs", "sq", "M", "K", "cov", "ldc",
             "sc", "ws", "wsb", "s")
    base = dict(X=c, ldx=D, N=N, D=D, var=c, ls=c, n_ls=1, A=c, lda=100, q=c, ldqs=M, sq=M * M, M=M, K=K, cov=c,
                ldc=100, sc=100 * N, ws=c, wsb=wsb, s=None)
    assert len(names) == len(_lib.SIGNATURES["mgp_full_cov_conditional"][1])
    call = lambda **kw: lib.mgp_full_cov_conditional(*[kw.get(n, base[n]) for n in names])
    assert call(X=None) == -1
    assert call(ldx=D - 1) == -2
    assert call(D=0) == -4
    assert call(D=33, ldx=64) == 3
    assert call(var=None) == -5
    assert call(ls=None) == -6
    assert call(n_ls=3) == -7 and call(n_ls=D) != -7
    assert call(A=None) == -8
    assert call(lda=N - 1) == -9
    assert call(q=None) == -10
    assert call(ldqs=M - 1) == -11
    assert call(sq=M * M - 4) == -12
    assert call(K=33) == 3
    assert call(cov=None) == -15
    assert call(ldc=N - 4) == -16
    assert call(sc=100 * N - 4) == -17
    # float4 rows: leading dimensions multiples of 4, 16-byte aligned bases
    assert call(ldc=102, sc=102 * N) == 2
    assert call(lda=102) == 2
    assert call(cov=ctypes.c_void_p(260)) == 2
    assert call(ws=ctypes.c_void_p(264)) == 2
    assert call(ws=None) == 1 and call(wsb=wsb - 1) == 1
    # one expert: the strides are not used
    assert call(K=1, sq=0, sc=0, wsb=0) == 1
    # empty problems: nothing to do, no launch
    assert call(N=0) == 0 and call(M=0) == 0 and call(K=0) == 0 and call(N=-1) == 0
