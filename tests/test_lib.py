"""CPU tests of the C-ABI boundary: libmgp_hip.so loads without a GPU and exports
every function declared in include/mgp_hip.h (no compute calls are made)."""
import os
import ctypes

import pytest

from modulatedgps_amd import _lib


def test_library_loads_and_reports_gfx950():
    lib = _lib.load()
    assert lib.mgp_version().decode().endswith("gfx950")


def test_exports_every_header_symbol():
    syms = _lib.header_symbols()
    assert len(syms) >= 18
    raw = ctypes.CDLL(_lib.LIB_PATH)
    missing = [s for s in syms if not hasattr(raw, s)]
    assert not missing, missing


C = ctypes
SMALL_HEADER = """
#ifndef SMALL_H
#define SMALL_H
#define mgp_macro(x) int mgp_from_define(int x);
#define mgp_long_macro(x) \\
  int mgp_from_continued_define(int x);
typedef void* mgp_stream_t; /* hipStream_t */
enum { MGP_OK = 0 };
/* int mgp_in_block_comment(int a);
   spread over lines */
// int mgp_after_slashes(int a);
const char* mgp_name(void);
void* mgp_handle();   // int mgp_trailing_comment(void);
size_t mgp_bytes(int a, int32_t b, int64_t c, uint64_t d, size_t e, float f, double g, mgp_stream_t s);
int mgp_broken(const float* const* Z, /* int mgp_inner(int a); */
               const int32_t *n_ls,
               float* out, int64_t ldo);
float* mgp_float_ptr(void* img, int64_t M);
int64_t mgp_unnamed(int64_t, const double*);
#endif
"""


def test_parser_reads_every_declaration_form():
    """Scalars by exact width, every pointer spelling as c_void_p, the three return kinds,
    (void) / (), a declaration over three lines; nothing from comments or #define lines."""
    table = _lib.parse_prototypes(SMALL_HEADER)
    assert table == {
        "mgp_name": (C.c_char_p, []),
        "mgp_handle": (C.c_void_p, []),
        "mgp_bytes": (C.c_size_t, [C.c_int, C.c_int32, C.c_int64, C.c_uint64, C.c_size_t, C.c_float, C.c_double,
                                   C.c_void_p]),
        "mgp_broken": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
        "mgp_float_ptr": (C.c_void_p, [C.c_void_p, C.c_int64]),
        "mgp_unnamed": (C.c_int64, [C.c_int64, C.c_void_p]),
    }
    assert list(table) == ["mgp_name", "mgp_handle", "mgp_bytes", "mgp_broken", "mgp_float_ptr", "mgp_unnamed"]
    for _, args in table.values():
        assert all(a is C.c_void_p or a in (C.c_int, C.c_int32, C.c_int64, C.c_uint64, C.c_size_t, C.c_float,
                                            C.c_double) for a in args)


@pytest.mark.parametrize("decl, named", [
    ("int mgp_bad(long n);", "mgp_bad"),
    ("int mgp_bad(int64_t M, struct foo v);", "struct foo v"),
    ("int mgp_bad(unsigned int n);", "unsigned int n"),
    ("long mgp_bad(void);", "mgp_bad"),
    ("unsigned mgp_bad(void);", "mgp_bad"),
    ("int mgp_bad(int32_t a, short b);", "parameter 2"),
])
def test_parser_refuses_types_outside_the_vocabulary(decl, named):
    with pytest.raises(_lib.MGPLibraryError, match="mgp_bad") as e:
        _lib.parse_prototypes("int mgp_fine(int a);\n" + decl)
    assert named in str(e.value)


@pytest.mark.parametrize("decl", [
    "int mgp_cb(int (*fn)(int), int64_t n);",
    "int mgp_attr(int a) __attribute__((deprecated));",
    "int mgp_open(int a;",
])
def test_parser_refuses_a_declaration_it_cannot_read(decl):
    """An entry the pattern misses would get no argtypes and ctypes' default int conversion."""
    with pytest.raises(_lib.MGPLibraryError, match="cannot parse"):
        _lib.parse_prototypes("int mgp_fine(int a);\n" + decl + "\nint mgp_after(void);")


def test_header_symbols_and_missing_header(tmp_path):
    h = tmp_path / "small.h"
    h.write_text(SMALL_HEADER)
    assert _lib.header_symbols(str(h)) == sorted(
        ["mgp_name", "mgp_handle", "mgp_bytes", "mgp_broken", "mgp_float_ptr", "mgp_unnamed"])
    with pytest.raises(_lib.MGPLibraryError, match="absent.h"):
        _lib.header_symbols(str(tmp_path / "absent.h"))


def test_prototypes_of_the_real_header_are_pinned():
    """Exact restype and argtypes of entries that carry each width the ABI uses."""
    P, I32, I64, U64, SZ, F, D = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_size_t, C.c_float, C.c_double
    S = _lib.SIGNATURES
    assert len(S) >= 115 and sorted(S) == _lib.header_symbols()
    assert S["mgp_version"] == (C.c_char_p, [])
    assert S["mgp_status_string"] == (C.c_char_p, [C.c_int])
    assert S["mgp_chol_workspace_bytes"] == (SZ, [I64, I32])
    assert S["mgp_x6_bound_ptr"] == (P, [P, I64, I64, I32])
    assert S["mgp_kl_grad"] == (C.c_int, [P, I64, P, I64, I64, I64, I32, D, P, I64, P, I64, I64, P])
    assert S["mgp_elbo_terms"] == (C.c_int, [P, P, P, P, I64, P, P, I64, I32, I32, F, F, P, P, U64, I64, P, P, SZ, P])
    assert S["mgp_kuu_potrf_trtri"] == (C.c_int, [P, I64, I64, I32, P, P, P, F, I32, P, P, I64, I64, P, P, SZ, P])
    lib = _lib.load()
    for name, (res, args) in S.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


class _FakeTensor:
    def __init__(self, ptr):
        self.ptr = ptr

    def data_ptr(self):
        return self.ptr


def test_marshal_converts_tensors_and_lists_only():
    import torch
    t = torch.zeros(4, 4)
    assert _lib.marshal(t) == t.data_ptr() and isinstance(_lib.marshal(t), int)
    assert _lib.marshal(_FakeTensor(4096)) == 4096
    u = torch.ones(3)
    for seq in ([t, None, u], (t, None, u)):
        arr = _lib.marshal(seq)
        assert isinstance(arr, C.c_void_p * 3)
        assert list(arr) == [t.data_ptr(), None, u.data_ptr()]
    assert len(_lib.marshal([])) == 0
    ready = (C.c_void_p * 2)(8, None)
    lengths = (C.c_int64 * 2)(4, 4)
    assert _lib.marshal(ready) is ready and _lib.marshal(lengths) is lengths
    handle = C.c_void_p(8)
    assert _lib.marshal(handle) is handle
    for v in (3, -1, 1 << 40, 0.25, None, True):
        assert _lib.marshal(v) is v


def test_call_marshals_lists_and_prebuilt_arrays_alike():
    """mgp_adam_step_set with all-empty blocks (rows = 0) is a no-op that needs no GPU
    (csrc/train.hip): the same call with the pointer arrays as lists of CPU tensors and as
    prebuilt ctypes arrays returns normally."""
    import torch
    n = 2
    theta, u, g, m1, m2 = ([torch.zeros(4, 4) for _ in range(n)] for _ in range(5))
    I64, I32 = C.c_int64 * n, C.c_int32 * n
    empty, four, f32 = I64(0, 0), I64(4, 4), I32(0, 0)
    hyper = (1e-3, 0.9, 0.999, 1e-7, 1, -1.0, None)   # lr, beta1, beta2, eps, t, grad_sign, stream
    assert _lib.call("mgp_adam_step_set", n, theta, [None, u[1]], g, f32, four, m1, m2, empty, four, four,
                     *hyper) is None
    at, au, ag, am1, am2 = (_lib.marshal(ts) for ts in (theta, u, g, m1, m2))
    assert _lib.call("mgp_adam_step_set", n, at, au, ag, f32, four, am1, am2, empty, four, four, *hyper) is None
    # with rows > 0 the same lists reach the size checks (ld < cols), still before any HIP call
    with pytest.raises(_lib.MGPError) as e:
        _lib.call("mgp_adam_step_set", n, theta, u, g, f32, four, m1, m2, four, four, I64(4, 3), *hyper)
    assert e.value.status == -11


def test_call_raw_takes_converted_arguments_only():
    """call_raw is call without the marshalling pass: the same no-op with prebuilt arrays,
    and a tensor is refused by ctypes instead of being converted."""
    import torch
    n = 1
    arr = [_lib.marshal([torch.zeros(4, 4)]) for _ in range(5)]
    one = (C.c_int64 * n)(4)
    tail = ((C.c_int64 * n)(0), one, one, 1e-3, 0.9, 0.999, 1e-7, 1, -1.0, None)
    assert _lib.call_raw("mgp_adam_step_set", n, arr[0], arr[1], arr[2], (C.c_int32 * n)(0), one, arr[3], arr[4],
                         *tail) is None
    with pytest.raises(C.ArgumentError):
        _lib.call_raw("mgp_adam_step_set", n, torch.zeros(4, 4), arr[1], arr[2], (C.c_int32 * n)(0), one, arr[3],
                      arr[4], *tail)
    with pytest.raises(_lib.MGPError) as e:
        _lib.call_raw("mgp_rbf_kuf", None, 1, None, 1, 10, 10, 1, None, None, 1, None, 12, None)
    assert e.value.status == -1


def test_refused_call_raises_mgp_error():
    import torch
    Z = torch.zeros(10, 1)
    with pytest.raises(_lib.MGPError) as e:
        _lib.call("mgp_rbf_kuf", None, 1, Z, 1, 10, 10, 1, None, None, 1, None, 12, None)
    assert e.value.status == -1


def test_status_strings_and_argument_checks():
    lib = _lib.load()
    assert lib.mgp_status_string(0) == b"ok"
    assert b"workspace" in lib.mgp_status_string(1)
    # invalid arguments are rejected before any HIP call (safe without a GPU)
    assert lib.mgp_rbf_kuf(None, 1, None, 1, 10, 10, 1, None, None, 1, None, 12, None) == -1
    assert lib.mgp_trsm_stats(None, 0, None, 0, 4, 4, None, 0, 1, None, 0, None, 0, None) == -1
    # per matrix float64 W, B [Mp][Mp] + D [nb][64][64]
    assert lib.mgp_chol_workspace_bytes(1024, 2) == 2 * (2 * 1024 * 1024 + 16 * 64 * 64) * 8
    assert lib.mgp_stats_tiles(1024) in (8, 16)   # 128- or 64-row tiles


def test_size_limits_are_refused_and_documented():
    """One past a size limit an entry returns MGP_ERR_UNSUPPORTED (3) before any HIP call or
    pointer read (so this runs without a GPU; tests/test_gpu_range_edges.py covers every entry
    on the device), and the header and INTEGRATION.md state the limits the code enforces."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)     # never dereferenced: the calls below are refused first
    assert lib.mgp_rbf_kuf(p, 33, p, 33, 10, 10, 33, p, p, 1, p, 12, None) == 3              # D <= 32
    assert lib.mgp_trsm_stats(p, 4, p, 4, 4, 4, p, 20, 17, p, 4, p, 4, None) == 3            # K4: K <= 16
    assert lib.mgp_relaxed_onehot_sample(p, 10, 33, 2, 0.01, None, 0, 0, p, None) == 3       # K6: K <= 32
    assert b"supported range" in lib.mgp_status_string(3)
    header = open(_lib.HEADER_PATH).read()
    assert "D > 64" not in header
    assert "D > 32" in header and "K > 16" in header and "K > 32" in header
    doc = open(os.path.join(os.path.dirname(_lib.HEADER_PATH), "..", "INTEGRATION.md")).read()
    assert "`D <= 32`" in doc and "`K <= 16`" in doc and "`K <= 32`" in doc


def test_product_path_fails_loudly_without_library(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "missing.so"))
    with pytest.raises(_lib.MGPLibraryError):
        _lib.load()


def test_jitter_argument_is_validated():
    """The reparameterisation jitter (default_jitter(), utils.py:26-27) is an ABI
    argument of K6 and the sampler; a negative value is rejected before any HIP call."""
    lib = _lib.load()
    c = ctypes.c_void_p(8)
    rc = lib.mgp_elbo_terms(c, c, c, c, 4, c, c, 4, 2, 3, 0.01, -1.0, None, None, 0, 0, c, c, 64, None)
    assert rc == -14


def test_library_reads_no_environment():
    """the only process-global state is the lazily loaded code object --
    kernel choices follow from the entry point and its arguments, so the library
    imports no getenv (round 4 removed its per-call variant switches)."""
    data = open(_lib.LIB_PATH, "rb").read()
    assert b"getenv\x00" not in data


def test_integration_lists_every_entry():
    """INTEGRATION.md §2a names every C-ABI entry of include/mgp_hip.h (with the
    reference call site it replaces)."""
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "INTEGRATION.md")).read()
    missing = [s for s in _lib.header_symbols() if f"`{s}`" not in text]
    assert not missing, missing


def test_batch_entries_reject_out_of_range_batch():
    """The layer-batch entries take batch in [1, 2] and reject anything else with a
    code of their own (documented in mgp_hip.h) before any HIP call."""
    lib = _lib.load()
    p = (ctypes.c_void_p * 3)(8, 8, 8)
    assert lib.mgp_split_upper_f16_bounded_batch(3, ctypes.c_void_p(8), 64, 4096, 64, p, 1 << 20, None) == -9
    assert lib.mgp_split_upper_f16_bounded_batch(0, ctypes.c_void_p(8), 64, 4096, 64, p, 1 << 20, None) == -9
    assert lib.mgp_split_upper_f16_bounded_batch(1, None, 64, 4096, 64, p, 1 << 20, None) == -2
    for bad in (0, 3):
        assert lib.mgp_qsqrt_images_kl_f16_batch(bad, p, 8, p, 64, 4096, 64, 8, p, 1 << 24, p, p, 1 << 20,
                                                 None) == -1
    assert lib.mgp_qsqrt_images_kl_f16_batch(2, None, 8, p, 64, 4096, 64, 8, p, 1 << 24, p, p, 1 << 20, None) == -2
    assert lib.mgp_qsqrt_images_kl_f16_batch(2, p, 8, p, 64, 4096, 64, 8, p, 16, p, p, 1 << 20, None) == -10


def test_tail_backward_batch_entries_check_arguments():
    """mgp_chol_backward_batch / mgp_rbf_backward_batch: batch in [1, 8], per-layer NULL
    pointers and sizes rejected with the codes documented in mgp_hip.h, a short
    workspace with MGP_ERR_WORKSPACE -- all before any HIP call."""
    lib = _lib.load()
    c = ctypes.c_void_p(8)
    p = (ctypes.c_void_p * 2)(8, 8)
    z = (ctypes.c_void_p * 2)(8, None)
    for bad in (0, 9):
        assert lib.mgp_chol_backward_batch(bad, p, 64, p, 64, p, 64, 64, p, 64, c, 1 << 30, None) == -1
        assert lib.mgp_rbf_backward_batch(bad, c, 8, 100, p, 8, 64, 8, p, p, 1, p, 100, p, 64, 1, p, 8, p, p,
                                          c, 1 << 30, None) == -1
    assert lib.mgp_chol_backward_batch(2, z, 64, p, 64, p, 64, 64, p, 64, c, 1 << 30, None) == -2
    assert lib.mgp_chol_backward_batch(2, p, 64, p, 64, z, 64, 64, p, 64, c, 1 << 30, None) == -6
    assert lib.mgp_chol_backward_batch(2, p, 64, p, 64, p, 64, -1, p, 64, c, 1 << 30, None) == -8
    assert lib.mgp_chol_backward_batch(2, p, 64, p, 64, p, 64, 64, p, 32, c, 1 << 30, None) == -10
    ws = lib.mgp_chol_backward_workspace_bytes(64)
    assert lib.mgp_chol_backward_batch(2, p, 64, p, 64, p, 64, 64, p, 64, c, 2 * ws - 1, None) == 1
    args = lambda **kw: [kw.get(k, v) for k, v in (
        ("batch", 2), ("X", c), ("ldx", 8), ("N", 100), ("Z", p), ("ldz", 8), ("M", 64), ("D", 8), ("var", p),
        ("ls", p), ("n_ls", 1), ("gKuf", p), ("ldgf", 100), ("gKuu", p), ("ldgu", 64), ("acc", 1), ("gZ", p),
        ("ldgz", 8), ("g_var", p), ("g_ls", p), ("ws", c), ("wsb", 1 << 30), ("s", None))]
    assert lib.mgp_rbf_backward_batch(*args(X=None)) == -2
    assert lib.mgp_rbf_backward_batch(*args(D=33, ldx=64, ldz=64, ldgz=64)) == 3
    assert lib.mgp_rbf_backward_batch(*args(n_ls=3)) == -11
    assert lib.mgp_rbf_backward_batch(*args(gKuu=z)) == -14
    assert lib.mgp_rbf_backward_batch(*args(g_ls=z)) == -19
    assert lib.mgp_rbf_backward_batch(*args(acc=3)) == -20 and lib.mgp_rbf_backward_batch(*args(acc=-1)) == -20
    wb = lib.mgp_rbf_backward_batch_workspace_bytes(100, 64, 8)
    assert lib.mgp_rbf_backward_batch(*args(wsb=2 * wb - 1)) == 1


def test_adam_step_set_checks_arguments():
    """mgp_adam_step_set: n in [1, 16], NULL arrays / entries and bad sizes rejected
    with the codes of mgp_hip.h before any HIP call; all-empty blocks are a no-op."""
    lib = _lib.load()
    P, I64, I32 = ctypes.c_void_p * 2, ctypes.c_int64 * 2, ctypes.c_int32 * 2
    p, z = P(8, 8), P(8, None)
    one, i32 = I64(4, 4), I32(0, 1)
    call = lambda n=2, theta=p, u=p, g=p, m1=p, rows=one, cols=one, ld=one, t=1: lib.mgp_adam_step_set(
        n, theta, u, g, i32, one, m1, p, rows, cols, ld, 1e-3, 0.9, 0.999, 1e-7, t, -1.0, None)
    assert call(n=0) == -1 and call(n=17) == -1
    assert call(theta=z) == -2
    assert call(theta=z, rows=I64(0, 0)) == 0   # an empty block's pointers are not used
    assert call(g=z) == -4
    assert call(m1=z) == -7
    assert call(rows=I64(4, -1)) == -9
    assert call(ld=I64(4, 3)) == -11
    assert call(t=0) == -16
    assert call(rows=I64(0, 0)) == 0   # nothing to update: no launch


def test_conditional_backward_prep_entries_check_arguments():
    """mgp_conditional_backward_prep_f16c / _f16c_prepped: NULL pointers, bad sizes and a
    short prep buffer rejected with the codes of mgp_hip.h before any HIP call."""
    lib = _lib.load()
    c = ctypes.c_void_p(256)
    M, K, N = 64, 3, 100
    pb = lib.mgp_conditional_backward_prep_bytes(M, K)
    assert pb >= lib.mgp_x6_lower_bytes(M, K) + K * M * M * 4
    prep = lambda q=c, ldqs=M, sq=M * M, m=M, k=K, lb=c, out=c, nb=pb: lib.mgp_conditional_backward_prep_f16c(
        q, ldqs, sq, m, k, lb, out, nb, None)
    assert prep(q=None) == -1 and prep(ldqs=M - 1) == -2 and prep(sq=M) == -3
    assert prep(m=0) == -4 and prep(k=0) == -5 and prep(k=17) == 3
    assert prep(lb=None) == -6 and prep(out=None) == -7 and prep(nb=pb - 1) == 1
    assert prep(out=ctypes.c_void_p(264)) == 2
    wsb = lib.mgp_conditional_backward_workspace_bytes(M, N, K)
    cb = lambda cfr=c, pr=c, nb=pb: lib.mgp_conditional_backward_f16c_prepped(
        c, 1 << 30, c, 128, c, M, M * M, c, K, c, M, c, c, 128, M, N, K, c, K, c, M, M * M, c, 128, c, M, c, c, wsb,
        cfr, 1 << 30, c, c, pr, nb, None, None)
    assert cb(cfr=None) == -30 and cb(pr=None) == -33 and cb(nb=pb - 1) == -34


def test_workspace_helpers_size_reuse_and_refuse():
    """ops._workspace keeps a buffer that is large enough and replaces one that is not
    (count scales the size for the batch entries); the *_workspace functions whose entry
    answers 0 bytes refuse the sizes with MGP_ERR_UNSUPPORTED.  Host memory: no GPU."""
    import torch
    from modulatedgps_amd import ops
    lib = _lib.load()
    entry = "mgp_chol_backward_workspace_bytes"
    nbytes = lib.mgp_chol_backward_workspace_bytes(64)
    ws = ops._workspace(entry, (64,), None, "cpu")
    assert ws.dtype == torch.uint8 and ws.numel() == nbytes > 16
    assert ops._workspace(entry, (64,), ws, "cpu") is ws
    both = ops._workspace(entry, (64,), ws, "cpu", count=2)
    assert both is not ws and both.numel() == 2 * nbytes
    assert ops._workspace(entry, (64,), both, "cpu") is both
    assert ops.natgrad_workspace(64, 3, "cpu").numel() == lib.mgp_natgrad_workspace_bytes(64, 3)
    with pytest.raises(_lib.MGPError) as e:
        ops.natgrad_workspace(0, 3, "cpu")
    assert e.value.status == 3 and "mgp_natgrad_workspace_bytes" in str(e.value)
    assert ops.full_cov_workspace_bytes(64, 100, 3) == lib.mgp_full_cov_workspace_bytes(64, 100, 3)
