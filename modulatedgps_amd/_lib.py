"""ctypes binding of libmgp_hip.so (the C-ABI declared in include/mgp_hip.h).

There is deliberately no fallback: if the HIP library is missing or cannot be
loaded, every op raises ``MGPLibraryError``.  The product path never computes
on the CPU.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MGP_HIP_LIB", os.path.join(_HERE, "libmgp_hip.so"))
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mgp_hip.h")


class MGPLibraryError(RuntimeError):
    """libmgp_hip.so is missing or could not be loaded."""


class MGPError(RuntimeError):
    """A libmgp_hip call returned a non-zero status."""

    def __init__(self, fn, status, msg):
        super().__init__(f"{fn} failed with status {status}: {msg}")
        self.status = status


class MGPLinAlgError(MGPError):
    """Cholesky of Kuu failed (non-positive pivot), like TF's InvalidArgumentError
    raised from base_conditional (MixtureGPs/models.py:141)."""


_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64,
            "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
            "double": ctypes.c_double, "mgp_stream_t": ctypes.c_void_p}


def _ctype(decl, where, is_return=False):
    """The ctypes type of one C return type or parameter; an unknown type raises (no width is guessed)."""
    words = decl.replace("*", " * ").split()
    if is_return and words == ["const", "char", "*"]:
        return ctypes.c_char_p   # a C string (mgp_version, mgp_status_string)
    words = [w for w in words if w != "const"]
    if "*" in words:
        return ctypes.c_void_p
    if not is_return and len(words) == 2:
        words.pop()   # the parameter's name
    if len(words) != 1 or words[0] not in _SCALARS:
        raise MGPLibraryError(f"{where}: type {decl.strip()!r} is outside the C-ABI's vocabulary")
    return _SCALARS[words[0]]


def parse_prototypes(text):
    """name -> (restype, [argtypes]) of every `ret mgp_name(params);` in the header text."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//.*", "", text)
    text = re.sub(r"^[ \t]*#(?:.*\\\n)*.*$", "", text, flags=re.M)
    table = {}
    for stmt in text.split(";"):
        m = re.fullmatch(r"\s*(.*?)\b(mgp_\w+)\s*\(([^()]*)\)\s*", re.split(r"[{}]", stmt)[-1], re.S)
        if not m:
            if re.search(r"\bmgp_\w+\s*\(", stmt):   # no prototype, no call: never a default int conversion
                raise MGPLibraryError(f"cannot parse the declaration {' '.join(stmt.split())!r}")
            continue
        ret, name, params = m.groups()
        params = [] if params.strip() in ("", "void") else params.split(",")
        table[name] = (_ctype(ret, f"{name}: return", is_return=True),
                       [_ctype(p, f"{name}: parameter {i + 1} ({p.strip()})") for i, p in enumerate(params)])
    return table


def header_prototypes(path=HEADER_PATH):
    try:
        with open(path) as f:
            return parse_prototypes(f.read())
    except OSError as e:
        raise MGPLibraryError(f"cannot read the C-ABI header {path}: {e}") from e


def header_symbols(path=HEADER_PATH):
    """Every function name declared in include/mgp_hip.h."""
    return sorted(header_prototypes(path))


# name -> (restype, argtypes), as include/mgp_hip.h declares them
SIGNATURES = header_prototypes()

_lib = None


def load():
    """Load libmgp_hip.so once (no HIP call is made by loading)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MGPLibraryError(
            f"{LIB_PATH} not found: build it with `python -m modulatedgps_amd.build` "
            "(there is no CPU fallback)")
    try:
        lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_LOCAL)
    except OSError as e:
        raise MGPLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(name, status):
    if status != 0:
        msg = load().mgp_status_string(status).decode()
        raise MGPError(name, status, msg)


def marshal(arg):
    """One argument as ctypes takes it: a tensor (anything with data_ptr()) becomes its
    pointer, a list / tuple of tensors a c_void_p array (None -> NULL); scalars, None
    and ctypes instances pass through.  Nothing is checked here."""
    kind = type(arg)
    if kind is int or kind is float or arg is None:
        return arg
    if kind is list or kind is tuple:
        return (ctypes.c_void_p * len(arg))(*[None if t is None else t.data_ptr() for t in arg])
    data_ptr = getattr(arg, "data_ptr", None)
    return arg if data_ptr is None else data_ptr()


def call(name, *args):
    """Call an int-returning entry point on marshalled arguments (the pointer arrays live
    until it returns) and raise MGPError on failure."""
    check(name, getattr(load(), name)(*[marshal(a) for a in args]))


def call_raw(name, *args):
    """call without the marshalling pass, for arguments that are ints, floats, None and
    ctypes instances already: the wrappers of the ELBO step, whose host time is the step
    time at small sizes, convert their own pointers."""
    check(name, getattr(load(), name)(*args))
