"""ctypes binding of include/tf_msda.h and include/tf_fused.h (libtf_msda.so).

This is the only place the package touches the native library.  There is deliberately no fallback:
if the library is missing, `lib()` raises, and so does every operator built on it.

The headers are the only declaration of the ABI: the names, the argument and return types and the ABI version are
read from them (`signatures`, `bind`).  Only the two structs are restated here; tests/test_cabi.py compares them.
"""
import ctypes
import os
import re

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TF_MSDA_LIB") or os.path.join(_PKG_DIR, "lib", "libtf_msda.so")

INCLUDE_DIR = os.path.join(os.path.dirname(_PKG_DIR), "include")

_lib = None


class ProjGroup(ctypes.Structure):
    """tf_proj_group of include/tf_fused.h (tf_linear_groups_f32)."""
    _fields_ = [("w_packed", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("y", ctypes.c_void_p), ("N", ctypes.c_int),
                ("add_x2", ctypes.c_int)]


class GnLevel(ctypes.Structure):
    """tf_gn_level of include/tf_fused.h (tf_groupnorm_levels_nhwc_f32)."""
    _fields_ = [("src", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("gamma", ctypes.c_void_p), ("beta", ctypes.c_void_p),
                ("pieces", ctypes.c_int), ("HW", ctypes.c_int), ("row0", ctypes.c_int64)]


class MSDAError(RuntimeError):
    """Raised when libtf_msda.so reports a non-zero status."""


_SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double}
_POINTERS = {"const char *": ctypes.c_char_p, "const tf_proj_group *": ctypes.POINTER(ProjGroup),
             "const tf_gn_level *": ctypes.POINTER(GnLevel)}
_PROTOTYPE = re.compile(r"([\w\s*]+?)\b(tf_[a-z0-9_]+)\s*\(([^()]*)\)\s*;")


def _ctype(c_type, func, is_return=False):
    """The ctypes type of a C type as the headers spell it.  Anything the rule does not name raises: a guess would pass
    wrong values silently."""
    t = " ".join(c_type.replace("*", " * ").split())
    if t in _SCALARS:
        return _SCALARS[t]
    if t in _POINTERS:
        return _POINTERS[t]
    if is_return and t == "void":
        return None
    if not is_return and re.fullmatch(r"(const )?(unsigned )?\w+ \*", t):
        return ctypes.c_void_p
    raise TypeError("%s: no ctypes binding for the %s type '%s'" % (func, "return" if is_return else "parameter", t))


def parse_prototypes(text):
    """{name: (restype, argtypes)} of every `tf_*` function prototype in the text of a C header."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)
    out = {}
    for ret, name, params in _PROTOTYPE.findall(text):
        params = " ".join(params.split())
        argtypes = []
        if params != "void":
            for decl in params.split(","):
                m = re.fullmatch(r"(.*[\s*])(\w+)", decl.strip())   # the type, then the parameter's name
                if m is None:
                    raise TypeError("%s: cannot read the parameter '%s'" % (name, decl.strip()))
                argtypes.append(_ctype(m.group(1), name))
        out[name] = (_ctype(ret, name, is_return=True), argtypes)
    return out


def _header_text():
    if not os.path.isdir(INCLUDE_DIR):
        raise RuntimeError("trackformer_amd: %s not found; the headers in it are the only declaration of the C ABI "
                           "(the package runs from its source tree)" % INCLUDE_DIR)
    return "\n".join(open(os.path.join(INCLUDE_DIR, h)).read() for h in sorted(os.listdir(INCLUDE_DIR)) if h.endswith(".h"))


_HEADER_TEXT = _header_text()
_SIGNATURES = parse_prototypes(_HEADER_TEXT)
EXPORTED_SYMBOLS = tuple(_SIGNATURES)
ABI_VERSION = int(re.search(r"^#define\s+TF_MSDA_ABI_VERSION\s+(\d+)", _HEADER_TEXT, flags=re.M).group(1))


def signatures():
    """{name: (restype, argtypes)} of every function include/*.h declares."""
    return _SIGNATURES


def bind(L):
    """Sets restype / argtypes of every declared function that the loaded library `L` exports (the emulated build of the
    same ABI leaves some out); returns L."""
    for name, (restype, argtypes) in _SIGNATURES.items():
        fn = getattr(L, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    return L


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "trackformer_amd: native library %s not found. Build it with "
            "`python -m trackformer_amd.build` (needs hipcc); there is no CPU fallback." % LIB_PATH)
    # PyTorch-ROCm bundles its own HIP runtime (torch/lib/libamdhip64.so, soname libamdhip64.so.7).
    # It must be the one already mapped when libtf_msda.so is loaded, otherwise the process ends up
    # with two HIP runtimes and torch's streams / device pointers mean nothing to ours.
    import torch  # noqa: F401
    L = bind(ctypes.CDLL(LIB_PATH))
    if L.tf_msda_abi_version() != ABI_VERSION:
        raise RuntimeError("libtf_msda.so ABI version %d != expected %d (rebuild)" %
                           (L.tf_msda_abi_version(), ABI_VERSION))
    _lib = L
    return _lib


def check(status, what):
    if status != 0:
        L = lib()
        msg = L.tf_msda_strerror(status).decode()
        raise MSDAError("%s failed: %s (status %d, hipError %d)" %
                        (what, msg, status, L.tf_msda_last_hip_error()))
