"""ctypes binding of libsplat_hip.so, built at import from include/splat_hip.h: the header is the only place where the C ABI is
declared.  Every struct of the header becomes a ctypes.Structure of the same name here, every integer #define and enumerator a
module constant, every prototype an entry of SIGNATURES (splat_slam_amd/_cdecl.py reads the header; a declaration it does not
understand fails the import).

There is deliberately no fallback: if the HIP library is missing or cannot be loaded the import of the
product path fails with a clear error (a silent CPU path would void every parity claim).
"""
import ctypes as C
import keyword
import os

from splat_slam_amd import _cdecl

_HERE = os.path.dirname(os.path.abspath(__file__))
# (SPLAT_HIP_LIB: another BUILD of the same library, for A/B measurements of kernel changes -- scripts/micro/ab_hash.py)
LIB_PATH = os.environ.get("SPLAT_HIP_LIB") or os.path.join(_HERE, "lib", "libsplat_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "splat_hip.h")      # where build.py takes it from

try:
    with open(HEADER_PATH) as _f:
        HEADER = _cdecl.parse(_f.read(), os.path.basename(HEADER_PATH))
except OSError as e:
    raise ImportError(f"{HEADER_PATH} is missing ({e}): the ctypes binding of libsplat_hip.so is generated from it") from e

_SCALARS = {"float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "int": C.c_int, "char": C.c_char,
            **{f"{u}int{b}_t": getattr(C, f"c_{u}int{b}") for u in ("", "u") for b in (8, 16, 32, 64)}}
assert set(_SCALARS) == set(_cdecl.SCALARS)


def _ctype(t, parameter=False):
    """The ctypes type of a field or parameter, decided by its declaration alone.  A pointer to a struct keeps its type; a pointer
    to a scalar or to void is a plain address (device memory, assigned from tensor.data_ptr()) unless the header marks it SGR_HOST:
    then it keeps its element type, so that ctypes arrays and byref() fit and a struct field keeps the assigned array alive."""
    base = globals().get(t.base) if t.base in HEADER.structs else _SCALARS.get(t.base)
    if t.pointer or (parameter and t.array is not None):
        c = C.POINTER(base) if t.base in HEADER.structs or t.host else C.c_void_p
        return c if parameter or t.array is None else c * t.array
    return base if t.array is None else base * t.array


def _restype(t):
    if t.base == "char" and t.pointer:
        return C.c_char_p
    return None if t.base == "void" and not t.pointer else _ctype(t)


def _py(name):
    return name + "_" if keyword.iskeyword(name) else name          # the C field `in` is `in_`


globals().update(HEADER.constants)
for _name, _fields in HEADER.structs.items():
    globals()[_name] = type(_name, (C.Structure,), {"_fields_": [(_py(f), _ctype(t)) for f, t in _fields]})
# name -> (restype, argtypes) of every function the header declares
SIGNATURES = {name: (_restype(res), [_ctype(t, True) for t in args]) for name, (res, args) in HEADER.functions.items()}


def _names(prefix, names):
    return {n: HEADER.constants[prefix + n.upper()] for n in names}


# what the Python layers may ask for by name (the remaining SGR_UPDATE_ACT_* are internal to sgr_update_forward)
SGR_UPDATE_ACTS = _names("SGR_UPDATE_ACT_", ("none", "relu", "sigmoid", "tanh"))
SGR_ENCODER_ACTS = _names("SGR_ENCODER_ACT_", ("none", "relu", "split"))
SGR_RESNET_ACTS = _names("SGR_RESNET_ACT_", ("none", "relu"))
SGR_VIT_EPI = _names("SGR_VIT_EPI_", ("store_f16", "gelu_f16", "residual", "readout", "embed", "store_f32"))
SGR_ENCODER_LAUNCHES = {HEADER.constants["SGR_ENCODER_NORM_" + n]: HEADER.constants["SGR_ENCODER_LAUNCHES_" + n]
                        for n in ("NONE", "INSTANCE")}      # by norm

_lib = None


def lib():
    """Loads (once) and returns the ctypes handle.  Raises, never falls back."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). splat_slam_amd has no CPU fallback by design.")
        # The caller's device memory and streams are torch's: load torch FIRST so that this process ends up with ONE HIP
        # runtime (torch's bundled libamdhip64). Loading /opt/rocm's copy first gives a second runtime that cannot see
        # the device ("no ROCm-capable device is detected").
        import torch  # noqa: F401
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(h, name)
            fn.restype = res
            fn.argtypes = args
        if h.sgr_abi_version() != HEADER.constants["SGR_ABI_VERSION"]:
            raise ImportError("libsplat_hip.so ABI version mismatch")
        _lib = h
    return _lib


def last_error():
    return lib().sgr_last_error().decode()


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {last_error()}")


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()
