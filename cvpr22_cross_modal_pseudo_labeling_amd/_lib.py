"""ctypes binding of libovis_hip.so (C ABI: include/ovis_hip.h).  No torch types cross it.

The header is the single source of the binding: every ``.hip`` file includes it, so the compiler checks each definition
against its declaration, and ``parse_header`` below turns the same declarations into the ``(restype, argtypes)`` table
and the ``OVIS_*`` constants at import.  It reads only the subset of C the two headers (this one and include/ovis_cpu.h)
use, and raises on anything else -- a type it does not know is never given a default.  Both libraries are built in-tree
by csrc/Makefile, so the headers are found in the checkout's ``include/``."""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libovis_hip.so")
INCLUDE_DIR = os.path.join(os.path.dirname(_HERE), "include")

_BY_VALUE = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double,
             "size_t": ctypes.c_size_t, "uint64_t": ctypes.c_uint64}
_POINTEES = {"void", "float", "double", "int32_t", "int64_t", "uint32_t", "uint64_t", "uint8_t"}


def _ctype(decl, where, is_return=False):
    """The ctypes type of one parameter (``const float* const* boxes``, ``float mean[3]``, ``long m``) or return type."""
    tokens = [t[0] if t[0] in "*[" else t for t in re.findall(r"\*|\[\d*\]|\w+", decl)]
    words = [t for t in tokens if t not in ("*", "[", "const")]
    # nothing but those tokens; at most the type and, for a parameter, its name
    if re.sub(r"\*|\[\d*\]|\w+|\s", "", decl) or not words or len(words) > (1 if is_return else 2):
        raise TypeError(f"{where}: cannot read '{decl.strip()}'")
    base, pointer = words[0], "*" in tokens or "[" in tokens
    if not pointer and base in _BY_VALUE:
        return _BY_VALUE[base]
    if pointer and is_return and base == "char":
        return ctypes.c_char_p
    if pointer and not is_return and base in _POINTEES:
        return ctypes.c_void_p
    raise TypeError(f"{where}: type '{decl.strip()}' is outside the vocabulary of the binding")


def parse_header(text):
    """-> ({name: (restype, argtypes)} of every ``ovis_*`` prototype, {name: value} of every integer ``#define OVIS_*``).
    Anything that is left over once comments, preprocessor lines, the ``extern "C"`` braces and the prototypes are taken
    out raises: a declaration this parser cannot read is never skipped."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants = {m[1]: int(m[2]) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(OVIS_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    signatures = {}

    def take(m):
        name = m[2]
        params = [] if m[3].strip() in ("", "void") else m[3].split(",")
        signatures[name] = (_ctype(m[1], f"{name}: return type", True),
                            [_ctype(p, f"{name}: parameter {i}") for i, p in enumerate(params)])
        return " "

    rest = re.sub(r"([\w\s*]+?)\b(ovis_\w+)\s*\(([^()]*)\)\s*;", take, text)
    rest = re.sub(r'extern\s+"C"\s*\{|\}', " ", rest).strip()
    if rest:
        raise TypeError(f"header text the binding cannot read: '{rest[:80]}'")
    return signatures, constants


def read_header(name):
    path = os.path.join(INCLUDE_DIR, name)
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: the binding of the native libraries is derived from it")
    with open(path) as f:
        return parse_header(f.read())


def bind(path, signatures):
    lib = ctypes.CDLL(path)
    for name, (res, args) in signatures.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


# name -> (restype, argtypes) of every symbol include/ovis_hip.h declares, and its constants as OVIS_OK, OVIS_ERANGE,
# OVIS_BOX_DECODE_MAX_IMAGES, ... attributes of this module
SIGNATURES, CONSTANTS = read_header("ovis_hip.h")
globals().update(CONSTANTS)
_ERRORS = {CONSTANTS[name]: f"{name} ({text})" for name, text in (
    ("OVIS_EINVAL", "bad size or null pointer"), ("OVIS_ENOSPC", "workspace too small"),
    ("OVIS_ERANGE", "problem size not supported by the kernel"))}

_lib = None


def load():
    """Load the HIP library; fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build the HIP extension first "
                "(make -C cvpr22_cross_modal_pseudo_labeling_amd/csrc). There is no CPU fallback.")
        _lib = bind(LIB_PATH, SIGNATURES)
    return _lib


def check(rc, what):
    if rc == OVIS_OK:  # noqa: F821 -- from the header
        return
    if rc < 0:
        raise RuntimeError(f"{what}: {_ERRORS.get(rc, rc)}")
    raise RuntimeError(f"{what}: HIP error {rc}")
