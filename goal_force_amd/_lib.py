"""ctypes binding of libgoalforce_hip.so — the C ABI declared in include/goalforce.h.

The product path has NO fallback: if the shared library is missing or an entry point
fails, a GoalForceError is raised (never a silent torch/CPU substitute).
"""
from __future__ import annotations

import ctypes
import os
import re
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgoalforce_hip.so")
# GOALFORCE_HIP_LIB: A/B a differently built libgoalforce_hip.so (kernel tuning); it is still the HIP library, never a fallback
LIB_PATH = os.environ.get("GOALFORCE_HIP_LIB", LIB_PATH)

HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "goalforce.h")

EPI_BIAS, EPI_BIAS_GELU_TANH, EPI_BIAS_GATE_RESID, EPI_BIAS_RESID, EPI_BIAS_SILU, EPI_BIAS_MUL = range(6)


class GoalForceError(RuntimeError):
    """Raised when the HIP library is missing or a gf_* call returns an error."""


# ---- the binding is READ from include/goalforce.h, the file the compiler checks every definition against: the symbol list, each
# entry point's restype / argtypes and the ABI revision have no second copy here.  A new entry point is declared there, defined
# in csrc, and ops.py gets its wrapper; GF_ABI_VERSION is bumped when a signature or a buffer contract changes (a library that only
# lacks a new symbol is caught by load(), with the rebuild hint).  The parser fails closed: a type outside _CTYPES or a GF_API
# line it cannot take apart raises GoalForceError at import — ctypes would accept a wrong row and hand a kernel a shifted pointer.
_CTYPES = {"void": None, "int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "uint32_t": ctypes.c_uint32}
_DECL = re.compile(r"\s+([\w\s*]+?)\s*\b(gf_\w+)\s*\(([^()]*)\)\s*;")


def _ctype(text, decl):
    """The ctypes type of one C type as the header spells it: the scalars of _CTYPES, `const char*` -> c_char_p, any other
    one-level pointer -> c_void_p (which takes None, an integer address and ctypes.byref(...))."""
    words = text.replace("*", " * ").split()
    if words == ["const", "char", "*"]:
        return ctypes.c_char_p
    if words[:1] == ["const"]:
        words = words[1:]
    if len(words) == 2 and words[1] == "*" and words[0].isidentifier():
        return ctypes.c_void_p
    if len(words) != 1 or words[0] not in _CTYPES:
        raise GoalForceError(f"goalforce.h: type {text.strip()!r} in `{decl}` is outside the binding's type map")
    return _CTYPES[words[0]]


def parse_header(text):
    """{name: (restype, [argtypes])} of every `GF_API <ret> gf_name(<params>);` in the text of a goalforce.h, in its order."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)          # the preprocessor lines (GF_API's own #define among them)
    out = {}
    for chunk in re.split(r"\bGF_API\b", text)[1:]:
        m = _DECL.match(chunk)
        if m is None:
            raise GoalForceError(f"goalforce.h: cannot take apart the declaration `GF_API{' '.join(chunk.split())[:100]}`")
        ret, name, params = m.groups()
        decl = " ".join(m.group(0).split())
        if name in out:
            raise GoalForceError(f"goalforce.h: {name} is declared twice")
        argtypes = []
        if params.strip() != "void":
            for p in params.split(","):
                pm = re.fullmatch(r"\s*(.*?[\s*])(\w+)\s*", p, flags=re.S)     # <type> <parameter name>
                if pm is None:
                    raise GoalForceError(f"goalforce.h: parameter {p.strip()!r} of `{decl}` is not `<type> <name>`")
                argtypes.append(_ctype(pm.group(1), decl))
                if argtypes[-1] is None:
                    raise GoalForceError(f"goalforce.h: a void parameter in `{decl}`")
        out[name] = (_ctype(ret, decl), argtypes)
    return out


def _read_header():
    try:
        with open(HEADER_PATH, encoding="utf-8") as f:
            text = f.read()
    except OSError as e:
        raise GoalForceError(f"{HEADER_PATH}: the C ABI's header, which these bindings are read from, cannot be read ({e})") from e
    rev = re.findall(r"^#define GF_ABI_VERSION (\d+)\s*$", text, flags=re.M)
    if len(rev) != 1:
        raise GoalForceError(f"{HEADER_PATH}: expected exactly one `#define GF_ABI_VERSION <n>`, found {len(rev)}")
    return parse_header(text), int(rev[0])


# BINDINGS: every entry point the header declares; ABI_VERSION: the C ABI revision it states (gf_abi_version() of a library built
# from it).  A stale or foreign .so whose entry points take differently sized buffers (gf_flash_attn_bwd's workspace grew 3x
# between revisions 7 and 10 under an unchanged signature) is refused at load time instead of overrunning memory.
BINDINGS, ABI_VERSION = _read_header()
SYMBOLS = tuple(BINDINGS)       # tests check the .so exports exactly these

_lib = None
_lock = threading.Lock()


def _declare(lib):
    for name, (restype, argtypes) in BINDINGS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes


def load():
    """Load (once) and return the ctypes handle; raises GoalForceError if the .so is absent."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            # torch ships its own libamdhip64.so.7; import it FIRST so this library binds to the same HIP
            # runtime instance (two runtimes in one process cannot both see the device).
            import torch  # noqa: F401
            if not os.path.exists(LIB_PATH):
                raise GoalForceError(
                    f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                    "or `make -C goal_force_amd/csrc` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
            try:
                lib = ctypes.CDLL(LIB_PATH)
            except OSError as e:  # pragma: no cover
                raise GoalForceError(f"cannot load {LIB_PATH}: {e}") from e
            # the revision is compared BEFORE the symbols are bound: a stale build usually lacks a symbol, and the rebuild hint
            # must reach the user instead of a bare AttributeError out of _declare
            rebuild = "rebuild the library (`make -C goal_force_amd/csrc`)"
            try:
                lib.gf_abi_version.restype = ctypes.c_int
                have = int(lib.gf_abi_version())
            except AttributeError as e:
                raise GoalForceError(f"{LIB_PATH} predates the C ABI revision export: {rebuild}") from e
            if have != ABI_VERSION:
                raise GoalForceError(f"{LIB_PATH} speaks C ABI revision {have}, these bindings revision {ABI_VERSION}: {rebuild} "
                                     "— mixing revisions can overrun caller-owned workspaces")
            try:
                _declare(lib)
            except AttributeError as e:
                raise GoalForceError(f"{LIB_PATH} lacks a symbol these bindings declare ({e}): {rebuild}") from e
            _lib = lib
    return _lib


def check(status: int, what: str):
    if status != 0:
        msg = load().gf_last_error().decode("utf-8", "replace")
        raise GoalForceError(f"{what} failed with status {status}: {msg}")


def version() -> str:
    return load().gf_version().decode()
