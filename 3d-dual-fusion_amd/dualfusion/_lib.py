"""ctypes binding of libdf3d_hip.so (the C ABI declared in include/df3d_hip.h).

The product path has NO CPU fallback: if the HIP library is missing or cannot be loaded
every op raises.  (The CPU restatement in oracle/ is test infrastructure and is never
imported from here.)
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "csrc", "libdf3d_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "..", "include", "df3d_hip.h")

c_int = ctypes.c_int
c_float = ctypes.c_float
c_void_p = ctypes.c_void_p

DF3D_OK, DF3D_EINVAL, DF3D_ENOMEM, DF3D_EHIP = 0, -1, -2, -3      # include/df3d_hip.h (pinned by tests/test_abi_layout.py)


class Df3dError(RuntimeError):
    """.rc / .entry: the status and the entry point, when the error is a refused library call."""
    rc = entry = None


# ---- the prototypes come from the header: a new entry point needs its declaration there and nothing here
_SCALARS = {
    "int": c_int, "int32_t": c_int,
    "unsigned": ctypes.c_uint, "unsigned int": ctypes.c_uint, "uint32_t": ctypes.c_uint,
    "long long": ctypes.c_longlong, "int64_t": ctypes.c_longlong,
    "unsigned long long": ctypes.c_ulonglong, "uint64_t": ctypes.c_ulonglong,
    "size_t": ctypes.c_size_t, "float": c_float, "double": ctypes.c_double,
}
_PROTOTYPE = re.compile(r"([\w\s*]+?)\b(df3d_\w+)\s*\(([^()]*)\)")


def _ctype(text, named, decl):
    """One return or parameter type.  Anything with `*` or `[]` is a pointer (c_void_p; `char *` is c_char_p); everything
    else must be one of _SCALARS.  Never guessed: what is neither raises, naming the declaration."""
    words = [w for w in re.sub(r"\[[^\]]*\]|\*", " ", text).split() if w != "const"]
    if named and len(words) > 1 and " ".join(words) not in _SCALARS:
        words.pop()                                  # the parameter's name
    base = " ".join(words)
    if base and ("*" in text or "[" in text):
        return ctypes.c_char_p if base == "char" and text.count("*") == 1 and "[" not in text else c_void_p
    if base not in _SCALARS:
        raise Df3dError("df3d_hip.h: cannot bind %r of %r" % (" ".join(text.split()), decl))
    return _SCALARS[base]


def parse_header(text):
    """C header text -> {name: (restype, argtypes)} of every `<ret> df3d_<name>(<params>);`.  Comments, preprocessor lines,
    the extern "C" braces and struct typedefs are dropped; whatever else is left must be such a prototype."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    text = re.sub(r"typedef\s+struct\s+\w*\s*\{[^{}]*\}\s*\w+\s*;", " ", text)
    table = {}
    for decl in text.split(";"):
        decl = " ".join(decl.split())
        if decl in ("", "}"):                        # (the closing brace of extern "C")
            continue
        m = _PROTOTYPE.fullmatch(decl)
        if m is None or m.group(2) in table:
            raise Df3dError("df3d_hip.h: not a df3d_ prototype, or declared twice: %r" % decl)
        ret, name, params = m.groups()
        params = [] if params.strip() in ("", "void") else params.split(",")
        table[name] = (_ctype(ret, False, decl), [_ctype(p, True, decl) for p in params])
    return table


def _read_header():
    if not os.path.exists(HEADER_PATH):
        raise Df3dError("the C header %s is missing: the binding of libdf3d_hip.so is made from it" % HEADER_PATH)
    with open(HEADER_PATH) as f:
        return parse_header(f.read())


SIGNATURES = _read_header()     # name -> (restype, argtypes)

_lib = None


class StreamArg(c_void_p):
    """What ops._stream() passes as the stream of a launch: lets a recording launch tape (dualfusion/tape.py) tell launches
    from queries and find the argument to rewrite."""


_recorder = None        # dualfusion/tape.py: stands in for the library while a launch tape records


def bind(handle, check=True):
    """Give every entry point of SIGNATURES on the ctypes.CDLL `handle` its restype / argtypes (AttributeError if a declared
    symbol is not exported) and return the handle.  check: every entry that returns `int` raises Df3dError on a negative
    result (the header's convention; a result >= 0 is a status or a value and is passed through)."""
    last_error = handle.df3d_last_error

    def errcheck(rc, fn, args):
        if rc < 0:
            msg = last_error()
            e = Df3dError("%s failed (rc=%d): %s" % (fn.__name__, rc, msg.decode() if msg else "?"))
            e.rc, e.entry = rc, fn.__name__
            raise e
        return rc

    for name, (res, args) in SIGNATURES.items():
        fn = getattr(handle, name)
        fn.restype = res
        fn.argtypes = args
        if check and res is c_int:
            fn.errcheck = errcheck
    return handle


def load():
    """Load (once) and return the ctypes handle.  Raises loudly when the library is absent."""
    global _lib
    if _recorder is not None:
        return _recorder
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise Df3dError(
            "libdf3d_hip.so not found at %s: build it with `python __graft_entry__.py build` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback on the product path." % LIB_PATH)
    _lib = bind(ctypes.CDLL(LIB_PATH))
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = load().df3d_last_error()
        raise Df3dError("%s failed (rc=%d): %s" % (what or "df3d call", rc, msg.decode() if msg else "?"))


def int3(v):
    """host int[3] argument"""
    arr = (c_int * 3)(*[int(x) for x in v])
    return ctypes.cast(arr, c_void_p), arr  # keep `arr` alive in the caller


def float_arr(v):
    arr = (c_float * len(v))(*[float(x) for x in v])
    return ctypes.cast(arr, c_void_p), arr
