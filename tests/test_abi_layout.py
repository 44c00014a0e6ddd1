"""The hand-written halves of the binding are pinned by the C compiler (no GPU needed): every ctypes.Structure mirror under
dualfusion/ has the size and the field offsets / sizes of the struct it names (`_c_name_`) in include/df3d_hip.h, and the
constants Python repeats have the values of the header's macros.  (The prototypes need no such test: dualfusion/_lib.py
reads them from the header.)"""
import ctypes
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


def _mirrors():
    from dualfusion import executor, ops, prefetch  # noqa: F401  (the modules that define mirrors)
    found, todo = [], list(ctypes.Structure.__subclasses__())
    while todo:
        cls = todo.pop()
        todo.extend(cls.__subclasses__())
        if cls.__module__.split(".")[0] == "dualfusion":
            found.append(cls)
    return sorted(found, key=lambda c: (c.__module__, c.__name__))


def _constants():
    """[(macro, the Python value that repeats it)].  DF3D_MAX_HEAD_TASKS has no Python copy (the library checks it)."""
    from dualfusion import _lib, ops, prefetch
    return [("DF3D_OK", _lib.DF3D_OK), ("DF3D_EINVAL", _lib.DF3D_EINVAL), ("DF3D_ENOMEM", _lib.DF3D_ENOMEM),
            ("DF3D_EHIP", _lib.DF3D_EHIP), ("DF3D_NMS_NORMAL", ops.NMS_NORMAL), ("DF3D_NMS_ROTATED", ops.NMS_ROTATED),
            ("DF3D_NMS_CIRCLE", ops.NMS_CIRCLE), ("DF3D_MAX_ANCHORS", ops.MAX_ANCHORS),
            ("DF3D_LOSS_MAX_CODES", ops.LOSS_MAX_CODES), ("DF3D_LOSS_FIELDS", ops.LOSS_FIELDS),
            ("DF3D_HEAD_MAX_PROJ", prefetch.MAX_PROJ), ("DF3D_CONV_PLAN_FIELDS", ops.CONV_PLAN_FIELDS)]


def _host_cc():
    """cc, else gcc, else the clang next to hipcc (there wherever the library was built)."""
    hip_bin = os.path.dirname(os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")))
    beside = [os.path.join(hip_bin, "clang"), os.path.join(hip_bin, "amdclang"),
              os.path.join(hip_bin, "..", "lib", "llvm", "bin", "clang")]
    tried = ["cc", "gcc"] + beside
    for cand in tried:
        path = shutil.which(cand)
        if path:
            return path
    raise AssertionError("no host C compiler: tried %s" % ", ".join(tried))


def _probe_source(mirrors, constants):
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "df3d_hip.h"', "int main(void) {"]
    for cls in mirrors:
        c = cls._c_name_
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (c, c))
        for field in cls._fields_:
            f = field[0]
            lines.append('  printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (c, f, c, f, c, f))
    for macro, _ in constants:
        lines.append('  printf("%s %%lld\\n", (long long)(%s));' % (macro, macro))
    return "\n".join(lines + ["  return 0;", "}", ""])


def test_struct_mirrors_and_constants_match_the_header(tmp_path):
    mirrors, constants = _mirrors(), _constants()
    unnamed = [c.__module__ + "." + c.__name__ for c in mirrors if not isinstance(c.__dict__.get("_c_name_"), str)]
    assert not unnamed, "ctypes mirrors without _c_name_ (the C struct they repeat): %s" % unnamed
    assert len(mirrors) >= 15 and len(set(c._c_name_ for c in mirrors)) == len(mirrors)
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(_probe_source(mirrors, constants))
    built = subprocess.run([_host_cc(), "-std=c99", "-I", INCLUDE, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert built.returncode == 0, "a mirror names a struct or a field the header does not have:\n" + built.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    c_side = {}
    for line in out.splitlines():
        key, *numbers = line.split()
        c_side[key] = tuple(int(v) for v in numbers)
    wrong = []
    for cls in mirrors:
        c = cls._c_name_
        if c_side[c] != (ctypes.sizeof(cls),):
            wrong.append("sizeof(%s) = %d, %s has %d" % (c, c_side[c][0], cls.__name__, ctypes.sizeof(cls)))
        for field in cls._fields_:
            d = getattr(cls, field[0])
            if c_side["%s.%s" % (c, field[0])] != (d.offset, d.size):
                wrong.append("%s.%s at %d, %d bytes; %s has it at %d, %d bytes"
                             % ((c, field[0]) + c_side["%s.%s" % (c, field[0])] + (cls.__name__, d.offset, d.size)))
    for macro, value in constants:
        if c_side[macro] != (value,):
            wrong.append("%s = %d, Python repeats it as %r" % (macro, c_side[macro][0], value))
    assert not wrong, "\n".join(wrong)
