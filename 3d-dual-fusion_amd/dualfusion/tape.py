"""Launch tape: the C-ABI launches of a FIXED-SHAPE section of the frame, recorded once and re-issued without the
interpreter work around them.

The neck and the detection head run on a dense [B, H, W] map: every launch of theirs has the same sizes, the same weights
and (given persistent buffers) the same addresses for every frame -- only the address of the section's input rows and the
stream change.  A step spends ~0.45 ms of host time on them (module plumbing, argument checks, ~40 allocations and views
around 20 launches); replaying the recorded (function, arguments) list costs ~0.07 ms.  This is the host-side half of what a
hipGraph would give, without capture restrictions: the launches are ordinary launches on the CURRENT stream (so the
library's event timer, the frame-head worker and several frames in flight keep working), and a changed input address is a
patched argument instead of a graph update.

How:  `record()` runs the section once for real while (a) `_lib.load()` hands out a recorder that notes every call whose
last argument is the current stream, (b) every allocation comes from a private `torch.cuda.MemPool` owned by the tape: the
addresses the recorded launches carry stay valid (and are handed to nobody else) for as long as the tape lives.  `replay()`
re-issues the calls with the stream argument and every pointer into an input tensor rewritten.

Contract (opt-in, `CenterPointDetector.launch_tape = True` / DF3D_LAUNCH_TAPE=1): the section's results live in the tape's
buffers -- they are valid until the next replay on this tape (the next frame of this detector), exactly like the outputs of
a replayed hipGraph.  Consumers on the same stream (loss, box decoding, NMS) are ordered by the stream.
"""
import ctypes

import torch
from torch.utils._python_dispatch import TorchDispatchMode

from . import _lib


StreamArg = _lib.StreamArg


class _Recorder(object):
    """Stands in for the ctypes library while a tape records: same attributes, launches are noted."""

    def __init__(self, lib, tape):
        self.__dict__["_lib"], self.__dict__["_tape"] = lib, tape

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        tape = self._tape

        def call(*args):
            rc = fn(*args)
            if args and isinstance(args[-1], StreamArg):
                tape._note(name, fn, args)
            return rc
        return call

    def __setattr__(self, name, value):              # (bench.py's API timer swaps entry points for timed ones)
        setattr(self._lib, name, value)


_FACTORIES = frozenset(("empty", "empty_strided", "empty_like", "new_empty", "new_empty_strided", "detach", "alias",
                        "lift_fresh", "sym_size", "sym_stride", "sym_numel", "sym_storage_offset", "is_pinned", "size",
                        "stride", "numel", "dim", "is_contiguous", "storage_offset", "_has_compatible_shallow_copy_type"))


def _launches_nothing(func):
    """True for ATen operators that neither launch a kernel nor touch device data: allocations and views."""
    packet = getattr(func, "overloadpacket", None)
    if getattr(packet, "__name__", None) in _FACTORIES:
        return True
    rets = func._schema.returns
    return bool(rets) and all(r.alias_info is not None and not r.alias_info.is_write for r in rets)


class _PurityMode(TorchDispatchMode):
    """Notes every ATen operator of a recording that would launch work of its own: such a launch is not on the
    tape, a replay would skip it and read its stale output -- a section that contains one is not taped."""

    def __init__(self):
        super(_PurityMode, self).__init__()
        self.impure = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if not _launches_nothing(func):
            self.impure.append(str(func))
        return func(*args, **(kwargs or {}))


class LaunchTape(object):
    def __init__(self, device):
        self.device = torch.device(device)
        self.pool = torch.cuda.MemPool()
        self.calls = []            # (name, fn, args list, index of the stream argument, [(arg index, input index, offset)])
        self.keep = []             # every tensor whose address a recorded call carries (ops._ptr): alive as long as the tape
        self.result = None
        self.impure = []           # ATen operators the recorded section ran besides the library's launches (must be empty)
        self._ranges = []

    # ------------------------------------------------------------------ record
    def record(self, fn, inputs):
        """Run `fn()` (the section, reading the tensors `inputs`) once, recording its launches; returns its result."""
        if _lib._recorder is not None:
            raise _lib.Df3dError("launch tape: a recording is already in progress")
        self._ranges = [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t in inputs]
        self.calls = []
        self.keep = []
        lib = _lib.load()
        _lib._recorder = _Recorder(lib, self)
        purity = _PurityMode()
        try:
            with torch.cuda.use_mem_pool(self.pool, device=self.device), purity:
                self.result = fn()
        finally:
            _lib._recorder = None
        self.impure = purity.impure
        return self.result

    def _note(self, name, fn, args):
        args = list(args)
        patches = []
        for i, a in enumerate(args[:-1]):
            if isinstance(a, ctypes.c_void_p) and a.value:
                for k, (lo, hi) in enumerate(self._ranges):
                    if lo <= a.value < hi:
                        patches.append((i, k, a.value - lo))
                        args[i] = None                       # always rewritten
        self.calls.append((name, fn, args, len(args) - 1, patches))

    # ------------------------------------------------------------------ replay
    def replay(self, inputs, stream):
        """Re-issue the recorded launches on `stream` (a ctypes pointer) with `inputs` in place of the recorded ones."""
        bases = [t.data_ptr() for t in inputs]
        for name, fn, args, si, patches in self.calls:
            args[si] = stream
            for i, k, off in patches:
                args[i] = bases[k] + off
            fn(*args)
        return self.result


class TapedSection(object):
    """Policy around a LaunchTape: the first call with a key runs the section normally (its lazily built plans, tables and
    packed weights end up in the ordinary allocator), the second records, later ones replay.  `key` must cover everything the
    launches depend on besides the input addresses: shapes, precision mode, parameter versions."""

    def __init__(self):
        self.tapes = {}
        self.retired = []          # tapes of stale keys: their pools are kept (plans built while recording may live there)
        self.stats = {"plain": 0, "recorded": 0, "replayed": 0, "refused": 0}
        self.refused_ops = []      # the operators that made the last recording unusable
        self._live = None          # the key of the last call

    def reset(self):
        self.retired.extend(t for t in self.tapes.values() if isinstance(t, LaunchTape))
        self.tapes = {}

    def run(self, key, fn, inputs, stream):
        if not isinstance(_lib._lib, ctypes.CDLL):
            # a measurement proxy stands in for the library (dualfusion/apitimer.py): it must see every call, and a tape must
            # not record its wrappers
            self.stats["plain"] += 1
            return fn()
        if key != self._live:
            # ONE live key at a time.  A recorded launch carries the addresses of everything the section read besides its
            # input -- packed filters, neighbour tables, plans the modules cache for their CURRENT precision mode / parameter
            # version and replace (free) when that changes.  A tape of an older key would replay with those stale addresses
            # once the key comes back (round 4: bench.py's split -> split3 -> split passes faulted in the pass that followed).
            # A returning key therefore warms up and records again.
            self.reset()
            self._live = key
        slot = self.tapes.get(key)
        if slot is None:
            self.tapes[key] = "warm"
            self.stats["plain"] += 1
            return fn()
        if slot == "plain":                              # this key's section is not pure C-ABI: never replayed
            self.stats["plain"] += 1
            return fn()
        if slot == "warm":
            tape = LaunchTape(inputs[0].device)
            out = tape.record(fn, inputs)
            if tape.impure:
                # the section launched through torch as well (e.g. the neck's torch.cat when its last layers cannot write
                # the concatenated rows in place: bf16 / exact-fp32 modes): a replay would skip those launches.  The result
                # of this (real) run is good; the key runs the module path from now on.
                self.retired.append(tape)
                self.tapes[key] = "plain"
                self.refused_ops = sorted(set(tape.impure))
                self.stats["refused"] += 1
                return out
            self.tapes[key] = tape
            self.stats["recorded"] += 1
            return out
        self.stats["replayed"] += 1
        return slot.replay(inputs, stream)
