"""Guarded device memory for the memory-contract tests (tests/test_gpu_memory_contract.py; tests/test_guarded_host.py
proves on the CPU that every check here can fail).  A plain helper module: nothing is registered with pytest.

Arena: one uint8 tensor filled with a guard byte, carved into regions.  Every region is a contiguous view whose first byte
sits `offset` bytes past a 256-byte boundary, filled with a poison byte (empty) or with a tensor's contents (place), with
a guard band on both sides; check() reads every band back.  A band is as wide as its buffer, at least 4 KiB and at most
1 MiB -- a contiguous overrun of up to the buffer's own size stays inside memory the arena owns -- and the arena ends in
one, since the last region's upper band has to fit.

patched(engine, arena): swaps the module globals engine.torch and engine.lib for proxies, so that every tensor the engine
allocates on the arena's device comes out of the arena (empty*: poisoned; zeros / full: their defined value) and every
library call is recorded by symbol name.  Nothing in the package changes for it.

SETTINGS: the three (poison, guard) byte pairs the tests run under.  Both bytes differ between any two settings, so a
result that depends on a byte the callee never wrote (stale data) or on a byte outside an input (a read out of bounds)
differs between them: differing_output() finds it.  0xFF is the nasty poison: NaN in float32 / float64 buffers, -1 in
counters, 255 in validity bytes."""
import contextlib

import numpy as np
import torch

SETTINGS = ((0x00, 0xFF), (0xFF, 0x00), (0x5A, 0xA5))
ALIGN = 256
GUARD_MIN, GUARD_MAX = 4096, 1 << 20


class GuardError(AssertionError):
    """A guard byte changed: label of the region, side ("before" / "after"), byte offset relative to the view's start."""

    def __init__(self, label, side, offset, found, guard):
        super().__init__(f"{label}: guard {side} the buffer damaged, first at byte offset {offset} relative to the buffer's "
                         f"start (found 0x{found:02X}, guard 0x{guard:02X})")
        self.label, self.side, self.offset = label, side, offset


class StaleError(AssertionError):
    """An output's bits depend on the (poison, guard) setting."""


def guard_width(nbytes):
    return min(max(int(nbytes), GUARD_MIN), GUARD_MAX)


def _same_device(a, b):
    a, b = torch.device(a), torch.device(b)
    if a.type != b.type:
        return False
    if a.type != "cuda" or a.index is None or b.index is None:
        return True            # ("cuda" is the current device: the tests run on one)
    return a.index == b.index


class Arena:
    def __init__(self, device, poison, guard, capacity=1 << 26):
        self.device = torch.device(device)
        self.poison, self.guard = int(poison), int(guard)
        if not (0 <= self.poison <= 255 and 0 <= self.guard <= 255) or self.poison == self.guard:
            raise ValueError("poison and guard are two different byte values")
        self.buf = torch.full((int(capacity) + ALIGN,), self.guard, dtype=torch.uint8, device=self.device)
        self._base = (-self.buf.data_ptr()) % ALIGN      # buf[_base] sits on a 256-byte boundary
        self._end = self._base + int(capacity)
        self._cursor = self._base
        self.regions = []                                # (label, band start, data start, data end, band end)

    # ---- carving
    def _carve(self, shape, dtype, offset, label):
        if isinstance(shape, (int, np.integer)):
            shape = (int(shape),)
        shape = tuple(int(s) for s in shape)
        item = torch.empty((), dtype=dtype).element_size()
        if not 0 <= offset < ALIGN:
            raise ValueError(f"offset must lie in 0..{ALIGN - 1}, got {offset}")
        if dtype != torch.uint8 and offset % item:
            raise ValueError(f"offset {offset} is no multiple of the size of {dtype} ({item})")
        nbytes = item * int(np.prod(shape, dtype=np.int64))
        g = guard_width(nbytes)
        lo = self._cursor
        start = lo + g
        start += (-(start - self._base)) % ALIGN + offset
        stop = start + nbytes
        if stop + g > self._end:
            raise MemoryError(f"arena of {self._end - self._base} bytes is full: {label or 'buffer'} needs {nbytes} bytes "
                              f"and {g} bytes of guard behind it")
        self._cursor = stop + g
        label = label or f"buffer {len(self.regions)} {dtype} {list(shape)}"
        self.regions.append((label, lo, start, stop, stop + g))
        flat = self.buf[start:stop]
        view = (flat if dtype == torch.uint8 else flat.view(dtype)).view(shape)
        assert view.data_ptr() % ALIGN == offset and view.is_contiguous()
        return view, flat

    def empty(self, shape, dtype, offset=0, label=None):
        """A contiguous view of `shape`, every byte the poison."""
        view, flat = self._carve(shape, dtype, offset, label)
        flat.fill_(self.poison)
        return view

    def place(self, tensor, offset=0, label=None):
        """A contiguous copy of `tensor` (a tensor of any device, or a numpy array) inside the arena."""
        if isinstance(tensor, np.ndarray):
            tensor = torch.from_numpy(np.array(tensor))          # (a copy: the source may be read-only)
        view, _ = self._carve(tuple(tensor.shape), tensor.dtype, offset, label)
        view.copy_(tensor)
        return view

    def filled(self, shape, dtype, value, label=None):
        """A view with a defined value (what torch.zeros / torch.full promise)."""
        view, _ = self._carve(shape, dtype, 0, label)
        view.fill_(value)
        return view

    # ---- checking
    @property
    def guard_bytes(self):
        return sum((start - lo) + (hi - stop) for _, lo, start, stop, hi in self.regions)

    def check(self):
        """Reads every guard byte (on the arena's device); GuardError for the first damaged one."""
        for label, lo, start, stop, hi in self.regions:
            for side, s, e in (("before", lo, start), ("after", stop, hi)):
                bad = self.buf[s:e] != self.guard
                if bool(bad.any()):
                    i = int(bad.nonzero()[0, 0])
                    raise GuardError(label, side, s + i - start, int(self.buf[s + i]), self.guard)

    def holds_poison(self, view):
        """Is every byte of `view` (a contiguous tensor) still the poison?"""
        flat = view.reshape(-1)
        flat = flat if flat.dtype == torch.uint8 else flat.view(torch.uint8)
        return bool((flat == self.poison).all())


# ---- proxies

class Calls(set):
    """The symbol names called through a LibProxy."""


class LibProxy:
    """Forwards every call to the library and records the symbol's name."""

    def __init__(self, real, calls):
        self.__dict__["_real"], self.__dict__["_calls"] = real, calls

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not callable(fn):
            return fn
        calls = self._calls

        def call(*args):
            calls.add(name)
            return fn(*args)
        call.__name__ = name
        return call


class TorchProxy:
    """torch, except that empty, empty_like, zeros, zeros_like and full on the arena's device allocate from the arena."""

    def __init__(self, real, arena):
        self.__dict__["_real"], self.__dict__["_arena"] = real, arena

    def __getattr__(self, name):
        return getattr(self._real, name)

    def _mine(self, device):
        return device is not None and _same_device(device, self._arena.device)

    @staticmethod
    def _shape(size):
        if len(size) == 1 and not isinstance(size[0], (int, np.integer)):
            return tuple(size[0])
        return tuple(size)

    def _dtype(self, dtype):
        return self._real.get_default_dtype() if dtype is None else dtype

    def empty(self, *size, dtype=None, device=None, **kw):
        if not self._mine(device) or kw:
            return self._real.empty(*size, dtype=dtype, device=device, **kw)
        return self._arena.empty(self._shape(size), self._dtype(dtype))

    def zeros(self, *size, dtype=None, device=None, **kw):
        if not self._mine(device) or kw:
            return self._real.zeros(*size, dtype=dtype, device=device, **kw)
        return self._arena.filled(self._shape(size), self._dtype(dtype), 0)

    def full(self, size, fill_value, dtype=None, device=None, **kw):
        if not self._mine(device) or kw or dtype is None:
            return self._real.full(size, fill_value, dtype=dtype, device=device, **kw)
        return self._arena.filled(self._shape((size,)), dtype, fill_value)

    def empty_like(self, t, **kw):
        if not self._mine(kw.get("device", t.device)) or set(kw) - {"dtype", "device"}:
            return self._real.empty_like(t, **kw)
        return self._arena.empty(tuple(t.shape), kw.get("dtype", t.dtype))

    def zeros_like(self, t, **kw):
        if not self._mine(kw.get("device", t.device)) or set(kw) - {"dtype", "device"}:
            return self._real.zeros_like(t, **kw)
        return self._arena.filled(tuple(t.shape), kw.get("dtype", t.dtype), 0)


@contextlib.contextmanager
def patched(engine, arena, calls=None):
    """Inside the block engine.torch and engine.lib are the proxies; yields the Calls set the library proxy fills (the
    one handed in, or a fresh one).  The real modules are back afterwards, whatever happened inside."""
    calls = Calls() if calls is None else calls
    real_torch, real_lib = engine.torch, engine.lib
    engine.torch, engine.lib = TorchProxy(real_torch, arena), LibProxy(real_lib, calls)
    try:
        yield calls
    finally:
        engine.torch, engine.lib = real_torch, real_lib


# ---- bit comparison

def bits(t):
    """The bytes of a tensor as a numpy uint8 vector (integer view: NaN payloads and signed zeros count)."""
    t = t.detach().contiguous().reshape(-1)
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    return (t if t.dtype == torch.uint8 else t.view(torch.uint8)).cpu().numpy().copy()


def first_difference(a, b):
    """None if two byte vectors are identical, else the first byte index at which they differ (the shorter length if one is
    a prefix of the other)."""
    if a.shape != b.shape:
        n = min(a.size, b.size)
        d = np.flatnonzero(a[:n] != b[:n])
        return int(d[0]) if d.size else n
    d = np.flatnonzero(a != b)
    return int(d[0]) if d.size else None


def differing_output(runs, names=None):
    """runs: one list of byte vectors (bits() of every output, defined part) per setting.  StaleError naming the first
    output whose bytes differ between the first setting and another: a cell the callee left unwritten, or a read outside an
    input that reached the result."""
    for s, run in enumerate(runs[1:], 1):
        if len(run) != len(runs[0]):
            raise StaleError(f"setting {s} returned {len(run)} outputs, setting 0 {len(runs[0])}")
        for k, (x, y) in enumerate(zip(runs[0], run)):
            i = first_difference(x, y)
            if i is not None:
                name = names[k] if names else f"output {k}"
                raise StaleError(f"{name} depends on the memory around it: byte {i} is "
                                 f"0x{int(x[i]) if i < x.size else -1:02X} under (poison, guard) = "
                                 f"{tuple(hex(q) for q in SETTINGS[0])} and 0x{int(y[i]) if i < y.size else -1:02X} under "
                                 f"{tuple(hex(q) for q in SETTINGS[s])}")


def run_one(device, setting, build, call, select=None, capacity=1 << 26, engine=None, calls=None, offset=0):
    """One guarded run: an Arena of the (poison, guard) setting, the inputs of build() placed in it (numpy arrays and
    tensors of a dict; other values pass through; `offset` applies to uint8 / uint16 inputs whose name starts with
    "frame"), call(inputs, arena) run -- inside patched(engine, arena) when an engine is given --, the guards checked.
    Returns (run, arena, outputs): run = [bits(t) for the outputs select(outputs, inputs) keeps], for differing_output."""
    arena = Arena(device, setting[0], setting[1], capacity)
    inputs = place_inputs(arena, build(), offset)
    if engine is None:
        out = call(inputs, arena)
    else:
        with patched(engine, arena, calls):
            out = call(inputs, arena)
    out = tuple(out) if isinstance(out, (tuple, list)) else (out,)
    arena.check()
    sel = select(out, inputs) if select else out
    return [bits(t) for t in sel if t is not None], arena, out


def run_settings(device, build, call, **kw):
    """The driver of sections (a) and (b): run_one under every setting.  Returns (runs, arenas, outputs), one entry per
    setting."""
    got = [run_one(device, s, build, call, **kw) for s in SETTINGS]
    return [g[0] for g in got], [g[1] for g in got], [g[2] for g in got]


def place_inputs(arena, inputs, offset=0):
    placed = {}
    for name, val in inputs.items():
        if isinstance(val, (np.ndarray, torch.Tensor)):
            t = torch.from_numpy(np.array(val)) if isinstance(val, np.ndarray) else val
            off = offset if name.startswith("frame") and t.element_size() <= 2 else 0
            placed[name] = arena.place(t, off, label=f"input {name}")
        else:
            placed[name] = val
    return placed
