"""Poisoned scratch: make every byte a kernel did not write itself visible in the result.

Every fused entry point carves an `ops.Workspace` buffer into activations, statistics partials, seam planes, coefficient
records and exponent partials, and every output and most stage-level scratch comes from `torch.empty`.  A slot that a
call reads without having written it holds whatever the allocator or the previous call left there -- usually the right
number from one call earlier.  The helpers here take that luck away:

  * `PoisonWorkspace` is an `ops.Workspace` whose `get()` fills the WHOLE buffer it hands out with one byte, on every
    call and on the current stream, and counts its calls;
  * `poisoned_empty(byte)` is a context manager that wraps `torch.empty` and `torch.empty_like` so that every CUDA
    tensor they return is filled with the byte first (everything else passes through), counts the tensors it filled and
    puts the originals back on exit, also after an exception;
  * `install(module, byte)` puts a `PoisonWorkspace` in place of `module._ws` (DISTS, ADISTS -- the A-DISTS module is
    the one `pair` takes its scratch from) and returns it; `poisoned(byte, *modules)` is the two together and yields a
    `Poison` record of the counters, whose `require()` fails a test that reached neither hook.

0xFF is NaN in half, bfloat16, float, double and in split16 records, 255 in uint8 and -1 in int32; 0x00 is zero in all
of them.  A result that is bit-equal under both fills and without any does not depend on what its scratch held.

A fill is an ordinary launch on the current stream, so none of this may run inside a hipGraph capture (the fill would
become part of the graph).  This is a helper module, not a conftest: nothing here runs unless a test calls it.
"""
from __future__ import annotations

import contextlib

import torch

from nerf_qa_amd import ops

FILLS = (0x00, 0xFF)


def fill_bytes(t: torch.Tensor, byte: int) -> torch.Tensor:
    """Every byte of the contiguous tensor t := byte, whatever its dtype (on the current stream for a CUDA tensor)."""
    if t.numel():
        t.view(-1).view(torch.uint8).fill_(int(byte))  # (flat first: a 0-d tensor has no last axis to re-view)
    return t


class PoisonWorkspace(ops.Workspace):
    """ops.Workspace (grow-only, one buffer per device and stream) that hands every buffer out filled with `byte`: the
    whole buffer, not only the bytes asked for, on every get(), on the stream the caller is about to launch on."""

    def __init__(self, byte: int):
        super().__init__()
        if not 0 <= int(byte) <= 255:
            raise ValueError(f"a fill byte lies in 0..255, got {byte}")
        self.byte = int(byte)
        self.gets = 0       # calls of get()
        self.filled = 0     # bytes filled over all of them

    def get(self, nbytes: int, dev: torch.device) -> torch.Tensor:
        buf = super().get(nbytes, dev)
        buf.fill_(self.byte)
        self.gets += 1
        self.filled += buf.numel()
        return buf


class EmptyHook:
    """The counters of poisoned_empty: `filled` CUDA tensors (and `filled_bytes`) got the byte, `passed` calls went
    through untouched (CPU tensors, meta tensors, anything that is not a tensor)."""

    def __init__(self, byte: int, device_types=("cuda",)):
        if not 0 <= int(byte) <= 255:
            raise ValueError(f"a fill byte lies in 0..255, got {byte}")
        self.byte = int(byte)
        self.device_types = tuple(device_types)  # ("cuda",) always, but for the helper's own CPU tests
        self.filled = 0
        self.filled_bytes = 0
        self.passed = 0

    def wrap(self, fn):
        def poisoned(*args, **kwargs):
            t = fn(*args, **kwargs)
            if torch.is_tensor(t) and t.device.type in self.device_types and t.numel() and t.is_contiguous():
                fill_bytes(t, self.byte)
                self.filled += 1
                self.filled_bytes += t.numel() * t.element_size()
            else:
                self.passed += 1
            return t
        poisoned.__wrapped__ = fn
        return poisoned


@contextlib.contextmanager
def poisoned_empty(byte: int, monkeypatch=None, device_types=("cuda",)):
    """with poisoned_empty(0xFF) as hook: every CUDA tensor torch.empty / torch.empty_like return inside the block is
    filled with the byte.  With pytest's `monkeypatch` the wrappers are set through it (and undone here, not only at
    the test's end); without, by plain assignment.  The originals are back after the block, also when it raises."""
    hook = EmptyHook(byte, device_types)
    saved = {name: getattr(torch, name) for name in ("empty", "empty_like")}
    try:
        for name, fn in saved.items():
            if monkeypatch is not None:
                monkeypatch.setattr(torch, name, hook.wrap(fn))
            else:
                setattr(torch, name, hook.wrap(fn))
        yield hook
    finally:
        for name, fn in saved.items():
            setattr(torch, name, fn)


def install(module, byte: int) -> PoisonWorkspace:
    """module._ws := a new PoisonWorkspace(byte); returns it.  The module must be one that keeps its scratch there (DISTS,
    ADISTS; pair.score_pair / score_group / forward_target read the A-DISTS module's)."""
    if not isinstance(getattr(module, "_ws", None), ops.Workspace):
        raise TypeError(f"{type(module).__name__} keeps no ops.Workspace in _ws")
    ws = PoisonWorkspace(byte)
    module.__dict__["_ws"] = ws
    return ws


def uninstall(module) -> None:
    """module._ws := a plain, empty ops.Workspace again."""
    module.__dict__["_ws"] = ops.Workspace()


class Poison:
    """What one poisoned block did: the workspaces it handed to the test (and those installed in modules), and the
    torch.empty hook."""

    def __init__(self, byte: int, hook: EmptyHook):
        self.byte, self.hook, self.workspaces = int(byte), hook, []

    def workspace(self) -> PoisonWorkspace:
        """A PoisonWorkspace of this block's byte, to pass as an entry point's ws= argument."""
        ws = PoisonWorkspace(self.byte)
        self.workspaces.append(ws)
        return ws

    @property
    def gets(self) -> int:
        return sum(ws.gets for ws in self.workspaces)

    @property
    def tensors(self) -> int:
        return self.hook.filled

    def report(self) -> str:
        return (f"fill 0x{self.byte:02X}: {self.gets} workspace get(s) over {len(self.workspaces)} workspace(s), "
                f"{self.tensors} torch.empty tensor(s), {self.hook.filled_bytes} bytes")

    def require(self, workspace: bool = True, empty: bool = True) -> None:
        """AssertionError where the block reached no poisoned workspace / filled no torch.empty tensor: a refactor that
        allocates past the hooks must fail its test, not pass it unpoisoned."""
        if workspace:
            assert self.gets > 0, "no poisoned workspace was asked for anything: the call allocates past ops.Workspace"
        if empty:
            assert self.tensors > 0, "no CUDA tensor came from torch.empty / torch.empty_like: the call allocates past the hook"


@contextlib.contextmanager
def poisoned(byte: int, *modules, monkeypatch=None, device_types=("cuda",)):
    """with poisoned(0xFF, dists, adists) as p: torch.empty / torch.empty_like are hooked and every module's _ws is a
    PoisonWorkspace for the block; p.workspace() gives further ones for ws= arguments.  On exit the hooks are gone and
    the modules hold plain, empty workspaces again."""
    with poisoned_empty(byte, monkeypatch, device_types) as hook:
        p = Poison(byte, hook)
        try:
            for m in modules:
                p.workspaces.append(install(m, byte))
            yield p
        finally:
            for m in modules:
                uninstall(m)
