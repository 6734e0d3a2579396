"""The poison helper itself (tests/poison.py), on the CPU: what tests/test_gpu_scratch_independence.py relies on.

A PoisonWorkspace must fill every byte of the buffer it hands out on EVERY get -- also the tail of a buffer that is
reused for a smaller request, which is where a stale partial of an earlier, larger call would sit --, the torch.empty
wrappers must be gone after the block whatever happened inside it, the counters must count, and a block that reached
no hook must say so instead of passing.
"""
import pytest
import torch

import poison
from nerf_qa_amd import ops

CPU = torch.device("cpu")


@pytest.mark.parametrize("byte", [0x00, 0xFF, 0xA5])
def test_workspace_fills_every_byte_on_every_get(byte):
    ws = poison.PoisonWorkspace(byte)
    buf = ws.get(1000, CPU)
    assert buf.dtype == torch.uint8 and buf.numel() >= 1000 and bool((buf == byte).all())
    assert (ws.gets, ws.filled) == (1, buf.numel())
    buf.fill_(0x3C)  # what a call leaves behind
    again = ws.get(1000, CPU)
    assert again.data_ptr() == buf.data_ptr(), "the parent's buffer is reused, not replaced"
    assert bool((again == byte).all()), "the fill happens on every get, not only on allocation"
    assert ws.gets == 2


def test_workspace_fills_the_tail_of_a_buffer_reused_smaller():
    ws = poison.PoisonWorkspace(0xFF)
    big = ws.get(4096, CPU)
    big.fill_(0x11)  # the larger call's partials
    small = ws.get(300, CPU)
    assert small.data_ptr() == big.data_ptr() and small.numel() == big.numel() == 4096  # (grow-only: the same bytes back)
    assert bool((small == 0xFF).all()), "bytes 300.. of the reused buffer still hold the earlier call's data"
    assert ws.filled == 2 * 4096
    # a larger request replaces the buffer; the new one is filled whole as well
    grown = ws.get(10000, CPU)
    assert grown.numel() == 10000 and bool((grown == 0xFF).all()) and ws.gets == 3


def test_workspace_is_an_ops_workspace_and_refuses_a_bad_byte():
    assert isinstance(poison.PoisonWorkspace(0), ops.Workspace)
    for bad in (-1, 256):
        with pytest.raises(ValueError):
            poison.PoisonWorkspace(bad)
        with pytest.raises(ValueError):
            poison.EmptyHook(bad)


@pytest.mark.parametrize("dtype,want", [(torch.float16, "nan"), (torch.bfloat16, "nan"), (torch.float32, "nan"),
                                        (torch.float64, "nan"), (torch.uint8, 255), (torch.int32, -1)])
def test_ff_is_nan_or_minus_one_in_every_format(dtype, want):
    t = poison.fill_bytes(torch.zeros(7, dtype=dtype), 0xFF)
    if want == "nan":
        assert bool(torch.isnan(t.double()).all())
    else:
        assert bool((t == want).all())
    assert bool((poison.fill_bytes(t, 0x00) == 0).all())
    scalar = poison.fill_bytes(torch.zeros((), dtype=dtype), 0xFF)  # a 0-d tensor (a loss value's buffer)
    assert bool(torch.isnan(scalar.double())) if want == "nan" else scalar.item() == want


def test_empty_hook_fills_counts_and_passes_through(monkeypatch):
    orig, orig_like = torch.empty, torch.empty_like
    with poison.poisoned_empty(0xFF, monkeypatch, device_types=("cpu",)) as hook:
        assert torch.empty is not orig and torch.empty_like is not orig_like
        a = torch.empty((3, 5), dtype=torch.float32)
        b = torch.empty_like(torch.zeros(4, dtype=torch.int32))
        c = torch.empty(0)                       # nothing to fill
        d = torch.empty(6, dtype=torch.uint8)
        assert bool(torch.isnan(a).all()) and bool((b == -1).all()) and bool((d == 255).all()) and c.numel() == 0
        assert (hook.filled, hook.passed, hook.filled_bytes) == (3, 1, 60 + 16 + 6)
    assert torch.empty is orig and torch.empty_like is orig_like


def test_empty_hook_leaves_other_devices_alone(monkeypatch):
    """The hook the GPU tests use fills CUDA tensors only: a CPU tensor (pack_vgg_weights' blob, a pinned flag buffer)
    goes through as torch.empty made it, and is counted as passed."""
    with poison.poisoned_empty(0xFF, monkeypatch) as hook:
        blob = torch.empty(64, dtype=torch.uint8).zero_()
        assert (hook.filled, hook.passed) == (0, 1) and bool((blob == 0).all())


def test_hooks_are_gone_after_an_exception(monkeypatch):
    orig, orig_like = torch.empty, torch.empty_like

    class Boom(Exception):
        pass

    for mp in (monkeypatch, None):
        with pytest.raises(Boom):
            with poison.poisoned_empty(0x00, mp, device_types=("cpu",)):
                assert torch.empty is not orig
                raise Boom()
        assert torch.empty is orig and torch.empty_like is orig_like


class _Module:
    """What install looks at: a module that keeps its scratch in _ws."""

    def __init__(self):
        self._ws = ops.Workspace()


def test_install_poisoned_and_the_counters():
    m, other = _Module(), _Module()
    with poison.poisoned(0xFF, m, other, device_types=("cpu",)) as p:
        assert isinstance(m._ws, poison.PoisonWorkspace) and isinstance(other._ws, poison.PoisonWorkspace)
        assert m._ws is not other._ws and m._ws.byte == 0xFF
        assert (p.gets, p.tensors) == (0, 0)
        m._ws.get(512, CPU)
        extra = p.workspace()
        extra.get(256, CPU)
        extra.get(256, CPU)
        torch.empty(8)
        assert (p.gets, p.tensors, len(p.workspaces)) == (3, 2 + 1, 3)  # (a workspace's own two allocations go through the hook too)
        assert "3 workspace get(s) over 3 workspace(s)" in p.report() and "0xFF" in p.report()
        p.require()
    assert type(m._ws) is ops.Workspace and type(other._ws) is ops.Workspace and not m._ws.bufs
    with pytest.raises(TypeError):
        poison.install(object(), 0)


def test_a_block_that_reaches_no_hook_is_reported(monkeypatch):
    m = _Module()
    with poison.poisoned(0x00, m, monkeypatch=monkeypatch) as p:  # (the CUDA-only hook, and nothing asks the workspace)
        torch.empty(8)
        with pytest.raises(AssertionError, match="workspace"):
            p.require()
        with pytest.raises(AssertionError, match="torch.empty"):
            p.require(workspace=False)
        p.require(workspace=False, empty=False)
        m._ws.get(16, CPU)
        p.require(empty=False)
        with pytest.raises(AssertionError, match="torch.empty"):
            p.require()
    # the modules get their plain workspace back after an exception as well
    with pytest.raises(RuntimeError):
        with poison.poisoned(0x00, m):
            raise RuntimeError("inside")
    assert type(m._ws) is ops.Workspace and torch.empty.__name__ == "empty"
