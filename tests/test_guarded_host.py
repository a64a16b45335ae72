"""tests/guarded.py can fail (CPU, no GPU): every check the memory-contract tests of tests/test_gpu_memory_contract.py rely
on is shown here to catch a stand-in "kernel" that commits the fault it is there for."""
import types

import numpy as np
import pytest
import torch

import guarded
from guarded import Arena, GuardError, StaleError, SETTINGS

CAP = 1 << 20


@pytest.mark.parametrize("poison,guard", SETTINGS)
def test_a_byte_before_and_after_a_view_is_reported(poison, guard):
    for side, where in (("before", -1), ("after", 0)):
        arena = Arena("cpu", poison, guard, CAP)
        arena.empty((5, 7), torch.float64, label="first")
        v = arena.empty((3, 11), torch.uint8, offset=3, label="second")
        arena.empty(9, torch.int32, label="third")
        arena.check()
        start = v.data_ptr() - arena.buf.data_ptr()
        at = start + (where if side == "before" else v.numel())
        arena.buf[at] = poison
        with pytest.raises(GuardError) as e:
            arena.check()
        assert (e.value.label, e.value.side) == ("second", side)
        assert e.value.offset == (-1 if side == "before" else v.numel())
        assert "second" in str(e.value) and side in str(e.value)


def test_the_far_end_of_a_guard_band_is_checked_too():
    arena = Arena("cpu", 0x00, 0xFF, CAP)
    v = arena.empty(100, torch.uint8, label="only")
    start = v.data_ptr() - arena.buf.data_ptr()
    width = guarded.guard_width(100)
    assert width == 4096 and guarded.guard_width(10 ** 5) == 10 ** 5 and guarded.guard_width(1 << 30) == 1 << 20
    arena.buf[start + 100 + width - 1] = 0
    with pytest.raises(GuardError) as e:
        arena.check()
    assert e.value.side == "after" and e.value.offset == 100 + width - 1
    assert arena.guard_bytes >= 2 * width


def test_a_write_inside_the_view_is_not_reported():
    arena = Arena("cpu", 0xFF, 0x00, CAP)
    v = arena.empty((4, 4), torch.float32)
    assert arena.holds_poison(v) and torch.isnan(v).all()
    v.fill_(1.5)
    v.view(-1)[0] = -0.0
    v.view(-1)[-1] = 7.0
    arena.check()
    assert not arena.holds_poison(v)


@pytest.mark.parametrize("dtype,offsets", [(torch.uint8, (0, 1, 2, 3, 15, 255)), (torch.uint16, (0, 2, 6, 14)),
                                           (torch.float64, (0, 8, 248)), (torch.int32, (0, 4))])
def test_offset_is_honoured(dtype, offsets):
    arena = Arena("cpu", 0x5A, 0xA5, CAP)
    for off in offsets:
        v = arena.empty((3, 5), dtype, offset=off)
        assert v.data_ptr() % 256 == off and v.is_contiguous() and v.dtype == dtype and tuple(v.shape) == (3, 5)
        assert arena.holds_poison(v)
        p = arena.place(torch.arange(15).reshape(3, 5).to(dtype), offset=off)
        assert p.data_ptr() % 256 == off and p.reshape(-1).tolist() == list(range(15))
    arena.check()
    if dtype != torch.uint8:
        with pytest.raises(ValueError):
            arena.empty(4, dtype, offset=1)
    with pytest.raises(ValueError):
        arena.empty(4, torch.uint8, offset=256)


def test_a_full_arena_refuses():
    arena = Arena("cpu", 0x00, 0xFF, 3 * 4096)
    arena.empty(16, torch.uint8)
    with pytest.raises(MemoryError):
        arena.empty(4096, torch.uint8)       # (4 KiB of data and 4 KiB of guard on both sides no longer fit)


def test_zeros_and_full_keep_their_value_and_empty_is_poisoned():
    arena = Arena("cpu", 0xFF, 0x00, CAP)
    fake = types.SimpleNamespace(torch=torch, lib=types.SimpleNamespace(tpiv_thing=lambda a, b: a + b, ABI=2))
    with guarded.patched(fake, arena) as calls:
        t = fake.torch
        e = t.empty(2, 3, dtype=t.float64, device="cpu")
        e2 = t.empty((2, 3), dtype=t.int32, device=torch.device("cpu"))
        z = t.zeros(4, dtype=t.int64, device="cpu")
        f = t.full((2, 2), 255, dtype=t.uint8, device="cpu")
        el, zl = t.empty_like(e), t.zeros_like(f)
        other = t.empty(3, dtype=t.uint8)                       # no device named: not the arena's business
        assert fake.lib.tpiv_thing(2, 3) == 5 and fake.lib.ABI == 2
        assert isinstance(e, t.Tensor) and t.float64 is torch.float64
    assert fake.torch is torch and calls == {"tpiv_thing"}
    inside = lambda v: arena.buf.data_ptr() <= v.data_ptr() < arena.buf.data_ptr() + arena.buf.numel()    # noqa: E731
    assert all(inside(v) for v in (e, e2, z, f, el, zl)) and not inside(other)
    assert torch.isnan(e).all() and torch.isnan(el).all() and (e2 == -1).all()
    assert (z == 0).all() and (f == 255).all() and (zl == 0).all() and zl.dtype == torch.uint8
    assert len(arena.regions) == 6
    arena.check()


def test_patched_restores_after_an_exception():
    arena = Arena("cpu", 0x00, 0xFF, CAP)
    fake = types.SimpleNamespace(torch=torch, lib=object())
    real_lib = fake.lib
    with pytest.raises(KeyError):
        with guarded.patched(fake, arena):
            raise KeyError("x")
    assert fake.torch is torch and fake.lib is real_lib


# ---- stand-in kernels on the CPU, through the same driver the GPU tests use

def _build():
    return {"frame": np.arange(1, 38, dtype=np.uint8), "gain": 3}


def _good(inp, arena):
    out = arena.empty(inp["frame"].shape, torch.int32, label="out")
    out.copy_(inp["frame"].to(torch.int32) * inp["gain"])
    return out


def _leaves_one_cell(inp, arena):
    out = arena.empty(inp["frame"].shape, torch.int32, label="out")
    out[:-1] = inp["frame"][:-1].to(torch.int32) * inp["gain"]
    return out


def _reads_one_past(inp, arena):
    f = inp["frame"]
    start = f.data_ptr() - arena.buf.data_ptr()
    window = arena.buf[start + 1:start + 1 + f.numel()]          # shifted by one: the last element is the guard byte behind
    out = arena.empty(f.shape, torch.int32, label="out")
    out.copy_(window.to(torch.int32) * inp["gain"])
    return out


def _writes_one_past(inp, arena):
    out = _good(inp, arena)
    start = out.data_ptr() - arena.buf.data_ptr()
    arena.buf[start + 4 * out.numel()] = arena.poison
    return out


def test_a_sound_stand_in_passes():
    runs, arenas, outs = guarded.run_settings("cpu", _build, _good, capacity=CAP, offset=3)
    guarded.differing_output(runs, ["out"])
    assert [a.poison for a in arenas] == [p for p, _ in SETTINGS]
    assert outs[0][0].tolist() == [3 * k for k in range(1, 38)]
    assert all(a.regions[0][0] == "input frame" for a in arenas)


def test_an_unwritten_output_cell_is_caught():
    runs, _, _ = guarded.run_settings("cpu", _build, _leaves_one_cell, capacity=CAP)
    with pytest.raises(StaleError, match="out depends"):
        guarded.differing_output(runs, ["out"])
    # ... and only by that comparison: under one setting alone the call looks fine
    assert guarded.first_difference(runs[0][0][:-4], runs[1][0][:-4]) is None


def test_a_read_past_an_input_is_caught():
    runs, _, _ = guarded.run_settings("cpu", _build, _reads_one_past, capacity=CAP)
    with pytest.raises(StaleError, match="out depends"):
        guarded.differing_output(runs, ["out"])
    assert guarded.first_difference(runs[0][0], runs[1][0]) == 4 * 36


def test_a_write_past_an_output_is_caught():
    with pytest.raises(GuardError) as e:
        guarded.run_settings("cpu", _build, _writes_one_past, capacity=CAP)
    assert (e.value.label, e.value.side, e.value.offset) == ("out", "after", 4 * 37)


def test_bits_tell_signed_zeros_and_nan_payloads_apart():
    a = torch.tensor([0.0, float("nan")], dtype=torch.float64)
    b = torch.tensor([-0.0, float("nan")], dtype=torch.float64)
    c = a.clone()
    c.view(torch.int64)[1] += 1                      # another NaN payload
    assert guarded.first_difference(guarded.bits(a), guarded.bits(a.clone())) is None
    assert guarded.first_difference(guarded.bits(a), guarded.bits(b)) == 7
    assert guarded.first_difference(guarded.bits(a), guarded.bits(c)) == 8
    assert guarded.first_difference(guarded.bits(a), guarded.bits(a[:1])) == 8
