"""The harness of tests/test_gpu_abi_buffers.py must be able to fail (no GPU): on a CPU arena, fake "calls" written in torch that
commit each fault the GPU table looks for - a store one element past a buffer's end, one before its start, an output element left
unwritten, a result that depends on a workspace byte, a ticket left non-zero - are each reported by tests/abi_arena.py, with the
buffer's name; a clean fake passes under all three fills."""
import numpy as np
import pytest
import torch

from abi_arena import (ALIGN, FILL_NAN, FILL_ONES, FILL_ZERO, FILLS, GUARD, Arena, assert_same_bits, assert_untouched, assert_written,
                       assert_zero, first_difference)

N = 37    # odd on purpose: 148 bytes, so the next buffer's alignment pad is part of a guard


def index_of(arena, t):
    return (t.data_ptr() - arena._words.data_ptr()) // 4


def fake_call(fill, fault=None):
    """y = 2 x + sum(scratch written by the call itself); `ticket` counts arrivals and is reset.  `fault` commits one of the bugs."""
    arena = Arena("cpu", fill, capacity=1 << 16)
    rng = np.random.Generator(np.random.PCG64(5))
    x = arena.buf(N, torch.float32, init=rng.standard_normal(N).astype(np.float32), name="x")
    ws = arena.buf(64, torch.float32, name="workspace")
    y = arena.buf(N, torch.float32, name="y")
    ticket = arena.buf(2, torch.int64, init=0, name="ticket")
    iy = index_of(arena, y)
    ws[:N] = x                                  # the call initialises what it later reads ...
    used = N + 1 if fault == "reads_workspace" else N      # ... except under this fault: one slot nobody wrote, "masked" by x 0
    y.copy_(2 * x + 0 * ws[:used].sum())
    ticket += 3
    if fault == "past_end":
        arena._words[iy + N] = 0x5A5A5A5A
    elif fault == "before_start":
        arena._words[iy - 1] = 0x5A5A5A5A
    elif fault == "unwritten":
        arena._words[iy + 5] = arena._words[0]      # the pattern back where a result should be
    if fault != "ticket":
        ticket.zero_()
    return arena, {"y": y, "ticket": ticket, "x": x}


def check(fault):
    """What tests/test_gpu_abi_buffers.py asserts of every case, on the fake."""
    runs = []
    for fill in FILLS:
        arena, out = fake_call(fill, fault)
        arena.check_guards()
        assert_written(arena, "y", out["y"])
        assert_zero("ticket", out["ticket"])
        runs.append(out)
    for other, fill in zip(runs[1:], FILLS[1:]):
        assert_same_bits("y", runs[0]["y"], other["y"], f"between fill 0x{FILL_ZERO:08x} and 0x{fill:08x}")


def test_a_clean_call_passes_under_every_fill():
    check(None)


@pytest.mark.parametrize("fault,words", [
    ("past_end", ["guard band damaged", "0 bytes past the end of 'y'"]),
    ("before_start", ["guard band damaged", "4 bytes before the start of 'y'"]),
    ("unwritten", ["'y'", "never written", "flat index 5"]),
    ("reads_workspace", ["'y'", "fill 0x7fc07fc0"]),     # 0 x NaN carries the poison's own payload into every element
    ("ticket", ["'ticket'", "left non-zero"]),
])
def test_each_fault_is_reported_with_the_buffers_name(fault, words):
    with pytest.raises(AssertionError) as e:
        check(fault)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_a_result_that_depends_on_a_finite_workspace_byte_differs_between_fills():
    """Poison that stays finite (a counter, an index) shows only in the run-to-run comparison."""
    def call(fill):
        arena = Arena("cpu", fill, capacity=1 << 14)
        ws = arena.buf(4, torch.int32, name="workspace")
        y = arena.buf(8, torch.float32, name="y")
        y.copy_(torch.arange(8.0) + (1.0 if int(ws[0]) < 5 else 0.0))     # "already arrived" under a garbage counter
        return y
    a, b = call(FILL_ZERO), call(FILL_NAN)
    assert first_difference(a, b) == 0
    with pytest.raises(AssertionError, match="'y' differs"):
        assert_same_bits("y", a, b)
    assert first_difference(a, call(FILL_ONES)) is None     # -1 < 5 as well: one fill alone would not have shown it


def test_buffers_are_exact_aligned_and_guarded():
    arena = Arena("cpu", FILL_NAN, capacity=1 << 16)
    a = arena.buf(3, torch.uint8, name="a")
    b = arena.buf((5, 7), torch.float32, name="b")
    c = arena.buf(2, torch.int64, init=0, name="c")
    base = arena._words.data_ptr()
    last_end = base
    for t in (a, b, c):
        assert t.data_ptr() % ALIGN == 0
        assert t.data_ptr() - last_end >= GUARD
        last_end = t.data_ptr() + t.numel() * t.element_size()
    assert a.numel() == 3 and b.shape == (5, 7) and c.dtype == torch.int64
    assert torch.isnan(b).all() and int(c.abs().sum()) == 0
    assert arena.unwritten(b).all() and arena.unwritten(a).all() and not arena.unwritten(c).any()
    assert_untouched(arena, "b", b)
    b[2, 3] = 0.5
    assert int(arena.unwritten(b).sum()) == 34 and not arena.unwritten(b)[2, 3]
    with pytest.raises(AssertionError, match="'b' was written"):
        assert_untouched(arena, "b", b)
    arena.check_guards()
    arena._bytes[a.data_ptr() - base + 3] = 0      # the byte behind a 3-byte buffer: inside a word the buffer shares
    with pytest.raises(AssertionError, match="0 bytes past the end of 'a'"):
        arena.check_guards()


def test_the_fills_read_as_the_issue_says():
    nan = Arena("cpu", FILL_NAN, capacity=1 << 16)
    assert torch.isnan(nan.buf(4, torch.float32)).all() and torch.isnan(nan.buf(4, torch.bfloat16)).all()
    ones = Arena("cpu", FILL_ONES, capacity=1 << 16)
    assert torch.isnan(ones.buf(4, torch.float32)).all()
    assert int(ones.buf(1, torch.int32)[0]) == -1 and int(ones.buf(1, torch.int64)[0]) == -1
    assert int(Arena("cpu", FILL_ZERO, capacity=1 << 16).buf(4, torch.int64).abs().sum()) == 0
    with pytest.raises(MemoryError):
        ones.buf(1 << 16)
