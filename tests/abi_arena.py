"""Poisoned, exactly sized buffers with guard bands for tests of the C ABI (include/vmlmf_hip.h).

torch.empty through the caching allocator hides three kinds of bug: fresh device memory is zero (a read of a slot nobody wrote,
masked by x 0, passes), allocations are rounded up (a store one row past the end lands in slack nobody looks at), and an output
element no launch writes keeps a plausible previous occupant.  An Arena is ONE allocation per call under test, filled - guards
included - with a 32-bit pattern; every buffer of the call is a view of exactly the requested size, 256-byte aligned, with at least
GUARD bytes of pattern on each side, so a buffer's neighbours are guard bands and not allocator slack.

    arena = Arena(device, fill)
    x = arena.buf((T, B, I), torch.float32, init=x_values, name="x")      # an input: exactly sized, between poisoned guards
    y = arena.buf((T, B, H), torch.float32, name="y")                     # an output: all poison until the call writes it
    ticket = arena.buf(2, torch.int64, init=0, name="ticket")             # a word the header requires to be zero
    ... the call ...
    arena.check_guards()               # AssertionError naming the buffer and the first damaged offset
    assert_written(arena, "y", y)      # no element still holds the pattern, every floating element finite

Works on CPU tensors as well (tests/test_abi_arena_cpu.py proves on fake calls that each check can fail).
"""
import numpy as np
import torch

GUARD = 4096     # bytes of pattern on each side of every buffer, at least
ALIGN = 256      # alignment of every buffer's first byte

# the three fills of tests/test_gpu_abi_buffers.py
FILL_ZERO = 0x00000000    # what fresh device memory holds: today's de-facto condition, the baseline
FILL_NAN = 0x7FC07FC0     # NaN as fp32, NaN in both bf16 halves, a huge unsigned counter
FILL_ONES = 0xFFFFFFFF    # negative NaN, the unsigned maximum, -1 as an int32 and as an int64
FILLS = (FILL_ZERO, FILL_NAN, FILL_ONES)


def _up(v, a):
    return (v + a - 1) // a * a


class Arena:
    """One allocation of `capacity` bytes on `device`, every 32-bit word of it `fill`; buf() carves guarded views out of it."""

    def __init__(self, device, fill, capacity=1 << 24):
        self.fill = int(fill) & 0xFFFFFFFF
        self.device = torch.device(device)
        words = _up(int(capacity), 4) // 4 + ALIGN // 4
        signed = self.fill - (1 << 32) if self.fill >= 1 << 31 else self.fill
        self._words = torch.full((words,), signed, dtype=torch.int32, device=self.device)
        self._bytes = self._words.view(torch.uint8)
        # the pattern is laid from the allocation's first byte; buffers start at multiples of ALIGN (a multiple of 4) of the ADDRESS,
        # so the shift between address phase and pattern phase is the base address modulo 4: zero (torch aligns to 64 and more)
        assert self._words.data_ptr() % 4 == 0
        self._cursor = _up(self._words.data_ptr() + GUARD, ALIGN) - self._words.data_ptr()
        self._bufs = []          # (name, first byte, bytes)
        self._pattern = np.frombuffer(np.uint32(self.fill).tobytes(), dtype=np.uint8)
        self._guard_index = None

    # ---- handing out buffers
    def buf(self, shape, dtype=torch.uint8, init=None, name=None):
        """A tensor view of exactly prod(shape) elements of `dtype` (an int `shape` is a length; with the default dtype, bytes).
        init: None leaves the pattern (outputs, scratch); a number fills; an array or tensor gives the values (inputs)."""
        shape = (int(shape),) if isinstance(shape, (int, np.integer)) else tuple(int(s) for s in shape)
        item = torch.empty((), dtype=dtype).element_size()
        n = int(np.prod(shape, dtype=np.int64)) if shape else 1
        nbytes = n * item
        off = self._cursor
        end = off + nbytes
        if end + GUARD > self._bytes.numel():
            raise MemoryError(f"Arena: {name or 'buffer'} of {nbytes} bytes does not fit (capacity {self._bytes.numel()}, used {off})")
        self._cursor = _up(self._words.data_ptr() + end + GUARD, ALIGN) - self._words.data_ptr()
        self._bufs.append((name or f"buf{len(self._bufs)}", off, nbytes))
        self._guard_index = None
        t = self._bytes[off:end].view(dtype).view(shape)
        assert t.data_ptr() % ALIGN == 0 and t.data_ptr() == self._words.data_ptr() + off
        if init is not None:
            if isinstance(init, (int, float)):
                t.fill_(init)
            else:
                src = init if isinstance(init, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(init))
                t.copy_(src.to(dtype).reshape(shape))
        return t

    def bytes_used(self):
        return self._cursor

    # ---- the checks
    def _expected(self, first, n):
        """The pattern's bytes at allocation offsets first .. first + n."""
        reps = np.tile(self._pattern, n // 4 + 2)
        return reps[first % 4:first % 4 + n]

    def _guards(self):
        """Index of every guard byte (int64 tensor), the bytes expected there, and the guards' bounds."""
        if self._guard_index is None:
            spans, prev_end = [], 0
            for _, off, nbytes in self._bufs:
                spans.append((prev_end, off))
                prev_end = off + nbytes
            spans.append((prev_end, min(prev_end + GUARD, self._bytes.numel())))
            idx = np.concatenate([np.arange(a, b, dtype=np.int64) for a, b in spans]) if spans else np.zeros(0, np.int64)
            exp = self._pattern[idx % 4]
            self._guard_index = (torch.as_tensor(idx, device=self.device), torch.as_tensor(exp, device=self.device), idx)
        return self._guard_index

    def check_guards(self):
        """AssertionError with the neighbouring buffer's name and the first damaged byte's offset from it if any guard byte changed."""
        idx, exp, idx_host = self._guards()
        bad = self._bytes[idx] != exp
        if not bool(bad.any()):
            return
        pos = int(idx_host[int(torch.nonzero(bad)[0, 0])])
        best = None
        for name, off, nbytes in self._bufs:     # the nearest buffer: a store past an end, or before a start
            d = pos - (off + nbytes) if pos >= off + nbytes else off - pos
            what = f"{pos - (off + nbytes)} bytes past the end of" if pos >= off + nbytes else f"{off - pos} bytes before the start of"
            if best is None or d < best[0]:
                best = (d, f"{what} '{name}' ({nbytes} bytes)")
        got = int(self._bytes[pos])
        raise AssertionError(f"guard band damaged {best[1]}: byte 0x{got:02x} where the fill 0x{self.fill:08x} was "
                             f"({int(bad.sum())} guard bytes changed)")

    def unwritten(self, t):
        """Mask (shape of t) of the elements of the arena view `t` that still hold the fill pattern in every byte."""
        item = t.element_size()
        off = t.data_ptr() - self._words.data_ptr()
        assert 0 <= off and off + t.numel() * item <= self._bytes.numel() and t.is_contiguous(), "not a view handed out by this arena"
        raw = self._bytes[off:off + t.numel() * item].view(-1, item)
        exp = torch.as_tensor(self._expected(off, t.numel() * item).copy(), device=self.device).view(-1, item)
        return (raw == exp).all(dim=1).view(t.shape)


# ---- assertions over a call's buffers (what the table of tests/test_gpu_abi_buffers.py applies to every case) ----
def _bits(t):
    t = t.contiguous().reshape(-1)
    return t.view(torch.int32) if t.element_size() % 4 == 0 else t.view(torch.uint8)


def first_difference(a, b):
    """None when the two tensors hold the same bits, else the flat index (in elements) of the first that differs."""
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    xa, xb = _bits(a), _bits(b)
    if torch.equal(xa, xb):
        return None
    return int(torch.nonzero(xa != xb)[0, 0]) // (a.element_size() // xa.element_size())


def assert_same_bits(name, a, b, what=""):
    """A result must not depend on what unspecified memory held: bit-identical between two runs."""
    at = first_difference(a, b)
    if at is not None:
        fa, fb = a.reshape(-1)[at].item(), b.reshape(-1)[at].item()
        raise AssertionError(f"'{name}' differs {what}: first at flat index {at} of {a.numel()}: {fa!r} vs {fb!r}")


def assert_written(arena, name, t):
    """No element of the output `t` still holds the arena's pattern (not asked under the zero fill, where a written zero looks the
    same), and every floating element is finite."""
    if arena.fill != FILL_ZERO:
        left = arena.unwritten(t)
        if bool(left.any()):
            at = int(torch.nonzero(left.reshape(-1))[0, 0])
            raise AssertionError(f"'{name}': {int(left.sum())} of {t.numel()} elements were never written (still the fill "
                                 f"0x{arena.fill:08x}), first at flat index {at}")
    if t.is_floating_point():
        ok = torch.isfinite(t)
        if not bool(ok.all()):
            at = int(torch.nonzero(~ok.reshape(-1))[0, 0])
            raise AssertionError(f"'{name}': {int((~ok).sum())} of {t.numel()} elements are not finite under fill 0x{arena.fill:08x}, "
                                 f"first at flat index {at}: {t.reshape(-1)[at].item()!r}")


def assert_untouched(arena, name, t):
    """Nothing was launched: every element of `t` still is the pattern."""
    left = arena.unwritten(t)
    if not bool(left.all()):
        at = int(torch.nonzero(~left.reshape(-1))[0, 0])
        raise AssertionError(f"'{name}' was written (flat index {at}) by a call that should have launched nothing")


def assert_zero(name, t):
    """A word the header says every launch leaves zero (tickets, guard verdict words)."""
    nz = _bits(t) != 0
    if bool(nz.any()):
        raise AssertionError(f"'{name}' was left non-zero: word {int(torch.nonzero(nz)[0, 0])} of {nz.numel()}")
