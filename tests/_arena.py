"""Placement arena for the device-call tests: every logical buffer of a call gets an allocation of its own, laid out as

    [front guard][displacement][payload][back guard]

so that a call can be handed pointers at exactly the alignment the C ABI accepts (and no more), and so that whatever it reads
or writes outside the documented extent of a buffer lands in memory the test owns and can look at.

  * Guards are GUARD_BYTES on each side.  That is a condition, not a measurement: it exceeds the largest contiguous burst one
    workgroup of any kernel of the library writes (256 lanes x 16 bytes x a few iterations), so an overrun damages a guard
    instead of leaving the allocation.
  * An OUTPUT buffer is pre-filled -- guards, displacement and payload -- with a seeded byte stream of values 1..254 (never
    0x00 or 0xFF, never constant).  After the call every byte outside the bytes the call is documented to write must still be
    the fill: the guards, and the holes inside the payload (pitch gaps, m_I, the plane a call does not write).
  * An INPUT buffer carries the caller's bytes; its guards are garbage from a seed the caller picks.  Running a case with two
    seeds and comparing both results with the reference shows an over-read that reaches the result, without a fault.
  * `displacement` is in bytes.  With a non-zero displacement the pointer handed out must be aligned to `align` and NOT to
    2 * align, otherwise the case proves nothing; displacement 0 is the natural placement and is not checked.

The memory behind an arena is anything with `alloc(nbytes)` returning an object with `.ptr`, `.upload(array)` and
`.download(dtype, count)`: x266_amd.Codec on a GPU, HostMemory below in the CPU test of this module."""
import numpy as np

GUARD_BYTES = 64 << 10


class ArenaDamage(AssertionError):
    """bytes outside a buffer's documented extent changed; first / last are offsets relative to the payload's first byte
    (negative: before the payload; >= the payload's size: behind it)"""

    def __init__(self, name, what, first, last, count):
        self.name, self.what, self.first, self.last, self.count = name, what, int(first), int(last), int(count)
        super().__init__("%s: %s damaged: %d byte(s), first at payload%+d, last at payload%+d"
                         % (name, what, self.count, self.first, self.last))


class ArenaAlignment(AssertionError):
    pass


def fill_bytes(seed, n):
    """the fill of output buffers and the garbage of input guards: seeded, non-constant, never 0x00 or 0xFF"""
    return np.random.RandomState(seed & 0x7FFFFFFF).randint(1, 255, n).astype(np.uint8)


class HostMemory:
    """in-memory stand-in for device memory (the CPU test of the arena): fake addresses, numpy storage"""

    class Buffer:
        def __init__(self, ptr, nbytes):
            self.ptr, self.nbytes = ptr, nbytes
            self.bytes = np.zeros(nbytes, np.uint8)

        def upload(self, arr):
            a = np.ascontiguousarray(arr).view(np.uint8).ravel()
            self.bytes[:a.size] = a

        def download(self, dtype, count):
            return self.bytes[:count * np.dtype(dtype).itemsize].copy().view(dtype)

    def __init__(self, base=0x7F0000000000):
        self.next = base

    def alloc(self, nbytes):
        b = HostMemory.Buffer(self.next, nbytes)
        self.next += (nbytes + 0xFFF) & ~0xFFF                            # allocations are page aligned, as xHipMalloc's
        return b


class Slot:
    """one placed buffer.  ptr = address of payload byte `origin` (what the call is given)"""

    def __init__(self, name, buf, image, start, size, origin, written, is_output):
        self.name, self.buf, self.image = name, buf, image
        self.start, self.size, self.origin = start, size, origin
        self.written, self.is_output = written, is_output
        self.ptr = buf.ptr + start + origin

    def _now(self):
        return self.buf.download(np.uint8, self.image.size)

    def _report(self, what, bad_abs):
        rel = bad_abs - self.start
        raise ArenaDamage(self.name, what, rel[0], rel[-1], rel.size)

    def payload(self, dtype=np.uint8):
        """the payload as the device holds it now"""
        return self._now()[self.start:self.start + self.size].copy().view(dtype)

    def check(self):
        """guards intact; holes of an output intact; an input wholly unchanged.  Returns the payload bytes."""
        now = self._now()
        diff = now != self.image
        outside = diff.copy()
        outside[self.start:self.start + self.size] = False
        if outside.any():
            self._report("guard band", np.flatnonzero(outside))
        inside = diff[self.start:self.start + self.size]
        if not self.is_output:
            if inside.any():
                self._report("input", np.flatnonzero(inside) + self.start)
        elif self.written is not None:
            holes = inside & ~self.written
            if holes.any():
                self._report("hole", np.flatnonzero(holes) + self.start)
        return now[self.start:self.start + self.size].copy()

    def check_untouched(self):
        """nothing at all changed (a rejected call launches nothing)"""
        diff = self._now() != self.image
        if diff.any():
            self._report("buffer of a rejected call", np.flatnonzero(diff))


class Arena:
    def __init__(self, memory, guard=GUARD_BYTES):
        self.memory, self.guard, self.slots = memory, guard, []

    def _place(self, name, payload, align, displacement, origin, written, is_output, seed):
        assert displacement >= 0 and align >= 1 and align & (align - 1) == 0
        size = payload.size
        image = fill_bytes(seed, self.guard + displacement + size + self.guard)
        start = self.guard + displacement
        image[start:start + size] = payload
        buf = self.memory.alloc(image.size)
        buf.upload(image)
        slot = Slot(name, buf, image, start, size, origin, written, is_output)
        if displacement:
            if slot.ptr % align or slot.ptr % (2 * align) == 0:
                raise ArenaAlignment("%s: pointer %#x is not aligned to exactly %d bytes (displacement %d)"
                                     % (name, slot.ptr, align, displacement))
        self.slots.append(slot)
        return slot

    def input(self, name, data, align, displacement, guard_seed, origin=0):
        """data: the bytes the call may read.  origin: offset inside them of the address the call is given (a frame with a border)"""
        payload = np.ascontiguousarray(data).view(np.uint8).ravel()
        return self._place(name, payload, align, displacement, origin, None, False, guard_seed)

    def output(self, name, nbytes, align, displacement, written=None, fill_seed=0x5EED):
        """written: boolean mask over the payload's bytes, True where the call is documented to write (None: everywhere)"""
        if written is not None:
            written = np.asarray(written, bool).ravel()
            assert written.size == nbytes
        seed = fill_seed + 7919 * len(self.slots)
        payload = fill_bytes(seed ^ 0x2A2A2A, nbytes)
        return self._place(name, payload, align, displacement, 0, written, True, seed)

    def check(self):
        """every slot's guards, holes and inputs; {name: payload bytes}"""
        return {s.name: s.check() for s in self.slots}

    def check_untouched(self):
        for s in self.slots:
            s.check_untouched()
