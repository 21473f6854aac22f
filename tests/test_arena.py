"""The placement arena of the GPU placement tests (tests/_arena.py), tested without a GPU: an in-memory stand-in plays the
device buffer, faults are planted into it by hand, and the helper must report each at the right offset -- and pass a clean write."""
import numpy as np
import pytest

from _arena import GUARD_BYTES, Arena, ArenaAlignment, ArenaDamage, HostMemory, fill_bytes


def _poke(slot, payload_offset, data):
    """what a kernel would do: write bytes at an offset relative to the payload's first byte, straight into the stand-in"""
    data = np.asarray(data, np.uint8).ravel()
    at = slot.start + payload_offset
    slot.buf.bytes[at:at + data.size] = data


def _other(slot, payload_offset):
    """a byte value different from what the buffer holds there"""
    return int(slot.buf.bytes[slot.start + payload_offset]) ^ 0x5A


def _output(n=1000, align=16, displacement=16, written=None):
    return Arena(HostMemory()).output("out", n, align, displacement, written)


def test_layout_and_fill():
    a = Arena(HostMemory())
    s = a.output("out", 1000, 16, 48)
    assert s.start == GUARD_BYTES + 48 and s.image.size == 2 * GUARD_BYTES + 48 + 1000
    assert s.ptr % 16 == 0 and s.ptr % 32 != 0
    img = s.image
    assert img.min() >= 1 and img.max() <= 254 and len(np.unique(img)) > 200          # never 0x00 / 0xFF, not constant
    assert GUARD_BYTES >= 256 * 16 * 8                                                  # the condition on the guard size
    i = a.input("in", np.arange(64, dtype=np.int16), 16, 80, guard_seed=1)
    j = Arena(HostMemory()).input("in", np.arange(64, dtype=np.int16), 16, 80, guard_seed=2)
    assert np.array_equal(i.payload(np.int16), np.arange(64)) and np.array_equal(j.payload(np.int16), np.arange(64))
    assert not np.array_equal(i.image[:GUARD_BYTES], j.image[:GUARD_BYTES])           # two seeds: different garbage
    assert not np.array_equal(fill_bytes(1, 64), fill_bytes(2, 64))


def test_a_clean_write_passes():
    written = np.zeros(1000, bool)
    written[:400] = True
    s = _output(written=written)
    _poke(s, 0, np.arange(400) & 0xFF)
    got = s.check()
    assert np.array_equal(got[:400], np.arange(400) & 0xFF)
    assert np.array_equal(got[400:], s.image[s.start + 400:s.start + 1000])
    full = _output()
    _poke(full, 0, np.zeros(1000))
    assert not full.check().any()
    with pytest.raises(ArenaDamage):                                                    # ... but a rejected call must not write at all
        full.check_untouched()
    _output().check_untouched()


def test_one_byte_before_the_payload():
    s = _output()
    _poke(s, -1, [_other(s, -1)])
    with pytest.raises(ArenaDamage) as e:
        s.check()
    assert (e.value.first, e.value.last, e.value.count, e.value.what) == (-1, -1, 1, "guard band")
    assert "payload-1" in str(e.value)


def test_one_byte_after_the_payload():
    s = _output()
    _poke(s, 1000, [_other(s, 1000)])
    with pytest.raises(ArenaDamage) as e:
        s.check()
    assert (e.value.first, e.value.last, e.value.count, e.value.what) == (1000, 1000, 1, "guard band")


def test_first_and_last_damaged_byte_are_reported():
    s = _output()
    _poke(s, -20, [_other(s, -20)])
    _poke(s, 1003, [_other(s, 1003)])
    _poke(s, GUARD_BYTES + 999, [_other(s, GUARD_BYTES + 999)])                       # the last byte of the back guard
    with pytest.raises(ArenaDamage) as e:
        s.check()
    assert (e.value.first, e.value.last, e.value.count) == (-20, GUARD_BYTES + 999, 3)


def test_one_byte_inside_a_declared_hole():
    written = np.ones(1000, bool)
    written[256:384] = False                                                            # a hole, as m_I in a tile
    s = _output(written=written)
    _poke(s, 0, np.zeros(256))
    _poke(s, 384, np.zeros(616))
    s.check()
    _poke(s, 300, [_other(s, 300)])
    with pytest.raises(ArenaDamage) as e:
        s.check()
    assert (e.value.first, e.value.last, e.value.count, e.value.what) == (300, 300, 1, "hole")


def test_an_input_must_not_change():
    a = Arena(HostMemory())
    s = a.input("in", np.arange(100, dtype=np.uint8), 16, 16, guard_seed=3)
    a.check()
    _poke(s, 7, [99])
    with pytest.raises(ArenaDamage) as e:
        a.check()
    assert (e.value.first, e.value.last, e.value.what) == (7, 7, "input")


def test_a_payload_aligned_more_than_asked_is_refused():
    with pytest.raises(ArenaAlignment):
        _output(align=16, displacement=32)                                              # 32-byte aligned when 16 was asked for
    with pytest.raises(ArenaAlignment):
        _output(align=16, displacement=8)                                               # not aligned at all
    with pytest.raises(ArenaAlignment):
        _output(align=1, displacement=2)                                                # "no alignment" must be an odd address
    for align, disp in ((16, 16), (16, 48), (8, 8), (8, 40), (4, 4), (4, 28), (1, 1), (1, 3)):
        s = _output(align=align, displacement=disp)
        assert s.ptr % align == 0 and s.ptr % (2 * align) != 0
    assert _output(align=16, displacement=0).ptr % 256 == 0                             # natural placement: not checked
    a = Arena(HostMemory())                                                             # a frame with a border: the address given counts
    s = a.input("ref", np.zeros(24 * 24, np.uint8), 1, 1, guard_seed=1, origin=4 * 24 + 4)
    assert s.ptr == s.buf.ptr + GUARD_BYTES + 1 + 100 and s.ptr % 2 == 1
    with pytest.raises(ArenaAlignment):
        a.input("ref", np.zeros(24 * 24, np.uint8), 1, 1, guard_seed=1, origin=3 * 24 + 3)
