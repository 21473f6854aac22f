"""CPU: the kit of the device tests (tests/_dev.py) on a stub codec whose stream sync and last error are Python functions that record
their arguments, and on the host stand-in for device memory of tests/_arena.py."""
import types

import numpy as np
import pytest

import _dev as K
from _arena import ArenaDamage, HostMemory
from _util import splitmix64
from x266_amd import X266Error


class Stub:
    """a codec as far as sync_or_exit looks: L.xHipStreamSync returns `sync` and records the stream it was given"""

    def __init__(self, sync=0):
        self.ctx, self.synced, self.asked = object(), [], 0
        self.L = types.SimpleNamespace(xHipStreamSync=self._sync, xHipLastError=self._last)
        self.sync = sync

    def _sync(self, ctx, stream):
        assert ctx is self.ctx
        self.synced.append(stream)
        return self.sync

    def _last(self, ctx):
        assert ctx is self.ctx
        self.asked += 1
        return b"stub error"


@pytest.mark.parametrize("rc,sync,exits", [(0, 0, False), (K.EINVAL, 0, False), (-2, 0, True), (0, 1, True)])
def test_sync_or_exit(rc, sync, exits):
    c, stream = Stub(sync), object()
    if exits:
        with pytest.raises(pytest.exit.Exception) as e:
            K.sync_or_exit(c, rc, stream)
        assert e.value.returncode == 3 and c.asked == 1
    else:
        K.sync_or_exit(c, rc, stream)
    assert c.synced == [stream]                                             # the stream it was given is the stream it syncs
    K.sync_or_exit(Stub(), 0)
    c = Stub()
    K.sync_or_exit(c, 0)
    assert c.synced == [None]                                               # the callers of the old two-argument form: the null stream


def test_run():
    c, stream, seen = Stub(), object(), []
    K.run(c, lambda *a, **kw: seen.append((a, kw)), 1, 2, stream=stream)
    assert seen == [((1, 2), {"stream": stream})] and c.synced == [stream]

    def refuses(*a, **kw):
        raise X266Error("refused")

    # a call that must succeed and raises counts as X266HIP_EDEVICE (-2), as in every copy of this function before the kit: the null
    # stream is synced once and the session ends, whatever the sync says, so the X266Error itself never reaches the test
    for sync in (0, 1):
        c = Stub(sync)
        with pytest.raises(pytest.exit.Exception) as e:
            K.run(c, refuses, 1, stream=stream)
        assert e.value.returncode == 3 and c.synced == [None] and "call -2, sync %d" % sync in str(e.value)
    c = Stub(sync=1)
    with pytest.raises(pytest.exit.Exception) as e:                         # the call succeeds, the sync reports an error
        K.run(c, lambda **kw: None, stream=stream)
    assert e.value.returncode == 3 and c.synced == [stream]


def test_displacements():
    ptrs = {"a": 1, "b": 4, "c": 8, "d": 16}
    d = K.displacements(ptrs)
    assert list(d) == list(ptrs)
    for p, align in ptrs.items():
        where, exact = d[p]
        assert exact == align and where % align == 0 and (where // align) % 2 == 1   # an odd multiple: aligned to no more than `align`
    assert len({where // align for (where, align) in d.values()}) == 4                # varying between the buffers
    for halved in ("b", "c", "d"):
        h = K.displacements(ptrs, halved=halved)
        assert h[halved] == (ptrs[halved] // 2, ptrs[halved] // 2)
        assert {p: v for p, v in h.items() if p != halved} == {p: v for p, v in d.items() if p != halved}


def test_records():
    mv = np.array([[1, -2], [32767, -32768], [0, 5]], np.int16)
    for cost, want in ((None, 0), (12345, 12345), (0xFFFFFFFF, 0xFFFFFFFF)):
        rec = K.records(mv, cost)
        assert rec.dtype == np.int16 and rec.shape == (3, 4)
        assert np.array_equal(rec[:, :2], mv) and (rec.view(np.uint32)[:, 1] == want).all()
    per_block = np.array([7, 0, 0xFFFFFFFF], np.uint32)
    assert np.array_equal(K.records(mv, per_block).view(np.uint32)[:, 1], per_block)


def test_tile_written():
    for planes, first, count in (("luma", 0, 256), ("chroma", 256, 128), ("both", 0, 384)):
        m = K.tile_written(6, planes)
        assert m.dtype == bool and m.shape == (6 * 512,)
        m = m.reshape(6, 512)
        assert (m.sum(axis=1) == count).all() and m[:, first:first + count].all()


def test_tiles_noise_and_sentinels(oracle):
    w, h = 64, 32
    y, u, v = K.noise(w * h, 1).reshape(h, w), K.noise(w * h // 4, 2).reshape(h // 2, w // 2), K.noise(w * h // 4, 3).reshape(h // 2, w // 2)
    t = K.tiles(oracle, (y, u, v), 9).reshape(-1, 512)
    assert t.shape[0] == 8 and t.dtype == np.uint8
    assert np.array_equal(t[:, :384], oracle.conv_input_fmt(y, u, v).reshape(-1, 512)[:, :384])
    assert np.array_equal(t[:, 384:].ravel(), (splitmix64(9, 0, 128 * 8) & np.uint64(255)).astype(np.uint8))
    assert np.array_equal(K.noise(100, 5), (splitmix64(5, 0, 100) & np.uint64(255)).astype(np.uint8))
    assert np.array_equal(K.sentinels(w, h), K.noise(w * h * 2, 77)) and np.array_equal(K.sentinels(w, h, 5), K.noise(w * h * 2, 5))


def test_same():
    a = np.arange(10)
    K.same(a, a.copy(), "equal")
    with pytest.raises(AssertionError):
        K.same(a, a + (a == 7), "differs")


def test_dev():
    d = K.dev(HostMemory(), np.arange(3, dtype=np.uint8))
    assert d.nbytes == 16 and d.download(np.uint8, 3).tolist() == [0, 1, 2]  # never an empty allocation


def _slots(disp=None):
    ptrs = {"d_in": 16, "d_side": 4, "d_out": 16, "d_n": 4}
    data = {"d_in": K.noise(1024, 1), "d_side": np.arange(8, dtype=np.uint32), "d_n": np.zeros(6, np.uint32)}
    return K.arena_slots(HostMemory(), ptrs, ("d_out", "d_n"), data, disp or K.displacements(ptrs), 31,
                         written={"d_out": K.tile_written(2, "both")}, sizes={"d_out": 1024}), ptrs, data


def test_arena_slots():
    (a, s), ptrs, data = _slots()
    assert list(s) == list(ptrs) and [x.name for x in a.slots] == list(ptrs)   # one slot per pointer, in ptrs order
    assert [x.is_output for x in a.slots] == [False, False, True, True]
    assert s["d_out"].size == 1024 and s["d_n"].size == 24 and s["d_side"].size == 32
    assert np.array_equal(s["d_in"].payload(), data["d_in"]) and s["d_out"].written.sum() == 768 and s["d_n"].written is None
    for p, align in ptrs.items():
        assert s[p].ptr % align == 0 and s[p].ptr % (2 * align) != 0
    a.check()
    a.check_untouched()
    for slot, at in ((s["d_in"], s["d_in"].start - 1), (s["d_out"], s["d_out"].start + s["d_out"].size), (s["d_out"], s["d_out"].start + 400)):
        slot.buf.bytes[at] ^= 0xFF                                          # a guard in front, a guard behind, m_I of an output
        with pytest.raises(ArenaDamage):
            a.check()
        slot.buf.bytes[at] ^= 0xFF
    a.check()
    (_, half), _, _ = _slots(K.displacements(ptrs, halved="d_side"))
    assert half["d_side"].ptr % 4 == 2 and half["d_in"].ptr == s["d_in"].ptr # that pointer alone sits at half its alignment
    (b, t), _, _ = _slots()
    (c, r), _, _ = K.arena_slots(HostMemory(), ptrs, ("d_out", "d_n"), data, K.displacements(ptrs), 32, sizes={"d_out": 1024}), 0, 0
    assert all(np.array_equal(s[p].image, t[p].image) for p in ptrs)        # the same seed: the same bytes
    assert not np.array_equal(s["d_in"].image, r["d_in"].image) and np.array_equal(s["d_out"].image, r["d_out"].image)   # the seed is the inputs' guards
