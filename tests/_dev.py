"""Device memory for the GPU tests through the C ABI only (xHipMalloc / xHipMemcpy*), and a ctypes view of the HIP
runtime THE LIBRARY loaded -- no torch in a test process: the library is validated on the runtime it is built for
(ROCm's libamdhip64 / librccl), which is what a plain-C host gets.

`Dev(codec)` hands out small tensor-like objects with the handful of methods the tests use (data_ptr, numel, stride,
cpu().numpy(), clone) so that test bodies read as they did when torch supplied the memory.

Below them is the kit every device test stands on: plain functions, no fixtures.  `sync_or_exit` is the suite's safety rule and its
only statement: after a device error nothing more is started on that GPU."""
import ctypes
import re

import numpy as np
import pytest

from x266_amd import X266Error

# _arena and _util are imported where they are used: tools/probes imports this module as tests._dev, without tests/ on its path
EINVAL = -1


def loaded_libraries(pattern):
    """paths of the shared objects mapped into this process whose file name matches `pattern` (a regex)"""
    seen = []
    for line in open("/proc/self/maps"):
        parts = line.split()
        if len(parts) >= 6 and re.search(pattern, parts[5].rsplit("/", 1)[-1]) and parts[5] not in seen:
            seen.append(parts[5])
    return seen


def hip_runtime():
    """ctypes handle of the libamdhip64 this process runs on (the library's own: there must be exactly one)"""
    import x266_amd
    x266_amd.load_library()
    libs = loaded_libraries(r"^libamdhip64\.so")
    assert len(libs) == 1, "expected exactly one HIP runtime in the process, found %r" % (libs,)
    return ctypes.CDLL(libs[0])


class DevArray:
    def __init__(self, codec, shape, dtype):
        self.codec = codec
        self.shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.dtype = np.dtype(dtype)
        self._n = int(np.prod(self.shape)) if self.shape else 1
        self.buf = codec.alloc(max(self._n * self.dtype.itemsize, 16))

    def data_ptr(self):
        return self.buf.ptr

    def numel(self):
        return self._n

    def stride(self, axis):
        s = 1
        for d in self.shape[axis + 1:]:
            s *= d
        return s

    def numpy(self):
        self.codec.stream_sync()
        return self.buf.download(self.dtype, self._n).reshape(self.shape)

    def cpu(self):
        return self

    def clone(self):
        c = DevArray(self.codec, self.shape, self.dtype)
        c.buf.upload(self.numpy())
        return c

    def upload(self, a):
        a = np.ascontiguousarray(a, self.dtype)
        assert a.size == self._n
        self.buf.upload(a)


class Dev:
    """factory bound to one context (= one device)"""

    def __init__(self, codec):
        self.codec = codec

    def from_numpy(self, a):
        a = np.ascontiguousarray(a)
        t = DevArray(self.codec, a.shape, a.dtype)
        t.buf.upload(a)
        return t

    def zeros(self, shape, dtype):
        t = DevArray(self.codec, shape, dtype)
        t.buf.upload(np.zeros(t._n, t.dtype))
        return t

    def empty(self, shape, dtype):
        return DevArray(self.codec, shape, dtype)

    def empty_like(self, t):
        return DevArray(self.codec, t.shape, t.dtype)

    def random_u8(self, shape, seed):
        return self.from_numpy(np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8))

    def synchronize(self):
        self.codec.stream_sync()

    @staticmethod
    def equal(a, b):
        return a.shape == b.shape and np.array_equal(a.numpy(), b.numpy())


# ---- the kit ----------------------------------------------------------------------------------------------------------------------------
def dev(codec, arr):
    """a device buffer that holds `arr`"""
    arr = np.ascontiguousarray(arr)
    d = codec.alloc(max(arr.nbytes, 16))
    d.upload(arr)
    return d


def sync_or_exit(codec, rc, stream=None):
    """sync the stream the call ran on; a device error (a failed sync, or a status that is neither success nor a refusal) ends the session"""
    sync = codec.L.xHipStreamSync(codec.ctx, stream)
    if sync != 0 or rc not in (0, EINVAL):                                  # a device error: nothing more is started on this GPU
        pytest.exit("device error (call %d, sync %d): %s" % (rc, sync, codec.L.xHipLastError(codec.ctx).decode()), returncode=3)


def run(codec, fn, *args, **kw):
    """a ..._dev call that must succeed, then a sync; a device error ends the session"""
    try:
        fn(*args, **kw)
    except X266Error:
        sync_or_exit(codec, -2)
        raise
    sync_or_exit(codec, 0, kw.get("stream") or None)


def call_struct(codec, name, p, stream=None):
    """a call that takes one parameter struct and must succeed, then a sync"""
    rc = getattr(codec.L, name)(codec.ctx, ctypes.byref(p), stream)
    sync_or_exit(codec, rc, stream)
    assert rc == 0, (name, codec.L.xHipLastError(codec.ctx))


def noise(n, seed):
    from _util import splitmix64
    return (splitmix64(seed, 0, n) & np.uint64(255)).astype(np.uint8)


def sentinels(w, h, seed=77):
    """the pre-fill of a w x h tile array"""
    return noise(w * h * 2, seed)


def same(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], want[bad[:8]])


def tiles(oracle, planes, seed):
    """the tile array of the planes (y, u, v) with random m_I bytes (which no call may read)"""
    t = oracle.conv_input_fmt(*planes).reshape(-1, 512)
    t[:, 384:] = noise(t.shape[0] * 128, seed).reshape(-1, 128)
    return t.ravel()


def records(mv, cost=None):
    """the x266_me_result_t array of the vectors; cost None leaves the cost field 0"""
    rec = np.zeros((len(mv), 4), np.int16)
    rec[:, :2] = mv
    if cost is not None:
        rec.view(np.uint32)[:, 1] = cost
    return rec


def displacements(ptrs, halved=None):
    """{pointer: (displacement, alignment)} of {pointer: alignment}: every pointer at exactly its documented alignment and no more (odd
    multiples, varying between the buffers); `halved`: that one at half its alignment"""
    return {p: (align // 2, align // 2) if p == halved else (align * (2 * i + 1), align) for i, (p, align) in enumerate(ptrs.items())}


def tile_written(n_tiles, planes):
    """the bytes of a tile array that a call on `planes` ("luma", "chroma", "both") writes: m_I, and the planes it does not own, are holes"""
    written = np.zeros((n_tiles, 512), bool)
    written[:, {"luma": slice(0, 256), "chroma": slice(256, 384), "both": slice(0, 384)}[planes]] = True
    return written.ravel()


def arena_slots(memory, ptrs, outputs, data, disp, guard_seed, written=None, sizes=None):
    """(arena, {pointer: slot}): one slot per pointer of `ptrs`, placed in that order by `disp` (see displacements).  An input holds
    data[p] between guards of seed guard_seed + its index in `ptrs`; an output is sizes[p] bytes (default: as many as data[p]) of
    fill, of which the call writes the mask written[p] (default: all)."""
    from _arena import Arena
    a, s = Arena(memory), {}
    for i, p in enumerate(ptrs):
        where, align = disp[p]
        if p in outputs:
            nbytes = sizes[p] if sizes and p in sizes else data[p].nbytes
            s[p] = a.output(p, nbytes, align, where, written=written.get(p) if written else None)
        else:
            s[p] = a.input(p, data[p], align, where, guard_seed + i)
    return a, s
