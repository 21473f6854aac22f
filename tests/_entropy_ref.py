"""The reference statement of the entropy coder of the level stream (include/x266hip.h, "the entropy coder": xEntropyEncodeLevelsGpu,
xEntropyDecodeLevelsGpu) in Python integers, and the data recipes of its test cases.  Written from the header, independently of
x266_entropy.hpp:

    encoder     `low` is ONE unbounded integer.  A renormalisation multiplies low and range by 256 and counts a shift; nothing is cached
                and no carry is ever propagated by hand.  After termination the substream is the big-endian bytes of low in 4 + shifts
                bytes, trailing zeros stripped (the C++ runs the 33-bit window with a cache byte and a pending run of 0xFF).
    syntax      walked over the region in scan order from _levels_ref.region_order, the last position found by a search from the end
                (the C++ starts from the coded-CG mask)
    bins        the encoder first lists its bins, (context id or None, bit), then codes the list: the count test reads the list
    decoder     the LZMA decoder on 32-bit values, every operation masked

Nothing here is derived from the library under test."""
import functools

import numpy as np

import _levels_ref as LR
import _rdoq_ref as RR

CONTEXTS = 100
PER_SIZE = 25
CBF, LAST_X, LAST_Y, CGF, SIG, GT1, GT2 = 0, 1, 10, 19, 20, 23, 24
P_MIN, P_MAX = 31, 2017
MAX_BYTES = 6848
RECORD_DTYPE = np.dtype([("ctx_bins", "<u4"), ("bypass_bins", "<u4"), ("offset", "<u8"), ("n_words", "<u4"), ("n_bytes", "<u4"), ("n_nz", "<u4"),
                         ("reserved", "<u4")])
assert RECORD_DTYPE.itemsize == 32
M32 = 0xFFFFFFFF


def p_zero(c0, c1):
    """the probability of a zero bin, in 1/2048, from the costs of a zero and of a one in 1/16 bit"""
    a, b = 2.0 ** (-c0 / 16.0), 2.0 ** (-c1 / 16.0)
    return min(max(int(np.floor(2048.0 * a / (a + b) + 0.5)), P_MIN), P_MAX)


def default_init(sig=RR.SIG, gt1=(10, 24), gt2=(11, 22), cgf=RR.CGF):
    row = [1024] * 19 + [p_zero(*cgf)] + [p_zero(*s) for s in sig] + [p_zero(*gt1), p_zero(*gt2)]
    return np.array(row * 4, np.uint16)


def worst_init():
    """the least favourable table for a region of large levels: every bin of such a region is a one, so every zero-probability at its top"""
    return np.full(CONTEXTS, P_MAX, np.uint16)


def group(t):
    """g of pos(t)"""
    if t < 4:
        return t
    k = t.bit_length() - 1
    return 2 * k + ((t >> (k - 1)) & 1)


# ---- the bins of a region ---------------------------------------------------------------------------------------------------------------------
def last_bins(t, n, base):
    g, top = group(t), 2 * n - 1
    bins = [(base + i, 1) for i in range(g)]
    if g < top:
        bins.append((base + g, 0))
    if g >= 4:
        count = (g >> 1) - 1
        bins += [(None, (t >> i) & 1) for i in reversed(range(count))]
    return bins


def level_bins(l):
    a = abs(l)
    bins = [(GT1, int(a > 1))]
    if a > 1:
        bins.append((GT2, int(a > 2)))
    if a > 2:
        r = a - 3
        bins += [(None, 1)] * min(r, 3)
        if r < 3:
            bins.append((None, 0))
        else:
            v = r - 3 + 1                                                     # Exp-Golomb order 0 of r - 3
            k = v.bit_length() - 1
            bins += [(None, 1)] * k + [(None, 0)] + [(None, (v >> i) & 1) for i in reversed(range(k))]
    bins.append((None, int(l < 0)))
    return bins


def region_bins(level, k):
    """the bins of a region of class k in coding order: (context id inside the block size's 25, or None for bypass, bit)"""
    lv = [int(x) for x in np.asarray(level).ravel()]
    assert len(lv) == 1024
    size, n = 4 << k, k + 2
    per_block = (size // 4) ** 2
    order = LR.region_order(k)
    bins = []
    for blk in range(64 // per_block):
        idx = [int(order[blk * per_block + s, i]) for s in range(per_block) for i in range(16)]      # the block in scan order
        vals = [lv[j] for j in idx]
        nz = [i for i, x in enumerate(vals) if x]
        bins.append((CBF, int(bool(nz))))
        if not nz:
            continue
        p = nz[-1]
        inside = idx[p] - blk * size * size
        bins += last_bins(inside % size, n, LAST_X) + last_bins(inside // size, n, LAST_Y)
        sp = p // 16
        for s in range(sp + 1):
            coded = any(vals[16 * s:16 * s + 16])
            if 0 < s < sp:
                bins.append((CGF, int(coded)))
                if not coded:
                    continue
            for i in range(16 * s, min(16 * s + 15, p) + 1):
                cls = 0 if i == 0 else 1 if s == 0 else 2
                if i != p:
                    bins.append((SIG + cls, int(vals[i] != 0)))
                if vals[i]:
                    bins += level_bins(vals[i])
    return bins


# ---- the coder ----------------------------------------------------------------------------------------------------------------------------------
def code_bins(bins, ctx):
    """the substream of a list of bins; ctx: the 25 probabilities, adapted in place"""
    low, rng, shifts = 0, M32, 0
    for c, bit in bins:
        if c is None:
            rng >>= 1
            if bit:
                low += rng
        else:
            p = ctx[c]
            bound = (rng >> 11) * p
            if bit:
                low += bound
                rng -= bound
                ctx[c] = p - (p >> 5)
            else:
                rng = bound
                ctx[c] = p + ((2048 - p) >> 5)
        while rng < 1 << 24:
            rng <<= 8
            low <<= 8
            shifts += 1
    low = (low + 0xFFFFFF) & ~0xFFFFFF
    return low.to_bytes(4 + shifts, "big").rstrip(b"\0")                       # the leading byte, byte 5 + shifts from the end, is always 0


def _init(init, k):
    table = default_init() if init is None else np.asarray(init)
    assert table.size == CONTEXTS and table.min() >= P_MIN and table.max() <= P_MAX
    return [int(x) for x in table[PER_SIZE * k:PER_SIZE * (k + 1)]]


def encode_region(level, k=3, init=None):
    """-> (bytes, context bins, bypass bins)"""
    bins = region_bins(level, k)
    data = code_bins(bins, _init(init, k))
    n_ctx = sum(1 for c, _ in bins if c is not None)
    return data, n_ctx, len(bins) - n_ctx


class Malformed(Exception):
    pass


class Decoder:
    def __init__(self, data, ctx):
        self.data, self.at, self.ctx = bytes(data), 0, ctx
        self.rng, self.code = M32, 0
        for _ in range(4):
            self.code = ((self.code << 8) | self.byte()) & M32

    def byte(self):
        b = self.data[self.at] if self.at < len(self.data) else 0
        self.at += 1
        return b

    def norm(self):
        if self.rng < 1 << 24:
            self.rng = (self.rng << 8) & M32
            self.code = ((self.code << 8) | self.byte()) & M32

    def bin(self, c):
        p = self.ctx[c]
        bound = (self.rng >> 11) * p
        if self.code < bound:
            self.rng, bit = bound, 0
            self.ctx[c] = p + ((2048 - p) >> 5)
        else:
            self.code, self.rng, bit = (self.code - bound) & M32, (self.rng - bound) & M32, 1
            self.ctx[c] = p - (p >> 5)
        self.norm()
        return bit

    def bypass(self):
        self.rng >>= 1
        bit = 0
        if self.code >= self.rng:
            self.code, bit = (self.code - self.rng) & M32, 1
        self.norm()
        return bit

    def bits(self, count):
        v = 0
        for _ in range(count):
            v = (v << 1) | self.bypass()
        return v

    def last(self, n, base):
        g = 0
        while g < 2 * n - 1 and self.bin(base + g):
            g += 1
        if g < 4:
            return g
        count = (g >> 1) - 1
        return ((2 | (g & 1)) << count) | self.bits(count)

    def level(self):
        a = 1
        if self.bin(GT1):
            a = 2
            if self.bin(GT2):
                r = 0
                while r < 3 and self.bypass():
                    r += 1
                if r == 3:
                    k = 0
                    while k < 15 and self.bypass():
                        k += 1
                    if k > 14:
                        raise Malformed("prefix")
                    r = 3 + ((1 << k) | self.bits(k)) - 1
                a = 3 + r
        negative = self.bypass()
        if a > 32768 or (a == 32768 and not negative):
            raise Malformed("magnitude")
        return -a if negative else a


def decode_region(data, k=3, init=None):
    """-> (levels int16 [1024], n_nz), or (zeros, 0) with malformed=True: (levels, n_nz, malformed)"""
    size, n = 4 << k, k + 2
    per_block = (size // 4) ** 2
    order = LR.region_order(k)
    d = Decoder(data, _init(init, k))
    out = np.zeros(1024, np.int16)
    count = 0
    try:
        for blk in range(64 // per_block):
            if not d.bin(CBF):
                continue
            u = d.last(n, LAST_X)
            v = d.last(n, LAST_Y)
            assert u < size and v < size                                          # by construction
            target = blk * size * size + v * size + u
            where = np.argwhere(order[blk * per_block:(blk + 1) * per_block] == target)[0]
            p = int(where[0]) * 16 + int(where[1])
            sp = p // 16
            for s in range(sp + 1):
                if 0 < s < sp and not d.bin(CGF):
                    continue
                for i in range(16 * s, min(16 * s + 15, p) + 1):
                    cls = 0 if i == 0 else 1 if s == 0 else 2
                    if i != p and not d.bin(SIG + cls):
                        continue
                    out[order[blk * per_block + s, i - 16 * s]] = d.level()
                    count += 1
    except Malformed:
        return np.zeros(1024, np.int16), 0, True
    return out, count, False


# ---- the calls ----------------------------------------------------------------------------------------------------------------------------------
def encode(levels, classes=None, nnz=None, cap_words=None, init=None):
    """xEntropyEncodeLevelsGpu -> (records [n] RECORD_DTYPE, stream uint16 [cap_words], total uint64 [2]); cap_words None: exactly the total.
    Words the call does not write are 0 here."""
    return assemble(code_regions(levels, classes, nnz, init), cap_words)


def code_regions(levels, classes=None, nnz=None, init=None):
    """per region (substream, context bins, bypass bins, non-zero levels): regions are independent, so a prefix of the list is the coding of
    the prefix of the regions"""
    lv = np.asarray(levels).reshape(-1, 1024)
    cls = LR._classes(classes, lv.shape[0])
    coded = []
    for r in range(lv.shape[0]):
        region = lv[r] if nnz is None or int(np.asarray(nnz).ravel()[r]) != 0 else np.zeros(1024, np.int16)
        coded.append(encode_region(region, int(cls[r]), init) + (int(np.count_nonzero(region)),))
    return coded


def assemble(coded, cap_words=None):
    """records, stream and totals of a list of coded regions"""
    n = len(coded)
    rec = np.zeros(n, RECORD_DTYPE)
    payloads = []
    for r, (data, n_ctx, n_byp, n_nz) in enumerate(coded):
        payloads.append(data + b"\0" * (len(data) & 1))
        rec["ctx_bins"][r], rec["bypass_bins"][r] = n_ctx, n_byp
        rec["n_bytes"][r], rec["n_words"][r], rec["n_nz"][r] = len(data), (len(data) + 1) // 2, n_nz
    ends = np.cumsum(rec["n_words"].astype(np.uint64), dtype=np.uint64)
    rec["offset"] = ends - rec["n_words"]
    total = int(ends[-1]) if n else 0
    cap = total if cap_words is None else int(cap_words)
    stream = np.zeros(cap, np.uint16)
    fit = 0
    for r in range(n):
        off, nw = int(rec["offset"][r]), int(rec["n_words"][r])
        if off + nw > cap:
            continue
        fit += 1
        stream[off:off + nw] = np.frombuffer(payloads[r], "<u2")
    return rec, stream, np.array([total, fit], np.uint64)


def decode(records, stream, n_regions, classes=None, cap_words=None, init=None):
    """xEntropyDecodeLevelsGpu -> (levels int16 [n, 1024], nnz uint32 [n], malformed bool [n]); only offset and n_bytes of a record are
    trusted, both held against cap_words; a region outside, or longer than MAX_BYTES, is zeros"""
    words = np.asarray(stream, np.uint16).ravel()
    cap = words.size if cap_words is None else int(cap_words)
    raw = words[:cap].astype("<u2").tobytes()
    cls = LR._classes(classes, n_regions)
    out = np.zeros((n_regions, 1024), np.int16)
    nnz = np.zeros(n_regions, np.uint32)
    bad = np.zeros(n_regions, bool)
    for r in range(n_regions):
        off, nb = int(records["offset"][r]), int(records["n_bytes"][r])
        if nb > MAX_BYTES or off > cap or (nb + 1) // 2 > cap - off:
            bad[r] = True
            continue
        out[r], nnz[r], bad[r] = decode_region(raw[2 * off:2 * off + nb], int(cls[r]), init)
    return out, nnz, bad


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def mixed(n, seed=3):
    """_levels_ref.mixed with a few large levels, -32768 among them, so that every branch of the remainder is taken"""
    lv, cls = LR.mixed(n, seed)
    lv = lv.copy()
    rng = np.random.RandomState(seed + 100)
    for r in range(0, n, 3):
        if lv[r].any():
            at = rng.randint(0, 1024, 4)
            lv[r, at] = [-32768, 32767, -3, 300]
    return lv, cls


def maximal():
    """all 1024 levels at +-32767: the longest region there is under worst_init()"""
    sign = np.where(np.arange(1024) % 3 == 0, -1, 1)
    return (32767 * sign).astype(np.int16)
