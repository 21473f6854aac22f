"""The compact level stream of include/x266hip.h (xLevelsPackGpu, xLevelsUnpackGpu, xLevelScan) in numpy int64: scan, pack, unpack,
and the fixtures the CPU and the GPU tests share.  Vectorised over regions; tests/test_levels_ref.py holds it against plain loops."""
import functools

import numpy as np

REGION = 1024
MAX_WORDS = 64 + 1024
RECORD_DTYPE = np.dtype([("cg_mask", "<u8"), ("offset", "<u8"), ("n_words", "<u4"), ("n_nz", "<u4"), ("sum_abs", "<u4"), ("max_abs", "<u4")])
assert RECORD_DTYPE.itemsize == 32


def diag(m):
    """the (x, y) of the diagonal scan of an m x m grid: by x + y ascending, then by x ascending"""
    return sorted(((x, y) for y in range(m) for x in range(m)), key=lambda p: (p[0] + p[1], p[0]))


@functools.lru_cache(None)
def scan(size):
    """xLevelScan: pos[s * 16 + i] = v * size + u of scan position i of CG s of a size x size block"""
    assert size in (4, 8, 16, 32)
    pos = []
    for cgx, cgy in diag(size // 4):
        for x, y in diag(4):
            pos.append((4 * cgy + y) * size + 4 * cgx + x)
    return np.array(pos, np.int64)


@functools.lru_cache(None)
def region_order(k):
    """[64, 16]: the index inside a region of class k (N = 4 << k) of scan position i of CG bit g"""
    n = 4 << k
    blocks = (32 // n) ** 2
    one = scan(n)
    return np.concatenate([b * n * n + one for b in range(blocks)]).reshape(64, 16)


def _classes(classes, n):
    if classes is None:
        return np.full(n, 3, np.int64)
    c = np.asarray(classes).astype(np.int64).ravel() & 3
    assert c.size == n
    return c


def _popcount16(x):
    x = np.asarray(x, np.int64)
    return sum((x >> i) & 1 for i in range(16))


def pack(levels, classes=None, nnz=None, cap_words=None):
    """-> (records [n] RECORD_DTYPE, stream uint16 [max(cap_words, 0)], total uint64 [2]).  cap_words None: exactly the total.  Words of
    the stream that the call does not write are 0 here (the device leaves them as they were)."""
    lv = np.asarray(levels).astype(np.int64).reshape(-1, REGION)
    n = lv.shape[0]
    cls = _classes(classes, n)
    ordered = np.empty((n, 64, 16), np.int64)
    for k in range(4):
        sel = cls == k
        if sel.any():
            ordered[sel] = lv[sel][:, region_order(k)]
    if nnz is not None:
        ordered[np.asarray(nnz).ravel() == 0] = 0
    sig = ordered != 0
    maps = (sig.astype(np.int64) << np.arange(16)).sum(2)                     # [n, 64]
    coded = maps != 0
    rec = np.zeros(n, RECORD_DTYPE)
    rec["cg_mask"] = (coded.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(1, dtype=np.uint64)
    rec["n_nz"] = sig.sum((1, 2))
    rec["n_words"] = coded.sum(1) + rec["n_nz"]
    rec["sum_abs"] = np.abs(ordered).sum((1, 2))
    rec["max_abs"] = np.abs(ordered).max((1, 2)) if n else 0
    ends = np.cumsum(rec["n_words"].astype(np.uint64), dtype=np.uint64)
    rec["offset"] = ends - rec["n_words"]
    total_words = int(ends[-1]) if n else 0
    cap = total_words if cap_words is None else int(cap_words)
    stream = np.zeros(cap, np.uint16)
    fit = 0
    for r in range(n):
        off, nw = int(rec["offset"][r]), int(rec["n_words"][r])
        if off + nw > cap:
            continue
        fit += 1
        if nw:
            c = coded[r]
            payload = np.concatenate([maps[r][c], ordered[r][c][sig[r][c]]])
            stream[off:off + nw] = payload.astype(np.int64).astype(np.uint16)
    return rec, stream, np.array([total_words, fit], np.uint64)


def unpack(records, stream, n_regions, classes=None, cap_words=None):
    """-> (levels int16 [n_regions, 1024], nnz uint32 [n_regions]); only cg_mask and offset of a record are trusted, and nothing at or
    beyond cap_words (None: len(stream)) is read"""
    stream = np.asarray(stream, np.uint16).ravel()
    cap = stream.size if cap_words is None else int(cap_words)
    assert cap <= stream.size
    cls = _classes(classes, n_regions)
    out = np.zeros((n_regions, REGION), np.int16)
    nnz = np.zeros(n_regions, np.uint32)
    for r in range(n_regions):
        mask, off = int(records["cg_mask"][r]), int(records["offset"][r])
        bits = [g for g in range(64) if (mask >> g) & 1]
        if off + len(bits) > cap:
            continue
        maps = stream[off:off + len(bits)].astype(np.int64)
        counts = _popcount16(maps) if len(bits) else np.zeros(0, np.int64)
        total = int(counts.sum())
        if off + len(bits) + total > cap:
            continue
        at = off + len(bits)
        order = region_order(int(cls[r]))
        for g, m in zip(bits, maps):
            for i in range(16):
                if (int(m) >> i) & 1:
                    out[r, order[g, i]] = stream[at:at + 1].view(np.int16)[0]
                    at += 1
        nnz[r] = total
    return out, nnz


# ---- the fixtures the CPU and GPU tests share ------------------------------------------------------------------------------------------
def one_hot(k):
    """1024 regions of class k, region i with one non-zero level at index i: every entry of every scan table"""
    lv = np.zeros((1024, REGION), np.int16)
    lv[np.arange(1024), np.arange(1024)] = ((np.arange(1024) * 37) % 255 - 127) | 1
    return lv, np.full(1024, k, np.uint8)


def dense(n=3, seed=5):
    """every level non-zero, the two int16 extremes included: 1088 words per region"""
    rng = np.random.RandomState(seed)
    lv = rng.randint(1, 32768, (n, REGION)).astype(np.int64) * rng.choice([-1, 1], (n, REGION))
    lv[0, 0], lv[0, 1023], lv[-1, 17] = -32768, 32767, -32768
    return lv.astype(np.int16)


def sparse(seed=11):
    """[4 classes x 10 regions]: geometric magnitudes, and per class: a coded region with an uncoded CG, a region with all 64 CGs coded,
    a level of -32768 and one of 32767, an all-zero region between two coded ones.  The class bytes carry garbage above their low bits."""
    rng = np.random.RandomState(seed)
    per = 10
    lv = np.zeros((4 * per, REGION), np.int64)
    cls = np.zeros(4 * per, np.uint8)
    for k in range(4):
        order = region_order(k)
        for j in range(per):
            r = k * per + j
            cls[r] = k | (int(rng.randint(0, 64)) << 2)
            if j == 4:
                continue                                                       # all zero, between two coded ones
            density = (0.002, 0.01, 0.05, 0.2, 0.0, 0.5, 0.03, 0.01, 0.1, 0.02)[j]
            hit = rng.rand(REGION) < density
            mag = np.minimum(rng.geometric(0.3 if j % 2 else 0.05, REGION), 32767) * rng.choice([-1, 1], REGION)
            lv[r] = np.where(hit, mag, 0)
            if j == 3:
                lv[r, order[:, 0]] = rng.choice([-3, 1, 2], 64)                 # all 64 CGs coded
                lv[r, order[5, 15]] = 0
            if j == 0:
                lv[r, order[9]] = 0                                            # an uncoded CG in a coded region
                lv[r, order[63, 15]] = -32768
                lv[r, order[0, 0]] = 32767
            if j in (5, 6) and not lv[r].any():
                lv[r, 0] = 1
    return lv.astype(np.int16), cls


def mixed(n, seed=3):
    """n regions of mixed classes and mixed sparsity, some all zero"""
    rng = np.random.RandomState(seed)
    cls = rng.randint(0, 256, n).astype(np.uint8)
    density = rng.choice([0.0, 0.003, 0.03, 0.3], n)[:, None]
    mag = np.minimum(rng.geometric(0.2, (n, REGION)), 32767) * rng.choice([-1, 1], (n, REGION))
    lv = np.where(rng.rand(n, REGION) < density, mag, 0)
    return lv.astype(np.int16), cls
