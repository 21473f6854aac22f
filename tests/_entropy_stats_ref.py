"""The reference statement of the per-context bin statistics (include/x266hip.h, "per-context bin statistics on the device":
xEntropyStatsLevelsGpu, xEntropyStatsSideGpu, xEntropyInitFromCounts, xEntropyCountRegion, xEntropyCountSideCtu) and the data recipes of
their tests.  The counts are counted off the (context, bit) lists that tests/_entropy_ref.py (region_bins) and tests/_entropy_side_ref.py
(ctu_bins) enumerate -- the references the coders are held against --, the table rule is the header's in Python integers.  Nothing here
is derived from the library under test."""
import functools

import numpy as np

import _entropy_ref as E
import _entropy_side_ref as S
import _levels_ref as LR

REGIONS_PER_ROW = 32                                                      # X266_ENTROPY_STATS_REGIONS
CTUS_PER_ROW = 64                                                         # X266_ENTROPY_SIDE_STATS_CTUS
CLASSES = [c for c in range(16) if (S.CLASSES >> c) & 1]                  # the 13 classes of X266_TDECIDE_CLASSES


def rows(n, per_row):
    return -(-n // per_row)


def count(bins, n_contexts, first=0):
    """[n_contexts, 2] Python-integer counts (zero bins, one bins) of a list of (context or None, bit); context c counts at first + c"""
    out = [[0, 0] for _ in range(n_contexts)]
    for c, bit in bins:
        if c is not None:
            out[first + c][int(bit)] += 1
    return out


def region_counts(level, cls, coded=True):
    """what xEntropyCountRegion adds: uint64 [100, 2]"""
    k = int(cls) & 3
    if not coded:
        bins = [(E.CBF, 0)] * (64 >> (2 * k))
    else:
        bins = E.region_bins(level, k)
    return np.array(count(bins, E.CONTEXTS, E.PER_SIZE * k), np.uint64)


def levels_stats(levels, classes=None, nnz=None):
    """xEntropyStatsLevelsGpu -> (d_counts uint64 [100, 2], d_part uint32 [rows, 100, 2])"""
    lv = np.asarray(levels).reshape(-1, 1024)
    n = lv.shape[0]
    cls = LR._classes(classes, n)
    part = np.zeros((rows(n, REGIONS_PER_ROW), E.CONTEXTS, 2), np.uint32)
    for r in range(n):
        coded = nnz is None or int(np.asarray(nnz).ravel()[r]) != 0
        part[r // REGIONS_PER_ROW] += region_counts(lv[r], cls[r], coded).astype(np.uint32)
    return part.astype(np.uint64).sum(axis=0, dtype=np.uint64).reshape(E.CONTEXTS, 2), part


def ctu_counts(ctu, qp=32, off=0):
    """what xEntropyCountSideCtu adds for a canonical CTU: uint64 [16, 2]"""
    return np.array(count(S.ctu_bins(ctu, qp, off), S.CONTEXTS), np.uint64)


def side_stats(n_ctu, kind=None, mode=None, cls=None, qpa=None, nnz=None, qp=32, off=0):
    """xEntropyStatsSideGpu -> (d_counts uint64 [16, 2], d_part uint32 [rows, 16, 2])"""
    part = np.zeros((rows(n_ctu, CTUS_PER_ROW), S.CONTEXTS, 2), np.uint32)
    for c, ctu in enumerate(S.canon_arrays(n_ctu, kind, mode, cls, qpa, nnz, qp, off)):
        part[c // CTUS_PER_ROW] += ctu_counts(ctu, qp, off).astype(np.uint32)
    return part.astype(np.uint64).sum(axis=0, dtype=np.uint64).reshape(S.CONTEXTS, 2), part


def init_from_counts(counts):
    """the header's rule in Python integers: counts [n, 2] -> n table entries"""
    out = []
    for z, o in [(int(z), int(o)) for z, o in np.asarray(counts, dtype=object).reshape(-1, 2)]:
        n = z + o
        out.append(1024 if n == 0 else min(max((4096 * z + n) // (2 * n), E.P_MIN), E.P_MAX))
    return out


# ---- data ---------------------------------------------------------------------------------------------------------------------------------------
def special_regions(k):
    """[(name, levels [1024])] of block size k: the header's three worked regions, and (k >= 1) a block whose CG 0 is empty under a coded CG"""
    out = []
    for name, at, v in (("DC = 1", 0, 1), ("DC = -32768", 0, -32768), ("a 3 at index 1023", 1023, 3)):
        lv = np.zeros(1024, np.int16)
        lv[at] = v
        out.append((name, lv))
    if k >= 1:
        order = LR.region_order(k)
        lv = np.zeros(1024, np.int16)
        lv[int(order[2, 5])] = -2                                            # block 0: CG 2 coded, CG 0 and CG 1 empty
        if k < 3:
            lv[int(order[(1 << (2 * k)) + 1, 0])] = 7                        # block 1: CG 1 coded at its first position, CG 0 empty
        out.append(("CG 0 empty under a coded CG", lv))
    return out


@functools.lru_cache(None)
def level_frame(n, seed=5):
    """(levels [n, 1024], classes [n] over all 13 classes of the transform decision, true nnz [n]): _entropy_ref.mixed with the special
    regions of its size written over regions 0 and n - 1 and, where they exist, over both sides of the first row boundary"""
    lv, _ = E.mixed(max(n, 1), seed)
    lv = lv[:n].copy()
    cls = np.array([CLASSES[(5 * r + seed) % len(CLASSES)] for r in range(n)], np.uint8)
    for j, r in enumerate([0, n - 1, REGIONS_PER_ROW - 1, REGIONS_PER_ROW]):
        if 0 <= r < n:
            special = special_regions(int(cls[r]) & 3)
            lv[r] = special[(j + r) % len(special)][1]
    if n > 2:
        lv[1] = E.maximal()
    nnz = np.count_nonzero(lv, axis=1).astype(np.uint32)
    for a in (lv, cls, nnz):
        a.setflags(write=False)
    return lv, cls, nnz
