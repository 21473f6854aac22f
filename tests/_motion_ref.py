"""The reference statement of the compact motion stream (include/x266hip.h, "compact motion stream": xMotionPackGpu, xMotionUnpackGpu) in
numpy and Python integers, and the data recipes of its test cases.  Written from the header, independently of x266_motion.hpp: the walk is
the recursion over the quadtree (the C++ asks, per block, which of its nodes is the partition), coding order is a list that the recursion
appends to (the C++ sorts nothing: it relies on ascending Morton order), "precedes" compares positions in that list's order.

    geometry        _partition_ref's: whole / exists of the node (nx, ny) of level k; CTUs are the nodes of level 3 in raster order
    morton(x, y)    bit 2b of i is bit b of x, bit 2b + 1 is bit b of y
    pack's walk     from level 3 down: a whole node whose first block says (level & 3) >= k is one partition, else it splits (a whole node
                    that splits costs one flag bit); a cut node always splits; children TL, TR, BL, BR; level 0 ends the walk
    predictor       A = (X - 1, Y), B = (X, Y - 1), C = (X + n, Y - 1) if inside the frame and coded before the partition, else (X - 1, Y - 1);
                    exactly one inside: that one; otherwise the component-wise median, a block outside counting as (0, 0)
    payload         qx, qy, dx & 0xFFFF, dy & 0xFFFF per partition; bits = sum of (k > 0) + L(dx) + L(dy) + the split flags

Nothing here is derived from the library under test."""
import numpy as np

import _partition_ref as PR

ME_DTYPE = PR.ME_DTYPE
CTU_DTYPE = np.dtype([("head_mask", "<u8"), ("offset", "<u8"), ("n_words", "<u4"), ("parts", "<u4"), ("bits", "<u4"), ("max_abs", "<u4")])
SIZES = [(16, 16), (64, 64), (80, 48), (144, 112), (1104, 16), (65664, 16)]


def morton(x, y):
    i = 0
    for b in range(3):
        i |= ((x >> b) & 1) << (2 * b) | ((y >> b) & 1) << (2 * b + 1)
    return i


def unmorton(i):
    x = y = 0
    for b in range(3):
        x |= ((i >> (2 * b)) & 1) << b
        y |= ((i >> (2 * b + 1)) & 1) << b
    return x, y


def grid(w, h):
    """(bw, bh, cw, ch)"""
    return w // 8, h // 8, (w + 63) // 64, (h + 63) // 64


def code_length(d):
    """L(d) for |d| <= 65535, written out: k = 2|d| - (d > 0), L = 2 floor(log2(k + 1)) + 1"""
    assert abs(d) <= 65535
    k = 2 * abs(d) - (1 if d > 0 else 0)
    return 2 * ((k + 1).bit_length() - 1) + 1


# ---- the walk -----------------------------------------------------------------------------------------------------------------------------
def walk_ctu(bw, bh, cx, cy, level_at):
    """pack's walk of CTU (cx, cy): ([(X, Y, k) per partition in coding order], the whole nodes that split); level_at(X, Y) = the level
    byte of a block, of which only & 3 counts"""
    parts, flags = [], [0]

    def node(k, X, Y):
        if X >= bw or Y >= bh:
            return                                                          # the child does not exist
        is_whole = PR.whole(bw, bh, k, X >> k, Y >> k)
        if k == 0 or (is_whole and (int(level_at(X, Y)) & 3) >= k):
            parts.append((X, Y, k))
            return
        flags[0] += 1 if is_whole else 0
        half = 1 << (k - 1)
        for dx, dy in ((0, 0), (half, 0), (0, half), (half, half)):
            node(k - 1, X + dx, Y + dy)

    node(3, 8 * cx, 8 * cy)
    return parts, flags[0]


def coding_position(bw, X, Y):
    """where block (X, Y) stands in coding order: (its CTU's raster index, its Morton index)"""
    return ((Y >> 3) * ((bw + 7) // 8) + (X >> 3), morton(X & 7, Y & 7))


def predictor_spots(bw, bh, X, Y, n):
    """the three blocks A, B, C (None where outside the frame) and how C was chosen: "right", "not yet coded" or "outside" """
    inside = lambda x, y: 0 <= x < bw and 0 <= y < bh
    right, why = (X + n, Y - 1), "right"
    if not inside(*right):
        why = "outside"
    elif not coding_position(bw, *right) < coding_position(bw, X, Y):
        why = "not yet coded"
    spots = [(X - 1, Y), (X, Y - 1), right if why == "right" else (X - 1, Y - 1)]
    return [p if inside(*p) else None for p in spots], why


def predictor(field, X, Y, n):
    """P of the partition of n blocks a side at (X, Y); field [bh, bw, 2] of integers, read where it stands"""
    bh, bw = field.shape[:2]
    spots, _ = predictor_spots(bw, bh, X, Y, n)
    at = lambda p: (int(field[p[1], p[0], 0]), int(field[p[1], p[0], 1]))
    have = [at(p) for p in spots if p is not None]
    if len(have) == 1:
        return have[0]
    three = [at(p) if p is not None else (0, 0) for p in spots]
    return PR.median3(*(v[0] for v in three)), PR.median3(*(v[1] for v in three))


# ---- pack ---------------------------------------------------------------------------------------------------------------------------------
def pack(mv, level, w, h, cap_words=None):
    """-> dict: ctu [n_ctu] CTU_DTYPE, stream uint16 [total words] (all of it, whatever cap_words is), total uint64 [2] under cap_words
    (None: everything fits), parts: per partition (ctu, head, X, Y, k, q, P, d, why C), mv / level: the canonical field"""
    bw, bh, cw, ch = grid(w, h)
    field = np.asarray(mv, np.int64).reshape(bh, bw, 2)
    lev = np.asarray(level).reshape(bh, bw)
    ctu = np.zeros(cw * ch, CTU_DTYPE)
    words, parts_info = [], []
    canon_mv, canon_level = np.zeros((bh, bw, 2), np.int16), np.zeros((bh, bw), np.uint8)
    for c in range(cw * ch):
        cx, cy = c % cw, c // cw
        parts, flags = walk_ctu(bw, bh, cx, cy, lambda X, Y: lev[Y, X])
        mask, bits, top = 0, flags, 0
        for X, Y, k in parts:
            n = 1 << k
            head = morton(X - 8 * cx, Y - 8 * cy)
            mask |= 1 << head
            q = (int(field[Y, X, 0]), int(field[Y, X, 1]))
            p = predictor(field, X, Y, n)
            d = (q[0] - p[0], q[1] - p[1])
            bits += (1 if k > 0 else 0) + code_length(d[0]) + code_length(d[1])
            top = max(top, abs(d[0]), abs(d[1]))
            words += [q[0] & 0xFFFF, q[1] & 0xFFFF, d[0] & 0xFFFF, d[1] & 0xFFFF]
            canon_mv[Y:Y + n, X:X + n] = q
            canon_level[Y:Y + n, X:X + n] = k
            parts_info.append((c, head, X, Y, k, q, p, d, predictor_spots(bw, bh, X, Y, n)[1]))
        ctu[c] = (mask, 0, 4 * len(parts), len(parts), bits, top)
    ctu["offset"] = np.concatenate([[0], np.cumsum(ctu["n_words"].astype(np.uint64))[:-1]]).astype(np.uint64)
    total = int(ctu["n_words"].astype(np.uint64).sum())
    cap = total if cap_words is None else int(cap_words)
    fit = int(np.count_nonzero(ctu["offset"].astype(object) + ctu["n_words"].astype(object) <= cap))
    return dict(ctu=ctu, stream=np.array(words, np.uint16), total=np.array([total, fit], np.uint64), parts=parts_info,
                mv=canon_mv.reshape(-1, 2), level=canon_level.ravel())


def written_words(ctu, cap_words):
    """how many leading words of the stream a pack call with this capacity writes: the payloads that fit are a prefix"""
    end = ctu["offset"].astype(object) + ctu["n_words"].astype(object)
    fits = end <= cap_words
    return int(max([0] + [e for e, f in zip(end, fits) if f]))


def wrap16(v):
    """(int16_t)v"""
    return ((int(v) + 32768) % 65536) - 32768


# ---- what a reader does ---------------------------------------------------------------------------------------------------------------------
def exist_mask(bw, bh, cx, cy):
    m = 0
    for i in range(64):
        x, y = unmorton(i)
        if 8 * cx + x < bw and 8 * cy + y < bh:
            m |= 1 << i
    return m


def level_from_mask(bw, bh, cx, cy, mask, head):
    """the largest k for which head is a multiple of 4^k, the node is whole and no other mask bit lies in (head, head + 4^k)"""
    x, y = unmorton(head)
    X, Y = 8 * cx + x, 8 * cy + y
    for k in (3, 2, 1):
        span = 4 ** k
        if head % span == 0 and PR.whole(bw, bh, k, X >> k, Y >> k) and not any((mask >> j) & 1 for j in range(head + 1, head + span)):
            return k
    return 0


def well_formed(bw, bh, cx, cy, mask):
    exist = exist_mask(bw, bh, cx, cy)
    if not mask & 1 or mask & ~exist:
        return False
    for i in range(64):
        if (exist >> i) & 1:
            heads = [j for j in range(i + 1) if (mask >> j) & 1]
            if not heads or i >= heads[-1] + 4 ** level_from_mask(bw, bh, cx, cy, mask, heads[-1]):
                return False
    return True


def unpack(ctu, stream, w, h, cap_words=None):
    """-> (mv [nb, 2] int16, level [nb] uint8); a CTU with a malformed mask or a payload that passes cap_words is all zero.  stream may be
    longer than cap_words: nothing at or beyond it is looked at"""
    bw, bh, cw, ch = grid(w, h)
    stream = np.asarray(stream, np.uint16)
    cap = len(stream) if cap_words is None else int(cap_words)
    mv, level = np.zeros((bh, bw, 2), np.int16), np.zeros((bh, bw), np.uint8)
    for c in range(cw * ch):
        cx, cy = c % cw, c // cw
        mask, offset = int(ctu["head_mask"][c]), int(ctu["offset"][c])
        if not well_formed(bw, bh, cx, cy, mask) or offset + 4 * bin(mask).count("1") > cap:
            continue
        heads = [i for i in range(64) if (mask >> i) & 1]
        for j, head in enumerate(heads):
            k = level_from_mask(bw, bh, cx, cy, mask, head)
            x, y = unmorton(head)
            X, Y, n = 8 * cx + x, 8 * cy + y, 1 << k
            q = stream[offset + 4 * j:offset + 4 * j + 2].view(np.int16)
            mv[Y:Y + n, X:X + n] = q
            level[Y:Y + n, X:X + n] = k
    return mv.reshape(-1, 2), level.ravel()


def decode_differences(ctu, stream, w, h):
    """what a host decoder does with words 2 and 3: rebuild every vector from the differences and the causal predictor of the field decoded so
    far -> mv [nb, 2] int16 (the masks are taken as well formed)"""
    bw, bh, cw, ch = grid(w, h)
    field = np.zeros((bh, bw, 2), np.int64)
    for c in range(cw * ch):
        cx, cy = c % cw, c // cw
        mask, offset = int(ctu["head_mask"][c]), int(ctu["offset"][c])
        for j, head in enumerate(i for i in range(64) if (mask >> i) & 1):
            k = level_from_mask(bw, bh, cx, cy, mask, head)
            x, y = unmorton(head)
            X, Y, n = 8 * cx + x, 8 * cy + y, 1 << k
            p = predictor(field, X, Y, n)
            d = stream[offset + 4 * j + 2:offset + 4 * j + 4].view(np.int16)
            field[Y:Y + n, X:X + n] = (wrap16(p[0] + int(d[0])), wrap16(p[1] + int(d[1])))
    return field.astype(np.int16).reshape(-1, 2)


# ---- data recipes ---------------------------------------------------------------------------------------------------------------------------
def random_tree(w, h, seed, merge=0.4):
    """a consistent field: a random quadtree per CTU -- a whole node of level k >= 1 is one partition with probability `merge`, else it
    splits; a cut node splits -- and one vector per partition, a quarter of the components drawn from the ends of int16.
    -> (mv [nb, 2] int16, level [nb] uint8)"""
    bw, bh, cw, ch = grid(w, h)
    rs = np.random.RandomState(seed)
    mv, level = np.zeros((bh, bw, 2), np.int16), np.zeros((bh, bw), np.uint8)

    def component():
        u = rs.randint(0, 8)
        return -32768 if u == 0 else 32767 if u == 1 else int(rs.randint(-300, 301))

    def node(k, X, Y):
        if X >= bw or Y >= bh:
            return
        n = 1 << k
        if k == 0 or (PR.whole(bw, bh, k, X >> k, Y >> k) and rs.random_sample() < merge):
            mv[Y:Y + n, X:X + n] = (component(), component())
            level[Y:Y + n, X:X + n] = k
            return
        half = n // 2
        for dx, dy in ((0, 0), (half, 0), (0, half), (half, half)):
            node(k - 1, X + dx, Y + dy)

    for c in range(cw * ch):
        node(3, 8 * (c % cw), 8 * (c // cw))
    return mv.reshape(-1, 2), level.ravel()


def inconsistent_field(w, h, seed):
    """legal input that is not canonical: the level map of a random tree with random high bits set in every byte and the bytes of blocks that
    are not first blocks replaced by anything, and a random vector in every block"""
    _, level = random_tree(w, h, seed)
    bw, bh, cw, ch = grid(w, h)
    rs = np.random.RandomState(seed + 1)
    first = np.zeros(bw * bh, bool)
    lev2 = level.reshape(bh, bw)
    for c in range(cw * ch):
        for X, Y, _ in walk_ctu(bw, bh, c % cw, c // cw, lambda X, Y: lev2[Y, X])[0]:
            first[Y * bw + X] = True
    noisy = np.where(first, level, rs.randint(0, 4, bw * bh)).astype(np.uint8) | (rs.randint(0, 64, bw * bh) << 2).astype(np.uint8)
    mv = rs.randint(-32768, 32768, (bw * bh, 2)).astype(np.int16)
    return mv, noisy


def field(w, h):
    """the consistent field of a shape's device tests; at 144 x 112 the seed's tree meets the fixture conditions (test_motion_ref.py)"""
    return random_tree(w, h, w + h + 3)
