"""The reference statement of the seeded SATD search (include/x266hip.h, "hierarchical motion search": xSatd8x8SeededSearchGpu) in
numpy and Python integers over luma planes, and the data recipes of its test cases.  For block (bx, by), 8x8 at (8 bx, 8 by):

    seed cell   (sx, sy) = (bx >> seed_scale, by >> seed_scale)
    centre      S(sx, sy) = clamp(seed << seed_scale, -8183, 8183)
    centre list own | (0, 0) bit 0 | left bit 1 | top bit 2 | right bit 3 | bottom bit 4; a neighbour outside the grid is skipped
    walk        centres in list order, dy = -r..r, then dx = -r..r: v = C + (dx, dy)
    J(v)        satd8x8(cur_block - ref_block_at(x + vx, y + vy)) + ((lambda_q4 * (L(vx - Px) + L(vy - Py))) >> 4), P = centre 0
    L(d)        k = 2 |d| - (d > 0); 2 floor(log2(k + 1)) + 1
    winner      the least J, the first of equal ones in the walk

The search is a brute-force walk in exactly that order; every SATD comes from the oracle (oracle.satd8x8), the reference samples from
the plane with clamped coordinates.  Nothing here is derived from the library under test."""
import numpy as np

from _util import splitmix64

ME_DTYPE = np.dtype([("mvx", "<i2"), ("mvy", "<i2"), ("cost", "<u4")])
CLAMP = 8183
BITS = (("zero", 1), ("left", 2), ("top", 4), ("right", 8), ("bottom", 16))


def code_length(d):
    """L(d) of one integer, by its definition"""
    d = int(d)
    k = 2 * abs(d) - (1 if d > 0 else 0)
    return 2 * ((k + 1).bit_length() - 1) + 1


def clamp_seed(seed, seed_scale):
    """S of one seed component; Python integers do not wrap"""
    return max(-CLAMP, min(CLAMP, int(seed) << seed_scale))


def grid(w, h, seed_scale):
    return (w // 8) >> seed_scale, (h // 8) >> seed_scale


def centre_list(seeds, gw, gh, sx, sy, seed_scale, centres):
    """the ordered centre list of cell (sx, sy): [(x, y), ...]; seeds [gh * gw, 2]"""
    S = lambda x, y: (clamp_seed(seeds[y * gw + x][0], seed_scale), clamp_seed(seeds[y * gw + x][1], seed_scale))
    out = [S(sx, sy)]
    if centres & 1:
        out.append((0, 0))
    if centres & 2 and sx - 1 >= 0:
        out.append(S(sx - 1, sy))
    if centres & 4 and sy - 1 >= 0:
        out.append(S(sx, sy - 1))
    if centres & 8 and sx + 1 < gw:
        out.append(S(sx + 1, sy))
    if centres & 16 and sy + 1 < gh:
        out.append(S(sx, sy + 1))
    return out


def walk(centres_xy, r):
    """the candidates of a centre list in the order they are tried: [(vx, vy), ...]"""
    return [(cx + dx, cy + dy) for cx, cy in centres_xy for dy in range(-r, r + 1) for dx in range(-r, r + 1)]


def vector_cost(lambda_q4, v, p):
    return (int(lambda_q4) * (code_length(v[0] - p[0]) + code_length(v[1] - p[1]))) >> 4


def ref_blocks(ref_y, x, y, cand):
    """[T, 8, 8] int16: the reference block of the block at (x, y) under every vector of cand [T, 2], coordinates clamped"""
    h, w = ref_y.shape
    k = np.arange(8)
    ys = np.clip(y + cand[:, 1, None] + k, 0, h - 1)
    xs = np.clip(x + cand[:, 0, None] + k, 0, w - 1)
    return ref_y[ys[:, :, None], xs[:, None, :]].astype(np.int16)


def search(oracle, cur_y, ref_y, seeds, seed_scale, centres, r, lambda_q4):
    """the brute-force walk -> (best [nb] of ME_DTYPE: the vector and its SATD, j [nb] uint32, walk index [nb])"""
    h, w = cur_y.shape
    bw, bh = w // 8, h // 8
    gw, gh = grid(w, h, seed_scale)
    seeds = np.asarray(seeds, np.int64).reshape(gw * gh, 2)
    cands, diffs = [], []
    for by in range(bh):
        for bx in range(bw):
            cl = centre_list(seeds, gw, gh, bx >> seed_scale, by >> seed_scale, seed_scale, centres)
            cand = np.array(walk(cl, r), np.int64)
            cands.append((cl[0], cand))
            cur = cur_y[8 * by:8 * by + 8, 8 * bx:8 * bx + 8].astype(np.int16)
            diffs.append((cur[None] - ref_blocks(ref_y, 8 * bx, 8 * by, cand)).reshape(-1, 64))
    satd = oracle.satd8x8(np.concatenate(diffs), threads=4).astype(np.int64)
    best, jout, index = np.zeros(bw * bh, ME_DTYPE), np.zeros(bw * bh, np.uint32), np.zeros(bw * bh, np.int64)
    at = 0
    for b, (p, cand) in enumerate(cands):
        s = satd[at:at + len(cand)]
        at += len(cand)
        j = s + np.array([vector_cost(lambda_q4, v, p) for v in cand], np.int64)
        t = int(np.argmin(j))                                               # numpy returns the first of equal minima
        assert j[t] < 1 << 32
        best[b] = (cand[t][0], cand[t][1], s[t])
        jout[b], index[b] = j[t], t
    return best, jout, index


# ---- planes <-> tiles, through the oracle ---------------------------------------------------------------------------------------------------
def tiles_of(oracle, y, seed=0):
    """the tile array [n, 512] of a luma plane: chroma and m_I are seeded garbage (the call reads only m_Y)"""
    h, w = y.shape
    junk = (splitmix64(0x5EED + seed, 0, w * h // 2) & np.uint64(255)).astype(np.uint8)
    t = oracle.conv_input_fmt(y, junk[:w * h // 4].reshape(h // 2, w // 2), junk[w * h // 4:].reshape(h // 2, w // 2)).reshape(-1, 512).copy()
    t[:, 384:] = (splitmix64(0x1F0 + seed, 0, t.shape[0] * 128) & np.uint64(255)).astype(np.uint8).reshape(-1, 128)
    return t


def luma_of(oracle, tiles, w, h):
    return oracle.conv_output_420(np.ascontiguousarray(tiles).ravel(), w, h)[0]


# ---- data recipes -----------------------------------------------------------------------------------------------------------------------
SIZES = [(16, 16), (32, 16), (16, 32), (48, 32), (96, 80)]
FRAMES = ("random", "constant", "ramps", "checker")
SEEDS = ("small", "pm64", "far", "pm8191", "extreme", "duplicates")


def smooth_texture(w, h, seed, taps=9):
    """low-pass-filtered noise, stretched back to the full range: [h, w] uint8"""
    r = (splitmix64(seed, 0, (h + 2 * taps) * (w + 2 * taps)) & np.uint64(255)).astype(np.float64).reshape(h + 2 * taps, w + 2 * taps)
    k = np.hanning(taps + 2)[1:-1]
    k /= k.sum()
    r = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), 0, r)
    r = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), 1, r)[taps:-taps, taps:-taps]
    r = (r - r.mean()) / r.std()
    return np.clip(128.0 + 48.0 * r, 0, 255).astype(np.uint8)


def frame_pair(kind, w, h, seed):
    """(cur, ref) luma planes [h, w] uint8"""
    xx, yy = np.meshgrid(np.arange(w), np.arange(h))
    if kind == "constant":                                                   # every SATD ties
        return np.full((h, w), 77, np.uint8), np.full((h, w), 77, np.uint8)
    if kind == "ramps":                                                      # many ties along the ramps' level lines
        return ((3 * xx + 5 * yy) & 255).astype(np.uint8), ((3 * xx + 5 * yy + 11) & 255).astype(np.uint8)
    if kind == "checker":                                                    # the largest coefficients, and ties at every even step
        return np.where((xx + yy) & 1, 255, 0).astype(np.uint8), np.where((xx + yy // 2) & 1, 255, 0).astype(np.uint8)
    r = splitmix64(0x5EEDED + seed, 0, 2 * w * h).reshape(2, h, w)
    cur = (r[0] & np.uint64(255)).astype(np.uint8)
    ref = np.where((r[1] >> np.uint64(8)) & np.uint64(3), np.roll(cur, (2, -3), (0, 1)), (r[1] & np.uint64(255)).astype(np.uint8))   # partly a moved copy
    return cur, ref.astype(np.uint8)


def seed_vectors(kind, w, h, seed_scale, seed):
    """[cells, 2] int16"""
    gw, gh = grid(w, h, seed_scale)
    n = gw * gh
    r = splitmix64(0xC0FFEE + seed, 0, 2 * n).reshape(n, 2)
    pick = lambda values: np.array(values, np.int64)[(r >> np.uint64(33)).astype(np.int64) % len(values)]
    if kind == "small":
        v = (r & np.uint64(15)).astype(np.int64) - 8
    elif kind == "pm64":
        v = pick([-64, 64, 63, -63])
    elif kind == "far":                                                      # wholly outside the frame, on every side
        v = np.where((r >> np.uint64(20)) & np.uint64(1), 1, -1) * (np.array([w, h], np.int64) + 9 + (r & np.uint64(63)).astype(np.int64))
    elif kind == "pm8191":
        v = pick([-8191, 8191, 8183, -8183, 8184, -8184, 4091, 4092, -4092])
    elif kind == "extreme":
        v = pick([-32768, 32767])
    else:                                                                    # duplicates: every cell the same vector, so the centres repeat
        v = np.tile(np.array([[2, -1]], np.int64), (n, 1))
    return v.astype(np.int16)
