"""The reference statement of the adaptive loop filter (include/x266hip.h: xAlfClassifyGpu / StatsGpu / SumStatsGpu / DecideGpu /
ApplyGpu) in numpy int64 over the planes that oracle.conv_output_420 unpacks, and the data recipe of its test cases.  Nothing here is
derived from the library under test; tests/test_alf_ref.py holds it against a plain-loop evaluation of the header's text.

r(x, y) is the plane padded by edge replication.  A class byte is class | tr << 5; tap i of a block turned by tr sits at G_tr(P[i]) and
at its mirror."""
import numpy as np

from _util import splitmix64

VAR = np.array([0, 1, 2, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3, 3, 4], np.int64)
TT = np.array([0, 1, 0, 2, 2, 3, 1, 3], np.int64)
P_LUMA = ((0, -3), (-1, -2), (0, -2), (1, -2), (-2, -1), (-1, -1), (0, -1), (1, -1), (2, -1), (-3, 0), (-2, 0), (-1, 0))
P_CHROMA = ((0, -2), (-1, -1), (0, -1), (1, -1), (-2, 0), (-1, 0))
K = np.array([256, 32, 8, 2], np.int64)
LUMA_WORDS, CHROMA_WORDS, CLASSES = 92, 29, 25
CTU_WORDS = CLASSES * LUMA_WORDS + 2 * CHROMA_WORDS                        # 2358
PAD = 4


def turn(tr, dx, dy):
    """G_tr"""
    return ((dx, dy), (dy, dx), (dx, -dy), (dy, -dx))[tr]


def ctus(w, h):
    return (w + 63) // 64, (h + 63) // 64


def triangle(n):
    """the (i, j), i <= j, of the A words of a record in their order"""
    return [(i, j) for i in range(n) for j in range(i, n)]


class Fetch:
    """r(x + dx, y + dy) for every (x, y) of a plane at once"""

    def __init__(self, plane):
        self.p = np.asarray(plane, np.int64)
        self.big = np.pad(self.p, PAD, mode="edge")

    def __call__(self, dx, dy):
        ph, pw = self.p.shape
        return self.big[PAD + dy:PAD + dy + ph, PAD + dx:PAD + dx + pw]


# ---- classification -------------------------------------------------------------------------------------------------------------------
def gradient_sums(luma):
    """(V, H, D0, D1), each [h / 4, w / 4]"""
    p = np.asarray(luma, np.int64)
    h, w = p.shape
    ext = np.pad(p, 3, mode="edge")                                        # ext[y + 3, x + 3] = r(x, y), x in -3 .. w + 2
    c2 = 2 * ext[1:-1, 1:-1]                                               # the positions x in -2 .. w + 1: index x + 2
    grads = (np.abs(c2 - ext[:-2, 1:-1] - ext[2:, 1:-1]), np.abs(c2 - ext[1:-1, :-2] - ext[1:-1, 2:]),
             np.abs(c2 - ext[:-2, :-2] - ext[2:, 2:]), np.abs(c2 - ext[:-2, 2:] - ext[2:, :-2]))
    out = []
    for g in grads:
        s = np.zeros((h // 4, w // 4), np.int64)
        for b in range(8):                                                 # y = 4 by - 2 + b
            for a in range(8):
                if (a + b) % 2 == 0:
                    s += g[b::4, a::4][:h // 4, :w // 4]
        out.append(s)
    return tuple(out)


def class_bytes(v, h, d0, d1):
    """the decision, elementwise on arrays of sums"""
    v, h, d0, d1 = (np.asarray(a, np.int64) for a in (v, h, d0, d1))
    vh = v > h
    hv1, hv0, dir_hv = np.where(vh, v, h), np.where(vh, h, v), np.where(vh, 1, 3)
    dd = d0 > d1
    dg1, dg0, dir_d = np.where(dd, d0, d1), np.where(dd, d1, d0), np.where(dd, 0, 2)
    diag = dg1 * hv0 > hv1 * dg0
    m1, m0 = np.where(diag, dg1, hv1), np.where(diag, dg0, hv0)
    dir1, dir2 = np.where(diag, dir_d, dir_hv), np.where(diag, dir_hv, dir_d)
    dir_s = np.where(2 * m1 > 9 * m0, 2, np.where(m1 > 2 * m0, 1, 0))
    act = VAR[np.minimum(15, (h + v) >> 5)]
    cls = act + np.where(dir_s != 0, 5 * (((dir1 & 1) << 1) + dir_s), 0)
    return (cls | (TT[2 * dir1 + (dir2 >> 1)] << 5)).astype(np.uint8)


def classify(luma):
    """uint8 [h / 4, w / 4]"""
    return class_bytes(*gradient_sums(luma))


def decode(class_map):
    """(class, tr) of the bytes, as the calls read a caller's map"""
    b = np.asarray(class_map, np.int64)
    return np.minimum(b & 31, 24), (b >> 5) & 3


def per_sample(class_map):
    return tuple(np.repeat(np.repeat(a, 4, axis=0), 4, axis=1) for a in decode(class_map))


# ---- filters --------------------------------------------------------------------------------------------------------------------------
def split_luma(packed):
    """uint8 [n, 600] -> (coef int64 [n, 25, 12], clip int64 [n, 25, 12])"""
    raw = np.asarray(packed, np.uint8).reshape(-1, 600)
    return raw[:, :300].view(np.int8).astype(np.int64).reshape(-1, 25, 12), raw[:, 300:].astype(np.int64).reshape(-1, 25, 12)


def split_chroma(packed):
    raw = np.asarray(packed, np.uint8).reshape(-1, 16)
    return raw[:, :6].view(np.int8).astype(np.int64), raw[:, 6:12].astype(np.int64)


def pack(luma_coef=None, luma_clip=None, chroma_coef=None, chroma_clip=None):
    """the structs as bytes: (uint8 [n_luma, 600], uint8 [n_chroma, 16]); zero[] of the chroma struct is filled with 0xA5 (not read)"""
    def one(coef, clip, taps, size):
        if coef is None:
            return np.zeros((0, size), np.uint8)
        c = np.asarray(coef, np.int64).reshape(-1, taps)
        k = np.zeros_like(c) if clip is None else np.asarray(clip, np.int64).reshape(-1, taps)
        out = np.full((c.shape[0], size), 0xA5, np.uint8)
        out[:, :taps] = c.astype(np.int8).view(np.uint8)
        out[:, taps:2 * taps] = k.astype(np.uint8)
        return out
    return one(luma_coef, luma_clip, 300, 600), one(chroma_coef, chroma_clip, 6, 16)


def _ctu_map(ctrl_column, count, edge, ph, pw):
    """per sample: the set index of its CTU, -1 where the CTU copies"""
    ny, nx = (ph + edge - 1) // edge, (pw + edge - 1) // edge
    k = np.asarray(ctrl_column, np.int64).reshape(ny, nx)
    pick = np.where((k >= 1) & (k <= count), k - 1, -1)
    return np.repeat(np.repeat(pick, edge, axis=0), edge, axis=1)[:ph, :pw]


# ---- apply ----------------------------------------------------------------------------------------------------------------------------
def apply_luma(luma, class_map, packed_sets, ctrl_column):
    coef, clip = split_luma(packed_sets)
    r = Fetch(luma)
    c = r.p
    ph, pw = c.shape
    pick = _ctu_map(ctrl_column, coef.shape[0], 64, ph, pw)
    if coef.shape[0] == 0 or not (pick >= 0).any():
        return c.astype(np.uint8)
    cls, tr = per_sample(class_map)
    s = np.zeros_like(c)
    use = np.maximum(pick, 0)
    for i, (dx, dy) in enumerate(P_LUMA):
        ci, ki = coef[use, cls, i], K[clip[use, cls, i] & 3]
        for t in range(4):
            gx, gy = turn(t, dx, dy)
            term = ci * (np.clip(r(gx, gy) - c, -ki, ki) + np.clip(r(-gx, -gy) - c, -ki, ki))
            s += np.where(tr == t, term, 0)
    out = np.clip(c + ((s + 64) >> 7), 0, 255)
    return np.where(pick >= 0, out, c).astype(np.uint8)


def apply_chroma(plane, packed_alts, ctrl_column):
    coef, clip = split_chroma(packed_alts)
    r = Fetch(plane)
    c = r.p
    ph, pw = c.shape
    pick = _ctu_map(ctrl_column, coef.shape[0], 32, ph, pw)
    if coef.shape[0] == 0:
        return c.astype(np.uint8)
    use = np.maximum(pick, 0)
    s = np.zeros_like(c)
    for i, (dx, dy) in enumerate(P_CHROMA):
        ci, ki = coef[use, i], K[clip[use, i] & 3]
        s += ci * (np.clip(r(dx, dy) - c, -ki, ki) + np.clip(r(-dx, -dy) - c, -ki, ki))
    out = np.clip(c + ((s + 64) >> 7), 0, 255)
    return np.where(pick >= 0, out, c).astype(np.uint8)


def apply(planes, class_map, packed_luma, packed_chroma, ctrl):
    """(y, u, v), a class map (None: classify(y)), the packed sets, d_ctrl [n_ctu, 3] -> the filtered (y, u, v)"""
    y, u, v = planes
    ctrl = np.asarray(ctrl, np.uint8).reshape(-1, 3)
    class_map = classify(y) if class_map is None else class_map
    return apply_luma(y, class_map, packed_luma, ctrl[:, 0]), apply_chroma(u, packed_chroma, ctrl[:, 1]), apply_chroma(v, packed_chroma, ctrl[:, 2])


def apply_tiles(oracle, tiles, w, h, class_map, packed_luma, packed_chroma, ctrl, base):
    """the tile array xAlfApplyGpu leaves: m_Y and m_C filtered from `tiles`, every other byte from `base`"""
    y, u, v = apply(oracle.conv_output_420(tiles, w, h), class_map, packed_luma, packed_chroma, ctrl)
    packed = oracle.conv_input_fmt(y, u, v).reshape(-1, 512)
    out = np.array(base, np.uint8).reshape(-1, 512)
    out[:, :384] = packed[:, :384]
    return out.ravel()


# ---- statistics -----------------------------------------------------------------------------------------------------------------------
def _features(org, dec, taps, tr):
    """[PH, PW, words]: per sample 1, y^2, E_i y, E_i E_j (i <= j); tr: per-sample transposition or None"""
    r = Fetch(dec)
    c = r.p
    y = np.asarray(org, np.int64) - c
    e = []
    for dx, dy in taps:
        if tr is None:
            e.append(r(dx, dy) + r(-dx, -dy) - 2 * c)
        else:
            ei = np.zeros_like(c)
            for t in range(4):
                gx, gy = turn(t, dx, dy)
                ei += np.where(tr == t, r(gx, gy) + r(-gx, -gy) - 2 * c, 0)
            e.append(ei)
    feats = [np.ones_like(c), y * y] + [ei * y for ei in e] + [e[i] * e[j] for i, j in triangle(len(taps))]
    return np.stack(feats, axis=-1)


def stats(org_planes, dec_planes, class_map=None):
    """d_stats as int64 [n_ctu, 2358]"""
    (oy, ou, ov), (dy, du, dv) = org_planes, dec_planes
    h, w = np.asarray(dy).shape
    nx, ny = ctus(w, h)
    class_map = classify(dy) if class_map is None else class_map
    cls, tr = per_sample(class_map)
    fy = _features(oy, dy, P_LUMA, tr)
    fu, fv = _features(ou, du, P_CHROMA, None), _features(ov, dv, P_CHROMA, None)
    out = np.zeros((ny * nx, CTU_WORDS), np.int64)
    for cy in range(ny):
        for cx in range(nx):
            win = (slice(64 * cy, 64 * cy + 64), slice(64 * cx, 64 * cx + 64))
            f, k = fy[win].reshape(-1, LUMA_WORDS), cls[win].ravel()
            onehot = (k[None, :] == np.arange(CLASSES)[:, None]).astype(np.int64)
            rec = out[cy * nx + cx]
            rec[:CLASSES * LUMA_WORDS] = (onehot @ f).ravel()
            cwin = (slice(32 * cy, 32 * cy + 32), slice(32 * cx, 32 * cx + 32))
            rec[CLASSES * LUMA_WORDS:][:CHROMA_WORDS] = fu[cwin].reshape(-1, CHROMA_WORDS).sum(axis=0)
            rec[CLASSES * LUMA_WORDS + CHROMA_WORDS:] = fv[cwin].reshape(-1, CHROMA_WORDS).sum(axis=0)
    return out


def stats_words(st):
    return np.asarray(st, np.int64).astype(np.int32).ravel()


def sum_stats(st, mask=None):
    """int64 [2358]: the records of the CTUs whose mask byte is non-zero"""
    st = np.asarray(st, np.int64).reshape(-1, CTU_WORDS)
    keep = np.ones(st.shape[0], bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    return st[keep].sum(axis=0)


# ---- decision -------------------------------------------------------------------------------------------------------------------------
def record_cost(rec, c):
    """sum c_i^2 A_ii + 2 sum_{i<j} c_i c_j A_ij - 256 sum c_i b_i of one record under coefficients c"""
    rec, c = np.asarray(rec, np.int64), np.asarray(c, np.int64)
    n = c.size
    tri = triangle(n)
    weight = np.array([(1 if i == j else 2) * c[i] * c[j] for i, j in tri], np.int64)
    return int((weight * rec[2 + n:2 + n + len(tri)]).sum() - 256 * (c * rec[2:2 + n]).sum())


def ceil_log2(n):
    return 0 if n <= 1 else int(np.ceil(np.log2(n)))


def ctu_costs(rec, packed_luma, packed_chroma):
    """(luma costs per set, U costs per alternative, V costs)"""
    lc, _ = split_luma(packed_luma)
    cc, _ = split_chroma(packed_chroma)
    luma = [sum(record_cost(rec[k * LUMA_WORDS:(k + 1) * LUMA_WORDS], lc[s, k]) for k in range(CLASSES)) for s in range(lc.shape[0])]
    base = CLASSES * LUMA_WORDS
    u = [record_cost(rec[base:base + CHROMA_WORDS], cc[s]) for s in range(cc.shape[0])]
    v = [record_cost(rec[base + CHROMA_WORDS:base + 2 * CHROMA_WORDS], cc[s]) for s in range(cc.shape[0])]
    return luma, u, v


def decide(st, packed_luma, packed_chroma, lam):
    """d_stats [n_ctu, 2358] -> d_ctrl uint8 [n_ctu, 3]"""
    st = np.asarray(st, np.int64).reshape(-1, CTU_WORDS)
    out = np.zeros((st.shape[0], 3), np.uint8)
    base = CLASSES * LUMA_WORDS
    for t, rec in enumerate(st):
        costs = ctu_costs(rec, packed_luma, packed_chroma)
        counts = (rec[0:base:LUMA_WORDS].sum(), rec[base], rec[base + CHROMA_WORDS])
        for m in range(3):
            rate = (lam << 10) * ceil_log2(len(costs[m]))
            best, pick = 0, 0
            for s, cost in enumerate(costs[m]):
                if cost + rate < best:
                    best, pick = cost + rate, s + 1
            out[t, m] = pick if counts[m] != 0 else 0
    return out


# ---- the solve (host side: float64) -----------------------------------------------------------------------------------------------------
def solve_record(rec, n):
    rec = np.asarray(rec, np.float64)
    a = np.zeros((n, n))
    for w, (i, j) in enumerate(triangle(n)):
        a[i, j] = a[j, i] = rec[2 + n + w]
    x = np.linalg.lstsq(a + 1e-3 * np.eye(n), rec[2:2 + n], rcond=None)[0]
    return np.clip(np.round(128 * x), -128, 127).astype(np.int64)


def solve(total):
    """frame totals [2358] -> (luma coef [25, 12], U coef [6], V coef [6]), clip index 0 throughout"""
    total = np.asarray(total, np.int64)
    base = CLASSES * LUMA_WORDS
    luma = np.stack([solve_record(total[k * LUMA_WORDS:(k + 1) * LUMA_WORDS], 12) for k in range(CLASSES)])
    return luma, solve_record(total[base:base + CHROMA_WORDS], 6), solve_record(total[base + CHROMA_WORDS:], 6)


# ---- the data recipe ------------------------------------------------------------------------------------------------------------------
SIZES = [(64, 64), (80, 48), (144, 80)]
LAMBDAS = (0, 37, 400)
CLASSIFY_KINDS = ("stripes", "quad", "blur", "noise")
STATS_KINDS = ("blur", "noise", "same", "far")
QUAD_SEED = 3


def _bits(seed, shape):
    return splitmix64(seed, 0, int(np.prod(shape))).reshape(shape)


def stripes(pw, ph, seed=11):
    """128 + amp round(cos(pi s / 2)), amp per 16x16 cell, s = x + y on even 16-row bands and x - y on odd ones"""
    yy, xx = np.mgrid[0:ph, 0:pw]
    s = np.where((yy // 16) % 2 == 0, xx + yy, xx - yy)
    wave = np.array([1, 0, -1, 0], np.int64)[s % 4]
    cells = _bits(seed, ((ph + 15) // 16, (pw + 15) // 16))
    amp = np.array([1, 2, 6, 20, 100], np.int64)[(cells % np.uint64(5)).astype(np.int64)]
    return (128 + np.repeat(np.repeat(amp, 16, axis=0), 16, axis=1)[:ph, :pw] * wave).astype(np.uint8)


QUAD_FACTORS = (0, .02, .05, .1, .25, .5, 1, 2, 4)


def quad(pw, ph, seed=QUAD_SEED):
    """12x12 patches of a x^2 + b y^2 + g (x + y)^2 / 2 + d (x - y)^2 / 2 about the patch centre, centred on 128, clipped to +-120"""
    out = np.zeros((ph, pw), np.int64)
    ny, nx = (ph + 11) // 12, (pw + 11) // 12
    r = _bits(seed, (ny, nx, 6))
    yy, xx = np.mgrid[0:12, 0:12] - 5.5
    for j in range(ny):
        for i in range(nx):
            f = [QUAD_FACTORS[int(r[j, i, k] % np.uint64(9))] for k in range(4)]
            zeroed = int(r[j, i, 4] % np.uint64(3))                       # up to two of the four are dropped
            for k in range(zeroed):
                f[int((r[j, i, 5] >> np.uint64(8 * k)) % np.uint64(4))] = 0
            q = f[0] * xx * xx + f[1] * yy * yy + f[2] * (xx + yy) ** 2 / 2 + f[3] * (xx - yy) ** 2 / 2
            q = np.clip(np.round(q - q.mean()), -120, 120).astype(np.int64) + 128
            out[12 * j:12 * j + 12, 12 * i:12 * i + 12] = q[:min(12, ph - 12 * j), :min(12, pw - 12 * i)]
    return out.astype(np.uint8)


def noise(pw, ph, seed):
    return (_bits(seed, (ph, pw)) & np.uint64(255)).astype(np.uint8)


def blur_pair(pw, ph, seed, scale=1):
    """(org, dec): org = a smooth two-sinusoid field plus two sign-of-sinusoid edge fields, the amplitude ramped across the width, plus
    Gaussian noise of sigma 6; dec = clip8(((4 c + left + right + up + down + 4) >> 3) + uniform{-3 .. 3})"""
    yy, xx = np.mgrid[0:ph, 0:pw] * scale
    ramp = 0.4 + 0.6 * xx / max(pw * scale - 1, 1)
    field = 40 * np.sin(xx / 7.0) * np.cos(yy / 11.0) + 25 * np.sin((xx + 2 * yy) / 17.0)
    edges = 22 * np.sign(np.sin((xx + yy) / 9.0)) + 18 * np.sign(np.sin((2 * xx - yy) / 13.0))
    gauss = np.random.RandomState(seed).normal(0.0, 6.0, (ph, pw))
    org = np.clip(np.round(128 + ramp * (field + edges) + gauss), 0, 255).astype(np.int64)
    r = Fetch(org)
    jitter = (_bits(seed + 1, (ph, pw)) % np.uint64(7)).astype(np.int64) - 3
    dec = np.clip(((4 * org + r(-1, 0) + r(1, 0) + r(0, -1) + r(0, 1) + 4) >> 3) + jitter, 0, 255)
    return org.astype(np.uint8), dec.astype(np.uint8)


def extreme(pw, ph, seed):
    """0 / 255 stripes, per 16x16 cell along x, along y, or a checkerboard: every E reaches +-510 somewhere"""
    yy, xx = np.mgrid[0:ph, 0:pw]
    cells = (_bits(seed, ((ph + 15) // 16, (pw + 15) // 16)) % np.uint64(3)).astype(np.int64)
    kind = np.repeat(np.repeat(cells, 16, axis=0), 16, axis=1)[:ph, :pw]
    bit = np.where(kind == 0, xx & 1, np.where(kind == 1, yy & 1, (xx + yy) & 1))
    return (255 * bit).astype(np.uint8)


def spikes(pw, ph, edge):
    """constant 100 except one bright sample within 3 samples of each corner and of each CTU seam (edge = the CTU's size on this plane)"""
    p = np.full((ph, pw), 100, np.uint8)
    spots = [(1, 2), (pw - 2, 0), (0, ph - 3), (pw - 3, ph - 1)]
    for i, sx in enumerate(range(edge, pw, edge)):
        spots += [(sx - 1 - i % 3, 9), (sx + i % 3, ph // 2), (sx + 2, ph - 2)]
    for i, sy in enumerate(range(edge, ph, edge)):
        spots += [(7, sy - 1 - i % 3), (pw // 2 + 1, sy + i % 3), (pw - 1, sy + 2)]
    for sx in range(edge, pw, edge):
        for sy in range(edge, ph, edge):
            spots += [(sx - 1, sy - 1), (sx, sy)]
    for x, y in spots:
        p[min(max(y, 0), ph - 1), min(max(x, 0), pw - 1)] = 250
    return p


def case(kind, w, h):
    """(org planes, dec planes), each (y, u, v) uint8"""
    seed = 7000 + 100 * (CLASSIFY_KINDS + STATS_KINDS + ("spikes",)).index(kind) + w + 3 * h
    dims = ((w, h, 1, 64), (w // 2, h // 2, 2, 32), (w // 2, h // 2, 2, 32))
    if kind in ("blur", "same"):
        pairs = [blur_pair(pw, ph, seed + m, scale) for m, (pw, ph, scale, _) in enumerate(dims)]
        if kind == "same":
            pairs = [(d, d) for _, d in pairs]
    elif kind == "far":
        pairs = [(255 - d, d) for d in (extreme(pw, ph, seed + m) for m, (pw, ph, _, _) in enumerate(dims))]
    elif kind == "noise":
        pairs = [(noise(pw, ph, seed + 10 + m), noise(pw, ph, seed + m)) for m, (pw, ph, _, _) in enumerate(dims)]
    elif kind == "stripes":
        pairs = [(noise(pw, ph, seed + 10 + m), stripes(pw, ph, 11 + m)) for m, (pw, ph, _, _) in enumerate(dims)]
    elif kind == "quad":
        pairs = [(noise(pw, ph, seed + 10 + m), quad(pw, ph, QUAD_SEED + m)) for m, (pw, ph, _, _) in enumerate(dims)]
    elif kind == "spikes":
        pairs = [(noise(pw, ph, seed + 10 + m), spikes(pw, ph, edge)) for m, (pw, ph, _, edge) in enumerate(dims)]
    else:
        raise KeyError(kind)
    return tuple(p[0] for p in pairs), tuple(p[1] for p in pairs)


def random_filters(n_luma, n_chroma, seed):
    """packed sets of random int8 coefficients with -128 and 127 among them and all four clip indices (as whole bytes: only two bits count)"""
    r = _bits(seed, (n_luma * 600 + n_chroma * 16,)).astype(np.uint8)
    luma, chroma = r[:n_luma * 600].reshape(n_luma, 600).copy(), r[n_luma * 600:].reshape(n_chroma, 16).copy()
    luma[:, 0], luma[:, 1], chroma[:, 0], chroma[:, 1] = 0x80, 0x7F, 0x80, 0x7F
    return luma, chroma


def squared_error(a, b):
    return int(((np.asarray(a, np.int64) - np.asarray(b, np.int64)) ** 2).sum())
