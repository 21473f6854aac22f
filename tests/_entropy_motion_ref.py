"""The reference statement of the entropy coder of the motion stream (include/x266hip.h, "the entropy coder of the motion stream":
xEntropyEncodeMvGpu, xEntropyDecodeMvGpu, xMotionReconstructGpu) in numpy and Python integers, on top of _entropy_ref.code_bins,
_entropy_ref.Decoder and _motion_ref.  Written from the header, independently of x266_entropy_motion.hpp: the syntax is the recursion
over the quadtree on both sides (the C++ loops over heads, respectively over a Morton cursor), the encoder first lists its bins and then
codes the list, and the reconstruction walks the CTUs in raster order (the device walks a wavefront).

Nothing here is derived from the library under test."""
import numpy as np

import _entropy_ref as ER
import _motion_ref as MR
import _partition_ref as PR

CONTEXTS = 7
MAX_BYTES = 720
SPLIT, NZ, GT1 = 0, 3, 5                                                       # split of level k is SPLIT + k - 1; nz and gt1 take the component
CODED_DTYPE = np.dtype([("ctx_bins", "<u4"), ("bypass_bins", "<u4"), ("offset", "<u8"), ("n_words", "<u4"), ("n_bytes", "<u4"), ("parts", "<u4"),
                        ("unreadable", "<u4")])
assert CODED_DTYPE.itemsize == 32


def default_init():
    return np.full(CONTEXTS, 1024, np.uint16)


def _init(init):
    table = default_init() if init is None else np.asarray(init)
    assert table.size == CONTEXTS and table.min() >= ER.P_MIN and table.max() <= ER.P_MAX
    return [int(x) for x in table]


def diff_bins(d, comp):
    a = abs(d)
    assert a <= 65535
    bins = [(NZ + comp, int(a != 0))]
    if a == 0:
        return bins
    bins.append((GT1 + comp, int(a > 1)))
    if a > 1:
        v = (a - 2) + 2                                                       # Exp-Golomb order 1 of r = a - 2
        k = v.bit_length() - 1
        bins += [(None, 1)] * (k - 1) + [(None, 0)] + [(None, (v >> i) & 1) for i in reversed(range(k))]
    bins.append((None, int(d < 0)))
    return bins


def true_diffs(words):
    """[(dx, dy)] per partition from pack's words: P = (int16)(q - (int16)w), d = q - P"""
    w = np.asarray(words, np.uint16).reshape(-1, 4).view(np.int16).astype(np.int64)
    out = []
    for qx, qy, wx, wy in w:
        out.append((int(qx) - MR.wrap16(int(qx) - int(wx)), int(qy) - MR.wrap16(int(qy) - int(wy))))
    return out


def ctu_bins(bw, bh, cx, cy, mask, diffs):
    """the bins of a CTU with a well-formed mask; diffs: the true differences per partition in coding order"""
    level = {h: MR.level_from_mask(bw, bh, cx, cy, mask, h) for h in range(64) if (mask >> h) & 1}
    bins, left = [], list(diffs)

    def node(k, X, Y):
        if X >= bw or Y >= bh:
            return
        head = MR.morton(X - 8 * cx, Y - 8 * cy)
        one = level.get(head) == k
        if k > 0 and PR.whole(bw, bh, k, X >> k, Y >> k):
            bins.append((SPLIT + k - 1, 0 if one else 1))
        if k == 0 or one:
            assert one
            dx, dy = left.pop(0)
            bins.extend(diff_bins(dx, 0) + diff_bins(dy, 1))
            return
        half = 1 << (k - 1)
        for ox, oy in ((0, 0), (half, 0), (0, half), (half, half)):
            node(k - 1, X + ox, Y + oy)

    node(3, 8 * cx, 8 * cy)
    assert not left
    return bins


def encode_ctu(w, h, c, mask, words, init=None):
    """-> (bytes, context bins, bypass bins), or None for a malformed mask"""
    bw, bh, cw, _ = MR.grid(w, h)
    cx, cy = c % cw, c // cw
    if not MR.well_formed(bw, bh, cx, cy, mask):
        return None
    bins = ctu_bins(bw, bh, cx, cy, mask, true_diffs(words))
    data = ER.code_bins(bins, _init(init))
    n_ctx = sum(1 for ctx, _ in bins if ctx is not None)
    return data, n_ctx, len(bins) - n_ctx


def _dec_diff(d, comp):
    if not d.bin(NZ + comp):
        return 0
    a = 1
    if d.bin(GT1 + comp):
        ones = 0
        while ones < 15 and d.bypass():
            ones += 1
        if ones > 14:
            raise ER.Malformed("prefix")
        k = ones + 1
        a = (1 << k) | d.bits(k)
    return -a if d.bypass() else a


def decode_ctu(w, h, c, data, init=None):
    """-> (mask, words uint16 [4 * parts], [(head, k, dx, dy)], bits, malformed); a malformed substream gives the flat CTU"""
    bw, bh, cw, _ = MR.grid(w, h)
    cx, cy = c % cw, c // cw

    def run(raw):
        d = ER.Decoder(raw, _init(init))
        parts, flags = [], [0]

        def node(k, X, Y):
            if X >= bw or Y >= bh:
                return
            split = k > 0
            if k > 0 and PR.whole(bw, bh, k, X >> k, Y >> k):
                flags[0] += 1
                split = bool(d.bin(SPLIT + k - 1))
            if not split:
                dx = _dec_diff(d, 0)
                parts.append((MR.morton(X - 8 * cx, Y - 8 * cy), k, dx, _dec_diff(d, 1)))
                return
            half = 1 << (k - 1)
            for ox, oy in ((0, 0), (half, 0), (0, half), (half, half)):
                node(k - 1, X + ox, Y + oy)

        node(3, 8 * cx, 8 * cy)
        return parts, flags[0]

    malformed = False
    try:
        parts, flags = run(bytes(data))
    except ER.Malformed:
        parts, flags = run(b"")
        malformed = True
    mask = sum(1 << p[0] for p in parts)
    words = np.array([[0, 0, p[2] & 0xFFFF, p[3] & 0xFFFF] for p in parts], np.uint16).ravel()
    bits = flags + sum(MR.code_length(p[2]) + MR.code_length(p[3]) for p in parts)
    return mask, words, parts, bits, malformed


# ---- the calls ----------------------------------------------------------------------------------------------------------------------------
def code_ctus(ctu, words, w, h, in_words=None, init=None):
    """per CTU (substream, context bins, bypass bins, parts, unreadable)"""
    src = np.asarray(words, np.uint16).ravel()
    n_in = src.size if in_words is None else int(in_words)
    coded = []
    for c in range(len(ctu)):
        mask, off = int(ctu["head_mask"][c]), int(ctu["offset"][c])
        n = 4 * bin(mask).count("1")
        got = encode_ctu(w, h, c, mask, src[off:off + n], init) if off + n <= n_in else None
        coded.append((b"", 0, 0, 0, 1) if got is None else got + (n // 4, 0))
    return coded


def assemble(coded, cap_words=None):
    n = len(coded)
    rec = np.zeros(n, CODED_DTYPE)
    payloads = []
    for c, (data, n_ctx, n_byp, parts, bad) in enumerate(coded):
        payloads.append(data + b"\0" * (len(data) & 1))
        rec[c] = (n_ctx, n_byp, 0, (len(data) + 1) // 2, len(data), parts, bad)
    ends = np.cumsum(rec["n_words"].astype(np.uint64), dtype=np.uint64)
    rec["offset"] = ends - rec["n_words"]
    total = int(ends[-1])
    cap = total if cap_words is None else int(cap_words)
    stream = np.zeros(cap, np.uint16)
    fit = 0
    for c in range(n):
        off, nw = int(rec["offset"][c]), int(rec["n_words"][c])
        if off + nw > cap:
            continue
        fit += 1
        stream[off:off + nw] = np.frombuffer(payloads[c], "<u2")
    return rec, stream, np.array([total, fit], np.uint64)


def encode(ctu, words, w, h, in_words=None, cap_words=None, init=None):
    """xEntropyEncodeMvGpu -> (coded [n_ctu] CODED_DTYPE, stream uint16 [cap_words], total uint64 [2]); words not written are 0"""
    return assemble(code_ctus(ctu, words, w, h, in_words, init), cap_words)


def decode(coded, stream, w, h, cap_words=None, init=None):
    """xEntropyDecodeMvGpu -> (records [n_ctu] MR.CTU_DTYPE, words uint16 [256 * n_ctu] with 0 where nothing is written, status uint8)"""
    src = np.asarray(stream, np.uint16).ravel()
    cap = src.size if cap_words is None else int(cap_words)
    raw = src[:cap].astype("<u2").tobytes()
    n = len(coded)
    ctu, words, status = np.zeros(n, MR.CTU_DTYPE), np.zeros(256 * n, np.uint16), np.zeros(n, np.uint8)
    for c in range(n):
        off, nb = int(coded["offset"][c]), int(coded["n_bytes"][c])
        data = b""
        if nb > MAX_BYTES or off > cap or (nb + 1) // 2 > cap - off:
            status[c] = 1
        else:
            data = raw[2 * off:2 * off + nb]
        mask, wds, parts, bits, bad = decode_ctu(w, h, c, data, init)
        if bad:
            status[c] = 2
        top = max([0] + [max(abs(p[2]), abs(p[3])) for p in parts])
        ctu[c] = (mask, 256 * c, 4 * len(parts), len(parts), bits, top)
        words[256 * c:256 * c + wds.size] = wds
    return ctu, words, status


def reconstruct(ctu, stream, w, h, cap_words=None):
    """xMotionReconstructGpu -> (mv [nb, 2] int16, level [nb] uint8): unpack's rules for a CTU it cannot read, otherwise every vector from
    the differences and the causal predictor over the field as rebuilt so far"""
    bw, bh, cw, ch = MR.grid(w, h)
    src = np.asarray(stream, np.uint16).ravel()
    cap = src.size if cap_words is None else int(cap_words)
    field, level = np.zeros((bh, bw, 2), np.int64), np.zeros((bh, bw), np.uint8)
    for c in range(cw * ch):
        cx, cy = c % cw, c // cw
        mask, off = int(ctu["head_mask"][c]), int(ctu["offset"][c])
        if not MR.well_formed(bw, bh, cx, cy, mask) or off + 4 * bin(mask).count("1") > cap:
            continue
        for j, head in enumerate(i for i in range(64) if (mask >> i) & 1):
            k = MR.level_from_mask(bw, bh, cx, cy, mask, head)
            x, y = MR.unmorton(head)
            X, Y, n = 8 * cx + x, 8 * cy + y, 1 << k
            p = MR.predictor(field, X, Y, n)
            d = src[off + 4 * j + 2:off + 4 * j + 4].view(np.int16)
            field[Y:Y + n, X:X + n] = (MR.wrap16(p[0] + int(d[0])), MR.wrap16(p[1] + int(d[1])))
            level[Y:Y + n, X:X + n] = k
    return field.astype(np.int16).reshape(-1, 2), level.ravel()


# ---- fixtures -------------------------------------------------------------------------------------------------------------------------------
def words_of(diffs):
    """pack-form words of partitions with the given true differences, |d| <= 65535: q = d with P = 0 where d fits int16, otherwise q at the
    end of int16 on d's side and P = q - d"""
    out = []
    for d in diffs:
        q = [max(-32768, min(32767, int(v))) for v in d]
        out += [q[0] & 0xFFFF, q[1] & 0xFFFF, int(d[0]) & 0xFFFF, int(d[1]) & 0xFFFF]
    return np.array(out, np.uint16)


def extreme_diffs(n_parts, seed=0):
    """n_parts differences whose components are all +-65535"""
    rs = np.random.RandomState(seed)
    return [tuple(int(v) for v in 65535 * (2 * rs.randint(0, 2, 2) - 1)) for _ in range(n_parts)]
