"""The reference statement of the entropy coder of the side information (include/x266hip.h, "the entropy coder of the side information":
xEntropyEncodeSideGpu, xEntropyDecodeSideGpu) in Python integers and lists, on top of _entropy_ref.code_bins and _entropy_ref.Decoder.
Written from the header, independently of x266_entropy_side.hpp: a CTU is five plain lists of six entries (the C++ packs it into
integers), the mode lists are Python lists and the ranks are taken by sorting (the C++ counts bits of a set), the encoder first lists its
bins and then codes the list.

Nothing here is derived from the library under test."""
import numpy as np

import _entropy_ref as ER

CONTEXTS = 16
MAX_BYTES = 80
KIND, MPM, LISTED, CODED, SMALL, SIZE, TYPE, NZ, GT1 = 0, 2, 3, 4, 6, 8, 10, 13, 15
CLASSES = 0x777F                                                               # X266_TDECIDE_CLASSES
CODED_DTYPE = np.dtype([("ctx_bins", "<u4"), ("bypass_bins", "<u4"), ("offset", "<u8"), ("n_words", "<u4"), ("n_bytes", "<u4"), ("n_intra", "<u4"),
                        ("n_coded", "<u4")])
assert CODED_DTYPE.itemsize == 32


def default_init():
    return np.full(CONTEXTS, 1024, np.uint16)


def _init(init):
    table = default_init() if init is None else np.asarray(init)
    assert table.size == CONTEXTS and table.min() >= ER.P_MIN and table.max() <= ER.P_MAX
    return [int(x) for x in table]


def clamp_qp(v):
    return max(0, min(51, v))


def predictors(Z, Q, qp, off):
    """per region (predictor, value): an uncoded region takes its predictor"""
    out, cur = [], qp
    for q in range(4):
        own = Q[q] if Z[q] else cur
        out.append((cur, own))
        cur = own
    pu = clamp_qp(cur + off)
    u = Q[4] if Z[4] else pu
    out.append((pu, u))
    out.append((u, Q[5] if Z[5] else u))
    return out


def canon(kind=None, mode=None, cls=None, qpa=None, nnz=None, qp=32, off=0):
    """(K, M, Z, C, Q), six entries each, from six entries of each input array (None: the NULL array of the encode call)"""
    assert not (kind is not None and mode is None)
    K = [0] * 6 if kind is None else [int(kind[q] != 0) for q in (0, 1, 2, 3, 4, 4)]
    M = [min(int(mode[q]), 34) if K[i] else 255 for i, q in enumerate((0, 1, 2, 3, 4, 4))] if mode is not None else [255] * 6
    Z = [1] * 6 if nnz is None else [int(int(v) != 0) for v in nnz]
    C = [3] * 6
    if cls is not None:
        for q in range(6):
            k = int(cls[q]) & 15
            C[q] = 3 if (k & 3) == 3 else k
    Q = [qp] * 4 + [clamp_qp(qp + off)] * 2 if qpa is None else [min(int(v), 51) for v in qpa]
    pv = predictors(Z, Q, qp, off)
    for q in range(6):
        if not Z[q]:
            C[q], Q[q] = 3, pv[q][1]
    assert all((CLASSES >> c) & 1 for c in C)
    return K, M, Z, C, Q


def flat(qp=32, off=0):
    return [0] * 6, [255] * 6, [0] * 6, [3] * 6, [qp] * 4 + [clamp_qp(qp + off)] * 2


def mpm_list(K, M, q):
    A = M[q - 1] if q & 1 and K[q - 1] else 1
    B = M[q - 2] if q >= 2 and K[q - 2] else 1
    if A == B:
        return [0, 1, 26] if A < 2 else [A, 2 + ((A + 29) & 31), 2 + ((A - 1) & 31)]
    return [A, B, next(m for m in (0, 1, 26) if m not in (A, B))]


def chroma_list(K, M):
    out = []
    for m in ([M[0]] if K[0] else []) + [0, 26, 10, 1]:
        if m not in out:
            out.append(m)
    return out


def unary(v, top, ctx=None):
    bins = [(None if ctx is None else ctx + i, 1) for i in range(v)]
    if v < top:
        bins.append((None if ctx is None else ctx + v, 0))
    return bins


def mode_bins(flag, lst, m):
    if m in lst:
        return [(flag, 1)] + unary(lst.index(m), len(lst) - 1)
    rank = sorted(x for x in range(35) if x not in lst).index(m)
    return [(flag, 0)] + [(None, (rank >> i) & 1) for i in (4, 3, 2, 1, 0)]


def class_bins(c, chroma):
    if c == 3:
        return [(SMALL + chroma, 0)]
    return [(SMALL + chroma, 1)] + unary(2 - (c & 3), 2, SIZE) + unary(c >> 2, 3, TYPE)


def dqp_bins(d, chroma):
    a = abs(d)
    assert a <= 51
    bins = [(NZ + chroma, int(a != 0))]
    if a == 0:
        return bins
    bins.append((GT1, int(a > 1)))
    if a > 1:
        v = (a - 2) + 1
        k = v.bit_length() - 1
        bins += [(None, 1)] * k + [(None, 0)] + [(None, (v >> i) & 1) for i in reversed(range(k))]
    return bins + [(None, int(d < 0))]


def ctu_bins(ctu, qp=32, off=0):
    K, M, Z, C, Q = ctu
    pv = predictors(Z, Q, qp, off)
    bins = []

    def residual(q, chroma):
        bins.append((CODED + chroma, Z[q]))
        if Z[q]:
            bins.extend(class_bins(C[q], chroma) + dqp_bins(Q[q] - pv[q][0], chroma))

    for q in range(4):
        bins.append((KIND, K[q]))
        if K[q]:
            bins.extend(mode_bins(MPM, mpm_list(K, M, q), M[q]))
        residual(q, 0)
    bins.append((KIND + 1, K[4]))
    if K[4]:
        bins.extend(mode_bins(LISTED, chroma_list(K, M), M[4]))
    residual(4, 1)
    residual(5, 1)
    return bins


def encode_ctu(ctu, qp=32, off=0, init=None):
    """-> (bytes, context bins, bypass bins) of a canonical CTU"""
    bins = ctu_bins(ctu, qp, off)
    data = ER.code_bins(bins, _init(init))
    n_ctx = sum(1 for c, _ in bins if c is not None)
    return data, n_ctx, len(bins) - n_ctx


def _dec_unary(d, top, ctx=None):
    v = 0
    while v < top and (d.bypass() if ctx is None else d.bin(ctx + v)):
        v += 1
    return v


def _dec_mode(d, flag, lst):
    if d.bin(flag):
        return lst[_dec_unary(d, len(lst) - 1)]
    others = sorted(x for x in range(35) if x not in lst)
    rank = d.bits(5)
    if rank >= len(others):
        raise ER.Malformed("rank")
    return others[rank]


def _dec_residual(d, chroma, pred):
    """(coded, class, qp)"""
    if not d.bin(CODED + chroma):
        return 0, 3, pred
    c = 3
    if d.bin(SMALL + chroma):
        c = 2 - _dec_unary(d, 2, SIZE)
        c |= _dec_unary(d, 3, TYPE) << 2
    dq = 0
    if d.bin(NZ + chroma):
        a = 1
        if d.bin(GT1):
            k = 0
            while k < 6 and d.bypass():
                k += 1
            if k > 5:
                raise ER.Malformed("prefix")
            a = ((1 << k) | d.bits(k)) + 1
        dq = -a if d.bypass() else a
    if not 0 <= pred + dq <= 51:
        raise ER.Malformed("qp")
    return 1, c, pred + dq


def decode_ctu(data, qp=32, off=0, init=None):
    """-> ((K, M, Z, C, Q), malformed reason or None); a malformed substream gives the flat CTU"""
    d = ER.Decoder(bytes(data), _init(init))
    K, M, Z, C, Q = [0] * 6, [255] * 6, [0] * 6, [3] * 6, [0] * 6
    try:
        cur = qp
        for q in range(4):
            K[q] = d.bin(KIND)
            if K[q]:
                M[q] = _dec_mode(d, MPM, mpm_list(K, M, q))
            Z[q], C[q], Q[q] = _dec_residual(d, 0, cur)
            cur = Q[q]
        K[4] = K[5] = d.bin(KIND + 1)
        if K[4]:
            M[4] = M[5] = _dec_mode(d, LISTED, chroma_list(K, M))
        Z[4], C[4], Q[4] = _dec_residual(d, 1, clamp_qp(cur + off))
        Z[5], C[5], Q[5] = _dec_residual(d, 1, Q[4])
    except ER.Malformed as e:
        return flat(qp, off), str(e)
    return (K, M, Z, C, Q), None


# ---- the calls ----------------------------------------------------------------------------------------------------------------------------
def canon_arrays(n_ctu, kind=None, mode=None, cls=None, qpa=None, nnz=None, qp=32, off=0):
    """the canonical CTUs of whole input arrays [6 n_ctu] (None: NULL)"""
    pick = lambda a, c: None if a is None else np.asarray(a).ravel()[6 * c:6 * c + 6]
    return [canon(pick(kind, c), pick(mode, c), pick(cls, c), pick(qpa, c), pick(nnz, c), qp, off) for c in range(n_ctu)]


def assemble(coded, cap_words=None):
    """coded: per CTU (bytes, context bins, bypass bins, n_intra, n_coded) -> (records, stream, total)"""
    n = len(coded)
    rec = np.zeros(n, CODED_DTYPE)
    payloads = []
    for c, (data, n_ctx, n_byp, n_intra, n_coded) in enumerate(coded):
        payloads.append(data + b"\0" * (len(data) & 1))
        rec[c] = (n_ctx, n_byp, 0, (len(data) + 1) // 2, len(data), n_intra, n_coded)
    ends = np.cumsum(rec["n_words"].astype(np.uint64), dtype=np.uint64)
    rec["offset"] = ends - rec["n_words"]
    total = int(ends[-1]) if n else 0
    cap = total if cap_words is None else int(cap_words)
    stream = np.zeros(cap, np.uint16)
    fit = 0
    for c in range(n):
        o, nw = int(rec["offset"][c]), int(rec["n_words"][c])
        if o + nw > cap:
            continue
        fit += 1
        stream[o:o + nw] = np.frombuffer(payloads[c], "<u2")
    return rec, stream, np.array([total, fit], np.uint64)


def encode(n_ctu, kind=None, mode=None, cls=None, qpa=None, nnz=None, qp=32, off=0, cap_words=None, init=None):
    """xEntropyEncodeSideGpu -> (coded [n_ctu] CODED_DTYPE, stream uint16 [cap_words], total uint64 [2]); words not written are 0"""
    coded = []
    for ctu in canon_arrays(n_ctu, kind, mode, cls, qpa, nnz, qp, off):
        coded.append(encode_ctu(ctu, qp, off, init) + (sum(ctu[0]), sum(ctu[2])))
    return assemble(coded, cap_words)


def decode(coded, stream, qp=32, off=0, cap_words=None, init=None):
    """xEntropyDecodeSideGpu -> (kind, mode, class, qp uint8 [6 n], nnz uint32 [6 n], status uint8 [n])"""
    src = np.asarray(stream, np.uint16).ravel()
    cap = src.size if cap_words is None else int(cap_words)
    raw = src[:cap].astype("<u2").tobytes()
    n = len(coded)
    out = [np.zeros(6 * n, np.uint8) for _ in range(4)] + [np.zeros(6 * n, np.uint32)]
    status = np.zeros(n, np.uint8)
    for c in range(n):
        o, nb = int(coded["offset"][c]), int(coded["n_bytes"][c])
        data = b""
        if nb > MAX_BYTES or o > cap or (nb + 1) // 2 > cap - o:
            status[c] = 1
        else:
            data = raw[2 * o:2 * o + nb]
        (K, M, Z, C, Q), bad = decode_ctu(data, qp, off, init)
        if bad:
            status[c] = 2
        for a, v in zip(out, (K, M, C, Q, Z)):
            a[6 * c:6 * c + 6] = v
    return out[0], out[1], out[2], out[3], out[4], status


# ---- fixtures -------------------------------------------------------------------------------------------------------------------------------
def worst_ctu():
    """the worst CTU the syntax can hold at qp 0, offset 0: every region intra with an unlisted mode, every class 0 of type 3, every
    qp difference +-51"""
    return canon([1] * 6, [34, 33, 32, 31, 33, 33], [12] * 6, [51, 0, 51, 0, 51, 0], [1] * 6, 0, 0)


def random_arrays(n_ctu, seed, flat_share=0.5, intra_share=0.15):
    """(kind, mode, cls, qp uint8 [6 n], nnz uint32 [6 n]): junk byte values everywhere, about flat_share flat CTUs, some all-intra CTUs,
    qp swinging between 0 and 51 in some"""
    rs = np.random.RandomState(seed)
    n = 6 * n_ctu
    kind = rs.choice(np.array([0, 0, 0, 1, 2, 3], np.uint8), n)
    mode = rs.randint(0, 256, n).astype(np.uint8)
    mode[rs.rand(n) < 0.6] %= 35
    cls = rs.randint(0, 256, n).astype(np.uint8)
    qpa = rs.randint(0, 256, n).astype(np.uint8)
    tame = rs.rand(n) < 0.7
    qpa[tame] = np.clip(30 + rs.randint(-3, 4, n), 0, 51).astype(np.uint8)[tame]
    nnz = rs.choice(np.array([0, 0, 1, 2 ** 31, 7], np.uint32), n)
    pick = rs.rand(n_ctu)
    for c in range(n_ctu):
        s = slice(6 * c, 6 * c + 6)
        if pick[c] < flat_share:
            kind[s], nnz[s] = 0, 0
        elif pick[c] < flat_share + intra_share:
            kind[s] = rs.randint(1, 4, 6)
        elif pick[c] < flat_share + intra_share + 0.1:
            qpa[s] = [0, 51, 0, 255, 51, 0] if c & 1 else [51, 0, 200, 0, 0, 51]
            nnz[s] = 1
    return kind, mode, cls, qpa, nnz
