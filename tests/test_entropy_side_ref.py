"""CPU: the reference statement of tests/_entropy_side_ref.py (the entropy coder of the side information) against the header's worked
values, its own round trip, hand-written mode lists and the derived bound, and the library's host helpers (xEntropySideDefaultInit,
xEntropyEncodeSideCtu, xEntropyDecodeSideCtu: the functions the kernels run) against the reference.  No GPU."""
import os
import re

import numpy as np
import pytest

import _entropy_ref as ER
import _entropy_side_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z0 = [0] * 6
# (canonical CTU, qp, bytes in hex, context bins, bypass bins): the header's list, in its order
WORKED = [
    (S.flat(), 32, "", 11, 0),
    (S.canon([1, 0, 0, 0, 0, 0], [26] * 6, None, None, Z0), 32, "f0", 12, 2),
    (S.canon([1, 0, 0, 0, 0, 0], [10] * 6, None, None, Z0), 32, "8f ff fc", 12, 5),
    (S.canon([0, 0, 0, 0, 1, 0], [34] * 6, None, None, Z0), 32, "01 0c 0e", 12, 5),
    (S.canon(None, None, [0, 14, 3, 3, 3, 3], None, [1, 1, 0, 0, 0, 0]), 32, "78 df ae", 22, 0),
    (S.canon(None, None, None, [33, 32, 32, 32, 32, 32], [1, 0, 0, 0, 0, 0]), 32, "50", 14, 1),
    (S.canon(None, None, None, [0] * 6, [1, 0, 0, 0, 0, 0], 51, 0), 51, "5f d2 7c", 14, 12),
    (S.canon(), 32, "44 4d 5a", 23, 0),
]
TABLES = [None, np.full(16, 31, np.uint16), np.full(16, 2017, np.uint16), np.random.RandomState(4).randint(31, 2018, 16).astype(np.uint16)]
SCALARS = [(32, 0), (0, -12), (51, 12), (20, 5)]
# seeds of 24 random bytes that reach each malformed case at (qp, offset) = (30, 0), found once on the CPU; most others decode to some CTU
MALFORMED_SEEDS = {"prefix": 81, "rank": 113}


def header_block():
    hdr = open(os.path.join(ROOT, "include", "x266hip.h")).read()
    return hdr[hdr.index("---- the entropy coder of the side information"):hdr.index("#define X266_ENTROPY_SIDE_CONTEXTS")]


def test_the_worked_values_of_the_header():
    text = header_block()
    lines = re.findall(r"^ \*     (.+?):\s+((?:[0-9a-f]{2} ?)+|no bytes) \((\d+), (\d+)\)$", text, re.M)
    assert len(lines) == len(WORKED) >= 6
    for (ctu, qp, data, n_ctx, n_byp), (_, said, c, b) in zip(WORKED, lines):
        got = S.encode_ctu(ctu, qp, 0)
        assert got == (bytes.fromhex(data), n_ctx, n_byp), (data, got[0].hex(" "))
        assert ("" if said == "no bytes" else said.strip()) == data and (int(c), int(b)) == (n_ctx, n_byp)
        back, bad = S.decode_ctu(got[0], qp, 0)
        assert bad is None and [list(v) for v in back] == [list(v) for v in ctu]


def test_the_flat_ctu_both_ways():
    for init in TABLES:
        for qp, off in SCALARS:
            assert S.encode_ctu(S.flat(qp, off), qp, off, init) == (b"", 11, 0)
            ctu, bad = S.decode_ctu(b"", qp, off, init)
            assert bad is None and [list(v) for v in ctu] == [list(v) for v in S.flat(qp, off)]
            assert ctu[1] == [255] * 6 and ctu[3] == [3] * 6 and ctu[4] == [qp] * 4 + [S.clamp_qp(qp + off)] * 2


def test_round_trip_to_the_canonical_form():
    """every class byte, kinds 0..3, modes and qp 0..255, d_nnz 0, 1 and 2^31: decode of encode is the canonical form, which is a fixed point"""
    rs = np.random.RandomState(2)
    seen_cls, seen_mode, seen_qp = set(), set(), set()
    for i in range(700):
        kind = rs.randint(0, 4, 6)
        mode, cls, qpa = rs.randint(0, 256, 6), (np.arange(6) * 43 + i) % 256 if i < 256 else rs.randint(0, 256, 6), rs.randint(0, 256, 6)
        nnz = rs.choice(np.array([0, 1, 2 ** 31], np.uint32), 6)
        qp, off = SCALARS[i % 4]
        init = TABLES[i % 4]
        seen_cls |= set(int(c) for c in cls)
        seen_mode |= set(int(m) for m in mode)
        seen_qp |= set(int(q) for q in qpa)
        ctu = S.canon(kind, mode, cls, qpa, nnz, qp, off)
        K, M, Z, C, Q = ctu
        assert K[4] == K[5] == int(kind[4] != 0) and M[4] == M[5] and all(m == 255 or m <= 34 for m in M) and all(q <= 51 for q in Q)
        assert all(Z[q] or C[q] == 3 for q in range(6)) and all((S.CLASSES >> c) & 1 for c in C)
        data, n_ctx, n_byp = S.encode_ctu(ctu, qp, off, init)
        assert len(data) <= S.MAX_BYTES and n_ctx <= 64 and n_byp <= 97
        back, bad = S.decode_ctu(data, qp, off, init)
        assert bad is None and [list(v) for v in back] == [list(v) for v in ctu], (i, ctu, back)
        again = S.canon(back[0], back[1], back[3], back[4], back[2], qp, off)
        assert [list(v) for v in again] == [list(v) for v in ctu] and S.encode_ctu(again, qp, off, init)[0] == data
    assert seen_cls == set(range(256)) and seen_mode == set(range(256)) and seen_qp == set(range(256))


def test_the_mode_lists():
    K, M = [1, 1, 1, 0, 0, 0], [10, 2, 10, 255, 255, 255]
    assert S.mpm_list(K, M, 0) == [0, 1, 26]                                   # no neighbour inside the CTU
    assert S.mpm_list(K, M, 1) == [10, 1, 0]                                   # A = 10, B absent = 1
    assert S.mpm_list(K, M, 2) == [1, 10, 0]                                   # A absent, B = 10
    assert S.mpm_list(K, M, 3) == [10, 2, 0]
    assert S.mpm_list(K, [10, 10, 10, 255, 255, 255], 3) == [10, 9, 11]
    assert S.mpm_list(K, [0, 2, 2, 255, 255, 255], 3) == [2, 33, 3]
    assert S.mpm_list(K, [0, 34, 34, 255, 255, 255], 3) == [34, 33, 3]
    assert S.mpm_list(K, [0, 0, 1, 255, 255, 255], 3) == [1, 0, 26]
    assert S.mpm_list(K, [0, 26, 0, 255, 255, 255], 3) == [0, 26, 1]
    assert S.mpm_list([0, 0, 1, 0, 0, 0], [255, 255, 7, 255, 255, 255], 3) == [7, 1, 0]    # an inter neighbour counts as mode 1
    assert S.mpm_list([0, 1, 0, 0, 0, 0], [255, 1, 255, 255, 255, 255], 3) == [0, 1, 26]
    assert S.chroma_list([1] + [0] * 5, [10] + [255] * 5) == [10, 0, 26, 1]
    assert S.chroma_list([1] + [0] * 5, [7] + [255] * 5) == [7, 0, 26, 10, 1]
    assert S.chroma_list([0, 1, 0, 0, 0, 0], [255, 7, 255, 255, 255, 255]) == [0, 26, 10, 1]
    # every mode of a region comes back, listed or not, with the bins the header counts
    for first in (7, 26):
        for m in range(35):
            ctu = S.canon([1, 0, 0, 0, 1, 1], [first, 0, 0, 0, m, 0], None, None, Z0)
            data, n_ctx, n_byp = S.encode_ctu(ctu)
            lst = S.chroma_list(ctu[0], ctu[1])
            index = lst.index(m) if m in lst else None
            assert n_byp - S.encode_ctu(S.canon([1, 0, 0, 0, 0, 0], [first] * 6, None, None, Z0))[2] == (5 if index is None else min(index + 1, len(lst) - 1))
            assert S.decode_ctu(data)[0][1][4:] == [m, m]


def test_the_worst_ctu_stays_within_the_bound():
    ctu = S.worst_ctu()
    sizes = {}
    for p in (1024, 31, 2017):
        data, n_ctx, n_byp = S.encode_ctu(ctu, 0, 0, np.full(16, p, np.uint16))
        assert (n_ctx, n_byp) == (64, 97) and len(data) <= S.MAX_BYTES
        sizes[p] = len(data)
        assert S.decode_ctu(data, 0, 0, np.full(16, p, np.uint16))[0][4] == [51, 0, 51, 0, 51, 0]
    text = header_block()
    assert sizes[1024] == 20 and sizes[2017] == 43 and "to 20 bytes under the default table and to 43 under a table of 2017s" in text
    # the derivation beside the constant: 64 context bins under 6.05 bits, 97 bypass bins under 1.0001, the termination, a multiple of 16
    bits = 64 * 6.05 + 97 * 1.0001
    assert bits < 485 and -(-485 // 8) == 61 and -(-(61 + 4) // 16) * 16 == S.MAX_BYTES == 80
    for said in ("64 in all", "= 97", "under 485 bits", "61 byte shifts", "65 bytes", "X266_ENTROPY_SIDE_MAX_BYTES =\n * 80"):
        assert said in text, said
    # an adversarial table per context cannot do worse than every context at its worse end
    worst = 0
    for seed in range(40):
        table = np.random.RandomState(seed).choice(np.array([31, 2017], np.uint16), 16)
        worst = max(worst, len(S.encode_ctu(ctu, 0, 0, table)[0]))
    assert worst <= S.MAX_BYTES


def test_decode_of_random_bytes_is_total_and_reaches_every_malformed_case():
    reached = set()
    for seed in range(120):
        data = bytes(np.random.RandomState(seed).randint(0, 256, 24).astype(np.uint8))
        for (qp, off), init in zip(SCALARS, TABLES):
            ctu, bad = S.decode_ctu(data, qp, off, init)
            K, M, Z, C, Q = ctu
            assert all(k in (0, 1) for k in K) and all(m == 255 or m <= 34 for m in M) and all(0 <= q <= 51 for q in Q) and all((S.CLASSES >> c) & 1 for c in C)
            if bad:
                reached.add(bad)
                assert [list(v) for v in ctu] == [list(v) for v in S.flat(qp, off)]
            else:                                                              # whatever came out is canonical and codes to something that decodes to it
                again, _ = S.decode_ctu(S.encode_ctu(ctu, qp, off, init)[0], qp, off, init)
                assert [list(v) for v in again] == [list(v) for v in ctu]
    for why, seed in MALFORMED_SEEDS.items():
        data = bytes(np.random.RandomState(seed).randint(0, 256, 24).astype(np.uint8))
        assert S.decode_ctu(data, 30, 0)[1] == why
        reached.add(why)
    assert S.decode_ctu(b"\xff" * 16, 30, 0)[1] == "prefix"
    assert reached == {"prefix", "rank", "qp"}                                 # the three malformed cases the header names
    text = header_block()
    for said in ("a decoded rank at or beyond their number is malformed", "A prefix of more than 5 ones is malformed", "outside 0..51 is malformed"):
        assert said in re.sub(r"\s*\n \*\s*", " ", text), said


def test_assembly_and_the_capacity_rule():
    n = 70
    arrays = S.random_arrays(n, 3)
    rec, stream, total = S.encode(n, *arrays, qp=30, off=-2)
    assert int(total[0]) == int(rec["n_words"].sum()) == stream.size and int(total[1]) == n
    assert np.array_equal(rec["n_words"], (rec["n_bytes"] + 1) // 2) and rec["n_intra"].max() <= 6 and rec["n_coded"].max() <= 6
    out = S.decode(rec, stream, qp=30, off=-2)
    assert not out[5].any()
    for c, ctu in enumerate(S.canon_arrays(n, *arrays, qp=30, off=-2)):
        for a, v in zip(out[:5], (ctu[0], ctu[1], ctu[3], ctu[4], ctu[2])):
            assert a[6 * c:6 * c + 6].tolist() == v
    cap = int(rec["offset"][n // 2]) + 1
    rec2, cut, total2 = S.encode(n, *arrays, qp=30, off=-2, cap_words=cap)
    assert np.array_equal(rec2, rec) and int(total2[0]) == int(total[0]) and int(total2[1]) < n and np.array_equal(cut[:int(rec["offset"][n // 2])],
                                                                                                                    stream[:int(rec["offset"][n // 2])])
    status = S.decode(rec, cut, qp=30, off=-2)[5]
    assert set(status.tolist()) == {0, 1} and status[0] == 0 and status[-1] == 1      # an offset beyond the capacity, whatever the length


# ---- the library's host helpers: the functions the kernels run ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def helpers():
    import x266_amd
    import x266_amd.entropy as X
    x266_amd.build_library()
    return X


def test_the_host_helpers_give_the_reference(helpers):
    X = helpers
    assert np.array_equal(X.entropy_side_default_init(), S.default_init())
    for ctu, qp, data, n_ctx, n_byp in WORKED:
        K, M, Z, C, Q = ctu
        got = X.entropy_encode_side_ctu(K, [m if m < 255 else 77 for m in M], C, Q, Z, qp=qp)
        assert got == (bytes.fromhex(data), len(bytes.fromhex(data)), n_ctx, n_byp)
    assert X.entropy_encode_side_ctu()[0] == bytes.fromhex("44 4d 5a")          # every array NULL
    kind, mode, cls, qpa, nnz = S.random_arrays(160, 8, 0.3)
    rs = np.random.RandomState(1)
    for c in range(160):
        s = slice(6 * c, 6 * c + 6)
        qp, off = SCALARS[c % 4]
        init = TABLES[(c // 4) % 4]
        ctu = S.canon(kind[s], mode[s], cls[s], qpa[s], nnz[s], qp, off)
        want = S.encode_ctu(ctu, qp, off, init)
        data, n_bytes, n_ctx, n_byp = X.entropy_encode_side_ctu(kind[s], mode[s], cls[s], qpa[s], nnz[s], qp, off, init)
        assert (data, n_ctx, n_byp) == want and n_bytes == len(data)
        assert X.entropy_encode_side_ctu(kind[s], mode[s], cls[s], qpa[s], nnz[s], qp, off, init, cap=3)[:2] == (data[:3], n_bytes)
        k, m, cl, q, z, bad = X.entropy_decode_side_ctu(data, qp, off, init)
        assert not bad and [k.tolist(), m.tolist(), z.tolist(), cl.tolist(), q.tolist()] == [list(v) for v in ctu]
        junk = bytes(rs.randint(0, 256, rs.randint(0, 40)).astype(np.uint8))
        ref, why = S.decode_ctu(junk, qp, off, init)
        k, m, cl, q, z, bad = X.entropy_decode_side_ctu(junk, qp, off, init)
        assert bad == (why is not None) and [k.tolist(), m.tolist(), z.tolist(), cl.tolist(), q.tolist()] == [list(v) for v in ref]
    for why, seed in list(MALFORMED_SEEDS.items()) + [("qp", 0)]:
        junk = bytes(np.random.RandomState(seed).randint(0, 256, 24).astype(np.uint8))
        qp, off = (0, -12) if why == "qp" else (30, 0)
        assert S.decode_ctu(junk, qp, off)[1] == why
        k, m, cl, q, z, bad = X.entropy_decode_side_ctu(junk, qp, off)
        assert bad and not k.any() and not z.any() and m.tolist() == [255] * 6 and cl.tolist() == [3] * 6 and q.tolist() == S.flat(qp, off)[4]


def test_the_host_helpers_refuse_bad_arguments(helpers):
    X = helpers
    from x266_amd import X266Error
    six = np.zeros(6, np.uint8)
    for bad in (dict(kind=six), dict(qp=-1), dict(qp=52), dict(chroma_qp_offset=-13), dict(chroma_qp_offset=13), dict(init=np.full(16, 30)),
                dict(init=np.full(16, 2018)), dict(init=np.full(15, 1024)), dict(classes=np.zeros(5, np.uint8))):
        with pytest.raises(X266Error):
            X.entropy_encode_side_ctu(**bad)
    for bad in (dict(data=b"\0" * 81), dict(data=b"", qp=52), dict(data=b"", chroma_qp_offset=13), dict(data=b"", init=np.full(16, 2018))):
        with pytest.raises(X266Error):
            X.entropy_decode_side_ctu(**bad)
    assert X.entropy_decode_side_ctu(b"\0" * 80)[5] is False
    assert ER.P_MIN == 31 and ER.P_MAX == 2017
