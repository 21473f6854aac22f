"""CPU: the reference of the entropy coder (tests/_entropy_ref.py) against the header's worked values and against the properties the contract
rests on; the default table recomputed from the rate functions the library exports; and the three host helpers of the built library
(xEntropyDefaultInit, xEntropyEncodeRegion, xEntropyDecodeRegion) against the reference.  No GPU."""
import math
import os
import re

import numpy as np
import pytest

import _entropy_ref as E
import _levels_ref as LR
import x266_amd
import x266_amd.entropy as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKED = {"DC = 1": (0, 1, "80", 4, 1), "DC = -32768": (0, -32768, "9f fffa eacd".replace(" ", ""), 5, 33), "3 at the last position": (1023, 3, "ffffff7efb800412", 114, 8)}


def regions():
    """(levels, k) over every size class: sparse, dense, the int16 extremes, all zero"""
    out = []
    lv, cls = LR.sparse()
    out += [(lv[r], int(cls[r]) & 3) for r in range(len(lv))]
    lv, cls = E.mixed(24)
    out += [(lv[r], int(cls[r]) & 3) for r in range(len(lv))]
    dense = LR.dense(4)
    out += [(dense[k], k) for k in range(4)]
    return out


# ---- the header's worked values ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(WORKED))
def test_worked_values_of_the_header(name):
    at, value, hexed, n_ctx, n_byp = WORKED[name]
    lv = np.zeros(1024, np.int16)
    lv[at] = value
    data, ctx, byp = E.encode_region(lv, 3)
    assert (data.hex(), ctx, byp) == (hexed, n_ctx, n_byp)
    assert X.entropy_encode_region(lv, 3) == (data, len(data), n_ctx, n_byp)
    hdr = open(os.path.join(ROOT, "include", "x266hip.h")).read()
    assert " ".join(hexed[i:i + 2] for i in range(0, len(hexed), 2)) in hdr     # the header states these bytes
    back, n_nz, bad = E.decode_region(data, 3)
    assert np.array_equal(back, lv) and n_nz == 1 and not bad


def test_an_all_zero_region_is_no_bytes():
    for k in range(4):
        data, ctx, byp = E.encode_region(np.zeros(1024, np.int16), k)
        assert data == b"" and ctx == 64 >> (2 * k) and byp == 0              # one cbf per block
        assert X.entropy_encode_region(np.zeros(1024, np.int16), k)[1:] == (0, ctx, 0)
        back, n_nz, bad = E.decode_region(b"", k)
        assert not back.any() and n_nz == 0 and not bad


def test_header_constants():
    hdr = open(os.path.join(ROOT, "include", "x266hip.h")).read()
    assert int(re.search(r"#define X266_ENTROPY_CONTEXTS\s+(\d+)", hdr).group(1)) == E.CONTEXTS == x266_amd.ENTROPY_CONTEXTS
    assert int(re.search(r"#define X266_ENTROPY_MAX_BYTES\s+(\d+)", hdr).group(1)) == E.MAX_BYTES == x266_amd.ENTROPY_MAX_BYTES
    assert x266_amd.ENTROPY_REGION_DTYPE == E.RECORD_DTYPE and x266_amd.ENTROPY_REGION_DTYPE.itemsize == 32
    for f in ("offset", "n_words"):                                          # the first 20 bytes are the level record's
        assert E.RECORD_DTYPE.fields[f][1] == x266_amd.LEVEL_REGION_DTYPE.fields[f][1]


# ---- the round trip -------------------------------------------------------------------------------------------------------------------------
def test_round_trip_over_every_size_class():
    seen = set()
    for lv, k in regions():
        data, ctx, byp = E.encode_region(lv, k)
        back, n_nz, bad = E.decode_region(data, k)
        assert not bad and np.array_equal(back, lv) and n_nz == np.count_nonzero(lv), k
        assert data == b"" or data[-1] != 0                                   # trailing zero bytes are not stored
        seen.add(k)
    assert seen == {0, 1, 2, 3}


def test_the_level_minus_32768():
    for k in range(4):
        lv = np.zeros(1024, np.int16)
        lv[[0, 517, 1023]] = [-32768, -32768, 32767]
        data, _, byp = E.encode_region(lv, k)
        back, n_nz, bad = E.decode_region(data, k)
        assert not bad and np.array_equal(back, lv) and n_nz == 3 and byp >= 3 * 33


def test_bin_counts_are_the_rate_models():
    """context bins of the last position and bypass bins of a level are pos() and rem() of the model, as the library exports them"""
    for n in range(2, 6):
        for t in range(1 << n):
            bins = E.last_bins(t, n, E.LAST_X)
            assert 16 * 2 * len(bins) == x266_amd.last_pos_bits(t, t, n), (t, n)
            assert all(c is None or E.LAST_X <= c < E.LAST_X + 9 for c, _ in bins)
    fixed = x266_amd.level_bits(3, 0) - 16                                   # sig + sign + gt1 + gt2 + one remainder bin, less that bin
    for l in [3, 4, 5, 6, 7, 8, 9, 10, 13, 14, 100, 32767, 32768]:
        bypass = sum(1 for c, _ in E.level_bins(-l) if c is None) - 1          # less the sign
        assert 16 * bypass == x266_amd.level_bits(l, 0) - fixed, l
    assert [len(E.level_bins(l)) for l in (1, 2, 3, -32768)] == [2, 3, 4, 35]     # gt1 + sign; + gt2; + rem(0) = 1; + rem(32765) = 32


# ---- the largest substream --------------------------------------------------------------------------------------------------------------------
def test_the_largest_substream_stays_within_the_bound():
    """all 1024 levels at +-32767 under the least favourable table, every size; and the bound's own arithmetic"""
    most_ctx = most_byp = 0
    for k in range(4):
        data, ctx, byp = E.encode_region(E.maximal(), k, E.worst_init())
        assert 4000 < len(data) <= E.MAX_BYTES
        most_ctx, most_byp = max(most_ctx, ctx), max(most_byp, byp)
        back, n_nz, bad = E.decode_region(data, k, E.worst_init())
        assert not bad and np.array_equal(back, E.maximal()) and n_nz == 1024
        assert X.entropy_encode_region(E.maximal(), k, E.worst_init()) == (data, len(data), ctx, byp)
    assert (most_ctx, most_byp) == (3456, 33824)
    lv = np.full(1024, -32768, np.int16)                                       # one bin more per level: the true maximum of the bypass count
    assert max(E.encode_region(lv, k, E.worst_init())[2] for k in range(4)) == 33824 + 0 and E.encode_region(lv, 1)[2] == 33824
    bits = 3456 * math.log2(2048 / 31 / (1 - 2.0 ** -13)) + 33824 * math.log2(2 / (1 - 2.0 ** -23))
    assert bits < 54740 and 54740 // 8 + 1 + 4 <= E.MAX_BYTES                   # shifts <= bits / 8; the termination adds four stored bytes


def test_probabilities_stay_in_their_interval():
    for start in (E.P_MIN, E.P_MAX, 1024):
        for bit in (0, 1):
            ctx = [start]
            for _ in range(400):
                E.code_bins([(0, bit)], ctx)
                assert E.P_MIN <= ctx[0] <= E.P_MAX
            assert ctx[0] == (E.P_MIN if bit else E.P_MAX)


# ---- decoding is total ------------------------------------------------------------------------------------------------------------------------
def test_decoding_random_bytes_terminates_and_is_canonical_or_malformed():
    rng = np.random.RandomState(17)
    malformed = 0
    for i in range(400):
        k = i & 3
        raw = rng.randint(0, 256, rng.randint(0, 120)).astype(np.uint8)
        if i % 4 == 0 and raw.size:
            raw[:rng.randint(1, raw.size + 1)] = 0xFF
        data = raw.tobytes()
        lv, n_nz, bad = E.decode_region(data, k)
        got = X.entropy_decode_region(data, k)
        assert np.array_equal(got[0], lv) and got[1:] == (n_nz, bad), i         # the library's decoder is the reference's on garbage too
        if bad:
            malformed += 1
            assert not lv.any() and n_nz == 0
            continue
        again = E.encode_region(lv, k)[0]
        back, n_back, bad_back = E.decode_region(again, k)
        assert not bad_back and np.array_equal(back, lv) and n_back == n_nz == np.count_nonzero(lv), i
    assert 20 < malformed < 380
    lv, n_nz, bad = E.decode_region(b"\xff" * 64, 3)                            # code = range: every bin a one, the prefix never ends
    assert bad and X.entropy_decode_region(b"\xff" * 64, 3)[2]


# ---- the default table -----------------------------------------------------------------------------------------------------------------------
def test_default_table_follows_the_rate_functions():
    """recomputed from xLevelBits and xCgFlagBits: sig[c][0] = R(0, c); sig[c][1], gt1 and gt2 from the differences of R(1), R(2), R(3)"""
    L = x266_amd.level_bits
    # R(1) = sig1 + 16 + gt1[0]; R(2) = sig1 + 16 + gt1[1] + gt2[0]; R(3) = sig1 + 16 + gt1[1] + gt2[1] + 16: three equations, four unknowns
    # per class -- the header's statement of the model gives gt1[0] = 10, the rest follows and must agree over the classes
    gt1_0 = 10
    rows = []
    for c in range(3):
        s1 = L(1, c) - 16 - gt1_0
        rows.append((s1, L(2, c) - L(1, c), L(3, c) - L(2, c)))                # sig1, gt1[1] + gt2[0] - gt1[0], gt2[1] - gt2[0] + 16
    assert len({r[1:] for r in rows}) == 1
    hdr = open(os.path.join(ROOT, "include", "x266hip.h")).read()
    m = re.search(r"gt1\[0/1\] = \{(\d+),(\d+)\}\s+gt2\[0/1\] = \{(\d+),(\d+)\}", hdr)
    gt1, gt2 = (int(m.group(1)), int(m.group(2))), (int(m.group(3)), int(m.group(4)))
    assert gt1[0] == gt1_0 and rows[0][1] == gt1[1] + gt2[0] - gt1[0] and rows[0][2] == gt2[1] - gt2[0] + 16
    sig = [(L(0, c), rows[c][0]) for c in range(3)]
    cgf = (x266_amd.cg_flag_bits(0), x266_amd.cg_flag_bits(1))
    want = E.default_init(sig, gt1, gt2, cgf)
    assert np.array_equal(want, E.default_init()) and np.array_equal(X.entropy_default_init(), want)
    assert want[:19].tolist() == [1024] * 19 and want[19:25].tolist() == [1385, 723, 1242, 1609, 1325, 1263]
    assert np.array_equal(want.reshape(4, 25), np.tile(want[:25], (4, 1))) and want.min() >= E.P_MIN and want.max() <= E.P_MAX
    src = open(os.path.join(ROOT, "x266_amd", "csrc", "x266_entropy.hpp")).read()
    assert "1385, 723, 1242, 1609, 1325, 1263" in src                          # written as literals there


# ---- the host helpers ---------------------------------------------------------------------------------------------------------------------------
def test_host_helpers_against_the_reference():
    table = np.random.RandomState(3).randint(E.P_MIN, E.P_MAX + 1, E.CONTEXTS).astype(np.uint16)
    for init in (None, table):
        for lv, k in regions():
            data, ctx, byp = E.encode_region(lv, k, init)
            assert X.entropy_encode_region(lv, k | 0xA4, init) == (data, len(data), ctx, byp)        # only cls & 3 counts
            back, n_nz, bad = X.entropy_decode_region(data, k, init)
            assert not bad and np.array_equal(back, lv) and n_nz == np.count_nonzero(lv)


def test_host_helpers_capacity_and_refusals():
    lv, k = LR.dense(1)[0], 3
    data, _, _ = E.encode_region(lv, k)
    for cap in (0, 1, len(data) - 1, len(data)):
        got = X.entropy_encode_region(lv, k, cap=cap)
        assert got[0] == data[:cap] and got[1] == len(data)                    # the count is whole, the bytes stop at the capacity
    for at, value in ((0, 30), (99, 2018)):
        table = E.default_init().copy()
        table[at] = value
        with pytest.raises(x266_amd.X266Error):
            X.entropy_encode_region(lv, k, table)
        with pytest.raises(x266_amd.X266Error):
            X.entropy_decode_region(data, k, table)
    with pytest.raises(x266_amd.X266Error):
        X.entropy_decode_region(b"\0" * (E.MAX_BYTES + 1), k)
    L = x266_amd.load_library()
    assert L.xEntropyDefaultInit(None) == -1 and L.xEntropyEncodeRegion(None, 3, None, None, 0, None) == -1
    assert L.xEntropyDecodeRegion(None, 0, 3, None, None, None) == -1
