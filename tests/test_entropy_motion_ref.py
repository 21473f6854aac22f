"""CPU: the reference of the entropy coder of the motion stream (tests/_entropy_motion_ref.py) against the header's worked values and the
properties the contract rests on, and the three host helpers of the built library (xEntropyMvDefaultInit, xEntropyEncodeMvCtu,
xEntropyDecodeMvCtu) against the reference.  No GPU."""
import os
import re

import numpy as np
import pytest

import _entropy_motion_ref as EM
import _motion_ref as MR
import x266_amd
import x266_amd.entropy as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (width, height, head mask, true differences in coding order, bytes, context bins, bypass bins)
WORKED = [
    (64, 64, 1, [(0, 0)], "", 3, 0),
    (64, 64, 1, [(1, 0)], "40", 4, 1),
    (64, 64, 1, [(-2, 5)], "67 90", 5, 8),
    (64, 64, 1, [(-65535, 65535)], "7f ff bb ff ff ff df ff c0", 5, 62),
    (32, 32, 0x1111, [(4, -8), (0, 0), (-1, 1), (0, 3)], "b8 78 3e d0 c2", 18, 17),
    (16, 16, 0xF, [(0, 0)] * 4, "80", 9, 0),
    (16, 16, 1, [(0, 0)], "", 3, 0),
]
CUSTOM = np.array([200, 1800, 31, 2017, 900, 1500, 640], np.uint16)
SIZES = MR.SIZES[:-1]


def header():
    return open(os.path.join(ROOT, "include", "x266hip.h")).read()


@pytest.mark.parametrize("case", range(len(WORKED)))
def test_worked_values_of_the_header(case):
    w, h, mask, diffs, hexed, n_ctx, n_byp = WORKED[case]
    words = EM.words_of(diffs)
    assert EM.true_diffs(words) == diffs
    data, ctx, byp = EM.encode_ctu(w, h, 0, mask, words)
    assert (data.hex(" "), ctx, byp) == (hexed, n_ctx, n_byp)
    assert X.entropy_encode_motion_ctu(w, h, 0, mask, words) == (data, len(data), n_ctx, n_byp)
    stated = "%s (%d, %d)" % (hexed or "no bytes", n_ctx, n_byp)
    assert stated in header()                                               # the header states these bytes and counts
    back_mask, back_words, parts, _, bad = EM.decode_ctu(w, h, 0, data)
    assert back_mask == mask and not bad and [(p[2], p[3]) for p in parts] == diffs
    lib_mask, lib_words, lib_bad = X.entropy_decode_motion_ctu(w, h, 0, data)
    assert lib_mask == mask and np.array_equal(lib_words, back_words) and not lib_bad


def flat_mask(w, h, c):
    """every whole node unsplit wherever the cut nodes lead"""
    bw, bh, cw, _ = MR.grid(w, h)
    parts, _ = MR.walk_ctu(bw, bh, c % cw, c // cw, lambda X, Y: 3)
    return sum(1 << MR.morton(X - 8 * (c % cw), Y - 8 * (c // cw)) for X, Y, _ in parts)


@pytest.mark.parametrize("w,h", [(16, 16), (64, 64), (80, 48)])
def test_the_flat_ctu_is_no_bytes_and_no_bytes_are_the_flat_ctu(w, h):
    _, _, cw, ch = MR.grid(w, h)
    for c in range(cw * ch):
        mask = flat_mask(w, h, c)
        n = bin(mask).count("1")
        words = EM.words_of([(0, 0)] * n)
        for init in (None, CUSTOM):
            assert EM.encode_ctu(w, h, c, mask, words, init)[0] == b""
            assert X.entropy_encode_motion_ctu(w, h, c, mask, words, init)[:2] == (b"", 0)
            back, wds, parts, _, bad = EM.decode_ctu(w, h, c, b"", init)
            assert back == mask and not wds.any() and len(parts) == n and not bad
            lib_mask, lib_words, lib_bad = X.entropy_decode_motion_ctu(w, h, c, b"", init)
            assert lib_mask == mask and lib_words.size == 4 * n and not lib_words.any() and not lib_bad


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("recipe", ["field", "inconsistent"])
def test_round_trip_and_bins_against_bits(w, h, recipe):
    """decode(encode(pack)) returns pack's records in every field but offset and pack's words 2 and 3, under the default and a custom table,
    reference and host helpers alike.  Bins against bits: L(0) = 1 = nz; L(+-1) = 3 = nz, gt1, sign; L(d) = 2 ilog2(|d|) + 3 = nz, gt1,
    2 ilog2(|d|) Exp-Golomb bins, sign; every flag of `bits` is one split bin.  So the bins of a CTU are exactly its bits."""
    mv, level = MR.field(w, h) if recipe == "field" else MR.inconsistent_field(w, h, 5)
    packed = MR.pack(mv, level, w, h)
    ctu, words = packed["ctu"], packed["stream"]
    for init in (None, CUSTOM):
        coded, stream, total = EM.encode(ctu, words, w, h, init=init)
        assert not coded["unreadable"].any() and np.array_equal(coded["parts"], ctu["parts"]) and int(total[1]) == len(ctu)
        assert np.array_equal(coded["ctx_bins"] + coded["bypass_bins"], ctu["bits"])
        assert int(coded["n_bytes"].max()) <= EM.MAX_BYTES
        back, out, status = EM.decode(coded, stream, w, h, init=init)
        assert not status.any()
        for name in ("head_mask", "n_words", "parts", "bits", "max_abs"):
            assert np.array_equal(back[name], ctu[name]), name
        assert np.array_equal(back["offset"], 256 * np.arange(len(ctu), dtype=np.uint64))
        for c in range(len(ctu)):
            off, n = int(ctu["offset"][c]), int(ctu["n_words"][c])
            want = words[off:off + n].reshape(-1, 4).copy()
            want[:, :2] = 0
            assert np.array_equal(out[256 * c:256 * c + n], want.ravel()) and not out[256 * c + n:256 * c + 256].any()
            raw = stream[int(coded["offset"][c]):int(coded["offset"][c]) + int(coded["n_words"][c])].astype("<u2").tobytes()[:int(coded["n_bytes"][c])]
            mask = int(ctu["head_mask"][c])
            assert X.entropy_encode_motion_ctu(w, h, c, mask, words[off:off + n], init) == (raw, len(raw), int(coded["ctx_bins"][c]), int(coded["bypass_bins"][c]))
            lib_mask, lib_words, lib_bad = X.entropy_decode_motion_ctu(w, h, c, raw, init)
            assert lib_mask == mask and np.array_equal(lib_words, want.ravel()) and not lib_bad
        if recipe == "field":                                               # differences are decodable for consistent fields
            got_mv, got_level = EM.reconstruct(back, out, w, h)
            assert np.array_equal(got_mv, packed["mv"]) and np.array_equal(got_level, packed["level"])


@pytest.mark.parametrize("w,h", SIZES)
def test_reference_reconstruct_is_unpack_on_consistent_fields(w, h):
    mv, level = MR.field(w, h)
    packed = MR.pack(mv, level, w, h)
    want_mv, want_level = MR.unpack(packed["ctu"], packed["stream"], w, h)
    junk = packed["stream"].reshape(-1, 4).copy()
    junk[:, :2] = 0xA5A5                                                    # words 0 and 1 are not read
    got_mv, got_level = EM.reconstruct(packed["ctu"], junk.ravel(), w, h)
    assert np.array_equal(got_mv, want_mv) and np.array_equal(got_level, want_level)
    assert np.array_equal(got_mv, MR.decode_differences(packed["ctu"], packed["stream"], w, h))


def test_the_worst_ctu_stays_under_the_bound():
    words = EM.words_of(EM.extreme_diffs(64))
    full = (1 << 64) - 1
    data, ctx, byp = EM.encode_ctu(64, 64, 0, full, words)
    assert (len(data), ctx, byp) == (511, 277, 3968)                        # the header's figure
    for init in (None, np.full(7, 31, np.uint16), np.full(7, 2017, np.uint16)):
        data = EM.encode_ctu(64, 64, 0, full, words, init)[0]
        assert len(data) <= EM.MAX_BYTES
        assert X.entropy_encode_motion_ctu(64, 64, 0, full, words, init)[:2] == (data, len(data))
        mask, back, bad = X.entropy_decode_motion_ctu(64, 64, 0, data, init)
        assert mask == full and not bad and np.array_equal(back.reshape(-1, 4)[:, 2:], words.reshape(-1, 4)[:, 2:])


def test_random_bytes_decode_to_something_and_re_encode_to_themselves():
    rs = np.random.RandomState(11)
    shapes = [(64, 64, 0), (80, 48, 1), (16, 16, 0), (144, 112, 5)]
    n_bad = 0
    for i in range(2000):
        w, h, c = shapes[i % len(shapes)]
        data = rs.randint(0, 256, rs.randint(0, 721)).astype(np.uint8).tobytes()
        if i % 7 == 0:
            data = b"\xff" * (len(data) // 8) + data                        # long runs of ones reach the prefix bound
            data = data[:720]
        init = None if i % 2 else CUSTOM
        mask, words, parts, _, bad = EM.decode_ctu(w, h, c, data, init)
        lib_mask, lib_words, lib_bad = X.entropy_decode_motion_ctu(w, h, c, data, init)
        assert (lib_mask, lib_bad) == (mask, bad) and np.array_equal(lib_words, words)
        n_bad += bad
        bw, bh, cw, _ = MR.grid(w, h)
        assert MR.well_formed(bw, bh, c % cw, c // cw, mask)
        if not bad:                                                         # the decoded CTU in pack's form codes to bytes that decode to it
            again = EM.words_of([(p[2], p[3]) for p in parts])
            coded = X.entropy_encode_motion_ctu(w, h, c, mask, again, init)[0]
            m2, w2, b2 = X.entropy_decode_motion_ctu(w, h, c, coded, init)
            assert (m2, b2) == (mask, False) and np.array_equal(w2, words)
    assert 0 < n_bad < 2000


def test_helpers_refuse_bad_arguments():
    words = EM.words_of([(0, 0)])
    with pytest.raises(x266_amd.X266Error):
        X.entropy_encode_motion_ctu(64, 64, 0, 2, words)                    # bit 0 is not set
    with pytest.raises(x266_amd.X266Error):
        X.entropy_encode_motion_ctu(64, 64, 1, 1, words)                    # ctu >= n_ctu
    with pytest.raises(x266_amd.X266Error):
        X.entropy_encode_motion_ctu(64, 60, 0, 1, words)
    with pytest.raises(x266_amd.X266Error):
        X.entropy_encode_motion_ctu(64, 64, 0, 1, words, np.full(7, 30, np.uint16))
    with pytest.raises(x266_amd.X266Error):
        X.entropy_decode_motion_ctu(64, 64, 0, b"\0" * 721)


def test_header_constants():
    hdr = header()
    assert int(re.search(r"#define X266_ENTROPY_MOTION_CONTEXTS\s+(\d+)", hdr).group(1)) == EM.CONTEXTS == x266_amd.ENTROPY_MOTION_CONTEXTS
    assert int(re.search(r"#define X266_ENTROPY_MOTION_MAX_BYTES\s+(\d+)", hdr).group(1)) == EM.MAX_BYTES == x266_amd.ENTROPY_MOTION_MAX_BYTES
    assert x266_amd.ENTROPY_MOTION_CTU_DTYPE == EM.CODED_DTYPE and x266_amd.ENTROPY_MOTION_CTU_DTYPE.itemsize == 32
    assert np.array_equal(X.entropy_motion_default_init(), EM.default_init())
    # the derivation of the largest substream, recomputed: 277 context bins under 6.05 bits, 3968 bypass bins under 1.0001
    bits = (21 + 64 * 4) * 6.05 + 64 * 2 * 31 * 1.0001
    assert bits < 5645 and -(-5645 // 8) + 4 == 710 <= EM.MAX_BYTES and EM.MAX_BYTES % 16 == 0
