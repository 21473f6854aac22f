"""GPU (-m gpu): the seeded SATD search (xSatd8x8SeededSearchGpu) against tests/_seeded_ref.py, bit-exact in d_best and d_j.  Every buffer of
every call sits between the guard bands of tests/_arena.py at exactly its documented alignment; the guards and the inputs are checked
after every call, and the stream is synchronised (or the session ended) after every call."""
import ctypes
import functools

import numpy as np
import pytest

import _seeded_ref as R
import x266_amd
from _arena import Arena
from _dev import EINVAL, call_struct, same, sync_or_exit
from _util import Oracle

pytestmark = pytest.mark.gpu

PTRS = {"d_cur": 16, "d_ref": 16, "d_seed": 8, "d_best": 8, "d_j": 4}
DISP = {name: align * (2 * i + 1) for i, (name, align) in enumerate(PTRS.items())}          # exactly the documented alignment, no more
CENTRES = [0, 31, 1, 2, 4, 8, 16]
RANGES = [0, 1, 2, 8]
LAMBDAS = [0, 16, 200, 65535]


@functools.lru_cache(None)
def _oracle():
    return Oracle()


@functools.lru_cache(None)
def frames(kind, w, h, seed=0):
    """(cur plane, ref plane, cur tiles, ref tiles), computed once and shared"""
    cur, ref = R.frame_pair(kind, w, h, seed)
    out = (cur, ref, R.tiles_of(_oracle(), cur, 1), R.tiles_of(_oracle(), ref, 2))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(None)
def seeds_of(kind, w, h, scale, seed=0):
    s = R.seed_vectors(kind, w, h, scale, seed)
    s.setflags(write=False)
    return s


@functools.lru_cache(None)
def want(kind, w, h, seed_kind, scale, centres, r, lam):
    """the reference's (best, j) of a case, computed once and shared"""
    cur, ref, _, _ = frames(kind, w, h)
    best, j, _ = R.search(_oracle(), cur, ref, seeds_of(seed_kind, w, h, scale), scale, centres, r, lam)
    best.setflags(write=False)
    j.setflags(write=False)
    return best, j


def records(seeds, junk_seed=7):
    """x266_me_result_t records of seed vectors; cost is ignored by the call, so it is garbage"""
    rec = np.zeros(len(seeds), R.ME_DTYPE)
    rec["mvx"], rec["mvy"] = seeds[:, 0], seeds[:, 1]
    rec["cost"] = np.random.RandomState(junk_seed).randint(0, 1 << 32, len(seeds), dtype=np.uint64).astype(np.uint32)
    return rec


def seeded(codec, cur_tiles, ref_tiles, w, h, seeds, scale, centres, r, lam, with_j=True, stream=None, guard_seed=51, same_frame=False):
    """the call inside an arena -> (d_best as records, d_j or None)"""
    nb = (w // 8) * (h // 8)
    a = Arena(codec)
    cur = a.input("d_cur", cur_tiles, 16, DISP["d_cur"], guard_seed)
    ref = cur if same_frame else a.input("d_ref", ref_tiles, 16, DISP["d_ref"], guard_seed + 1)
    seed = a.input("d_seed", records(seeds, guard_seed).view(np.uint8), 8, DISP["d_seed"], guard_seed + 2)
    best = a.output("d_best", 8 * nb, 8, DISP["d_best"])
    dj = a.output("d_j", 4 * nb, 4, DISP["d_j"]) if with_j else None
    p = codec.seed_params(w, h, scale, centres, r, lam, d_cur=cur.ptr, d_ref=ref.ptr, d_seed=seed.ptr, d_best=best.ptr, d_j=dj.ptr if with_j else 0)
    call_struct(codec, "xSatd8x8SeededSearchGpu", p, stream)
    got = a.check()                                                         # guard bands, and every input unchanged
    return got["d_best"].view(R.ME_DTYPE), got["d_j"].view(np.uint32) if with_j else None


def check_case(codec, kind, w, h, seed_kind, scale, centres, r, lam, **kw):
    _, _, cur_t, ref_t = frames(kind, w, h)
    best, j = want(kind, w, h, seed_kind, scale, centres, r, lam)
    got, got_j = seeded(codec, cur_t, ref_t, w, h, seeds_of(seed_kind, w, h, scale), scale, centres, r, lam, **kw)
    what = (kind, w, h, seed_kind, scale, centres, r, lam)
    same(got, best, ("d_best",) + what)
    if got_j is not None:
        same(got_j, j, ("d_j",) + what)
    return got, got_j


# ---- 1. the grid: sizes x seed_scale, and along each of centres, r and lambda ------------------------------------------------------------
@pytest.mark.parametrize("scale", [0, 1])
@pytest.mark.parametrize("w,h", R.SIZES)
def test_sizes_scales_centres_ranges_lambdas(codec, w, h, scale):
    if (w, h) == (96, 80):                                                   # the largest size: along each axis; the smaller ones: every combination
        cases = [(c, 1, 16) for c in CENTRES] + [(31, r, 200) for r in RANGES] + [(31, 2, lam) for lam in LAMBDAS] + [(0, 8, 0), (16, 0, 65535)]
    else:
        cases = [(c, r, lam) for c in CENTRES for r in RANGES for lam in LAMBDAS]
    for centres, r, lam in cases:
        check_case(codec, "random", w, h, "small", scale, centres, r, lam)
    check_case(codec, "random", w, h, "small", scale, 31, 2, 16, guard_seed=97)     # whatever lies around the buffers must not reach the result


# ---- 2. contents and seeds --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [0, 1])
@pytest.mark.parametrize("kind", R.FRAMES)
def test_frame_contents(codec, kind, scale):
    w, h = 48, 32
    for r, lam in ((2, 0), (2, 16), (8, 200), (0, 65535)):
        got, j = check_case(codec, kind, w, h, "small", scale, 31, r, lam)
        if kind == "constant":                                               # every SATD ties
            s = seeds_of("small", w, h, scale).astype(np.int64) << scale
            gw = R.grid(w, h, scale)[0]
            cell = np.array([((b // (w // 8)) >> scale) * gw + ((b % (w // 8)) >> scale) for b in range(got.size)])
            off = 0 if lam else r                                           # lambda 0: the first walk entry, own + (-r, -r); else the predictor
            assert np.array_equal(got["mvx"], s[cell, 0] - off) and np.array_equal(got["mvy"], s[cell, 1] - off) and not got["cost"].any()
            assert (j == ((lam * 2) >> 4)).all()


@pytest.mark.parametrize("scale", [0, 1])
@pytest.mark.parametrize("seed_kind", R.SEEDS)
def test_seed_vectors(codec, seed_kind, scale):
    w, h = 48, 32
    for kind, centres, r, lam in (("random", 31, 2, 16), ("random", 0, 0, 0), ("ramps", 31, 1, 200), ("random", 6, 8, 65535)):
        got, _ = check_case(codec, kind, w, h, seed_kind, scale, centres, r, lam)
        assert np.abs(got["mvx"].astype(np.int64)).max() <= 8191 and np.abs(got["mvy"].astype(np.int64)).max() <= 8191
    if seed_kind == "extreme":
        got, _ = check_case(codec, "random", w, h, seed_kind, scale, 0, 0, 0)
        assert set(np.abs(got["mvx"].astype(np.int64)).tolist()) == {8183}


def test_one_frame_as_both_and_without_d_j(codec):
    """d_cur == d_ref is allowed; with d_j NULL d_best holds the same bytes"""
    w, h = 96, 80
    cur, _, cur_t, ref_t = frames("random", w, h)
    for scale in (0, 1):
        s = seeds_of("small", w, h, scale)
        best, j, _ = R.search(_oracle(), cur, cur, s, scale, 31, 2, 16)
        got, got_j = seeded(codec, cur_t, None, w, h, s, scale, 31, 2, 16, same_frame=True)
        same(got, best, "d_best, one frame")
        same(got_j, j, "d_j, one frame")
        with_j, _ = check_case(codec, "random", w, h, "small", scale, 31, 2, 16)
        without, none = seeded(codec, cur_t, ref_t, w, h, s, scale, 31, 2, 16, with_j=False)
        assert none is None and with_j.tobytes() == without.tobytes()


# ---- 3. what follows from the contract, against the calls that are already there ----------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(16, 16), (48, 32), (96, 80)])
def test_a_zero_seed_is_the_exhaustive_search_at_range_8(codec, w, h):
    for kind in ("random", "ramps", "checker"):
        _, _, cur_t, ref_t = frames(kind, w, h)
        nb = (w // 8) * (h // 8)
        got, j = seeded(codec, cur_t, ref_t, w, h, np.zeros((nb, 2), np.int16), 0, 0, 8, 0)
        mv, cost, _ = codec.search_tiles(cur_t, ref_t, w, h, 8)
        sync_or_exit(codec, 0)
        assert np.array_equal(got["mvx"], mv[:, 0]) and np.array_equal(got["mvy"], mv[:, 1]), kind
        assert np.array_equal(got["cost"], cost) and np.array_equal(j, cost), kind


@pytest.mark.parametrize("scale", [0, 1])
def test_range_0_is_the_centre_entry_of_the_refinement(codec, scale):
    w, h = 96, 80
    _, _, cur_t, ref_t = frames("random", w, h)
    gw = R.grid(w, h, scale)[0]
    cell = np.array([((b // (w // 8)) >> scale) * gw + ((b % (w // 8)) >> scale) for b in range((w // 8) * (h // 8))])
    for seed_kind in ("small", "pm64", "far"):
        s = seeds_of(seed_kind, w, h, scale)
        vec = s.astype(np.int64)[cell] << scale
        assert np.abs(vec).max() <= 8183
        got, j = seeded(codec, cur_t, ref_t, w, h, s, scale, 0, 0, 0)
        _, _, costs = codec.refine_qpel_tiles(cur_t, ref_t, w, h, vec.astype(np.int16), want_costs=True)
        sync_or_exit(codec, 0)
        assert np.array_equal(got["mvx"], vec[:, 0]) and np.array_equal(got["mvy"], vec[:, 1])
        assert np.array_equal(got["cost"], costs[:, 24]) and np.array_equal(j, costs[:, 24])


# ---- 4. one graph: the seeded search, then the quarter-sample refinement ---------------------------------------------------------------------------
def test_seeded_search_and_refinement_in_one_graph(codec):
    w, h, scale = 96, 80, 1
    nb = (w // 8) * (h // 8)
    _, _, cur_t, ref_t = frames("random", w, h)
    s = records(seeds_of("small", w, h, scale))
    d_cur, d_ref, d_seed = codec._upload(cur_t.ravel()), codec._upload(ref_t.ravel()), codec._upload(s.view(np.uint8))
    d_best, d_j, d_q = codec.alloc(8 * nb), codec.alloc(4 * nb), codec.alloc(8 * nb)
    p = codec.seed_params(w, h, scale, 31, 2, 16, d_cur=d_cur.ptr, d_ref=d_ref.ptr, d_seed=d_seed.ptr, d_best=d_best.ptr, d_j=d_j.ptr)
    fill = lambda: [b.upload(np.full(n, 0x5A, np.uint8)) for b, n in ((d_best, 8 * nb), (d_j, 4 * nb), (d_q, 8 * nb))]
    grab = lambda: (d_best.download(np.uint8, 8 * nb), d_j.download(np.uint8, 4 * nb), d_q.download(np.uint8, 8 * nb))
    fill()
    codec.satd_seeded_search_dev(p)
    codec.satd_refine_qpel_from_tiles_dev(d_cur.ptr, d_ref.ptr, w, h, d_best.ptr, d_q.ptr)
    sync_or_exit(codec, 0)
    plain = grab()
    best, j = want("random", w, h, "small", scale, 31, 2, 16)
    same(plain[0].view(R.ME_DTYPE), best, "d_best, plain")
    same(plain[1].view(np.uint32), j, "d_j, plain")
    st = codec.stream_create()
    try:
        codec.graph_begin(st)                                                # no xHipMeScratchReserve: neither call uses the scratch
        codec.satd_seeded_search_dev(p, stream=st)
        codec.satd_refine_qpel_from_tiles_dev(d_cur.ptr, d_ref.ptr, w, h, d_best.ptr, d_q.ptr, stream=st)
        graph = codec.graph_end(st)
        try:
            for _ in range(2):
                fill()
                codec.graph_launch(graph, st)
                sync_or_exit(codec, 0, st)
                for a, b, what in zip(grab(), plain, ("d_best", "d_j", "the refined field")):
                    assert a.tobytes() == b.tobytes(), what
        finally:
            codec.graph_free(graph)
    finally:
        codec.stream_destroy(st)


def test_numpy_convenience(codec):
    w, h = 48, 32
    _, _, cur_t, ref_t = frames("random", w, h)
    for scale in (0, 1):
        best, j = want("random", w, h, "small", scale, 31, 2, 16)
        mv, satd, got_j = codec.seeded_search_tiles(cur_t, ref_t, w, h, seeds_of("small", w, h, scale), scale, 31, 2, 16)
        assert np.array_equal(mv[:, 0], best["mvx"]) and np.array_equal(mv[:, 1], best["mvy"]) and np.array_equal(satd, best["cost"]) and np.array_equal(got_j, j)


# ---- 5. refusals through the ABI --------------------------------------------------------------------------------------------------------------
def test_argument_errors(codec):
    """every rule once: X266HIP_EINVAL, the call named in the error text, nothing launched, the buffers untouched"""
    L, ctx = codec.L, codec.ctx
    name = "xSatd8x8SeededSearchGpu"
    M = 1 << 18
    names = list(PTRS)
    buf = codec.alloc((len(names) + 1) * M)
    fill = np.random.RandomState(9).randint(1, 255, (len(names) + 1) * M).astype(np.uint8)
    buf.upload(fill)
    w, h = 96, 80
    n_tiles, nb = 30, 120
    good = {field: buf.ptr + (i + 1) * M for i, field in enumerate(names)}
    good.update(width=w, height=h, seed_scale=1, centres=31, range=2, lambda_q4=16)
    extent = dict(d_cur=n_tiles * 512, d_ref=n_tiles * 512, d_seed=8 * n_tiles, d_best=8 * nb, d_j=4 * nb)

    def refused(**change):
        p = codec.seed_params(**dict(good, **change))
        assert L.xSatd8x8SeededSearchGpu(ctx, ctypes.byref(p), None) == EINVAL, change
        assert name.encode() in L.xHipLastError(ctx), change

    assert L.xSatd8x8SeededSearchGpu(ctx, None, None) == EINVAL and name.encode() in L.xHipLastError(ctx)      # NULL p
    assert L.xSatd8x8SeededSearchGpu(None, ctypes.byref(codec.seed_params(**good)), None) == EINVAL
    for field in ("d_cur", "d_ref", "d_seed", "d_best"):
        refused(**{field: 0})
    for field in names:
        refused(**{field: good[field] + PTRS[field] // 2})
        refused(**{field: 2 ** 64 - PTRS[field]})                            # aligned, and the extent does not fit behind it
    for side in ("width", "height"):
        for v in (0, -16, 8, 24, 104 if side == "width" else 88):
            refused(**{side: v})
    for change in (dict(seed_scale=-1), dict(seed_scale=2), dict(centres=-1), dict(centres=32), dict(range=-1), dict(range=9), dict(lambda_q4=-1),
                   dict(lambda_q4=65536)):
        refused(**change)
    for field in ("d_best", "d_j"):                                          # an output over any other buffer of the call, the seeds included
        for other in names:
            if other != field:
                refused(**{field: good[other] + (extent[other] - 1) // PTRS[field] * PTRS[field]})   # onto the other's last bytes
                refused(**{field: good[other]})
    refused(seed_scale=0, d_best=good["d_seed"] + 8 * nb - 8)                # the seeds' extent follows the scale
    sync_or_exit(codec, 0)
    assert np.array_equal(buf.download(np.uint8, fill.size), fill)          # nothing was launched
    # the edges of what is accepted: d_j NULL, one frame as both, every scalar at either end of its range
    _, _, cur_t, ref_t = frames("random", w, h)
    image = fill.copy()
    image[M:M + n_tiles * 512] = cur_t.ravel()
    image[2 * M:2 * M + n_tiles * 512] = ref_t.ravel()
    for scale, centres, r, lam, one in ((0, 0, 0, 0, False), (1, 31, 8, 65535, False), (1, 31, 2, 16, True)):
        s = seeds_of("small", w, h, scale)
        rec = records(s).view(np.uint8)
        image[3 * M:3 * M + rec.size] = rec
        buf.upload(image)
        p = codec.seed_params(**dict(good, seed_scale=scale, centres=centres, range=r, lambda_q4=lam, d_j=0, d_ref=good["d_cur"] if one else good["d_ref"]))
        rc = L.xSatd8x8SeededSearchGpu(ctx, ctypes.byref(p), None)
        sync_or_exit(codec, rc)
        assert rc == 0, L.xHipLastError(ctx)
        now = buf.download(np.uint8, fill.size)
        cur, ref, _, _ = frames("random", w, h)
        best, _, _ = R.search(_oracle(), cur, cur if one else ref, s, scale, centres, r, lam)
        same(now[4 * M:4 * M + 8 * nb].view(R.ME_DTYPE), best, ("d_best", scale, centres, r, lam, one))
        now[4 * M:4 * M + 8 * nb] = image[4 * M:4 * M + 8 * nb]
        assert np.array_equal(now, image)                                    # ... and nothing else was written, d_j's region included
