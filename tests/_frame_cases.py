"""Seeded case lists for the randomised differential tests of the frame-chain calls (numpy only: no GPU, no torch; the content comes from
the families' own recipes, imported where a function needs them).

cases(family, scale=1) returns a deterministic list of dicts.  A case holds the size, a content kind and a seed, every scalar parameter of
the family's calls, which optional pointers are NULL, and whether a call that may run in place does.  tests/test_frame_cases.py runs the
lists through the reference statements alone (coverage conditions, shape classes); tests/test_gpu_fuzz_frames.py runs the same lists on
the device.  The shape classes of a list come first and are there by construction (U = the family's unit: 16, 32 for the lookahead, 64
for the calls that take whole CTUs):

  one unit; one unit wide and six high; six wide and one high; cut CTUs (sides = 16, 32, 48 mod 64, in width, in height, and in both)
  where any multiple of 16 is a size; for every kernel of the family that shares a workgroup between units, every residue of the unit
  count modulo the units of a workgroup, in frames of at least three workgroups (GEOMETRY names the kernels and restates their launch
  arithmetic); a row longer than 64 units (U = 64: longer than 4 CTUs); for the kernels that give a thread to a block or tile, counts
  just below, at and just above 256 in frames at least ten units wide.

The rest of a list is random: sides up to 24 x 16 tiles, everything else drawn jointly from a RandomState seeded by (family, index), the
documented ends of a range a quarter of the time each.  The region calls of "quant", "levels" and "rdoq" take 6 n_ctu - drop regions,
drop in 0..5 being part of the case.  "rdoq" and "tdecide" draw their random frames within 12 x 8 tiles (their statements walk every block
of every region in python); "rdoq" has content whose 64-bit sums pass 2^32 (rdoq_content), and the statement of "tdecide" runs on the
regions of tdecide_sample.  The two refinements, whose statement forms 49 whole-frame predictions, run on a stated subset of the
shapes (_refines: every shape class but the larger cut-both and residue frames, and every second random frame).  X266_FUZZ_SCALE=k lengthens every list k-fold by continuing the index; nothing else depends on the environment."""
import functools
import os
import zlib

import numpy as np

SCALE = int(os.environ.get("X266_FUZZ_SCALE", "1"))


def ctu_count(w, h):
    return ((w + 63) // 64) * ((h + 63) // 64)


def tiles(w, h):
    return (w // 16) * (h // 16)


def waves(count, per_wave):
    """a kernel whose wave takes `per_wave` units: what a workgroup's waves are counted in"""
    return lambda w, h: -(-count(w, h) // per_wave)


def deblock_units(w, h):
    return ((w + 4 + 63) // 64) * ((h + 4 + 63) // 64)


def la_low_tiles(w, h):
    return (w // 32) * (h // 32)


def regions(w, h, drop=0):
    return 6 * ctu_count(w, h) - drop


def count_of(count, case):
    """a kernel's unit count for a case"""
    return count(case["w"], case["h"], case["drop"]) if "drop" in case else count(case["w"], case["h"])


# per family: the unit of its sizes, whether any multiple of 16 is a size (cut CTUs), the kernels that share a workgroup between units as
# (name, count of what a workgroup is shared between, how many of them a workgroup takes), the count a thread-per-unit kernel walks (or
# None), and the number of random cases behind the mandatory ones.  Next to each: the length of the default list and the time the family's
# statements take for it on a CPU (tests/test_frame_cases.py); a residue that an earlier shape of the list already has adds no case.  The
# two refining families are over the 3 s the others keep to: their lists are no longer than the shape classes of the refinements need.
GEOMETRY = {
    # deblock_chroma_kernel: u = blockIdx.x * 4 + wave, one 64x64 unit (shifted by 4 samples) per wave
    "deblock": dict(long=(1104, 32), unit=16, cut=True, kernels=[("deblock_chroma_kernel", deblock_units, 4)], threads=None, random=6),        # 23 cases, 0.2 s
    # sao_decide_kernel: ctu = blockIdx.x * 4 + wave
    "sao": dict(long=(1104, 32), unit=16, cut=True, kernels=[("sao_decide_kernel", ctu_count, 4)], threads=None, random=6),                    # 23 cases, 0.3 s
    # alf_decide_kernel: ctu = blockIdx.x * 4 + wave
    "alf": dict(long=(1104, 32), unit=16, cut=True, kernels=[("alf_decide_kernel", ctu_count, 4)], threads=None, random=4),                    # 21 cases, 2.2 s
    # aq_stats_kernel: a wave takes four tiles, kAqWavesPerWg = 4; aq_decide_kernel: 16 threads per CTU, one per tile, 256 per workgroup
    "aq": dict(long=(1104, 16), unit=16, cut=True, kernels=[("aq_stats_kernel", waves(tiles, 4), 4), ("aq_decide_kernel", waves(ctu_count, 4), 4)],
               threads=tiles, random=6),                                                                                      # 29 cases, 0.1 s
    # la_downscale_kernel: a wave takes four lowres tiles; la_intra_costs_kernel: a wave takes eight blocks; la_tree_qp_kernel: 16 threads per
    # CTU; kLaWavesPerWg = 4 for the three.  la_frame_cost_kernel, la_propagate_kernel: b = blockIdx.x * 256 + threadIdx.x
    "la": dict(long=(1120, 32), unit=32, cut=False, kernels=[("la_downscale_kernel", waves(la_low_tiles, 4), 4), ("la_intra_costs_kernel", waves(tiles, 8), 4),
                                            ("la_tree_qp_kernel", waves(ctu_count, 4), 4)], threads=tiles, random=4),        # 23 cases, 0.7 s
    # quant_regions_kernel: r = blockIdx.x * kQuantWavesPerWg + wave, over the first 6 n_ctu - drop regions of the frame (drop in 0..5 is part
    # of the case: the fused coding call always has 6 n_ctu regions, the region call takes any count)
    "quant": dict(long=(320, 128), unit=64, cut=False, drop=True, salt=3, kernels=[("quant_regions_kernel", regions, 4)], threads=None, random=5),     # 13 cases, 0.2 s
    # levels_pack_kernel, levels_unpack_kernel: r = blockIdx.x * kLevelsWavesPerWg + wave, over 6 n_ctu - drop regions
    "levels": dict(long=(320, 64), unit=64, cut=False, drop=True, salt=5, kernels=[("levels_pack_kernel", regions, 4)], threads=None, random=5),      # 13 cases, 0.1 s
    # intra32_refs_from_tiles_kernel: set = blockIdx.x * 4 + wave; 4 n_ctu luma sets, n_ctu sets of a chroma component
    "intra_frame": dict(long=(320, 128), unit=64, cut=False, kernels=[("intra32_refs_from_tiles_kernel", ctu_count, 4)], threads=None, random=4),   # 12 cases, 0.3 s
    # mixed_inter_regions_kernel: wave_grid(5 n_ctu, 4): luma regions and the chroma pair of every CTU, one per wave
    "mixed": dict(long=(320, 128), unit=64, cut=False, kernels=[("mixed_inter_regions_kernel", lambda w, h: 5 * ctu_count(w, h), 4)], threads=None, random=4),   # 11 cases, 0.3 s
    # mc_luma_kernel: tile = blockIdx.x * 4 + wave; mc_chroma_kernel: blockIdx.x * 8 + half wave; mc_kernel (both planes): blockIdx.x * 2 + wave.
    # satd_refine_qpel_kernel takes kRefineWavesPerWg = 4 blocks of 8x8 per workgroup, and a frame has a multiple of four of them
    "qpel": dict(long=(1104, 16), refines=True, unit=16, cut=True, kernels=[("mc_chroma_kernel", tiles, 8), ("mc_luma_kernel", tiles, 4), ("mc_kernel", tiles, 2)], threads=None, random=6),   # 24 cases, 3.4 s
    # mc_bi_luma_kernel, mc_bi_chroma_kernel, mc_bi_kernel: as the three above; satd_bi_costs_kernel: wave_grid(n_tiles, 4)
    "bipred": dict(long=(1104, 16), refines=True, unit=16, cut=True, kernels=[("mc_bi_chroma_kernel", tiles, 8), ("mc_bi_luma_kernel", tiles, 4), ("mc_bi_kernel", tiles, 2),
                                               ("satd_bi_costs_kernel", tiles, 4)], threads=None, random=6),                                  # 24 cases, 3.8 s
    # seeded_search_kernel: cell = blockIdx.x * kSeedWavesPerWg + wave, a cell being a 16x16 tile
    "seeded": dict(long=(1104, 16), salt=2, unit=16, cut=True, kernels=[("seeded_search_kernel", tiles, 4)], threads=None, random=5),                 # 20 cases, 0.4 s
    # rdoq_regions_kernel, levels_bits_kernel: r = blockIdx.x * kRdoqWavesPerWg + wave, over 6 n_ctu - drop regions.  `within`: the random
    # frames are drawn within 12 x 8 tiles (at most 36 regions), eighteen of them: three of every content kind
    "rdoq": dict(long=(320, 64), unit=64, cut=False, drop=True, salt=2, within=(12, 8), kernels=[("rdoq_regions_kernel", regions, 4)], threads=None, random=18),   # 26 cases, 1.3 s
    # tdecide_kernel: r = blockIdx.x * kRdoqWavesPerWg + wave over the 6 n_ctu regions of the frame: the count is even, so of the four
    # residues only 0 and 2 exist (`residues`; _smallest would raise on 1 and 3).  The long row is 16 whole CTUs and one cut in width.
    # No J of this call reaches 2^32: J = dist + lambda (bits + side cost).  Where levels are kept dist is a few 2^22 a region; the rate
    # grows with the logarithm of a level and the residual's energy is bounded, so the dearest region is a residual of +-255 at every
    # sample at qp 0: 405 000 sixteenths of a bit in the statement, and J <= 8192 (405 000 + 65535) = 2^31.85.  The list must reach
    # 2^31, the upper half of the low dword, instead (tests/test_frame_cases.py)
    "tdecide": dict(long=(1040, 64), unit=16, cut=True, salt=0, within=(12, 8), kernels=[("tdecide_kernel", lambda w, h: 6 * ctu_count(w, h), 4)], residues=(0, 2),
                    threads=None, random=5),                                                                                  # 19 cases, 3.1 s
}
FAMILIES = tuple(GEOMETRY)
THREADS_PER_WG = 256
LONG_ROW = 1104                                                             # 69 tiles, 18 CTUs


# ---- the mandatory shapes ---------------------------------------------------------------------------------------------------------------
def _smallest(count, modulus, residue, unit, drops=(None,)):
    """the smallest frame (by samples, then by width) at least three units each way -- or two, or one, where no such frame exists -- with
    count = residue mod modulus and more than two workgroups' worth of units: the last workgroup is ragged in a frame that has inner
    units too.  -> (w, h) or (w, h, drop)"""
    for least in (3, 2, 1):
        best = None
        for w in range(least * unit, 1216 + 1, unit):
            for h in range(least * unit, 512 + 1, unit):
                for drop in drops:
                    c = count(w, h) if drop is None else count(w, h, drop)
                    if c % modulus == residue and c > 2 * modulus and (best is None or (w * h, w) < (best[0] * best[1], best[0])):
                        best = (w, h) if drop is None else (w, h, drop)
        if best is not None:
            return best
    raise AssertionError((modulus, residue))


def _around_a_workgroup(count, unit):
    """three frames at least ten units wide whose counts are the largest below, exactly, and the smallest above THREADS_PER_WG"""
    found = {}
    for w in range(10 * unit, 40 * unit + 1, unit):
        for h in range(unit, 40 * unit + 1, unit):
            c = count(w, h)
            key = "below" if c < THREADS_PER_WG else "at" if c == THREADS_PER_WG else "above"
            d = abs(c - THREADS_PER_WG)
            if key not in found or (d, abs(w - h)) < found[key][0]:
                found[key] = ((d, abs(w - h)), (w, h))
    return [found[k][1] for k in ("below", "at", "above")]


def mandatory_shapes(family):
    """[(class name, w, h)] or, in a family whose region call takes a count of its own, [(class name, w, h, drop)] for some"""
    g = GEOMETRY[family]
    u = g["unit"]
    out = [("one unit", u, u), ("one unit wide", u, 6 * u), ("one unit high", 6 * u, u)]
    if g["cut"]:
        for r in (16, 32, 48):
            out += [("cut width %d" % r, 64 + r, 64), ("cut height %d" % r, 64, 64 + r), ("cut both %d" % r, 64 + r, 128 - r if r != 32 else 96)]
    elif u == 32:
        out += [("cut width 32", 96, 64), ("cut height 32", 64, 96), ("cut both 32", 96, 96)]
    if g.get("refines"):
        out.append(("cut both 16, refined", 80, 80))
    for name, count, modulus in g["kernels"]:
        for r in g.get("residues", range(modulus)):
            if not g.get("drop") and any(count(*x[1:]) % modulus == r and count(*x[1:]) > 2 * modulus for x in out):
                continue                                                    # a shape of the list has it already
            out.append(("%s residue %d" % (name, r),) + _smallest(count, modulus, r, u, range(6) if g.get("drop") else (None,)))
    out.append(("long row",) + g["long"])
    if g["threads"]:
        out += [("workgroup %s" % k, w, h) for k, (w, h) in zip(("below", "at", "above"), _around_a_workgroup(g["threads"], u))]
    return out


# ---- draws --------------------------------------------------------------------------------------------------------------------------------
def _rng(family, index):
    """the draws of case `index`; a family's salt is the first value with which its default list meets tests/test_frame_cases.py"""
    return np.random.RandomState((zlib.crc32(family.encode()) + 7919 * index + 104729 * GEOMETRY[family].get("salt", 0)) & 0xFFFFFFFF)


def _ends(r, lo, hi):
    """lo..hi with both ends a quarter of the time each"""
    k = r.randint(0, 4)
    return int(lo if k == 0 else hi if k == 1 else r.randint(lo, hi + 1))


def _pick(r, seq):
    return seq[r.randint(0, len(seq))]


def _subset(r, names, p=0.25):
    return tuple(n for n in names if r.random_sample() < p)


DEBLOCK_KINDS = ("blocks", "smooth", "steps", "extreme", "constant", "profile", "noise", "ends")
SAO_KINDS = ("sharp0", "sharp1", "sharp2", "sharp3", "band", "noise", "far", "same", "uniform", "ends")
ALF_KINDS = ("stripes", "quad", "blur", "noise", "same", "far", "spikes")           # "noise" is uniform, "far" is {0, 255}
AQ_KINDS = ("zeros", "ones", "max", "noise", "halves", "distinct", "ends")
LA_KINDS = ("zeros", "ones", "random", "hramp", "vramp", "checker", "smooth")       # "random" is uniform, "checker" is {0, 255}


QPEL_KINDS = ("random", "extreme")                                                    # uniform noise and {0, 255}
WEIGHT_NAMES = (None, "fade", "denominator 0", "field extremes")                      # None: the default weights; else _bipred_ref.WEIGHTS
SEEDED_FRAMES = ("random", "constant", "ramps", "checker")                            # "random" is uniform, "checker" is {0, 255}
SEEDED_SEEDS = ("small", "pm64", "far", "pm8191", "extreme", "duplicates")
# the refinements' statement forms 49 whole-frame predictions, so they run on the frames of at most 5120 samples, on 96x64, 112x64 and 80x80
# and on the long row: one unit, the one-unit strips, every cut width, a cut height, a frame cut both ways, the long row, and every second
# random frame, which is drawn within 6 x 4 tiles.  The other calls of the family run on every case
def _refines(w, h):
    return w * h <= 5120 or (w, h) in ((96, 64), (112, 64), (80, 80), (LONG_ROW, 16))


QUANT_KINDS = ("mix", "near", "noise", "ends")
LEVELS_KINDS = ("mixed", "dense", "sparse", "one_hot", "zeros")
INTRA_KINDS = ("oriented", "noise", "flat", "extreme")                                # "noise" is uniform, "extreme" is {0, 255} patches
# case 0 of "mixed" (64x64, "oriented", every region deciding, qp 22): inter cost - intra cost of the first region, so that it ties -- and a
# tie is inter.  Worked out with the statement; tests/test_frame_cases.py asserts that the tie is there.
MIXED_TIE_PENALTY = 28768


RDOQ_KINDS = ("laplacian", "heavy_head", "heavy_cg", "fullrange", "ends", "zeros")
RDOQ_WIDE_KINDS = ("heavy_head", "heavy_cg")                                          # every block (of N >= 8 for "heavy_cg") has a sum of D(0) of 2^32 and more
RDOQ_LAMBDAS = (0, 0, 1, 368, 8191, 8192)
TDECIDE_KINDS = ("five", "noise", "ends_flat", "ends_ends")                           # _tdecide_ref's five residuals, uniform, {0, 255} against 128 and against {0, 255}
TDECIDE_BITS = ("zero", "equal", "random", "cheap")
TDECIDE_CLASSES = 0x777F


@functools.lru_cache(None)
def wide_qp(n, magnitude):
    """the largest qp at which one coefficient of `magnitude` in a block of 1 << n has D(0) >= 2^32 (D(0) falls as qp grows: f falls
    within six steps and halves against 2^qbits over them), from the statement's own D; -1 where there is none"""
    from _quant_ref import F as f_of, qbits
    from _rdoq_ref import dist
    wide = [int(dist(np.int64(magnitude) * f_of[qp % 6], 0, int(qbits(n, qp)))) >= 1 << 32 for qp in range(52)]
    assert wide == sorted(wide, reverse=True)
    return sum(wide) - 1


def _mask(r):
    """a non-empty subset of the 13 classes: all of them, a single one, or each with probability 1/2"""
    valid = [k for k in range(16) if (TDECIDE_CLASSES >> k) & 1]
    how = r.randint(0, 4)
    m = TDECIDE_CLASSES if how == 0 else 0 if how == 1 else sum(1 << k for k in valid if r.randint(0, 2))
    return int(m if m else 1 << _pick(r, valid))


def _draw(family, r, index, w, h):
    """everything of a case but its size"""
    if family == "rdoq":
        kind = RDOQ_KINDS[index % len(RDOQ_KINDS)]
        lo = _pick(r, (12000, 20000, 28000))                                # the magnitudes of the wide kinds
        mag = (lo, _pick(r, (lo + 4000, 32767)))
        top = wide_qp(2, lo) if kind in RDOQ_WIDE_KINDS else 51             # the scalar qp serves every class: a 4x4 block has the lowest bound
        return dict(kind=kind, qp=_ends(r, 0, top), lam=_pick(r, RDOQ_LAMBDAS + (int(r.randint(0, 8193)),)), heads=int(r.randint(1, 5)), mag=mag,
                    null=_subset(r, ("d_class", "d_qp", "d_nnz", "d_stat"), 0.3), inplace=bool(r.randint(0, 2)))
    if family == "tdecide":
        return dict(kind=TDECIDE_KINDS[index % len(TDECIDE_KINDS)], qp=_ends(r, 0, 51), lam=_pick(r, RDOQ_LAMBDAS + (int(r.randint(0, 8193)),)),
                    cand_luma=_mask(r), cand_chroma=_mask(r), bits=TDECIDE_BITS[(index // 2) % len(TDECIDE_BITS)],
                    null=_subset(r, ("d_qp", "d_cand", "d_nnz", "d_stat", "d_cost"), 0.35), inplace=False, same_frame=bool(r.randint(0, 6) == 0))
    if family == "deblock":
        from _deblock_ref import OFFSETS
        kind = DEBLOCK_KINDS[index % len(DEBLOCK_KINDS)]
        bo, to = _ends(r, -6, 6), _ends(r, -6, 6)
        if kind in OFFSETS and r.randint(0, 2):                             # the pair the recipe's content was built for (the +-2 tc clamp needs it)
            bo, to = OFFSETS[kind]
        return dict(kind=kind, qp=_ends(r, 0, 51), beta_offset_div2=bo, tc_offset_div2=to,
                    null=_subset(r, ("cls", "intra", "nnz", "qps", "mv")), inplace=bool(r.randint(0, 2)))
    if family == "sao":
        return dict(kind=SAO_KINDS[index % len(SAO_KINDS)], lam=_pick(r, (0, 0, 4, 37, 400, 65535, int(r.randint(0, 65536)))),
                    null=_subset(r, ("d_stats",), 0.5), inplace=False)
    if family == "alf":
        return dict(kind=ALF_KINDS[index % len(ALF_KINDS)], n_luma=_ends(r, 0, 8) if ctu_count(w, h) <= 12 else int(r.randint(0, 3)), n_chroma=_ends(r, 0, 8),
                    lam=_pick(r, (0, 0, 37, 400, 65535, int(r.randint(0, 65536)))), null=_subset(r, ("d_class", "d_mask"), 0.5), inplace=False)
    if family == "aq":
        return dict(kind=AQ_KINDS[index % len(AQ_KINDS)], mode=int(r.randint(1, 3)), strength_q8=_ends(r, 0, 1024), qp=_ends(r, 0, 51),
                    chroma_qp_offset=_ends(r, -12, 12), null=_pick(r, ((), (), ("d_offset",), ("d_qp",))), inplace=False)
    if family == "la":
        return dict(kind=LA_KINDS[index % len(LA_KINDS)], intra_penalty=_pick(r, (0, 300, 300, 65535, int(r.randint(0, 65536)))),
                    strength_q8=_ends(r, 0, 1024), qp=_ends(r, 0, 51), chroma_qp_offset=_ends(r, -12, 12),
                    null=_subset(r, ("d_mode", "d_inter0", "d_inter1", "d_prop", "d_prop_ref0", "d_prop_ref1", "d_aq_offset", "d_offset", "d_qp")),
                    inplace=False)
    if family == "quant":
        return dict(kind=QUANT_KINDS[index % len(QUANT_KINDS)], qp=_ends(r, 0, 51), rounding=_ends(r, 0, 511),
                    null=_subset(r, ("d_class", "d_qp", "d_nnz"), 0.4), inplace=bool(r.randint(0, 2)))
    if family == "levels":
        return dict(kind=LEVELS_KINDS[index % len(LEVELS_KINDS)], cap_q8=_pick(r, (None, None, 1, 100, 200, 255)), count_only=bool(r.randint(0, 2)),
                    null=_subset(r, ("d_class", "d_nnz", "d_nnz of unpack"), 0.4), inplace=False)
    if family == "intra_frame":
        return dict(kind=INTRA_KINDS[index % len(INTRA_KINDS)], qp=_ends(r, 0, 51), rounding=_ends(r, 0, 511),
                    null=_subset(r, ("d_qp", "d_nnz", "d_mode_in"), 0.5), inplace=bool(r.randint(0, 2)))
    if family == "mixed":
        penalty = MIXED_TIE_PENALTY if index == 0 else _pick(r, (0, 0, 64, 4096, 1 << 24, int(r.randint(0, (1 << 24) + 1))))
        return dict(kind=INTRA_KINDS[index % len(INTRA_KINDS)], flip=int(r.randint(0, 2)), qp=22 if index == 0 else _ends(r, 0, 51),
                    rounding=_ends(r, 0, 511), intra_penalty=penalty,
                    null=("d_qp", "d_kind_in", "d_mode_in") if index == 0 else _subset(r, ("d_qp", "d_kind_in", "d_mode_in", "d_nnz", "d_cost"), 0.4),
                    inplace=bool(r.randint(0, 2)))
    if family == "qpel":
        return dict(kind=QPEL_KINDS[index % 2], source="planted" if w == LONG_ROW else ("planted", "mix", "search")[(index // 2) % 3], refine=_refines(w, h), null=_subset(r, ("d_costs",), 0.5),
                    inplace=bool(r.randint(0, 2)))
    if family == "bipred":
        return dict(kind=QPEL_KINDS[index % 2], weights=WEIGHT_NAMES[index % len(WEIGHT_NAMES)], bi_penalty=_pick(r, (0, 0, 9, 40, 65535, int(r.randint(0, 65536)))),
                    list=int(r.randint(0, 2)), refine=_refines(w, h),
                    null=_subset(r, ("d_dir", "d_costs"), 0.4) + _pick(r, ((), (), ("d_costs of the cost call",), ("d_dir of the cost call",))),
                    inplace=bool(r.randint(0, 2)))
    if family == "seeded":
        nb = (w // 8) * (h // 8)
        return dict(kind=SEEDED_FRAMES[index % len(SEEDED_FRAMES)], seed_kind=SEEDED_SEEDS[index % len(SEEDED_SEEDS)], seed_scale=int(r.randint(0, 2)),
                    centres=_ends(r, 0, 31), range=_ends(r, 0, 8 if nb <= 48 else 4 if nb <= 160 else 2 if nb <= 600 else 1),     # (2 r + 1)^2 candidates per centre and block
                    lam=_pick(r, (0, 16, 200, 65535, int(r.randint(0, 65536)))), null=_subset(r, ("d_j",), 0.4), inplace=False)
    raise KeyError(family)


def cases(family, scale=None):
    g = GEOMETRY[family]
    shapes = mandatory_shapes(family)
    total = (len(shapes) + g["random"]) * (SCALE if scale is None else scale)
    out = []
    for index in range(total):
        r = _rng(family, index)
        drop = None
        if index < len(shapes):
            cls, w, h = shapes[index][:3]
            drop = shapes[index][3] if len(shapes[index]) > 3 else None
        else:
            cls, w, h = "random", g["unit"] * int(r.randint(1, 384 // g["unit"] + 1)), g["unit"] * int(r.randint(1, 256 // g["unit"] + 1))
            if g.get("refines") and (index - len(shapes)) % 2 == 0:          # within 6 x 4 tiles: a random frame that the refinements run on too
                w, h = 16 * (1 + (w // 16 - 1) % 6), 16 * (1 + (h // 16 - 1) % 4)
            if g.get("within"):
                w, h = 16 * (1 + (w // 16 - 1) % g["within"][0]), 16 * (1 + (h // 16 - 1) % g["within"][1])
        case = dict(family=family, index=index, shape=cls, w=w, h=h, seed=int(r.randint(1, 1 << 30)))
        if g.get("drop"):
            case["drop"] = int(r.randint(0, 6)) if drop is None else drop
        case.update(_draw(family, r, index, w, h))
        if "d_offset" in case["null"] and "d_qp" in case["null"]:           # the header wants one of the two outputs
            case["null"] = tuple(n for n in case["null"] if n != "d_qp")
        out.append(case)
    return out


def tag(case):
    return "%s[%d] %s %dx%d %s" % (case["family"], case["index"], case["shape"], case["w"], case["h"], {k: v for k, v in case.items() if k not in ("family", "index", "shape", "w", "h")})


# ---- content: the families' own recipes, called with the drawn size and seed --------------------------------------------------------------
def _uniform(pw, ph, seed):
    from _util import splitmix64
    return (splitmix64(seed, 0, pw * ph) & np.uint64(255)).astype(np.uint8).reshape(ph, pw)


def _ends_plane(pw, ph, seed):
    from _util import splitmix64
    return (((splitmix64(seed, 0, pw * ph) >> np.uint64(17)) & np.uint64(1)) * np.uint64(255)).astype(np.uint8).reshape(ph, pw)


def _three(fn, w, h, seed):
    return fn(w, h, seed), fn(w // 2, h // 2, seed + 1), fn(w // 2, h // 2, seed + 2)


def deblock_content(case):
    """(y, u, v, side): the recipe's planes and side mix at the drawn seed, the drawn scalars and NULL arrays over them"""
    import _deblock_ref as D
    kind, w, h, seed = case["kind"], case["w"], case["h"], case["seed"]
    if kind in D.KINDS:
        y, u, v = D.planes(kind, w, h, seed)
        side = D.side_mix(kind, w, h, seed + 7)
    else:
        y, u, v = _three(_uniform if kind == "noise" else _ends_plane, w, h, seed)
        side = D.side_mix("blocks" if kind == "noise" else "extreme", w, h, seed + 7)
    changes = {n: None for n in case["null"]}
    changes.update(qp=case["qp"], beta_offset_div2=case["beta_offset_div2"], tc_offset_div2=case["tc_offset_div2"])
    return y, u, v, side.replace(**changes)


def sao_content(case):
    """(org planes, dec planes).  The recipe's kinds are keyed by kind and size (_sao_ref.case takes no seed): two cases of one kind and size
    have the same planes, and the case's seed reaches only the uniform and {0, 255} kinds, m_I and the pre-fills"""
    import _sao_ref as S
    kind, w, h, seed = case["kind"], case["w"], case["h"], case["seed"]
    if kind in S.KINDS:
        return S.case(kind, w, h)
    fn = _uniform if kind == "uniform" else _ends_plane
    return _three(fn, w, h, seed), _three(fn, w, h, seed + 10)


def alf_content(case):
    """(org planes, dec planes).  _alf_ref.case is keyed by kind and size and takes no seed: the case's seed reaches the class map, the
    filters, the control bytes, the mask, m_I and the pre-fills, not these planes"""
    import _alf_ref as A
    return A.case(case["kind"], case["w"], case["h"])


def aq_content(case):
    """the tile array [n, 512]"""
    import _aq_ref as Q
    kind, w, h, seed = case["kind"], case["w"], case["h"], case["seed"]
    if kind == "zeros":
        return Q.constant_frame(w, h, 0)
    if kind == "ones":
        return Q.constant_frame(w, h, 255)
    if kind == "max":
        return Q.max_energy_frame(w, h)
    if kind == "noise":
        return Q.noise_frame(w, h, seed)
    if kind == "halves":
        return Q.halves_frame(w, h, seed)
    if kind == "distinct":
        return Q.distinct_frame(w, h)
    return Q.tiles_from_planes(*_three(_ends_plane, w, h, seed), seed=seed % 1000)


def la_content(case):
    """the tile array [n, 512]"""
    import _la_ref as L
    return L.frame(case["kind"], case["w"], case["h"], case["seed"] % 100000)


# ---- the side inputs of a case, shared by the CPU conditions and the device tests ----------------------------------------------------------
def alf_class_map(case):
    """a caller's class map: bytes over the whole range, so classes 25..31 (read as 24), every transposition and the unused top bit occur"""
    return _uniform(case["w"] // 4, case["h"] // 4, case["seed"] + 21)


def alf_sets(case, st):
    """(packed luma sets, packed chroma alternatives, d_ctrl [n_ctu, 3], mask or None): random int8 filters with every clip index, the
    first set solved from the statistics `st` so that the decision has something to choose; control bytes of every kind"""
    import _alf_ref as A
    n = ctu_count(case["w"], case["h"])
    r = np.random.RandomState(case["seed"] + 5)
    luma, chroma = A.random_filters(max(case["n_luma"], 1), max(case["n_chroma"], 1), case["seed"] % 100000 + 5)
    lc, uc, vc = A.solve(A.sum_stats(st))
    solved_l, solved_c = A.pack(lc[None], None, np.stack([uc, vc]), None)
    luma[0] = solved_l[0]
    chroma[:2] = solved_c[:chroma.shape[0]][:2]
    luma, chroma = luma[:case["n_luma"]], chroma[:case["n_chroma"]]
    ctrl = np.zeros((n, 3), np.uint8)
    for m, count in enumerate((case["n_luma"], case["n_chroma"], case["n_chroma"])):
        how = r.randint(0, 4, n)
        valid = r.randint(1, count + 1, n) if count else np.zeros(n, np.int64)
        ctrl[:, m] = np.select([how == 0, how == 1, how == 2], [0, valid, r.randint(count + 1, 255, n)], 255)
    mask = None if "d_mask" in case["null"] else (r.randint(0, 2, n) * r.randint(1, 256, n)).astype(np.uint8)
    return luma, chroma, ctrl, mask


def la_side(case, cost):
    """(list 0, list 1, d_prop, d_aq_offset) around the intra costs, each None where the case has a NULL pointer; the lists are the
    fixed tests' recipe (ties of every kind), d_prop has values at and above 2^32"""
    from _la_ref import lists
    r = np.random.RandomState(case["seed"] + 9)
    l0, l1 = lists(cost, case["seed"] % 100000)
    prop = r.randint(0, 1 << 20, cost.size).astype(np.uint64)
    prop[::11] = np.array([2 ** 32 - 1, 2 ** 32, 2 ** 63, 2 ** 64 - 1], np.uint64)[np.arange(prop[::11].size) % 4]
    aq = r.randint(-3072, 3073, cost.size).astype(np.int16)
    null = case["null"]
    return (None if "d_inter0" in null else l0, None if "d_inter1" in null else l1, None if "d_prop" in null else prop,
            None if "d_aq_offset" in null else aq)


def la_accumulators(case, n):
    """the two accumulators as they stand before xLaPropagateGpu (None: a NULL target), one of them high enough to carry past 2^63"""
    r = np.random.RandomState(case["seed"] + 10)
    a0, a1 = r.randint(0, 1 << 30, n).astype(np.uint64), np.full(n, 2 ** 63 - 5, np.uint64) + r.randint(0, 10, n).astype(np.uint64)
    return None if "d_prop_ref0" in case["null"] else a0, None if "d_prop_ref1" in case["null"] else a1


# ---- the 64-granular families -----------------------------------------------------------------------------------------------------------------
def quant_content(case):
    """(coefficients [n, 1024] for the forward call, levels [n, 1024] for the inverse call, class bytes, qp bytes) of the region call, n = 6
    n_ctu - drop; the class and qp bytes carry garbage above the bits that count (qp bytes above 51 are clamped)"""
    from _quant_ref import _bytes, _coefficients, _levels
    n, seed = regions(case["w"], case["h"], case["drop"]), case["seed"]
    return _coefficients(n, seed), _levels(n, seed + 1), _bytes(n, seed + 2, 15), _bytes(n, seed + 3, 63)


def quant_frames(case):
    """(cur, pred, pre-fill of d_recon) tile arrays of the fused coding call and its qp bytes [6 n_ctu]"""
    from _util import splitmix64
    from _quant_ref import _bytes, _tiles_mix
    w, h, seed, kind = case["w"], case["h"], case["seed"], case["kind"]
    cur, pred, base = _tiles_mix(w, h, seed + 4), _tiles_mix(w, h, seed + 5), _tiles_mix(w, h, seed + 6)
    if kind == "noise":
        cur, pred = _uniform(w * 2, h, seed + 4).ravel(), _uniform(w * 2, h, seed + 5).ravel()
    elif kind == "ends":
        cur, pred = _ends_plane(w * 2, h, seed + 4).ravel(), _ends_plane(w * 2, h, seed + 5).ravel()
    elif kind == "near":                                                    # pred = cur +- 2 in half of the CTUs: regions without a level at a high qp
        c = cur.reshape(-1, 512).copy()
        c[:, :384] = 2 + (c[:, :384].astype(np.int32) * 251 // 255).astype(np.uint8)
        step = (splitmix64(seed + 7, 0, c[:, :384].size) % np.uint64(5)).astype(np.int16).reshape(-1, 384) - 2
        near = c.copy()
        near[:, :384] = (c[:, :384].astype(np.int16) + step).astype(np.uint8)
        tx = np.arange(c.shape[0]) % (w // 16)
        p = pred.reshape(-1, 512).copy()
        p[(tx // 4) % 2 == 0] = near[(tx // 4) % 2 == 0]
        cur, pred = c.ravel(), p.ravel()
    return cur, pred, base, _bytes(6 * ctu_count(w, h), seed + 8, 63)


def levels_content(case):
    """(levels [n, 1024] int16, class bytes [n]) from the family's generators, n = 6 n_ctu - drop"""
    import _levels_ref as V
    n, seed, kind = regions(case["w"], case["h"], case["drop"]), case["seed"] % 100000, case["kind"]
    if kind == "mixed":
        return V.mixed(n, seed)
    if kind == "dense":
        return V.dense(n, seed), np.random.RandomState(seed).randint(0, 256, n).astype(np.uint8)
    if kind == "zeros":
        return np.zeros((n, 1024), np.int16), np.arange(n, dtype=np.uint8)
    lv, cls = V.sparse(seed) if kind == "sparse" else V.one_hot(seed % 4)
    rows = (np.arange(n) * (1 if kind == "sparse" else 37) + seed) % lv.shape[0]
    return lv[rows], cls[rows]


def frame_side(case):
    """(qp bytes [6 n_ctu] up to 69: clamped at 51, modes [n_ctu, 6] in 0..34, kinds [n_ctu, 6]) of the two frame coding calls"""
    import _mixed_frame_ref as M
    from _util import splitmix64
    n, seed = ctu_count(case["w"], case["h"]), case["seed"]
    qps = (splitmix64(seed + 1, 0, 6 * n) % np.uint64(70)).astype(np.uint8)
    modes = (splitmix64(seed + 2, 0, 6 * n) % np.uint64(35)).astype(np.uint8).reshape(n, 6)
    return qps, modes, M.kinds_mixed(n, seed % 100000 + 3)


# ---- the inter families -----------------------------------------------------------------------------------------------------------------------
def qpel_content(case, oracle):
    """(reference planes (y, u, v), quarter-sample vectors [nb, 2]) of the motion compensation calls, and -- where the case refines --
    (cur luma, ref luma, integer vectors [nb, 2]) of the refinement: a moved copy searched by the oracle; a {0, 255} reference under
    vectors far outside the frame and at the int16 extremes (the clamp to +-8191); or cur = the prediction of a random reference under
    4 m + the candidate (b + seed) mod 49 of block b, so that every one of the 49 candidates is some block's exact match"""
    import _subpel_ref as R
    from _util import me_frames
    w, h, seed = case["w"], case["h"], case["seed"]
    nb = (w // 8) * (h // 8)
    mc = (R.planes(case["kind"], w, h, seed), R.mv_mix_q(nb, w, h, seed + 3))
    if not case["refine"]:
        return mc, None
    cur, ref = me_frames(w, h, 0, seed % 100000 + 4, mv=(2, -1), noise=4)
    if case["source"] == "search":
        mv_int = oracle.satd_search(cur, np.pad(ref, 4, mode="edge"), 4, 4)[0]
    elif case["source"] == "planted":
        ref = R.plane("random", w, h, seed + 5)
        mv_int = (R.mv_mix_q(nb, w, h, seed + 6).astype(np.int64) >> 2).clip(-64, 64)
        k = (np.arange(nb) + seed) % 49
        cur = R.mc_luma(ref, 4 * mv_int + np.stack([k % 7 - 3, k // 7 - 3], axis=1))[0]
    else:
        ref, mv_int = R.plane("extreme", w, h, seed + 5), R._mv_mix(nb, w, h, seed + 6)
    return mc, (cur, ref, np.asarray(mv_int, np.int16))


def bipred_content(case):
    """a dict: the two references' planes, the two lists' vectors, direction bytes (None: NULL), the weights (None: default); the
    decision recipe (cur per block one list's prediction or the bi prediction, so every direction can win); and, where the case
    refines, (cur, fixed plane, refined plane, mv_fix, integer vectors)"""
    import _bipred_ref as B
    import _subpel_ref as R
    from _util import me_frames
    w, h, seed = case["w"], case["h"], case["seed"]
    nb = (w // 8) * (h // 8)
    out = dict(p0=R.planes(case["kind"], w, h, seed), p1=R.planes(case["kind"], w, h, seed + 500), mv0=R.mv_mix_q(nb, w, h, seed + 3),
               mv1=R.mv_mix_q(nb, w, h, seed + 4), direction=None if "d_dir" in case["null"] else B.directions(nb, seed + 5),
               wp=None if case["weights"] is None else B.WEIGHTS[case["weights"]], decision=B.decision_case(None, w, h, seed + 6), refine=None)
    if case["refine"]:
        cur, ref = me_frames(w, h, 0, seed % 100000 + 7, mv=(2, -1), noise=4)
        out["refine"] = (cur, R.plane("extreme", w, h, seed + 8), ref, R.mv_mix_q(nb, w, h, seed + 9), R._mv_mix(nb, w, h, seed + 10))
    return out


def seeded_content(case):
    """(cur luma, ref luma, seed vectors [cells, 2])"""
    import _seeded_ref as E
    w, h = case["w"], case["h"]
    cur, ref = E.frame_pair(case["kind"], w, h, case["seed"])
    return cur, ref, E.seed_vectors(case["seed_kind"], w, h, case["seed_scale"], case["seed"])


# ---- RDOQ and the transform decision -----------------------------------------------------------------------------------------------------------
def rdoq_content(case):
    """(coefficients [n, 1024] int16, class bytes [n], qp bytes [n]), n = 6 n_ctu - drop; the coefficients are made for the classes and
    qps the call will use (N = 32 where d_class is NULL, the scalar qp where d_qp is).  The class bytes carry garbage above the low two
    bits, half of them are 32x32; a sixth of the qp bytes is above 51.  The wide kinds lie on Laplacian regions of 3 steps at DC and
    have every qp byte within wide_qp of the region's class:
      "heavy_head": the first case["heads"] scan positions of every block at a magnitude within case["mag"], random signs
      "heavy_cg":   one whole CG other than CG 0 of every block of N >= 8 at such magnitudes, the last four of the 16 chosen within
                    case["mag"] so that the CG's sum of D(0) is as little above a multiple of 2^32 as the last one can bring it (the
                    three before it bring the sum within its reach of one): Jz has a high dword and a small low one, and a
                    comparison of low dwords zeroes the CG (4x4 regions stay Laplacian)"""
    import _levels_ref as V
    import _rdoq_ref as R
    from _quant_ref import F as f_of, qbits, region_n, region_qp
    n, seed, kind, (lo, hi) = regions(case["w"], case["h"], case["drop"]), case["seed"], case["kind"], case["mag"]
    r = np.random.RandomState(seed)
    cls = (r.choice(4, n, p=(0.125, 0.125, 0.25, 0.5)) | r.randint(0, 64, n) << 2).astype(np.uint8)
    used_cls = None if "d_class" in case["null"] else cls
    n_of = region_n(used_cls, n)
    if kind in RDOQ_WIDE_KINDS:
        qps = np.array([_ends(r, 0, wide_qp(int(m), lo)) for m in n_of], np.uint8)
    else:
        qps = np.where(r.randint(0, 6, n) == 0, r.randint(52, 256, n), r.randint(0, 52, n)).astype(np.uint8)
    used_qps = None if "d_qp" in case["null"] else qps
    qp_of = region_qp(used_qps, case["qp"], n)
    if kind == "fullrange":
        return r.randint(-32768, 32768, (n, 1024)).astype(np.int16), cls, qps
    if kind == "ends":
        return np.array([-32768, 0, 32767], np.int16)[r.randint(0, 3, (n, 1024))], cls, qps
    if kind == "zeros":
        return np.zeros((n, 1024), np.int16), cls, qps
    coef = R.laplacian(n, used_cls, used_qps, case["qp"], 10.0 if kind == "laplacian" and case["lam"] > 368 else 3.0, seed % 100000)
    if kind == "laplacian":
        return coef, cls, qps
    for reg in range(n):
        k, qp = int(n_of[reg]) - 2, int(qp_of[reg])
        assert qp <= wide_qp(k + 2, lo), (case, reg)
        idx = V.region_order(k).reshape(-1, 16 << 2 * k)                    # [block, scan position] -> index in the region
        if kind == "heavy_head":
            shape = (idx.shape[0], case["heads"])
            coef[reg, idx[:, :case["heads"]]] = r.randint(lo, hi + 1, shape) * (1 - 2 * r.randint(0, 2, shape))
            continue
        if k == 0:
            continue
        f, qb = int(f_of[qp % 6]), int(qbits(k + 2, qp))
        every = np.arange(lo, hi + 1, dtype=np.int64)
        d0 = R.dist(every * f, 0, qb)
        for b in range(idx.shape[0]):
            s = int(r.randint(1, 1 << 2 * k))
            m = r.randint(lo, hi + 1, 16).astype(np.int64)
            for i in (12, 13, 14):                                          # the sum with the rest at `lo` as little below a multiple of 2^32 as i can bring it
                m[i] = every[np.argmax((int(R.dist(m[:i] * f, 0, qb).sum()) + d0 + (15 - i) * int(d0[0])) & 0xFFFFFFFF)]
            m[15] = every[np.argmin((int(R.dist(m[:15] * f, 0, qb).sum()) + d0) & 0xFFFFFFFF)]
            coef[reg, idx[b, 16 * s:16 * s + 16]] = m * (1 - 2 * r.randint(0, 2, 16))
    return coef, cls, qps


def region_extents(w, h):
    """[6 n_ctu, 2]: how many columns and rows of each region lie inside the frame (0: the region is wholly outside)"""
    nx, ny = (w + 63) // 64, (h + 63) // 64
    out = np.zeros((ny, nx, 6, 2), np.int64)
    for cy in range(ny):
        for cx in range(nx):
            for q in range(4):
                out[cy, cx, q] = np.clip(w - (cx * 64 + (q & 1) * 32), 0, 32), np.clip(h - (cy * 64 + (q >> 1) * 32), 0, 32)
            out[cy, cx, 4:] = np.clip(w // 2 - cx * 32, 0, 32), np.clip(h // 2 - cy * 32, 0, 32)
    out = out.reshape(-1, 2)
    out[(out == 0).any(1)] = 0
    return out


def tdecide_sample(w, h):
    """the regions the python statement decides (13 transforms and quantisations a region): all of them in frames up to two CTUs, else
    every cut region, the first region wholly outside the frame, and the first whole region of every q"""
    ext = region_extents(w, h)
    n = ext.shape[0]
    if n <= 12:
        return np.arange(n)
    whole, outside = (ext == 32).all(1), (ext == 0).all(1)
    keep = ~whole & ~outside
    keep[np.flatnonzero(outside)[:1]] = True
    for q in range(6):
        keep[np.flatnonzero(whole & (np.arange(n) % 6 == q))[:1]] = True
    return np.flatnonzero(keep)


def tdecide_content(case, oracle):
    """a dict: cur and pred tile arrays; qp bytes [n] up to 69 (clamped at 51); d_cand [n] uint16 -- a quarter each 0, bits outside
    0x777F alone (both fall back to the scalar masks), one class, a random subset, the last two under garbage outside 0x777F; and the
    16 side costs: all 0, all equal, random, or 40000 but for one cheap class"""
    import _tdecide_ref as T
    w, h, seed, kind = case["w"], case["h"], case["seed"], case["kind"]
    n = 6 * ctu_count(w, h)
    r = np.random.RandomState(seed)
    if kind == "five":
        cur, pred = T.content_frames(oracle, w, h, seed % 1000)
    else:
        cur = T.tiles_of_planes(oracle, *_three(_uniform if kind == "noise" else _ends_plane, w, h, seed))
        if kind == "ends_flat":
            pred = T.tiles_of_planes(oracle, *(np.full((ph, pw), 128, np.uint8) for pw, ph in ((w, h), (w // 2, h // 2), (w // 2, h // 2))))
        else:
            pred = T.tiles_of_planes(oracle, *_three(_uniform if kind == "noise" else _ends_plane, w, h, seed + 10))
    valid = np.array(T.CLASS_LIST)
    how = r.randint(0, 4, n)
    one = 1 << valid[r.randint(0, valid.size, n)]
    some = (r.randint(0, 2, (n, valid.size)) << valid).sum(1)
    garbage = r.randint(0, 1 << 16, n) & ~T.CLASSES & 0xFFFF
    cand = np.select([how == 0, how == 1, how == 2], [0, garbage | (garbage == 0) * 0x8000, one | garbage], some | garbage).astype(np.uint16)
    bits = {"zero": [0] * 16, "equal": [int(r.randint(1, 65536))] * 16, "random": [int(v) for v in r.randint(0, 65536, 16)], "cheap": [40000] * 16}[case["bits"]]
    if case["bits"] == "cheap":
        bits[int(valid[r.randint(0, valid.size)])] = int(r.randint(0, 64))
    return dict(cur=cur, pred=pred, qps=r.randint(0, 70, n).astype(np.uint8), cand=cand, class_bits=bits)


def tdecide_args(case, d):
    """the keyword arguments that the statement, the composition and the device driver share"""
    null = case["null"]
    return dict(qps=None if "d_qp" in null else d["qps"], qp=case["qp"], lam=case["lam"], cand_luma=case["cand_luma"], cand_chroma=case["cand_chroma"],
                cand=None if "d_cand" in null else d["cand"], class_bits=d["class_bits"])
