"""The case lists of tests/_frame_cases.py, on the CPU: every list is deterministic, holds its mandatory shape classes, and -- run through
the family's reference statement alone -- reaches what the family's fixed tests require of their own inputs.  These are conditions on the
lists, not measurements: a list that misses one is lengthened or reseeded, the condition stays."""
import collections

import numpy as np
import pytest

import _alf_ref as A
import _aq_ref as Q
import _bipred_ref as B
import _deblock_ref as D
import _decode_ref
import _frame_cases as F
import _intra_frame_ref as I
import _la_ref as L
import _levels_ref as V
import _mixed_frame_ref as M
import _quant_ref as QR
import _rdoq_ref as RQ
import _sao_ref as S
import _seeded_ref as E
import _subpel_ref as P
import _tdecide_ref as TD


# ---- the lists themselves -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", F.FAMILIES)
def test_lists_are_deterministic_and_scale_by_continuing(family):
    one, again, two = F.cases(family, 1), F.cases(family, 1), F.cases(family, 2)
    assert one == again and len(two) == 2 * len(one) and two[:len(one)] == one
    assert [c["index"] for c in two] == list(range(len(two)))
    assert all(c["shape"] == "random" for c in two[len(one):])
    g = F.GEOMETRY[family]
    for c in two:
        assert c["w"] % g["unit"] == 0 and c["h"] % g["unit"] == 0 and c["w"] > 0 and c["h"] > 0, c


@pytest.mark.parametrize("family", F.FAMILIES)
def test_mandatory_shape_classes(family):
    """recomputed from the sizes, not read from the names the generator gave them"""
    g = F.GEOMETRY[family]
    u = g["unit"]
    cs = F.cases(family, 1)
    sizes = [(c["w"], c["h"]) for c in cs]
    assert (u, u) in sizes
    assert any(w == u and h >= 5 * u for w, h in sizes) and any(w >= 5 * u and h == u for w, h in sizes)
    for r in (16, 32, 48) if g["cut"] else (32,) if u == 32 else ():
        assert any(w % 64 == r and h % 64 == 0 for w, h in sizes), r
        assert any(w % 64 == 0 and h % 64 == r for w, h in sizes), r
        assert any(w % 64 == r and h % 64 for w, h in sizes) and any(w % 64 and h % 64 == r for w, h in sizes), r
    for name, count, modulus in g["kernels"]:
        for r in g.get("residues", range(modulus)):                        # the residues the family's counts can have
            assert any(F.count_of(count, c) % modulus == r and F.count_of(count, c) > 2 * modulus for c in cs), (name, r)
    assert any(w // u > (64 if u == 16 else 32 if u == 32 else 4) for w, h in sizes)
    if g["threads"]:
        counts = sorted(g["threads"](w, h) for w, h in sizes if w >= 10 * u)
        assert F.THREADS_PER_WG in counts
        assert any(F.THREADS_PER_WG - 8 <= c < F.THREADS_PER_WG for c in counts) and any(F.THREADS_PER_WG < c <= F.THREADS_PER_WG + 8 for c in counts)
    assert sum(c["shape"] == "random" for c in F.cases(family, 1)) == g["random"] >= 4


@pytest.mark.parametrize("family", F.FAMILIES)
def test_parameters_reach_both_ends_and_every_null_form(family):
    cs = F.cases(family, 1)
    ranges = {"deblock": dict(qp=(0, 51), beta_offset_div2=(-6, 6), tc_offset_div2=(-6, 6)), "sao": dict(lam=(0, 65535)),
              "alf": dict(lam=(0, 65535), n_luma=(0, 8), n_chroma=(0, 8)),
              "aq": dict(strength_q8=(0, 1024), qp=(0, 51), chroma_qp_offset=(-12, 12), mode=(1, 2)),
              "la": dict(intra_penalty=(0, 65535), strength_q8=(0, 1024), qp=(0, 51), chroma_qp_offset=(-12, 12)),
              "quant": dict(qp=(0, 51), rounding=(0, 511), drop=(0, 5)), "levels": dict(drop=(0, 5)),
              "intra_frame": dict(qp=(0, 51), rounding=(0, 511)),
              "mixed": dict(qp=(0, 51), rounding=(0, 511), intra_penalty=(0, 1 << 24), flip=(0, 1)),
              "qpel": dict(), "bipred": dict(bi_penalty=(0, 65535), list=(0, 1)),
              "seeded": dict(seed_scale=(0, 1), centres=(0, 31), range=(0, 8), lam=(0, 65535)),
              "rdoq": dict(qp=(0, 51), lam=(0, 8192), drop=(0, 5), heads=(1, 4)), "tdecide": dict(qp=(0, 51), lam=(0, 8192), same_frame=(False, True))}[family]
    for name, (lo, hi) in ranges.items():
        vals = [c[name] for c in cs]
        assert min(vals) == lo and max(vals) == hi, (name, min(vals), max(vals))
    nulls = {"deblock": ("cls", "intra", "nnz", "qps", "mv"), "sao": ("d_stats",), "alf": ("d_class", "d_mask"), "aq": ("d_offset", "d_qp"),
             "la": ("d_mode", "d_inter0", "d_inter1", "d_prop", "d_prop_ref0", "d_prop_ref1", "d_aq_offset", "d_offset", "d_qp"),
             "quant": ("d_class", "d_qp", "d_nnz"), "levels": ("d_class", "d_nnz", "d_nnz of unpack"), "intra_frame": ("d_qp", "d_nnz", "d_mode_in"),
             "mixed": ("d_qp", "d_kind_in", "d_mode_in", "d_nnz", "d_cost"), "qpel": ("d_costs",), "bipred": ("d_dir", "d_costs", "d_costs of the cost call", "d_dir of the cost call"),
             "seeded": ("d_j",), "rdoq": ("d_class", "d_qp", "d_nnz", "d_stat"), "tdecide": ("d_qp", "d_cand", "d_nnz", "d_stat", "d_cost")}[family]
    for name in nulls:
        assert any(name in c["null"] for c in cs) and any(name not in c["null"] for c in cs), name
    if family in ("deblock", "quant", "intra_frame", "mixed", "qpel", "bipred", "rdoq"):              # the families with a call that may run in place
        assert {c["inplace"] for c in cs} == {False, True}
    kinds = {"deblock": F.DEBLOCK_KINDS, "sao": F.SAO_KINDS, "alf": F.ALF_KINDS, "aq": F.AQ_KINDS, "la": F.LA_KINDS, "quant": F.QUANT_KINDS,
             "levels": F.LEVELS_KINDS, "intra_frame": F.INTRA_KINDS, "mixed": F.INTRA_KINDS, "qpel": F.QPEL_KINDS, "bipred": F.QPEL_KINDS,
             "seeded": F.SEEDED_FRAMES, "rdoq": F.RDOQ_KINDS, "tdecide": F.TDECIDE_KINDS}[family]
    assert {c["kind"] for c in cs} == set(kinds)
    if family == "seeded":                                                  # the interior of the search range too
        assert len({c["range"] for c in cs}) >= 6


@pytest.mark.parametrize("family", [f for f in F.FAMILIES if F.GEOMETRY[f].get("refines")])
def test_the_refining_cases_hold_their_shape_classes(family):
    """the refinements run on a part of the list (their statement forms 49 predictions of the frame): that part has one unit, both strips,
    every cut width, a cut height, a frame cut both ways, the long row and at least three random frames"""
    cs = [c for c in F.cases(family, 1) if c["refine"]]
    sizes = [(c["w"], c["h"]) for c in cs]
    assert (16, 16) in sizes and any(w == 16 and h >= 80 for w, h in sizes) and any(w >= 80 and h == 16 for w, h in sizes)
    for r in (16, 32, 48):
        assert any(w > 64 and w % 64 == r for w, h in sizes), r
    assert any(h > 64 and h % 64 and w % 64 == 0 for w, h in sizes) and any(w > 64 and h > 64 and w % 64 and h % 64 for w, h in sizes)
    assert any(w // 16 > 64 for w, h in sizes) and sum(c["shape"] == "random" for c in cs) >= 3
    assert all(c["refine"] == F._refines(c["w"], c["h"]) for c in F.cases(family, 2))


# ---- the statements over the lists --------------------------------------------------------------------------------------------------------
def test_deblock_list_reaches_every_counter():
    total = D.new_counts()
    for c in F.cases("deblock", 1):
        y, u, v, side = F.deblock_content(c)
        D.deblock_luma(y, side, total)
        D.deblock_chroma(u, v, side, total)
    D.assert_coverage(272, 208, total)                                      # everything a size from 64x64 on, wider and higher than a CTU, must reach


def test_sao_list_chooses_every_type():
    info = collections.Counter()
    for c in F.cases("sao", 1):
        org, dec = F.sao_content(c)
        S.decide(S.stats(org, dec), c["lam"], info)
    for comp in ("luma", "chroma"):
        for typ in ("off", "bo", "eo0", "eo1", "eo2", "eo3"):
            assert info["%s_%s" % (comp, typ)] > 0, (comp, typ, dict(info))
    assert info["clamped_to_7"] and info["cut_by_rate"] and info["band_position_tie"] and info["tie_to_earlier"]


def test_alf_list_reaches_every_class_transposition_and_control_byte():
    pairs, picked = set(), set()
    ctrl_kinds = [set(), set(), set()]
    for c in F.cases("alf", 1):
        org, dec = F.alf_content(c)
        classes = A.classify(dec[0])
        cls, tr = A.decode(classes)
        pairs |= set((cls * 4 + tr).ravel().tolist())
        n = F.ctu_count(c["w"], c["h"])
        st = A.stats(org, dec, None if "d_class" in c["null"] else F.alf_class_map(c))
        luma, chroma, ctrl, mask = F.alf_sets(c, st)
        for m, count in enumerate((c["n_luma"], c["n_chroma"], c["n_chroma"])):
            ctrl_kinds[m] |= {"off" if v == 0 else "valid" if v <= count else "255" if v == 255 else "above" for v in ctrl[:, m].tolist()}
        A.sum_stats(st, mask)
        picked |= set(A.decide(st, luma, chroma, c["lam"]).ravel().tolist())
        assert ctrl.shape == (n, 3)
    assert {p // 4 for p in pairs} == set(range(25)) and {p % 4 for p in pairs} == {0, 1, 2, 3}
    for kinds in ctrl_kinds:
        assert kinds == {"off", "valid", "above", "255"}, kinds
    assert 0 in picked and 1 in picked                                      # the solved set wins somewhere and something stays off


def test_aq_list_reaches_both_clamps_and_both_signs():
    qps, signs = set(), set()
    for c in F.cases("aq", 1):
        tiles = F.aq_content(c)
        rec = Q.tile_stats(tiles)
        off, qp = Q.decide(rec, Q.totals(rec), c["w"], c["h"], c["mode"], c["strength_q8"], c["qp"], c["chroma_qp_offset"])
        qps |= set(qp.tolist())
        signs |= set(np.sign(off).tolist())
        if abs(int(off.min())) == 3072 or int(off.max()) == 3072:
            signs.add("clamp")
    assert {0, 51} <= qps and signs == {-1, 0, 1, "clamp"}, (sorted(qps), signs)


def test_la_list_reaches_every_frame_cost_kind():
    kinds, qps = set(), set()
    for c in F.cases("la", 1):
        w, h = c["w"], c["h"]
        tiles = F.la_content(c)
        low = L.downscale(tiles, w, h)
        cost, mode = L.intra_costs(low, w, h)
        l0, l1, prop, aq = F.la_side(c, cost)
        rec, tot = L.frame_cost(cost, None if "d_mode" in c["null"] else mode, l0, l1, c["intra_penalty"])
        kinds |= set(rec["kind"].tolist())
        L.propagate(rec, prop, *F.la_accumulators(c, rec.size), w, h)
        qps |= set(L.tree_qp(rec, prop, aq, w, h, c["strength_q8"], c["qp"], c["chroma_qp_offset"])[1].tolist())
    assert kinds == {0, 1, 2} and {0, 51} <= qps


def test_quant_list_has_empty_and_coded_regions_in_every_component(oracle):
    empty, coded, clipped = set(), set(), False
    for c in F.cases("quant", 1):
        coef, lev, cls, qps = F.quant_content(c)
        kw = dict(classes=None if "d_class" in c["null"] else cls, qps=None if "d_qp" in c["null"] else qps, qp=c["qp"])
        QR.quant_regions(coef, False, rounding=c["rounding"], **kw)
        back = QR.quant_regions(lev, True, **kw)
        clipped |= bool((back == 32767).any() and (back == -32768).any())
        cur, pred, base, frame_qps = F.quant_frames(c)
        _, nnz, _ = QR.code_ctu_tiles(oracle, cur, pred, c["w"], c["h"], None if "d_qp" in c["null"] else frame_qps, c["qp"], c["rounding"], base=base)
        empty |= set(np.nonzero(nnz == 0)[1].tolist())
        coded |= set(np.nonzero(nnz != 0)[1].tolist())
    assert empty == set(range(6)) and coded == set(range(6)) and clipped


def test_levels_list_has_empty_dense_and_one_coefficient_regions():
    seen = collections.Counter()
    for c in F.cases("levels", 1):
        lv, cls = F.levels_content(c)
        assert lv.shape == (F.regions(c["w"], c["h"], c["drop"]), 1024) and cls.shape == lv.shape[:1]
        rec, stream, total = V.pack(lv, None if "d_class" in c["null"] else cls)
        seen.update(empty=int((rec["n_nz"] == 0).sum()), dense=int((rec["n_nz"] == 1024).sum()), one=int((rec["n_nz"] == 1).sum()),
                    extreme=int((rec["max_abs"] == 32768).sum()), capped=int(c["cap_q8"] is not None and int(total[0]) > 0))
    assert all(seen[k] > 0 for k in ("empty", "dense", "one", "extreme", "capped")), seen


def test_intra_frame_list_codes_and_leaves_regions_and_the_decoder_rebuilds_them(oracle):
    seen = collections.Counter()
    for c in F.cases("intra_frame", 1):
        w, h = c["w"], c["h"]
        qps, modes, _ = F.frame_side(c)
        qps = None if "d_qp" in c["null"] else qps
        want = I.code_frame(oracle, I.case(c["kind"], w, h, c["seed"] % 100000), w, h, qps, c["qp"], c["rounding"], None if "d_mode_in" in c["null"] else modes)
        seen.update(empty=int((want.nnz == 0).sum()), coded=int((want.nnz != 0).sum()), dm=int((want.chroma_pos == 4).sum()), decided=int("d_mode_in" in c["null"]),
                    given=int("d_mode_in" not in c["null"]))
        if c["index"] < 3:                                                  # the decoder on the statement's own stream: the statement's frame
            rec, stream, _ = V.pack(want.levels.reshape(-1, 1024), None, want.nnz.ravel())
            planes, levels = _decode_ref.decode(oracle, rec, stream, w, h, np.ones_like(want.modes), want.modes, qps, c["qp"])
            assert np.array_equal(levels, want.levels) and all(np.array_equal(a, b) for a, b in zip(planes, want.planes)), F.tag(c)
    assert all(seen[k] > 0 for k in ("empty", "coded", "dm", "decided", "given")), seen


def mixed_statement(oracle, c):
    w, h = c["w"], c["h"]
    qps, modes, kinds = F.frame_side(c)
    cur, pred = M.pred_planes(w, h, c["flip"], c["kind"], c["seed"] % 100000)
    want = M.code_frame(oracle, cur, pred, w, h, None if "d_qp" in c["null"] else qps, c["qp"], c["rounding"], c["intra_penalty"],
                        None if "d_kind_in" in c["null"] else kinds, None if "d_mode_in" in c["null"] else modes)
    return cur, pred, want


def test_mixed_list_decides_both_ways_and_ties_and_the_decoder_rebuilds_it(oracle):
    seen = collections.Counter()
    for c in F.cases("mixed", 1):
        qps, _, kinds = F.frame_side(c)
        cur, pred, want = mixed_statement(oracle, c)
        deciding = np.ones_like(want.kinds, bool) if "d_kind_in" in c["null"] else kinds >= 2
        inter, intra = want.costs[..., 0].astype(np.int64), want.costs[..., 1].astype(np.int64)
        seen.update(to_intra=int((deciding & (want.kinds == 1)).sum()), to_inter=int((deciding & (want.kinds == 0)).sum()),
                    tie=int((deciding & (intra + c["intra_penalty"] == inter)).sum()), given_intra=int((~deciding & (want.kinds == 1)).sum()),
                    given_inter=int((~deciding & (want.kinds == 0)).sum()))
        if c["index"] < 3:
            rec, stream, _ = V.pack(want.levels.reshape(-1, 1024), None, want.nnz.ravel())
            planes, levels = _decode_ref.decode(oracle, rec, stream, c["w"], c["h"], want.kinds, want.modes, None if "d_qp" in c["null"] else qps, c["qp"], pred)
            assert np.array_equal(levels, want.levels) and all(np.array_equal(a, b) for a, b in zip(planes, want.planes)), F.tag(c)
    assert all(seen[k] > 0 for k in ("to_intra", "to_inter", "tie", "given_intra", "given_inter")), seen


def test_qpel_list_reaches_every_phase_both_clips_and_every_refinement_winner(oracle):
    luma, chroma, winners, refined = P.Counts(4), P.Counts(8), set(), 0
    for c in F.cases("qpel", 1):
        (planes, mv), refine = F.qpel_content(c, oracle)
        luma += P.mc_luma(planes[0], mv)[1]
        chroma += P.mc_chroma(planes[1], planes[2], mv)[2]
        if refine is not None:
            cur, ref, mv_int = refine
            want_mv, _, costs = P.refine(oracle, cur, ref, mv_int)
            winners |= set(P.winner(costs).tolist())
            refined += 1
    for counts in (luma, chroma):                                           # every phase class, and both clips and a negative intermediate somewhere
        assert (counts.samples > 0).all() and counts.below.sum() > 0 and counts.above.sum() > 0 and counts.negative_v.sum() > 0, counts
    assert winners == set(range(49)) and refined >= 12, (sorted(set(range(49)) - winners), refined)


def test_bipred_list_lets_every_direction_win(oracle):
    won, weights, refined = set(), set(), 0
    for c in F.cases("bipred", 1):
        d = F.bipred_content(c)
        cur, ref0, ref1, mv0, mv1 = d["decision"]
        costs, direction = B.costs3(oracle, cur, ref0, ref1, mv0, mv1, d["wp"], c["bi_penalty"])
        won |= set(direction.tolist())
        weights.add(c["weights"])
        for comp, kind in ((0, "luma"), (1, "chroma"), (2, "chroma")):
            B.bi_plane(d["p0"][comp], d["p1"][comp], d["mv0"], d["mv1"], d["direction"], d["wp"], kind, comp, d["p0"][comp])
        if d["refine"] is not None:
            cur, fix, ref, mv_fix, mv_int = d["refine"]
            B.refine_bi(oracle, cur, fix, mv_fix, ref, mv_int, c["list"], d["wp"])
            refined += 1
    assert won == {1, 2, 3} and weights == set(F.WEIGHT_NAMES) and refined >= 12, (won, weights, refined)


def test_seeded_list_has_winners_on_the_seed_and_off_it(oracle):
    on = off = 0
    for c in F.cases("seeded", 1):
        cur, ref, seeds = F.seeded_content(c)
        best, j, index = E.search(oracle, cur, ref, seeds, c["seed_scale"], c["centres"], c["range"], c["lam"])
        r = c["range"]
        centre = index == (2 * r + 1) * r + r                               # the walk's entry of the own centre itself
        on, off = on + int(centre.sum()), off + int((~centre).sum())
    assert on > 0 and off > 0, (on, off)


# ---- RDOQ: sums at and above 2^32 ---------------------------------------------------------------------------------------------------------
WIDE = 1 << 32


def rdoq_blocks(c, coef, cls, qps):
    """the statement block by block over a case of "rdoq" and its content -> [(class k, sum of D(0) or None where no level survives
    step 2, Totals, {CG: (Jz, Jc)}, changed, CGs zeroed, last moved)]"""
    n_of = QR.region_n(None if "d_class" in c["null"] else cls, coef.shape[0])
    qp_of = QR.region_qp(None if "d_qp" in c["null"] else qps, c["qp"], coef.shape[0])
    out = []
    for reg in range(coef.shape[0]):
        n = int(n_of[reg])
        for idx in RQ._region_blocks(n - 2):
            totals, cgs = {}, {}
            _, _, _, changed, zeroed, moved = RQ.rdoq_block(coef[reg, idx].astype(np.int64), n, int(qp_of[reg]), c["lam"], totals=totals, cgs=cgs)
            out.append((n - 2, totals.get(None), totals, cgs, changed, zeroed, moved))
    return out


def test_rdoq_list_decides_on_sums_past_2_to_the_32():
    """A block is wide when its sum of D(0) is 2^32 or more.  Per class: wide blocks in which step 3 moved or removed the last position,
    and (N >= 8) in which step 2 zeroed a CG; wide blocks whose step-3 choice differs when the Totals are compared by their low dwords,
    and step-2 decisions that differ when Jz and Jc are: a kernel that drops, swaps or truncates the high half of a 64-bit sum gives
    other levels than the statement on this list.  The narrow blocks still fire all three steps, and the bytes the call clamps or
    masks are among those it is given."""
    seen = collections.Counter()
    for c in F.cases("rdoq", 1):
        coef, cls, qps = F.rdoq_content(c)
        assert coef.dtype == np.int16 and coef.shape == (F.regions(c["w"], c["h"], c["drop"]), 1024) and cls.shape == qps.shape == coef.shape[:1], F.tag(c)
        seen["a qp byte above 51"] += int("d_qp" not in c["null"] and (qps > 51).any())
        seen["a class byte with high bits"] += int("d_class" not in c["null"] and (cls > 3).any())
        for k, d0, totals, cgs, changed, zeroed, moved in rdoq_blocks(c, coef, cls, qps):
            wide = d0 is not None and d0 >= WIDE
            if wide:
                seen["wide", k] += 1
                seen["wide, step 3 acts", k] += moved
                seen["wide, step 2 acts", k] += zeroed > 0
                seen["step 3 by low dwords differs", k] += RQ.step3_choice(totals) != RQ.step3_choice(totals, 32)
            elif c["lam"] > 0:
                seen.update(changed=changed, cg_zeroed=zeroed, last_moved=moved)
            seen["step 2 by low dwords differs", k] += sum((jz < jc) != (jz % WIDE < jc % WIDE) for jz, jc in cgs.values())
    for k in range(4):
        assert seen["wide, step 3 acts", k] >= 8 and seen["step 3 by low dwords differs", k] >= 4, (k, seen)
        assert k == 0 or (seen["wide, step 2 acts", k] >= 8 and seen["step 2 by low dwords differs", k] >= 4), (k, seen)
    assert seen["changed"] > 0 and seen["cg_zeroed"] > 0 and seen["last_moved"] > 0, seen
    assert seen["a qp byte above 51"] > 0 and seen["a class byte with high bits"] > 0, seen


# ---- the transform decision -----------------------------------------------------------------------------------------------------------------
def tdecide_statement(oracle, c, d):
    """the statement on the regions of F.tdecide_sample -> (regions, class bytes, levels, records, costs)"""
    sel = F.tdecide_sample(c["w"], c["h"])
    return (sel,) + TD.decide(oracle, d["cur"], d["cur"] if c["same_frame"] else d["pred"], c["w"], c["h"], regions=sel, **F.tdecide_args(c, d))


def test_tdecide_list_lets_every_class_win_and_ties_and_cuts(oracle):
    """every class wins a region; two candidates tie exactly; the side costs move a winner; cut regions and regions wholly outside the
    frame; the scalar masks, d_cand, the side costs and the qp bytes in every form they are drawn in.  J stays below 2^32 whatever the
    content (see GEOMETRY): the list must reach 2^31, the upper half of the low dword."""
    seen, winners, largest = collections.Counter(), set(), 0
    for c in F.cases("tdecide", 1):
        d = F.tdecide_content(c, oracle)
        sel, cls, level, stat, cost = tdecide_statement(oracle, c, d)
        bits = d["class_bits"]
        ext = F.region_extents(c["w"], c["h"])[sel]
        winners |= set(cls.tolist())
        seen.update(cut=int(((ext != 32).any(1) & (ext != 0).all(1)).sum()), outside=int((ext == 0).all(1).sum()), whole=int((ext == 32).all(1).sum()))
        seen["side costs: " + c["bits"]] += 1
        for m in (c["cand_luma"], c["cand_chroma"]):
            assert m and m & ~TD.CLASSES == 0, F.tag(c)
            seen["a scalar mask of one class"] += bin(m).count("1") == 1
            seen["a scalar mask of every class"] += m == TD.CLASSES
        if "d_cand" not in c["null"]:
            valid, invalid = d["cand"].astype(np.int64) & TD.CLASSES, d["cand"].astype(np.int64) & ~TD.CLASSES
            seen["d_cand of 0"] += int((d["cand"] == 0).any())
            seen["d_cand of invalid bits alone"] += int(((valid == 0) & (invalid != 0)).any())
            seen["d_cand of valid bits under invalid ones"] += int(((valid != 0) & (invalid != 0)).any())
        seen["a qp byte above 51"] += int("d_qp" not in c["null"] and (d["qps"] > 51).any())
        for i in range(sel.size):
            js = sorted((int(cost[i, k]), k) for k in TD.CLASS_LIST if cost[i, k] != TD.ALL_ONES)
            assert js[0][0] == int(cost[i, cls[i]]), F.tag(c)
            seen["winner moved by the side costs"] += min((j - c["lam"] * bits[k], k) for j, k in js)[1] != int(cls[i])
            seen["tie of the two best"] += len(js) > 1 and js[0][0] == js[1][0]
            largest = max(largest, js[-1][0])
    assert winners == set(TD.CLASS_LIST), sorted(winners)
    for name in ["cut", "outside", "whole", "tie of the two best", "winner moved by the side costs", "a scalar mask of one class", "a scalar mask of every class", "d_cand of 0",
                 "d_cand of invalid bits alone", "d_cand of valid bits under invalid ones", "a qp byte above 51"] + ["side costs: " + b for b in F.TDECIDE_BITS]:
        assert seen[name] > 0, (name, seen)
    assert 1 << 31 <= largest < WIDE, largest
