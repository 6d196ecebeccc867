"""The guard of the case table of tests/test_gpu_pcs_free_points.py (CPU): tests/pcs_plan_model.py restates the host decisions
of the Goldilocks opening, and the table must reach every value of every one of them at least once; exactly the cases marked
as refusals have three points at one LDE height. A threshold that moves in the source changes the constants the model reads
from it, so a branch that the table no longer reaches fails here instead of silently losing its test."""
import pcs_plan_model as M


def _plans(runs=None):
    k = M.source_constants()
    return [(c, knob, M.plan(c, knob, k)) for c, knob in (runs or M.RUNS)]


def reached(plans):
    """decision value -> the runs that reach it"""
    seen = {}

    def hit(key, c, knob):
        seen.setdefault(key, []).append((c.name, knob))

    for c, knob, p in plans:
        if p["refused"]:
            hit("refused: three points at one height", c, knob)
            if any(v == "next" for v in p["pair"].values()):
                hit("refused: a next pair plus a third point", c, knob)
            else:
                hit("refused: three points of their own", c, knob)
            continue
        for key, v in p["pair"].items():
            hit("pair: " + v, c, knob)
            if v == "next" and c.rounds[key[0]][key[1]].points[0].turn:
                hit("pair: next, first point is not z", c, knob)
        nxt = [key for key, v in p["pair"].items() if v == "next"]
        dem = [key for key, v in p["pair"].items() if v == "demoted"]
        for key in dem:
            lh = c.rounds[key[0]][key[1]].log_n
            by = [(ri, mi) for ri, r in enumerate(c.rounds) for mi, m in enumerate(r) if m.log_n == lh and (ri, mi) != key and
                  c.rounds[key[0]][key[1]].points[1] in m.points]
            for ri, mi in by:
                hit("demoted by %s matrix of %s round" % ("a later" if (ri, mi) > key else "an earlier", "the same" if ri == key[0] else "another"), c, knob)
        if nxt and dem:
            hit("a next pair kept beside a demoted one", c, knob)
        if nxt:
            own = {m.points[1] for key in nxt for m in [c.rounds[key[0]][key[1]]]}
            if any(z in own for z, _ in p["points"]):
                hit("the second point of a next pair is another height's own point", c, knob)
        for z in p["raised_after_first_use"]:
            hit("a point's tallest matrix comes after its first use", c, knob)
        if p["reads_a_prefix"]:
            hit("a shorter matrix reads a prefix of the denominators", c, knob)
        for route, blocks in p["inv_denoms"]:
            hit("inv_denoms: %s, %s" % (route, "one block" if blocks == 1 else "%d blocks" % blocks), c, knob)
        for lg in (12, 13, 14):
            if sum(1 for _, h in p["points"] if h == lg) >= 2:
                hit("two points of their own on the 2^%d domain" % lg, c, knob)
        hit("side stream: " + ("used" if p["use_side"] else "not used"), c, knob)
        if p["side_points"]:
            hit("side stream: a short point's denominators", c, knob)
        if p["short_matrix_reads_tall_point"]:
            hit("side stream: a short matrix opens a tall point", c, knob)
        for b in p["bary"].values():
            hit("bary: %d row block%s" % (b["nblk"], "" if b["nblk"] == 1 else "s"), c, knob)
            hit("bary: last column group %s" % ("ragged" if b["ragged"] else "full"), c, knob)
            hit("bary: %s" % ("one point" if b["np"] == 1 else "two points, next" if b["next"] else "two points of their own"), c, knob)
        hit("bary: " + ("batched" if p["bary_batched"] else "one launch pair per matrix"), c, knob)
        for n in p["bary_launches"]:
            hit("bary batch: %s" % ("full launch" if n == 8 else "partial launch"), c, knob)
        if len(p["bary_launches"]) >= 2 and not p["use_side"]:
            hit("bary batch: second launch", c, knob)
        if len(p["bary_launches"]) >= 2 and p["use_side"]:
            hit("bary batch: one launch per stream", c, knob)
        if p["job_index_differs_from_matrix_index"]:
            hit("bary batch: a job's index is not its matrix's", c, knob)
        order = sorted(p["heights"], reverse=True)
        for lh in order:
            h = p["heights"][lh]
            where = "tallest" if h["tallest"] else "middle" if lh != order[-1] else "shortest"
            if h["kernel"] == "memset":
                hit("reduced openings: memset at the %s height" % where, c, knob)
                continue
            hit("reduced openings: %s kernel, leaves %s" % (h["kernel"], "on" if h["leaves"] else "off"), c, knob)
            hit("reduced openings: %d point%s at a height" % (h["points"], "" if h["points"] == 1 else "s"), c, knob)
            if h["shifted_point"]:
                hit("reduced openings: %s kernel reads a shifted point" % h["kernel"], c, knob)
            if h["tallest"] and (1 << lh) >= 8192 and not h["leaves"]:
                hit("reduced openings: leaves off at a tallest height of 8192 rows or more (%s)" % ("knob" if "LEAVES" in str(M.KNOBS[knob]) else "arity"
                    if c.params[3] > 1 else "?"), c, knob)
            if h["total_w"] in (511, 512) and (1 << lh) == 8192:
                hit("reduced openings: total width %d at 8192 rows: %s" % (h["total_w"], h["kernel"]), c, knob)
            if h["kernel"] == "plain":
                for w in h["widths"]:
                    hit("plain kernel: width %s" % ("below 8" if w < 8 else "8" if w == 8 else "16n + r" if w > 16 and w % 8 else "8 + r" if w % 8 else "8n"), c, knob)
            else:
                for w in h["widths"]:
                    hit("wide kernel: width = %d mod 64" % (w % 64) if w % 64 in (63, 0, 1, 2) else "wide kernel: another width", c, knob)
            if h["on_side"]:
                hit("reduced openings on the side stream", c, knob)
        if c.params[3] > 1:
            hit("wide fold", c, knob)
    return seen


WANTED = [
    "pair: next", "pair: demoted", "pair: suppressed", "pair: coincident", "pair: reversed", "pair: other generator", "pair: unrelated",
    "pair: next, first point is not z",
    "demoted by a later matrix of the same round", "demoted by an earlier matrix of the same round", "demoted by a later matrix of another round",
    "a next pair kept beside a demoted one", "the second point of a next pair is another height's own point",
    "a point's tallest matrix comes after its first use", "a shorter matrix reads a prefix of the denominators",
    "inv_denoms: slow, one block", "inv_denoms: fast, one block", "inv_denoms: fast, 2 blocks",
    "two points of their own on the 2^12 domain", "two points of their own on the 2^13 domain", "two points of their own on the 2^14 domain",
    "side stream: used", "side stream: not used", "side stream: a short point's denominators", "side stream: a short matrix opens a tall point",
    "reduced openings on the side stream",
    "bary: 1 row block", "bary: 2 row blocks", "bary: last column group ragged", "bary: last column group full",
    "bary: one point", "bary: two points, next", "bary: two points of their own", "bary: batched", "bary: one launch pair per matrix",
    "bary batch: full launch", "bary batch: partial launch", "bary batch: second launch", "bary batch: one launch per stream",
    "bary batch: a job's index is not its matrix's",
    "reduced openings: memset at the tallest height", "reduced openings: memset at the middle height", "reduced openings: memset at the shortest height",
    "reduced openings: plain kernel, leaves on", "reduced openings: plain kernel, leaves off",
    "reduced openings: wide kernel, leaves on", "reduced openings: wide kernel, leaves off",
    "reduced openings: 1 point at a height", "reduced openings: 2 points at a height",
    "reduced openings: plain kernel reads a shifted point", "reduced openings: wide kernel reads a shifted point",
    "reduced openings: leaves off at a tallest height of 8192 rows or more (knob)", "reduced openings: leaves off at a tallest height of 8192 rows or more (arity)",
    "reduced openings: total width 512 at 8192 rows: wide", "reduced openings: total width 511 at 8192 rows: plain",
    "reduced openings: total width 512 at 8192 rows: plain",  # MSAMD_NO_DEEP_WIDE
    "plain kernel: width below 8", "plain kernel: width 8", "plain kernel: width 8 + r", "plain kernel: width 16n + r",
    "wide kernel: width = 63 mod 64", "wide kernel: width = 0 mod 64", "wide kernel: width = 1 mod 64", "wide kernel: width = 2 mod 64",
    "wide fold",
    "refused: three points at one height", "refused: a next pair plus a third point", "refused: three points of their own",
]


def test_the_model_reads_the_thresholds_the_issue_names():
    k = M.source_constants()
    assert k["BARY_T"] * k["BARY_ROWS"] == 4096 and k["BARY_MAX_JOBS"] == 8
    assert (k["WIDE_MAX_HEIGHT"], k["WIDE_MIN_WIDTH"], k["LEAVES_MIN_HEIGHT"]) == (8192, 512, 8192)
    assert k["DEN_FAST_LOG"] == 13 and k["DEN_BLOCK"] == 8192 and k["MAX_POINTS_PER_HEIGHT"] == 2


def test_case_table_reaches_every_decision():
    seen = reached(_plans())
    missing = [w for w in WANTED if not seen.get(w)]
    assert not missing, "no case reaches: %s" % "; ".join(missing)


def test_exactly_the_refusal_cases_have_three_points_at_a_height():
    for c, knob, p in _plans():
        assert p["refused"] == c.refused, "%s under %s: the model %s, the table says otherwise" % (c.name, knob, "refuses" if p["refused"] else "accepts")
    assert sum(1 for c in M.CASES if c.refused) >= 2


def test_every_case_serves_a_purpose():
    """removing a whole family of cases un-covers a decision (the guard can fail), and the names are unique"""
    names = [c.name for c in M.CASES]
    assert len(set(names)) == len(names)
    for family, lost in (("demote", "pair: demoted"), ("threshold_512", "reduced openings: wide kernel, leaves on"),
                         ("none_", "reduced openings: memset at the tallest height"), ("matrices_", "bary batch: second launch"),
                         ("wide_slices", "wide kernel: width = 63 mod 64"), ("one_row", "pair: coincident"),
                         ("refuse_pair", "refused: a next pair plus a third point")):
        runs = [(c, knob) for c, knob in M.RUNS if family not in c.name]
        assert len(runs) < len(M.RUNS)
        assert not reached(_plans(runs)).get(lost), "%s is still reached without the %s cases" % (lost, family)


def test_model_on_hand_worked_examples():
    """the restated rules on three patterns worked out by hand from prover.hip / open_plan.h"""
    k = M.source_constants()
    by = {c.name: c for c in M.CASES}
    p = M.plan(by["demote-p1"], "none", k)
    assert p["is_next_before"][0, 0] and not p["is_next"][0, 0] and p["is_next"][1, 0]
    assert [h for _, h in p["points"]] == [11, 11] and p["heights"][11]["points"] == 2 and p["heights"][10]["shifted_point"]
    p = M.plan(by["refuse_pair_and_third-p1"], "none", k)
    assert p["is_next"][0, 0] and p["refused"]
    p = M.plan(by["refuse_pair_and_third-p1"]._replace(refused=False), "no_next", k)
    assert p["refused"]  # z, z g and a are three points either way
    p = M.plan(by["threshold_512_next"], "none", k)
    assert p["heights"][13] == dict(p["heights"][13], kernel="wide", leaves=True, total_w=512, points=2)
    p = M.plan(by["threshold_512_next_below_taller"], "none", k)
    assert p["heights"][13]["kernel"] == "wide" and not p["heights"][13]["leaves"] and p["heights"][14]["leaves"]
    p = M.plan(by["side_own_point"], "side4", k)
    assert p["use_side"] and [z.base for z in p["side_points"]] == ["a", "b"] and not p["short_matrix_reads_tall_point"]
    p = M.plan(by["matrices_17"], "none", k)
    assert p["bary_launches"] == [8, 4] or sum(p["bary_launches"]) == len(p["bary"])
