"""The host decisions of the Goldilocks opening (csrc/prover.hip::pcs_open, csrc/open_plan.h, csrc/open.hip) restated in plain
Python, and the case table of tests/test_gpu_pcs_free_points.py. The model works from a case's shapes, parameters and point
pattern alone; nothing here touches the library or a device. tests/test_pcs_plan_model.py asserts that the table reaches every
value of every decision below (a guard against an edit of the table, or a moved threshold, un-covering a branch: it does not
test the kernels).

Points are symbolic: a base name ("z", "a", "b": three independent samples of the transcript) times a power of a two-adic
generator, kept as the exponent's fraction of a full turn - g(k)^e is e / 2^k mod 1 - so equality is exact.
  pt("z")          z
  pt("z", 10)      z * g(10), g(k) the generator of the 2^k-row trace domain
  pt("z", 10, -1)  z * g(10)^-1"""
import os
import re
from collections import namedtuple
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-stark_amd", "csrc")


# ------------------------------------------------------------------ constants without a public query: read from the source
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text, what):
    m = re.findall(pattern, text)
    assert len(m) == 1, "%s: %d matches of %r in the source (the model must be revisited)" % (what, len(m), pattern)
    return m[0]


def source_constants():
    o, p, h, m, c = _src("open.hip"), _src("prover.hip"), _src("open_plan.h"), _src("msamd.h"), _src("ctx.hip")
    k = {}
    for name in ("BARY_T", "BARY_ROWS", "BARY_COLS", "BARY_MAX_JOBS", "DEN_CHUNK", "DEN_LOG_CHUNK"):
        k[name] = int(_one(r"constexpr int %s = (\d+);" % name, o, name))
    fast = _one(r"const bool fast = log_h >= (\d+) \+ DEN_LOG_CHUNK && \(row0 & \(size_t\((\d+) \* DEN_CHUNK\) - 1\)\) == 0;", o, "inv_denoms fast route")
    k["DEN_FAST_LOG"] = int(fast[0]) + k["DEN_LOG_CHUNK"]
    k["DEN_BLOCK"] = int(fast[1]) * k["DEN_CHUNK"]
    assert int(_one(r"size_t blocks = \(rows \+ (\d+) \* DEN_CHUNK - 1\) / \(\d+ \* DEN_CHUNK\);", o, "inv_denoms grid")) * k["DEN_CHUNK"] == k["DEN_BLOCK"]
    wide = _one(r"if \(height <= (\d+) && total_w >= (\d+) && !getenv\(\"MSAMD_NO_DEEP_WIDE\"\)\)", o, "wide reduced openings")
    k["WIDE_MAX_HEIGHT"], k["WIDE_MIN_WIDTH"] = int(wide[0]), int(wide[1])
    k["WIDE_SLICES"] = int(_one(r"for \(int sl = 1; sl < (\d+); sl\+\+\)", o, "wide slices"))
    k["DEEP_UNROLL"] = int(_one(r"for \(; c \+ (\d+) <= mw; c \+= \d+\)", o, "plain column loop"))
    k["LEAVES_MIN_HEIGHT"] = int(_one(r"if \(inputs\.empty\(\) && h >= (\d+) && prm\.max_log_arity == 1 && !getenv\(\"MSAMD_NO_DEEP_LEAVES\"\)\)", p,
                                      "leaf hashing in the reduced openings"))
    k["MAX_POINTS_PER_HEIGHT"] = int(_one(r"if \(local == (\d+)\) throw std::runtime_error\(\"pcs_open: more than two opening points at one LDE height\"\);",
                                          h, "points per height"))
    k["SIDE_MAX_LOG"] = int(_one(r"unsigned side_max_log = (\d+);", m, "side_max_log"))
    assert int(_one(r"side_max_log = v \? \(unsigned\)atoi\(v\) : (\d+)u;", c, "side_max_log default")) == k["SIDE_MAX_LOG"]
    _one(r"const size_t short_h = size_t\(1\) << \(ctx\.side_max_log \+ lb\);\n  const bool use_side = ctx\.side_enabled && gmax > short_h", p, "side stream")
    return k


REFUSAL_TEXT = "more than two opening points at one LDE height"

# ------------------------------------------------------------------ symbolic points
Point = namedtuple("Point", "base turn")


def pt(base, k=None, e=1):
    return Point(base, Fraction(0) if k is None else Fraction(e, 1 << k) % 1)


def times_g(p, k):
    return Point(p.base, (p.turn + Fraction(1, 1 << k)) % 1)


Z, A, B = pt("z"), pt("a"), pt("b")

# Params words: log_blowup, cap_height, log_final_poly_len, max_log_arity, num_queries, commit pow bits, query pow bits
Case = namedtuple("Case", "name params rounds refused knobs alternate")
Mat = namedtuple("Mat", "log_n width points")

KNOBS = {
    "none": {},
    "no_next": {"MSAMD_NO_NEXT_SHIFT": "1"},
    "no_batch": {"MSAMD_NO_BARY_BATCH": "1"},
    "no_leaves": {"MSAMD_NO_DEEP_LEAVES": "1"},
    "no_wide": {"MSAMD_NO_DEEP_WIDE": "1"},
    "side4": {"MSAMD_SIDE_MAX_LOG": "4"},
    "side4_side_delay": {"MSAMD_SIDE_MAX_LOG": "4", "MSAMD_SIDE_DELAY_US": "1500"},
    "side4_main_delay": {"MSAMD_SIDE_MAX_LOG": "4", "MSAMD_MAIN_DELAY_US": "1500"},
}
FOUR = ("none", "no_next", "no_batch", "no_leaves", "no_wide")
SIDE = ("side4", "side4_side_delay", "side4_main_delay")


# ------------------------------------------------------------------ the model
def plan(case, knob, k=None):
    """every host decision of pcs_open for one case under one knob, in the order the code takes them"""
    k = k or source_constants()
    env = KNOBS[knob]
    lb, max_log_arity = case.params[0], case.params[3]
    mats = [(ri, mi, m) for ri, r in enumerate(case.rounds) for mi, m in enumerate(r)]
    lde_log = {(ri, mi): m.log_n + lb for ri, mi, m in mats}
    gmax_log = max(lde_log.values())
    out = {}

    # is_next, then the demotion (a matrix of the same height opens the second point in its own right)
    allow_next = "MSAMD_NO_NEXT_SHIFT" not in env
    before = {}
    for ri, mi, m in mats:
        p = m.points
        before[ri, mi] = bool(allow_next and len(p) == 2 and p[1] == times_g(p[0], m.log_n) and p[0] != p[1])
    after = dict(before)
    for ri, mi, m in mats:
        if not after[ri, mi]:
            continue
        for rj, mj, q in mats:
            if lde_log[rj, mj] != lde_log[ri, mi]:
                continue
            for pj, z in enumerate(q.points):
                if not (pj == 1 and after[rj, mj]) and z == m.points[1]:
                    after[ri, mi] = False
    out["is_next_before"], out["is_next"] = before, after
    pair = {}
    for ri, mi, m in mats:
        p = m.points
        if len(p) != 2:
            continue
        pair[ri, mi] = ("next" if after[ri, mi] else "demoted" if before[ri, mi] else "suppressed" if not allow_next and p[1] == times_g(p[0], m.log_n)
                        and p[0] != p[1] else "coincident" if p[0] == p[1] else "reversed" if p[0] == times_g(p[1], m.log_n) else
                        "other generator" if p[0].base == p[1].base else "unrelated")
    out["pair"] = pair

    # unique points in the order of first notes, the tallest matrix at each, and whether a later note raised it
    upts, uh, raised, prefix = [], [], [], []
    for ri, mi, m in mats:
        for pi, z in enumerate(m.points):
            if pi == 1 and after[ri, mi]:
                continue
            if z not in upts:
                upts.append(z)
                uh.append(0)
                raised.append(False)
            i = upts.index(z)
            if uh[i] and lde_log[ri, mi] > uh[i]:
                raised[i] = True
            uh[i] = max(uh[i], lde_log[ri, mi])
    out["points"] = list(zip(upts, uh))
    out["raised_after_first_use"] = [z for z, r in zip(upts, raised) if r]
    for ri, mi, m in mats:
        for pi, z in enumerate(m.points):
            src = m.points[0] if pi == 1 and after[ri, mi] else z
            if uh[upts.index(src)] > lde_log[ri, mi]:
                prefix.append((ri, mi, pi))
    out["reads_a_prefix"] = prefix
    out["inv_denoms"] = [("fast" if h >= k["DEN_FAST_LOG"] else "slow", -(-(1 << h) // k["DEN_BLOCK"])) for h in uh]

    # the side stream
    side_max = int(env.get("MSAMD_SIDE_MAX_LOG", k["SIDE_MAX_LOG"]))
    short_log = side_max + lb
    use_side = gmax_log > short_log and any(lde_log[ri, mi] <= short_log and m.points for ri, mi, m in mats)
    out["use_side"] = use_side
    out["side_points"] = [z for z, h in zip(upts, uh) if use_side and h <= short_log]
    short_main = []
    for ri, mi, m in mats:
        if use_side and lde_log[ri, mi] <= short_log:
            for pi, z in enumerate(m.points):
                src = m.points[0] if pi == 1 and after[ri, mi] else z
                if uh[upts.index(src)] > short_log:
                    short_main.append((ri, mi, pi))
    out["short_matrix_reads_tall_point"] = short_main

    # opened values: row blocks, column groups, jobs per launch pair (one list per stream)
    rows_per_block = k["BARY_T"] * k["BARY_ROWS"]
    bary, launches, shifted = {}, [], False
    for on_side in (False, True):
        jobs, seen_mats = [], 0
        for ri, mi, m in mats:
            if m.points and (use_side and lde_log[ri, mi] <= short_log) == on_side:
                nblk = -(-(1 << m.log_n) // rows_per_block)
                bary[ri, mi] = {"nblk": nblk, "ngrp": -(-m.width // k["BARY_COLS"]), "ragged": m.width % k["BARY_COLS"] != 0,
                                "np": len(m.points), "next": after[ri, mi]}
                if len(jobs) != seen_mats:
                    shifted = True
                jobs.append((ri, mi))
            seen_mats += 1
        if "MSAMD_NO_BARY_BATCH" not in env:
            launches += [len(jobs[i: i + k["BARY_MAX_JOBS"]]) for i in range(0, len(jobs), k["BARY_MAX_JOBS"])]
    out["bary"], out["bary_launches"], out["job_index_differs_from_matrix_index"] = bary, launches, shifted
    out["bary_batched"] = "MSAMD_NO_BARY_BATCH" not in env

    # reduced openings per LDE height, tallest first: local points (a next-point counts as one), kernel, leaves
    heights, refused = {}, False
    for lh in sorted(set(lde_log.values()), reverse=True):
        local, total_w, listed = [], 0, 0
        for ri, mi, m in mats:
            if lde_log[ri, mi] != lh or not m.points:
                continue
            listed += 1
            total_w += m.width
            for pi, z in enumerate(m.points):
                nx = pi == 1 and after[ri, mi]
                gk = (upts.index(m.points[0] if nx else z), nx)
                if gk not in local:
                    local.append(gk)
        if len(local) > k["MAX_POINTS_PER_HEIGHT"]:
            refused = True
        tallest = lh == gmax_log
        if not listed:
            kernel, leaves = "memset", False
        else:
            kernel = "wide" if (1 << lh) <= k["WIDE_MAX_HEIGHT"] and total_w >= k["WIDE_MIN_WIDTH"] and "MSAMD_NO_DEEP_WIDE" not in env else "plain"
            leaves = tallest and (1 << lh) >= k["LEAVES_MIN_HEIGHT"] and max_log_arity == 1 and "MSAMD_NO_DEEP_LEAVES" not in env
        heights[lh] = {"points": len(local), "kernel": kernel, "leaves": leaves, "tallest": tallest, "total_w": total_w,
                       "widths": [m.width for ri, mi, m in mats if lde_log[ri, mi] == lh and m.points],
                       "shifted_point": any(nx for _, nx in local), "on_side": use_side and lh <= short_log}
    out["heights"], out["refused"] = heights, refused
    return out


# ------------------------------------------------------------------ the case table
P3 = ((2, 1, 1, 1, 15, 4, 5), (1, 0, 0, 1, 30, 0, 0), (3, 2, 2, 1, 9, 6, 0))  # test_pcs_commit_open_verify_mixed_rounds
FLAT = (1, 0, 0, 1, 8, 0, 0)       # dispatch cases: blow-up 2, few queries
WIDE_FOLD = (2, 0, 1, 3, 10, 2, 0)  # max_log_arity = 3
G10, G9, G7 = pt("z", 10), pt("z", 9), pt("z", 7)


def _rounds(*rounds):
    return tuple(tuple(Mat(ln, w, tuple(p)) for ln, w, p in r) for r in rounds)


def _case(name, params, rounds, refused=False, knobs=("none",), alternate=False):
    return Case(name, tuple(params), rounds, refused, tuple(knobs), alternate)


def _none_tallest(top):
    return _rounds([(top, 5, []), (7, 2, [Z, G7]), (top, 1, [])], [(9, 9, [Z, A])])


def point_structure_cases():
    """trace heights 2^10, 2^7, 2^10 | 2^9 with the widths of test_pcs_commit_open_verify_mixed_rounds"""
    t = {
        "unrelated": _rounds([(10, 5, [Z, A]), (7, 2, [Z]), (10, 1, [A, Z])], [(9, 9, [A, B])]),
        "demote": _rounds([(10, 5, [Z, G10]), (7, 2, [Z]), (10, 1, [G10])], [(9, 9, [Z, G9])]),
        "demote_swapped": _rounds([(10, 5, [G10]), (7, 2, [Z]), (10, 1, [Z, G10])], [(9, 9, [Z, G9])]),
        "demote_other_round": _rounds([(10, 5, [Z, G10]), (7, 2, [Z])], [(9, 9, [Z, G9]), (10, 1, [G10])]),
        "no_demotion_by_other_heights": _rounds([(10, 5, [Z, G10]), (7, 2, [G10]), (10, 1, [Z])], [(9, 9, [G10])]),
        # (z g, z) is no next pair; (z g^-1, z) is one, with first point z g^-1
        "reversed": _rounds([(10, 5, [G10, Z]), (7, 2, [Z]), (10, 1, [Z])], [(9, 9, [pt("z", 9, -1), Z])]),
        "reversed_inverse": _rounds([(10, 5, [pt("z", 10, -1), Z]), (7, 2, [Z]), (10, 1, [pt("z", 10, -1)])], [(9, 9, [Z, pt("z", 10, -1)])]),
        "generator_of_another_height": _rounds([(10, 5, [Z, G7]), (7, 2, [Z, G7]), (10, 1, [Z])], [(9, 9, [Z])]),
        # g of half and of twice the matrix's own height: neither is a next pair
        "generator_of_neighbouring_heights": _rounds([(10, 5, [Z, G9]), (7, 2, [Z]), (10, 1, [Z])], [(9, 9, [Z, G10])]),
        "none_on_one_matrix": _rounds([(10, 5, []), (7, 2, [Z]), (10, 1, [Z, G10])], [(9, 9, [Z, G9])]),
        "none_at_middle_height": _rounds([(10, 5, [Z, G10]), (7, 2, [Z]), (10, 1, [Z]), (9, 4, [])], [(9, 9, [])]),
        "none_at_tallest_height": _none_tallest(10),
        "none_on_first_round": _rounds([(10, 5, []), (7, 2, []), (10, 1, [])], [(9, 9, [Z, G9])]),
        "none_on_second_round": _rounds([(10, 5, [Z, G10]), (7, 2, [A]), (10, 1, [Z])], [(9, 9, [])]),
        "shared_point_tallest_last": _rounds([(7, 2, [Z]), (9, 9, [Z, A])], [(10, 5, [Z])]),
        "refuse_three_points": _rounds([(10, 5, [Z, A]), (7, 2, [Z]), (10, 1, [B])], [(9, 9, [Z])]),
        "refuse_pair_and_third": _rounds([(10, 5, [Z, G10]), (7, 2, [Z]), (10, 1, [A])], [(9, 9, [Z])]),
    }
    cases = []
    for name, rounds in t.items():
        for i, params in enumerate(P3):
            cases.append(_case("%s-p%d" % (name, i), params, rounds, refused=name.startswith("refuse")))
    # the tallest LDE at 2^13 rows (round 0's leaves would otherwise come from the reduced-opening pass)
    for i, params in enumerate(P3):
        knobs = FOUR if i == 1 else ("none",)
        cases.append(_case("none_at_tallest_height_13-p%d" % i, params, _none_tallest(13 - params[0]), knobs=knobs))
    # a one-row trace: g(0) = 1, the two points coincide. p3-fri refuses a matrix that is not taller than blowup * final
    # polynomial length, so the parameter sets keep a constant final polynomial
    for i, params in enumerate(((1, 0, 0, 1, 30, 0, 0), (2, 1, 0, 1, 15, 4, 5))):
        cases.append(_case("one_row-q%d" % i, params, _rounds([(10, 5, [Z, G10]), (0, 3, [Z, Z]), (10, 1, [Z])], [(9, 9, [Z, G9])])))
    return cases


def dispatch_cases():
    cases = []
    for lde in (12, 13, 14):  # slow, one full block, two blocks of inv_denoms, for two points of their own; row blocks 1 and 2
        for w in (1, 2, 3):
            knobs = FOUR if (lde, w) == (14, 3) else ("none",)
            cases.append(_case("lde%d_w%d" % (lde, w), FLAT, _rounds([(lde - 1, w, [Z, A]), (6, 2, [A])]), knobs=knobs))
    for w in (7, 8, 9, 17):  # the plain kernel's column loop: eight at a time, then one at a time
        cases.append(_case("columns_%d" % w, FLAT, _rounds([(8, w, [Z, pt("z", 8)]), (6, 3, [Z])])))
    # the wide kernel's slice loops: 16 slices, four columns of a slice at a time, then one
    five = [(4, 63, [Z, pt("z", 4)]), (4, 64, [Z]), (4, 65, [Z, pt("z", 4)]), (4, 130, [Z, pt("z", 4)]), (4, 400, [Z])]
    cases.append(_case("wide_slices", FLAT, _rounds(five)))
    cases.append(_case("wide_slices_reordered", FLAT, _rounds(five[::-1])))
    # the threshold total_w 511 / 512 at an LDE of 8192 rows: tallest, so leaves are on in both; with a taller narrow matrix, off
    for last in (12, 11):
        for pname, first, second in (("next", [Z, pt("z", 12)], [Z]), ("pair", [Z, A], [A])):
            base = [(12, 500, first), (12, last, second)]
            knobs = FOUR if (last, pname) == (12, "next") else ("none",)
            cases.append(_case("threshold_%d_%s" % (500 + last, pname), FLAT, _rounds(base), knobs=knobs))
            cases.append(_case("threshold_%d_%s_below_taller" % (500 + last, pname), FLAT, _rounds(base + [(13, 1, [Z])])))
    for n in (9, 17):  # more matrices than one batch launch takes
        lists = ([Z, A], [], [A])
        mats = [(4 + i % 3, 1 + i % 4, lists[(i + i // 3) % 3]) for i in range(n)]
        cases.append(_case("matrices_%d" % n, FLAT, _rounds(mats), knobs=FOUR if n == 17 else ("none",)))
    # short matrices on the side stream
    cases.append(_case("side_tall_point", FLAT, _rounds([(10, 3, [Z, G10]), (3, 2, [Z]), (4, 5, [Z, pt("z", 4)])]), knobs=SIDE, alternate=True))
    cases.append(_case("side_own_point", FLAT, _rounds([(10, 3, [Z, G10]), (3, 2, [A]), (4, 5, [A, B])]), knobs=SIDE, alternate=True))
    ps = {c.name: c for c in point_structure_cases()}
    cases.append(_case("wide_fold_unrelated", WIDE_FOLD, ps["unrelated-p0"].rounds))
    cases.append(_case("wide_fold_unrelated_13", WIDE_FOLD, _rounds([(11, 5, [Z, A]), (7, 2, [Z]), (11, 1, [A, Z])], [(9, 9, [A, B])])))
    cases.append(_case("wide_fold_none_at_tallest", WIDE_FOLD, ps["none_at_tallest_height-p0"].rounds))
    return cases


def _with_knobs(cases):
    out = []
    for c in cases:
        if c.name == "demote-p2":  # (blow-up 8: the 2^10-row traces have 8192-row LDEs, leaves on)
            c = c._replace(knobs=FOUR)
        out.append(c)
    return out


CASES = _with_knobs(point_structure_cases()) + dispatch_cases()
RUNS = [(c, knob) for c in CASES for knob in c.knobs]


def run_id(run):
    return run[0].name if run[1] == "none" else "%s-%s" % (run[0].name, run[1])
