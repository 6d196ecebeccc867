"""Pcs::open of the BabyBear / Poseidon2 configuration on its own (msbb_pcs_open: csrc/bb_prover.hip pcs_open), against the
oracle compiled for that configuration - the first PCS-level differential test in this field; tests/test_gpu_bb_level2.py
drives the entry point with the prover's points only. The opening keys everything by point (denominators, weights) and by
LDE height (the running column count of the reduced openings); it has no limit on the points per height, no next-point
shortcut and no side stream, so the cases are the point structures alone: unrelated pairs, three points at one height, no
points on a matrix / a height / the tallest height / a round, a one-row trace, one point across heights, and a 2^14-row
column (two row chunks of the barycentric sums), over parameter sets with and without caps, wide folds and commit proof of
work, so both the device-driven and the host-driven FRI rounds run.

Per case: extend each matrix (msbb_coset_lde_batch), commit the LDEs on both sides (msbb_mmcs_commit yields the handle
msbb_pcs_open takes; equal caps), sample z, a, b on both transcripts, open on both: equal opened values, equal FRI bytes,
equal transcript state. This field has no library-side PCS verifier: the oracle's accepts the device's output and rejects
it with one word flipped in the opened values of any one matrix."""
import zlib

import numpy as np
import pytest

import oracle_bb as ob
from __graft_entry__ import load_package
from pcs_plan_model import A, B, Z, pt

pytestmark = pytest.mark.gpu
pkg = load_package()
fe = pkg.frontend
bb = pkg.babybear
P = fe.BABYBEAR["P"]
K = fe.poseidon2_constants()


@pytest.fixture(scope="module")
def ctx():
    c = pkg.Context(0)
    bb.set_poseidon2(c, K)
    ob.set_poseidon2(K)
    return c


def rand_field(rng, shape):
    v = rng.integers(0, P, shape, dtype=np.uint64)
    edge = np.array([0, 1, 2, P - 1, P - 2, 1 << 27, (1 << 27) + 1], dtype=np.uint64)
    mask = rng.random(shape) < 0.1
    return np.where(mask, edge[rng.integers(0, len(edge), shape)], v)


def _gen(bits):
    """BabyBear::two_adic_generator(bits): 0x1a427a41 has order 2^27"""
    g = 0x1A427A41
    for _ in range(27 - bits):
        g = g * g % P
    return g


# log_blowup, cap_height, log_final_poly_len, max_log_arity, num_queries, commit pow bits, query pow bits
PARAMS = {
    "plain": (1, 0, 0, 1, 20, 0, 0),         # root-only, no proof of work: the FRI rounds run on the device transcript
    "cap_pow": (2, 1, 1, 1, 12, 3, 5),       # caps and commit proof of work: host-driven rounds
    "arity3": (1, 0, 0, 3, 12, 0, 2),        # wide folds on the device transcript
    "arity3_cap_pow": (2, 1, 0, 3, 10, 2, 0),  # wide folds, host-driven
}
G10, G9, G7 = pt("z", 10), pt("z", 9), pt("z", 7)
# rounds of (log2 rows of the trace, width, points): the heights and widths of test_pcs_commit_open_verify_mixed_rounds
CASES = {
    "prover_pattern": [[(10, 5, [Z, G10]), (7, 2, [Z, G7]), (10, 1, [Z])], [(9, 9, [Z, G9])]],
    "unrelated": [[(10, 5, [Z, A]), (7, 2, [Z]), (10, 1, [A, Z])], [(9, 9, [A, B])]],
    "second_point_first_elsewhere": [[(10, 5, [Z, A]), (7, 2, [A, Z]), (10, 1, [B, A])], [(9, 9, [B])]],
    "three_points_at_one_height": [[(10, 5, [Z, A]), (7, 2, [Z]), (10, 1, [B])], [(9, 9, [Z])]],
    "pair_and_third_at_one_height": [[(10, 5, [Z, G10]), (7, 2, [Z]), (10, 1, [A])], [(9, 9, [Z])]],
    "four_points_at_one_height": [[(10, 5, [Z, G10]), (7, 2, [Z]), (10, 1, [A, B])], [(9, 9, [Z, A]), (10, 3, [B, Z])]],
    "none_on_one_matrix": [[(10, 5, []), (7, 2, [Z]), (10, 1, [Z, G10])], [(9, 9, [Z, G9])]],
    "none_at_middle_height": [[(10, 5, [Z, G10]), (7, 2, [Z]), (10, 1, [Z]), (9, 4, [])], [(9, 9, [])]],
    "none_at_tallest_height": [[(10, 5, []), (7, 2, [Z, G7]), (10, 1, [])], [(9, 9, [Z, A])]],
    "none_on_first_round": [[(10, 5, []), (7, 2, []), (10, 1, [])], [(9, 9, [Z, G9])]],
    "none_on_second_round": [[(10, 5, [Z, G10]), (7, 2, [A]), (10, 1, [Z])], [(9, 9, [])]],
    "shared_point_tallest_last": [[(7, 2, [Z]), (9, 9, [Z, A])], [(10, 5, [Z])]],
    "one_row": [[(10, 5, [Z, G10]), (0, 3, [Z, Z]), (10, 1, [Z])], [(9, 9, [Z, G9])]],
    "two_row_chunks": [[(14, 1, [Z, A]), (6, 2, [A])]],
}


def _runs():
    out = []
    for name in CASES:
        for pname, words in PARAMS.items():
            if name == "one_row" and words[2]:
                continue  # p3-fri refuses a matrix that is not taller than blowup * final polynomial length
            if name == "two_row_chunks" and pname != "plain":
                continue  # (the one large shape: once)
            out.append((name, pname))
    return out


_systems = {}


def _system(ctx, pname):
    """any small system on the context supplies the parameters (and the permutation) of msbb_pcs_open"""
    if pname not in _systems:
        with fe.field(fe.BABYBEAR):
            params = fe.Params(*PARAMS[pname])
            _systems[pname] = (bb.System.new(ctx, params, fe.mul_air_inputs(), K), params)
    return _systems[pname]


def _value(p, base):
    z = base[p.base]
    if not p.turn:
        return z
    g = pow(_gen(p.turn.denominator.bit_length() - 1), p.turn.numerator, P)
    return tuple(x * g % P for x in z)


def _words(cap_bytes):
    return np.frombuffer(cap_bytes, dtype=np.uint32)


def _sample(ch):
    return {"z": ch.sample_ext(), "a": ch.sample_ext(), "b": ch.sample_ext()}


def _assert_same_bytes(got, want, what):
    same = got == want
    where = "" if same else "lengths %d / %d" % (len(got), len(want)) if len(got) != len(want) else "first at byte %d" % next(
        i for i in range(len(got)) if got[i] != want[i])
    assert same, "%s: bytes differ, %s" % (what, where)


@pytest.mark.parametrize("name,pname", _runs(), ids=lambda v: v)
def test_open_at_free_points(ctx, name, pname):
    system, params = _system(ctx, pname)
    rounds = CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    g_rounds, o_rounds = [], []
    for r in rounds:
        ldes = [bb.coset_lde_batch(ctx, rand_field(rng, (1 << ln, w)), params.log_blowup) for ln, w, _ in r]
        g, o = bb.Mmcs(ctx, ldes, params.cap_height), ob.Mmcs(ldes, params.cap_height)
        assert np.array_equal(g.cap, _words(o.cap))
        g_rounds.append(g)
        o_rounds.append(o)
    gc, oc = bb.Challenger(system), ob.Challenger.for_params(params)
    for g, o in zip(g_rounds, o_rounds):
        gc.observe_digests(g.cap)
        oc.observe_digests(o.cap)
    base = _sample(gc)
    assert base == _sample(oc)
    pts = [[[_value(p, base) for p in ps] for _, _, ps in r] for r in rounds]
    widths = [[w for _, w, _ in r] for r in rounds]
    o_open, o_fri = ob.pcs_open(params, list(zip(o_rounds, pts)), oc)
    g_open, g_fri = bb.pcs_open(system, [(g, ws, per) for g, ws, per in zip(g_rounds, widths, pts)], gc)
    g_open = g_open.astype(np.uint64)
    if not np.array_equal(g_open, o_open):
        bad = np.flatnonzero(g_open != o_open) if g_open.shape == o_open.shape else []
        raise AssertionError("opened values differ (%d of %d words, first at word %s)" % (len(bad), o_open.size, bad[:1]))
    _assert_same_bytes(g_fri, o_fri, "FriProof")
    assert gc.sample_bits(20) == oc.sample_bits(20), "the transcripts end in different states"
    desc = [(o.cap, [(ln, w) for ln, w, _ in r], per) for o, r, per in zip(o_rounds, rounds, pts)]

    def fresh():
        c = ob.Challenger.for_params(params)
        for o in o_rounds:
            c.observe_digests(o.cap)
        assert _sample(c) == base
        return c

    assert ob.pcs_verify(params, desc, g_open, g_fri, fresh()), "the oracle's verifier rejects the device's opening"
    off = 0
    for r in rounds:
        for _, w, ps in r:
            if ps:
                bad = g_open.copy()
                bad[off] ^= 1
                assert not ob.pcs_verify(params, desc, bad, g_fri, fresh()), "flipped word %d: the oracle's verifier accepts" % off
            off += 4 * len(ps) * w


def test_more_than_two_points_on_one_matrix_are_refused(ctx):
    """the limit this field does have (include/mstark_bb.h): two points per matrix; the context and the system survive"""
    system, params = _system(ctx, "plain")
    lde = bb.coset_lde_batch(ctx, rand_field(np.random.default_rng(3), (32, 2)), params.log_blowup)
    g = bb.Mmcs(ctx, [lde], params.cap_height)
    ch = bb.Challenger(system)
    ch.observe_digests(g.cap)
    base = _sample(ch)
    with pytest.raises(pkg.MstarkError, match="at most two opening points per matrix"):
        bb.pcs_open(system, [(g, [2], [[base["z"], base["a"], base["b"]]])], ch)
    o = ob.Mmcs([lde], params.cap_height)
    gc, oc = bb.Challenger(system), ob.Challenger.for_params(params)
    gc.observe_digests(g.cap)
    oc.observe_digests(o.cap)
    assert _sample(gc) == _sample(oc) == base
    pts = [[[base["a"], base["b"]]]]
    g_open, g_fri = bb.pcs_open(system, [(g, [2], pts[0])], gc)
    o_open, o_fri = ob.pcs_open(params, [(o, pts[0])], oc)
    assert np.array_equal(g_open.astype(np.uint64), o_open)
    _assert_same_bytes(g_fri, o_fri, "FriProof after a refused call")
