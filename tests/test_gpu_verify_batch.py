"""Batched verification on the device: ms_mmcs_verify_batch (one thread per Merkle opening) and ms_verify_batch (N proofs of
one system: host transcript replay, then the per-query arithmetic and every Merkle path in two launches). The reference is
always ms_verify on the same bytes, proof by proof, and the oracle's verifier where it is named. Every corrupted input is
expected to give a verdict; nothing here depends on a fault."""
import os
import sys

import numpy as np
import pytest

import proof_codec as pc
from conftest import rand_field
from test_reference_verifier_cases import EXPECT, _tamper_cases

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from fuzz_verifier import mutate  # noqa: E402

pytestmark = pytest.mark.gpu
P = 0xFFFFFFFF00000001

# ---------------------------------------------------------------- kernel level: ms_mmcs_verify_batch

SHAPES = [[(1, 3)], [(2, 1)], [(8, 7)], [(8, 8)], [(8, 9)], [(4, 127)], [(4, 128)], [(4, 129)], [(4, 257)],
          [(8, 3), (8, 5), (4, 2), (1, 7)], [(16, 2), (2, 300)]]


def _commit(pkg, ctx, shapes, cap_height, seed=5):
    rng = np.random.default_rng(seed)
    mats = [rand_field(rng, (h, w)) for h, w in shapes]
    m = pkg.Mmcs(ctx, mats, cap_height)
    maxh = max(h for h, _ in shapes)
    opened = [m.open(i) for i in range(maxh)]
    return mats, m, maxh, opened


def _run(m, idx, opened):
    return m.verify_batch(idx, [o[0] for o in opened], [o[1] for o in opened]).tolist()


@pytest.mark.parametrize("which_cap", ["0", "1", "log_max"])
@pytest.mark.parametrize("shapes", SHAPES, ids=lambda s: "-".join("%dx%d" % hw for hw in s))
def test_mmcs_verify_batch(pkg, ctx, oracle, shapes, which_cap):
    maxh = max(h for h, _ in shapes)
    log_max = maxh.bit_length() - 1
    cap_height = {"0": 0, "1": 1, "log_max": log_max}[which_cap]
    if cap_height > log_max:
        cap_height = log_max  # (the one-row commitments: a cap cannot be taller than the tree)
    mats, m, maxh, opened = _commit(pkg, ctx, shapes, cap_height)
    path = log_max - cap_height
    idx = list(range(maxh))
    got = _run(m, idx, opened)
    om = oracle.Mmcs(mats, cap_height)
    assert m.cap == om.cap
    ref = [1 if om.verify(i, opened[i][0], opened[i][1]) else 0 for i in idx]
    assert got == ref
    reachable = all(h >= (maxh >> path) for h, _ in shapes)  # a matrix below the cap layer is never injected: every opening refused
    assert got == [1 if reachable else 0] * maxh
    if shapes in ([(8, 3), (8, 5), (4, 2), (1, 7)], [(16, 2), (2, 300)]):  # the oracle's own openings are the same bytes
        for i in idx:
            ov, op = om.open(i)
            assert ov.tolist() == opened[i][0].tolist() and op == opened[i][1]
    if not reachable:
        return
    widths = [w for _, w in shapes]
    order = sorted(range(len(shapes)), key=lambda i: -shapes[i][0])  # stable, descending height
    col0 = np.concatenate([[0], np.cumsum(widths)]).astype(int)
    last = maxh - 1

    def tampered(k, f):
        t = [(v.copy(), bytearray(p)) for v, p in opened]
        f(t[k])
        return [(v, bytes(p)) for v, p in t]

    def only(k):
        return [0 if i == k else 1 for i in idx]

    def flip_val(col):
        def f(o):
            o[0][col] ^= np.uint64(1)
        return f

    for k in {0, last}:
        assert _run(m, idx, tampered(k, flip_val(col0[order[0]]))) == only(k), "value of the tallest group"
        short = [i for i in order if shapes[i][0] < maxh]
        if short:
            assert _run(m, idx, tampered(k, flip_val(col0[short[-1] + 1] - 1))) == only(k), "value of an injected group"
        if path:
            def lo(o):
                o[1][0] ^= 1

            def hi(o):
                o[1][32 * (path - 1) + 31] ^= 0x80
            assert _run(m, idx, tampered(k, lo)) == only(k), "lowest sibling"
            assert _run(m, idx, tampered(k, hi)) == only(k), "highest sibling"
    cap = bytearray(m.cap)
    cap[3] ^= 4  # cap entry 0: the openings below it are refused, the others are not
    hs = [h for h, _ in shapes]
    got = pkg.mmcs_verify_batch(ctx, bytes(cap), len(cap) // 32, hs, widths, idx, [o[0] for o in opened], [o[1] for o in opened]).tolist()
    assert got == [0 if (i >> path) == 0 else 1 for i in idx]
    if maxh > 1:  # a right opening under a wrong index
        wrong = idx[:]
        wrong[0] = 1
        assert _run(m, wrong, opened) == only(0)
        wrong[0] = maxh  # beyond the tree
        assert _run(m, wrong, opened) == only(0)


def test_mmcs_verify_batch_counts(pkg, ctx):
    """0 openings; 65 and 257 (a wavefront and a 256-thread block boundary), by repeating indices"""
    shapes = [(8, 3), (8, 5), (4, 2), (1, 7)]
    mats, m, maxh, opened = _commit(pkg, ctx, shapes, 0)
    assert m.verify_batch([], [], []).tolist() == []
    for n in (65, 257):
        idx = [i % maxh for i in range(n)]
        ops = [opened[i] for i in idx]
        assert _run(m, idx, ops) == [1] * n
        bad = [(v.copy(), p) for v, p in ops]
        bad[n - 1][0][0] ^= np.uint64(2)
        bad[63][0][9] ^= np.uint64(1)
        assert _run(m, idx, bad) == [0 if i in (63, n - 1) else 1 for i in range(n)]


# ---------------------------------------------------------------- whole proofs: ms_verify_batch

def _prove(g, fe, traces, claims):
    packed = fe.pack_claims(claims)
    return packed, g.prove_multiple_claims(g.witness(traces, packed)).to_bytes()


def _check(g, items, o=None, expect=None):
    """the batch against ms_verify one by one (and the oracle where given); returns the verdicts"""
    got = g.verify_batch(items)
    ref = [g.verify(c, p) for c, p in items]
    assert got == ref
    if o is not None:
        assert got == [o.verify(c, p) for c, p in items]
    if expect is not None:
        assert got == expect
    return got


_CACHE = {}


def _u32(pkg, ctx, fe, params, adds, key):
    """(system, packed claims, proof) of the u32_add + byte table system, proved once per parameter set"""
    k = (key, adds)
    if k not in _CACHE:
        if ("sys", key) not in _CACHE:
            _CACHE[("sys", key)] = pkg.System.new(ctx, params, fe.u32_add_system_inputs())
        g = _CACHE[("sys", key)]
        t, c = fe.u32_add_bench_witness(adds)
        _CACHE[k] = (g,) + _prove(g, fe, t, c)
    return _CACHE[k]


def test_valid_u32_add_bench_params(pkg, ctx, oracle, fe):
    g, c16, p16 = _u32(pkg, ctx, fe, fe.bench_params(), 1 << 4, "bench")
    _, c128, p128 = _u32(pkg, ctx, fe, fe.bench_params(), 1 << 7, "bench")
    o = oracle.System(g.blob)
    _check(g, [(c128, p128)], o, [0])
    _check(g, [(c16, p16), (c128, p128)], o, [0, 0])
    _check(g, [(c16, p16), (c128, p128), (c16, p16)] * 11, None, [0] * 33)


def test_valid_other_systems(pkg, ctx, oracle, fe):
    packed0 = fe.pack_claims([])
    # even/odd lookups with a claim; the same with an inactive circuit
    for with_dead in (False, True):
        g = pkg.System.new(ctx, fe.test_params(), fe.even_odd_inputs(with_dead=with_dead))
        traces = fe.even_odd_traces() + ([np.zeros((0, 6), dtype=np.uint64)] if with_dead else [])
        c, p = _prove(g, fe, traces, [[0, 4, 1]])
        _check(g, [(c, p)] * 2, oracle.System(g.blob), [0, 0])
    # a preprocessed trace (squares); a single circuit at 2^4 and 2^7 rows in one batch: the number of FRI rounds differs
    g = pkg.System.new(ctx, fe.test_params(), fe.squares_inputs())
    items = [_prove(g, fe, fe.squares_traces(n), []) for n in (16, 128)]
    _check(g, items, oracle.System(g.blob), [0, 0])
    g = pkg.System.new(ctx, fe.test_params(), fe.pythagorean_inputs())
    items = [_prove(g, fe, [fe.pythagorean_trace(n)], []) for n in (16, 128, 64)]
    _check(g, items, oracle.System(g.blob), [0, 0, 0])
    # the verifier's own test system (quotient degree 2), 4 + 2 rows and 16-row traces
    g = pkg.System.new(ctx, fe.test_params(), fe.verifier_test_inputs())
    items = [(packed0, g.prove_multiple_claims(g.witness(fe.verifier_test_traces(d), packed0)).to_bytes()) for d in (0, 4)]
    _check(g, items, oracle.System(g.blob), [0, 0])


def test_unopened_matrix_row_width_differs_between_queries(pkg, ctx, fe):
    """The one proof shape the flat device layout cannot hold. System: even_odd_inputs() plus the preprocessed byte table of
    squares_inputs() as a third, inactive circuit (even_odd_inputs(with_dead=True)'s dead circuit has no preprocessed trace),
    under test_params(). The table's committed matrix is opened at no point, so only its Merkle path binds the row a query
    shows for it. One zero word is appended to that row in the second query only, and the proof sits between two untouched
    ones in one call. BLAKE3 takes the length in: the collector refuses on the host what ms_verify refuses by hashing (2)."""
    g = pkg.System.new(ctx, fe.test_params(), fe.even_odd_inputs() + [fe.squares_inputs()[0]])
    c, p = _prove(g, fe, fe.even_odd_traces() + [np.zeros((0, 1), dtype=np.uint64)], [[0, 4, 1]])
    t = pc.parse(p)
    assert t["active"] == [1, 1, 0] and t["preprocessed_opened_values"] == [[]]
    rows = t["opening_proof"]["query_proofs"][1]["input_proof"][-1]["opened_values"]  # the preprocessed round comes last
    assert [len(r) for r in rows] == [1]
    rows[0].append(0)
    items = [(c, p), (c, pc.serialize(t)), (c, p)]
    got, ref = g.verify_batch(items), [g.verify(ci, pi) for ci, pi in items]
    print("width-mismatch proof (Goldilocks): ms_verify %d, ms_verify_batch %d" % (ref[1], got[1]))
    assert got == ref
    assert got[0] == 0 and got[2] == 0


VARIANTS = {
    "caps_final": dict(log_blowup=2, cap_height=2, log_final_poly_len=2, num_queries=10, commit_proof_of_work_bits=3, query_proof_of_work_bits=4),
    "arity2": dict(log_blowup=1, cap_height=1, log_final_poly_len=1, max_log_arity=2, num_queries=10, commit_proof_of_work_bits=2,
                   query_proof_of_work_bits=2),
    "arity3": dict(log_blowup=2, max_log_arity=3, num_queries=12, commit_proof_of_work_bits=3, query_proof_of_work_bits=4),
    "arity6": dict(log_blowup=2, max_log_arity=6, num_queries=8),  # the byte table is 2^8 rows: the first round folds 64 values
    "blowup1": dict(log_blowup=1, num_queries=16),
}


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_parameter_variants(pkg, ctx, oracle, fe, name):
    params = fe.Params(**VARIANTS[name])
    g, c, p = _u32(pkg, ctx, fe, params, 1 << 7, name)
    _, c2, p2 = _u32(pkg, ctx, fe, params, 1 << 4, name)
    if name == "arity6":
        assert 6 in [s["log_arity"] for s in pc.parse(p)["opening_proof"]["query_proofs"][0]["commit_phase_openings"]]
    _check(g, [(c, p), (c2, p2), (c, p)], oracle.System(g.blob), [0, 0, 0])


def _bump(x):
    return (x + 1) % P


def _flip(d, byte=0):
    b = bytearray(d)
    b[byte] ^= 1
    return bytes(b)


def _field_tampers(proof, q):
    """name -> tampered bytes, in query `q`"""
    out = {}

    def case(name, f):
        t = pc.parse(proof)
        f(t, t["opening_proof"], t["opening_proof"]["query_proofs"][q])
        out["%s[q%d]" % (name, q)] = pc.serialize(t)

    n_in = len(pc.parse(proof)["opening_proof"]["query_proofs"][q]["input_proof"])
    for r in range(n_in):
        def val(t, f, qp, r=r):
            qp["input_proof"][r]["opened_values"][-1][0] = _bump(qp["input_proof"][r]["opened_values"][-1][0])
        case("input value, round %d" % r, val)
    case("lowest input sibling", lambda t, f, qp: qp["input_proof"][0]["proof"].__setitem__(0, _flip(qp["input_proof"][0]["proof"][0])))
    case("highest input sibling", lambda t, f, qp: qp["input_proof"][1]["proof"].__setitem__(-1, _flip(qp["input_proof"][1]["proof"][-1], 31)))
    for which in (0, -1):
        def sib(t, f, qp, which=which):
            qp["commit_phase_openings"][which]["sibling_values"][-1][1] = _bump(qp["commit_phase_openings"][which]["sibling_values"][-1][1])
        case("FRI sibling value, round %d" % which, sib)
    case("FRI path digest", lambda t, f, qp: qp["commit_phase_openings"][0]["proof"].__setitem__(0, _flip(qp["commit_phase_openings"][0]["proof"][0], 7)))
    return out


def _global_tampers(proof):
    out = {}

    def case(name, f, verdict=None):
        t = pc.parse(proof)
        f(t, t["opening_proof"])
        out[name] = (pc.serialize(t), verdict)

    case("final polynomial", lambda t, f: f["final_poly"][-1].__setitem__(0, _bump(f["final_poly"][-1][0])), 2)
    case("commit-phase proof-of-work witness", lambda t, f: f["commit_pow_witnesses"].__setitem__(0, _bump(f["commit_pow_witnesses"][0])), 2)
    case("query proof-of-work witness", lambda t, f: f.__setitem__("query_pow_witness", _bump(f["query_pow_witness"])), 2)
    case("commit-phase cap", lambda t, f: f["commit_phase_commits"][-1].__setitem__(0, _flip(f["commit_phase_commits"][-1][0], 5)), 2)
    case("opened value at zeta", lambda t, f: t["stage_2_opened_values"][0][0][0].__setitem__(0, _bump(t["stage_2_opened_values"][0][0][0][0])), 2)
    case("last accumulator", lambda t, f: t["intermediate_accumulators"].__setitem__(-1, [1, 0]), 6)
    case("log_degrees too long", lambda t, f: t["log_degrees"].append(3), 3)
    return out


@pytest.mark.parametrize("name", ["bench", "arity3"])
def test_fieldwise_tampering(pkg, ctx, oracle, fe, name):
    """Each tampered proof sits in one slot of a batch of otherwise valid proofs; arity 1 (bench parameters) and arity 3.
    A quotient opened value that passes the opening but fails the constraint check (verdict 5) cannot be made with the codec:
    any change of an opened value changes the reduced opening the FRI fold chain starts from, and a consistent forgery would
    need a new commitment, i.e. the prover - the case is dropped as the issue allows."""
    params = fe.bench_params() if name == "bench" else fe.Params(**VARIANTS["arity3"])
    g, c, p = _u32(pkg, ctx, fe, params, 1 << 7, name)
    o = oracle.System(g.blob)
    nq = params.num_queries
    bad, want = [], []
    for q in (0, nq - 1):
        for nm, b in _field_tampers(p, q).items():
            bad.append((nm, b))
            want.append(2)
    for nm, (b, v) in _global_tampers(p).items():
        bad.append((nm, b))
        want.append(v)
    items, expect = [], []
    for (nm, b), v in zip(bad, want):  # valid, tampered, valid, tampered ... valid
        items += [(c, p), (c, b)]
        expect += [0, v]
    items.append((c, p))
    expect.append(0)
    got = _check(g, items, o)
    assert got == expect, [(bad[i // 2][0], got[i], expect[i]) for i in range(1, len(got), 2) if got[i] != expect[i]]


def test_reference_tamper_cases(pkg, ctx, oracle, fe):
    g = pkg.System.new(ctx, fe.test_params(), fe.verifier_test_inputs())
    packed = fe.pack_claims([])
    proof = g.prove_multiple_claims(g.witness(fe.verifier_test_traces(0), packed)).to_bytes()
    cases = _tamper_cases(proof)
    names = sorted(cases)
    items = [(fe.pack_claims(cases[n][1]), cases[n][0]) for n in names]
    items.insert(3, (packed, proof))
    got = _check(g, items, oracle.System(g.blob))
    assert got.pop(3) == 0
    for n, v in zip(names, got):
        assert v != 0, n
        if EXPECT[n] is not None:
            assert v == EXPECT[n], (n, v)


FUZZ_SEED = 20260


@pytest.mark.parametrize("name", ["bench", "arity3", "caps_final"])
def test_mutation_fuzz(pkg, ctx, oracle, fe, name):
    params = fe.bench_params() if name == "bench" else fe.Params(**VARIANTS[name])
    g, c, p = _u32(pkg, ctx, fe, params, 1 << 7, name)
    o = oracle.System(g.blob)
    rng = np.random.default_rng(FUZZ_SEED)
    rejected = total = 0
    for _ in range(6):
        muts = [mutate(rng, p) for _ in range(16)]
        items = [(c, m) for m in muts] + [(c, p)]
        got = g.verify_batch(items)  # (raises unless the call returned MS_OK)
        ref = [g.verify(cc, m) for cc, m in items]
        assert got == ref
        assert [v == 0 for v in got] == [o.verify(cc, m) == 0 for cc, m in items]
        assert got[-1] == 0
        rejected += sum(1 for v in ref[:-1] if v != 0)
        total += 16
    assert total == 96 and rejected >= 0.9 * total, "the seed exercises too few rejections: %d of %d" % (rejected, total)
    ctx.sync()
    assert g.verify_batch([(c, p)] * 3) == [0, 0, 0]


def test_claims(pkg, ctx, oracle, fe):
    g, c_small, p_small = _u32(pkg, ctx, fe, fe.bench_params(), 1 << 7, "bench")
    t, cl = fe.u32_add_bench_witness(1 << 12)
    c_big, p_big = _prove(g, fe, t, cl)
    offs, data = c_big
    assert 1 + (len(offs) - 1) + len(data) > 8192  # the transcript words of the claims: above the device threshold
    assert 1 + (len(c_small[0]) - 1) + len(c_small[1]) <= 8192
    o = oracle.System(g.blob)
    _check(g, [(c_big, p_big), (c_small, p_small)], o, [0, 0])
    wrong = fe.pack_claims([[1, 2, 3, 6]])
    got = _check(g, [(c_small, p_small), (wrong, p_small), (c_big, p_big), (c_small, p_big)], o)
    assert got[0] == 0 and got[2] == 0 and got[1] != 0 and got[3] != 0
    # an empty claim list (n_claims[i] = 0)
    g2 = pkg.System.new(ctx, fe.test_params(), fe.pythagorean_inputs())
    c0, p0 = _prove(g2, fe, [fe.pythagorean_trace(16)], [])
    assert len(c0[0]) == 1
    _check(g2, [(c0, p0), (c0, p0)], oracle.System(g2.blob), [0, 0])


def test_host_waits_do_not_grow_with_the_batch(pkg, ctx, fe):
    g = pkg.System.new(ctx, fe.test_params(), fe.even_odd_inputs())
    c, p = _prove(g, fe, fe.even_odd_traces(), [[0, 4, 1]])
    g.verify_batch([(c, p)] * 32)  # (the staging buffer has its final size)
    waits = []
    for n in (1, 32):
        before = ctx.sync_count()
        assert g.verify_batch([(c, p)] * n) == [0] * n
        waits.append(ctx.sync_count() - before)
    assert waits[0] == waits[1]


def test_edges(pkg, ctx, fe):
    g = pkg.System.new(ctx, fe.test_params(), fe.pythagorean_inputs())
    c, p = _prove(g, fe, [fe.pythagorean_trace(16)], [])
    assert g.verify_batch([]) == []
    assert _check(g, [(c, p), (c, b""), (c, p), (c, p[:7]), (c, p)]) == [0, 3, 0, 3, 0]
    assert g.verify_batch([(c, p)] * 64) == [0] * 64
