"""Batched verification on the device for the BabyBear / Poseidon2 configuration: msbb_mmcs_verify_batch (one thread per
Merkle opening, the Poseidon2 sponge inside the thread) and msbb_verify_batch (N proofs of one system: host transcript
replay, then the per-query arithmetic and every Merkle path in two launches). The reference is always msbb_verify on the
same bytes, proof by proof, and the oracle's verifier for accept / reject. Every corrupted input is expected to give a
verdict; nothing here depends on a fault."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import oracle_bb as ob
import proof_codec as pc
from __graft_entry__ import load_package
from test_gpu_verify_batch import VARIANTS

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from fuzz_verifier import mutate  # noqa: E402  (byte-level mutations: the element size does not matter to it)

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


# ---------------------------------------------------------------- kernel level: msbb_mmcs_verify_batch

# widths around the sponge rate of 8 (a short block, an exact block, one word into the next), mixed heights with
# injected groups, a one-row matrix
SHAPES = [[(8, 1)], [(8, 7)], [(8, 8)], [(8, 9)], [(8, 16)], [(8, 17)], [(64, 8), (64, 9), (16, 1)], [(256, 24), (128, 3), (2, 17)], [(1, 5)]]


def _run(m, idx, opened):
    return m.verify_batch(idx, [o[0] for o in opened], [o[1] for o in opened]).tolist()


@pytest.mark.parametrize("which_cap", ["0", "1", "log_max"])
@pytest.mark.parametrize("shapes", SHAPES, ids=lambda s: "-".join("%dx%d" % hw for hw in s))
def test_mmcs_verify_batch(ctx, shapes, which_cap):
    maxh = max(h for h, _ in shapes)
    log_max = maxh.bit_length() - 1
    cap_height = min({"0": 0, "1": 1, "log_max": log_max}[which_cap], log_max)  # (a cap cannot be taller than the tree)
    if which_cap == "1" and log_max == 0:
        cap_height = 0
    path = log_max - cap_height
    rng = np.random.default_rng(100 * len(shapes) + cap_height)
    mats = [rand_field(rng, s) for s in shapes]
    m, om = bb.Mmcs(ctx, mats, cap_height), ob.Mmcs(mats, cap_height)
    assert np.array_equal(m.cap, np.frombuffer(om.cap, dtype=np.uint32))
    if maxh <= 64:
        idx = list(range(maxh))
    else:
        idx = sorted({0, maxh - 1} | {int(x) for x in rng.integers(0, maxh, 10)})
    opened = [m.open(i) for i in idx]
    for i, (v, p) in zip(idx[:3] + idx[-1:], opened[:3] + opened[-1:]):  # the oracle opens the same words
        ov, op = om.open(i)
        assert np.array_equal(v, ov) and np.array_equal(p, np.frombuffer(op, dtype=np.uint32)), i
    reachable = all(h >= (maxh >> path) for h, _ in shapes)  # a matrix below the cap layer is never injected: every opening refused
    assert _run(m, idx, opened) == [1 if reachable else 0] * len(idx)
    if not reachable:
        return

    # one of each tamper in ONE call, each at its own position between untouched openings
    n = len(idx)
    widths = [w for _, w in shapes]
    tampers = []

    def add(name, f):
        tampers.append((name, f))

    def val_plus_one(i, v, p):
        v[0] = (int(v[0]) + 1) % P
        return i, v, p
    add("value + 1", val_plus_one)

    def last_val_plus_one(i, v, p):
        v[-1] = (int(v[-1]) + 1) % P
        return i, v, p
    add("last value + 1 (the lowest group)", last_val_plus_one)

    def val_p(i, v, p):
        v[len(v) // 2] = P
        return i, v, p
    add("value = p", val_p)
    if path:
        def sib_plus_one(i, v, p):
            p[8 * (path - 1) + 3] = (int(p[8 * (path - 1) + 3]) + 1) % P
            return i, v, p
        add("sibling word + 1", sib_plus_one)

        def sib_p(i, v, p):
            p[0] = P
            return i, v, p
        add("sibling word = p", sib_p)
    if maxh > 1:
        add("index ^ 1", lambda i, v, p: (i ^ 1, v, p))
    add("index = max height", lambda i, v, p: (maxh, v, p))
    if len(shapes) > 1 and shapes[0][0] == shapes[1][0]:
        def swap(i, v, p):
            w0, w1 = widths[0], widths[1]
            return i, np.concatenate([v[w0:w0 + w1], v[:w0], v[w0 + w1:]]), p
        add("rows of two equal-height matrices swapped", swap)
    bi, bo, want, names = [], [], [], []
    for k, (name, f) in enumerate(tampers):
        for src, tam in ((k % n, None), ((3 * k + 1) % n, f)):
            i, (v, p) = idx[src], opened[src]
            v, p = v.copy(), p.copy()
            if tam:
                i, v, p = tam(i, v, p)
            bi.append(i), bo.append((v, p)), want.append(0 if tam else 1), names.append(name if tam else "untouched")
    bi.append(idx[-1]), bo.append(opened[-1]), want.append(1), names.append("untouched")
    got = _run(m, bi, bo)
    assert got == want, [(nm, g, w) for nm, g, w in zip(names, got, want) if g != w]


def test_mmcs_verify_batch_counts(ctx):
    """0 openings; 257 openings (a 256-thread block boundary) by repeating indices; the free function with a wrong cap"""
    shapes = [(8, 3), (8, 5), (4, 2), (1, 7)]
    rng = np.random.default_rng(9)
    mats = [rand_field(rng, s) for s in shapes]
    m = bb.Mmcs(ctx, mats, 0)
    assert m.verify_batch([], [], []).tolist() == []
    hs0 = np.array([8], dtype=np.uint64)
    assert pkg.lib().msbb_mmcs_verify_batch(ctx.h, C.c_size_t(1), hs0.ctypes.data_as(bb.u64p), hs0.ctypes.data_as(bb.u64p), None, C.c_uint32(0),
                                            C.c_size_t(0), None, None, None, None) == 0  # n_openings = 0 is MS_OK
    opened = [m.open(i) for i in range(8)]
    idx = [i % 8 for i in range(257)]
    ops = [(opened[i][0].copy(), opened[i][1].copy()) for i in idx]
    assert _run(m, idx, ops) == [1] * 257
    ops[256][0][0] ^= np.uint32(2)
    ops[255][1][5] ^= np.uint32(1)
    ops[63][0][9] ^= np.uint32(1)
    assert _run(m, idx, ops) == [0 if i in (63, 255, 256) else 1 for i in range(257)]
    cap = m.cap.copy()
    cap[2] = (int(cap[2]) + 1) % P
    hs = [h for h, _ in shapes]
    assert bb.mmcs_verify_batch(ctx, cap, 1, hs, m.widths, idx[:8], [o[0] for o in opened], [o[1] for o in opened]).tolist() == [0] * 8
    assert bb.mmcs_verify_batch(ctx, m.cap, 1, hs, m.widths, idx[:8], [o[0] for o in opened], [o[1] for o in opened]).tolist() == [1] * 8


# ---------------------------------------------------------------- whole proofs: msbb_verify_batch

_CACHE = {}


def _system(ctx, key, params, inputs_fn):
    if ("sys", key) not in _CACHE:
        with fe.field(fe.BABYBEAR):
            _CACHE[("sys", key)] = bb.System.new(ctx, params, inputs_fn(), K)
    return _CACHE[("sys", key)]


def _prove(g, traces, claims):
    with fe.field(fe.BABYBEAR):
        packed = fe.pack_claims(claims)
    return packed, g.prove_multiple_claims(g.witness(traces, packed)).to_bytes()


def _mul(ctx, key, params, log_rows):
    """(system, packed claims, proof) of the MulAir at 2^log_rows rows, proved once per parameter set and height"""
    k = ("mul", key, log_rows)
    if k not in _CACHE:
        g = _system(ctx, ("mul", key), params, fe.mul_air_inputs)
        with fe.field(fe.BABYBEAR):
            trace = fe.mul_air_trace(1 << log_rows)
        _CACHE[k] = (g,) + _prove(g, [trace], [])
    return _CACHE[k]


def _u32(ctx, key, params, adds):
    k = ("u32", key, adds)
    if k not in _CACHE:
        g = _system(ctx, ("u32", key), params, fe.u32_add_system_inputs)
        with fe.field(fe.BABYBEAR):
            t, c = fe.u32_add_bench_witness(adds)
        _CACHE[k] = (g,) + _prove(g, t, c)
    return _CACHE[k]


def _check(g, items, expect=None):
    """the batch against msbb_verify one by one, exactly; accept / reject against the oracle; returns the verdicts"""
    got = g.verify_batch(items)
    ref = [g.verify(c, p) for c, p in items]
    assert got == ref
    o = ob.System(g.blob)
    assert [v == 0 for v in got] == [o.verify(c, p) == 0 for c, p in items]
    if expect is not None:
        assert got == expect
    return got


def test_valid_mul_air_heights(ctx):
    """2^2, 2^4 and 2^7 rows in one batch: the number of FRI rounds differs per proof; 33 items cross a 256-thread block"""
    three = [_mul(ctx, "test", fe.test_params(), lr) for lr in (2, 4, 7)]
    g = three[0][0]
    items = [(c, p) for _, c, p in three]
    _check(g, items, [0, 0, 0])
    assert g.verify_batch((items * 11)) == [0] * 33


def test_valid_other_systems(ctx):
    for with_dead in (False, True):
        g = _system(ctx, ("evenodd", with_dead), fe.test_params(), lambda: fe.even_odd_inputs(with_dead=with_dead))
        with fe.field(fe.BABYBEAR):
            traces = fe.even_odd_traces() + ([np.zeros((0, 6), dtype=np.uint64)] if with_dead else [])
        c, p = _prove(g, traces, [[0, 4, 1]])
        _check(g, [(c, p)] * 2, [0, 0])
    g, c, p = _u32(ctx, "mixed", fe.Params(2, 0, 0, 1, 20, 2, 2), 1 << 4)  # preprocessed byte table, mixed heights
    _check(g, [(c, p)] * 2, [0, 0])
    g = _system(ctx, "squares", fe.Params(2, 1, 1, 1, 10, 0, 0), fe.squares_inputs)  # quotient degree 2
    with fe.field(fe.BABYBEAR):
        traces = fe.squares_traces(16)
    c, p = _prove(g, traces, [])
    _check(g, [(c, p)] * 2, [0, 0])


def test_unopened_matrix_row_width_differs_between_queries(ctx):
    """The one proof shape the flat device layout cannot hold (COLLECT_HOST). System: even_odd_inputs() plus the preprocessed
    byte table of squares_inputs() as a third, inactive circuit (even_odd_inputs(with_dead=True)'s dead circuit has no
    preprocessed trace), under test_params(). The table's committed matrix is opened at no point, so only its Merkle path
    binds the row a query shows for it. One zero word is appended to that row in the second query only, and the proof sits
    between two untouched ones in one call. The padding-free sponge hashes [x] and [x, 0] to one digest, so msbb_verify may
    accept the proof; whatever it says, the batch says the same (it runs pcs_verify on the host for this proof)."""
    g = _system(ctx, "evenodd+dead table", fe.test_params(), lambda: fe.even_odd_inputs() + [fe.squares_inputs()[0]])
    with fe.field(fe.BABYBEAR):
        traces = fe.even_odd_traces() + [np.zeros((0, 1), dtype=np.uint64)]
    c, p = _prove(g, traces, [[0, 4, 1]])
    t = pc.parse(p, 4, 4)
    assert t["active"] == [1, 1, 0] and t["preprocessed_opened_values"] == [[]]
    rows = t["opening_proof"]["query_proofs"][1]["input_proof"][-1]["opened_values"]  # the preprocessed round comes last
    assert [len(r) for r in rows] == [1]
    rows[0].append(0)
    items = [(c, p), (c, pc.serialize(t, 4, 4)), (c, p)]
    got, ref = g.verify_batch(items), [g.verify(ci, pi) for ci, pi in items]
    print("width-mismatch proof (BabyBear): msbb_verify %d, msbb_verify_batch %d" % (ref[1], got[1]))
    assert got == ref
    assert got[0] == 0 and got[2] == 0


@pytest.mark.parametrize("name", ["caps_final", "arity2", "arity3", "blowup1"])
def test_parameter_variants(ctx, name):
    g, c, p = _mul(ctx, name, fe.Params(**VARIANTS[name]), 7)
    _check(g, [(c, p)] * 3, [0, 0, 0])


def test_arity6(ctx):
    """The u32_add system under max_log_arity = 6. At 2^4 additions the schedule is [4, 4]: the roll-in of the 2^4-row
    trace (LDE 2^6) stops the first round of the 2^8-row byte table (LDE 2^10) after 16 values, so no round folds 64 there.
    At 2^7 additions it is [1, 6, 1]; both proofs are in the batch and the 64-value fold is asserted on the second."""
    g, c4, p4 = _u32(ctx, "arity6", fe.Params(**VARIANTS["arity6"]), 1 << 4)
    _, c7, p7 = _u32(ctx, "arity6", fe.Params(**VARIANTS["arity6"]), 1 << 7)
    arities = [[s["log_arity"] for s in pc.parse(p, 4, 4)["opening_proof"]["query_proofs"][0]["commit_phase_openings"]] for p in (p4, p7)]
    assert arities[0] == [4, 4] and 6 in arities[1], arities
    _check(g, [(c4, p4), (c7, p7), (c4, p4)], [0, 0, 0])


def _bump(x):
    return (x + 1) % P


def _bump_digest(d, word):
    w = np.frombuffer(d, dtype=np.uint32).copy()
    w[word] = _bump(int(w[word]))
    return w.tobytes()


def _query_tampers(proof, q):
    """name -> bytes tampered inside query proof `q` only: nothing the transcript absorbs changes"""
    out = {}

    def case(name, f):
        t = pc.parse(proof, 4, 4)
        f(t["opening_proof"]["query_proofs"][q])
        out["%s [query %d]" % (name, q)] = pc.serialize(t, 4, 4)

    n_in = len(pc.parse(proof, 4, 4)["opening_proof"]["query_proofs"][q]["input_proof"])
    for r in range(n_in):
        def val(qp, r=r):
            qp["input_proof"][r]["opened_values"][-1][0] = _bump(qp["input_proof"][r]["opened_values"][-1][0])
        case("opened input row value, round %d" % r, val)
    case("lowest input path digest", lambda qp: qp["input_proof"][0]["proof"].__setitem__(0, _bump_digest(qp["input_proof"][0]["proof"][0], 0)))
    case("highest input path digest", lambda qp: qp["input_proof"][n_in - 1]["proof"].__setitem__(-1, _bump_digest(qp["input_proof"][n_in - 1]["proof"][-1], 7)))
    for coord in range(4):
        def sib(qp, coord=coord):
            step = qp["commit_phase_openings"][0 if coord % 2 == 0 else -1]
            step["sibling_values"][-1][coord] = _bump(step["sibling_values"][-1][coord])
        case("FRI sibling coordinate %d" % coord, sib)
    case("FRI path digest", lambda qp: qp["commit_phase_openings"][0]["proof"].__setitem__(0, _bump_digest(qp["commit_phase_openings"][0]["proof"][0], 5)))
    return out


@pytest.mark.parametrize("name", ["binary", "arity3"])
def test_tampering_inside_query_proofs(ctx, name):
    """Query-proof contents are never absorbed by the transcript: these pass every host check and only the kernels can
    refuse them. Both proof-of-work widths are 0, so no tamper can be caught by a witness either. First, a middle and the
    last query, so that a wrong per-query stride shows."""
    if name == "binary":
        params = fe.Params(1, 0, 0, 1, 9, 0, 0)
    else:
        params = fe.Params(**dict(VARIANTS["arity3"], commit_proof_of_work_bits=0, query_proof_of_work_bits=0))
    g, c, p = _mul(ctx, "tamper-" + name, params, 7)
    nq = params.num_queries
    steps = pc.parse(p, 4, 4)["opening_proof"]["query_proofs"][0]["commit_phase_openings"]
    assert (3 in [s["log_arity"] for s in steps]) == (name == "arity3")
    items, expect, names = [(c, p)], [0], ["untouched"]
    for q in (0, nq // 2, nq - 1):
        for nm, b in _query_tampers(p, q).items():
            items += [(c, b), (c, p)]
            expect += [2, 0]
            names += [nm, "untouched"]
    got = _check(g, items)
    assert got == expect, [(n, a, b) for n, a, b in zip(names, got, expect) if a != b]


def test_tampered_final_polynomial(ctx):
    """absorbed by the transcript, so the query indices move and any layer may refuse it: never accepted, same verdict"""
    g, c, p = _mul(ctx, "tamper-binary", fe.Params(1, 0, 0, 1, 9, 0, 0), 7)
    t = pc.parse(p, 4, 4)
    t["opening_proof"]["final_poly"][-1][2] = _bump(t["opening_proof"]["final_poly"][-1][2])
    got = _check(g, [(c, p), (c, pc.serialize(t, 4, 4)), (c, p)])
    assert got[0] == 0 and got[2] == 0 and got[1] != 0


def test_host_refused_inputs_among_good_ones(ctx):
    g = _system(ctx, ("evenodd", False), fe.test_params(), fe.even_odd_inputs)
    with fe.field(fe.BABYBEAR):
        traces = fe.even_odd_traces()
        wrong, none, twice = fe.pack_claims([[0, 4, 0]]), fe.pack_claims([]), fe.pack_claims([[0, 4, 1], [0, 4, 1]])
    c, p = _prove(g, traces, [[0, 4, 1]])

    def tamper(f):
        t = pc.parse(p, 4, 4)
        f(t, t["opening_proof"])
        return pc.serialize(t, 4, 4)

    bad = [
        ("truncated", c, p[: len(p) // 2]),
        ("five trailing bytes", c, p + b"\1\2\3\4\5"),
        ("a field word >= p", c, tamper(lambda t, f: f["final_poly"][0].__setitem__(1, P))),
        ("wrong log_arity", c, tamper(lambda t, f: f["query_proofs"][1]["commit_phase_openings"][0].__setitem__("log_arity", 2))),
        ("one query missing", c, tamper(lambda t, f: f["query_proofs"].pop())),
        ("wrong claim", wrong, p),
        ("no claim", none, p),
        ("claim twice", twice, p),
    ]
    items, names = [(c, p)], ["untouched"]
    for nm, cl, b in bad:
        items += [(cl, b), (c, p)]
        names += [nm, "untouched"]
    got = _check(g, items)
    for nm, v in zip(names, got):
        assert (v == 0) == (nm == "untouched"), (nm, v)
    # the reference's own tamper (baby_bear_config.rs:199-203) on its one-circuit system: the channel no longer balances
    g1, c1, p1 = _mul(ctx, "test", fe.test_params(), 2)
    t = pc.parse(p1, 4, 4)
    t["intermediate_accumulators"][0][0] = (t["intermediate_accumulators"][0][0] + (1 << 32) % P) % P
    _check(g1, [(c1, p1), (c1, pc.serialize(t, 4, 4)), (c1, p1)], [0, 6, 0])


def test_mutation_fuzz(ctx):
    """200 mutations of one proof in ONE call, element-wise equal to msbb_verify"""
    g = _system(ctx, "fuzz", fe.Params(2, 1, 1, 1, 9, 3, 4), fe.even_odd_inputs)
    with fe.field(fe.BABYBEAR):
        traces = fe.even_odd_traces()
    c, p = _prove(g, traces, [[0, 4, 1]])
    rng = np.random.default_rng(20261)
    muts = [mutate(rng, p) for _ in range(200)]
    items = [(c, m) for m in muts] + [(c, p)]
    got = g.verify_batch(items)  # (raises unless the call returned MS_OK)
    ref = [g.verify(cc, m) for cc, m in items]
    assert got == ref
    assert got[-1] == 0
    assert sum(1 for v in got[:-1] if v != 0) >= 150, "the seed exercises too few rejections"
    assert g.verify_batch([(c, p)] * 3) == [0, 0, 0]


def test_host_waits_do_not_grow_with_the_batch(ctx):
    g, c, p = _mul(ctx, "test", fe.test_params(), 4)
    g.verify_batch([(c, p)] * 16)  # (the staging buffer has its final size)
    waits = []
    for n in (1, 16):
        before = ctx.sync_count()
        assert g.verify_batch([(c, p)] * n) == [0] * n
        waits.append(ctx.sync_count() - before)
    assert waits[0] == waits[1]


def test_edges(ctx):
    g, c, p = _mul(ctx, "test", fe.test_params(), 2)
    assert g.verify_batch([]) == []
    assert _check(g, [(c, p), (c, b""), (c, p), (c, p[:7]), (c, p)]) == [0, 3, 0, 3, 0]
    # a null proof pointer is an error of the call, not a verdict
    lens, ncl = np.array([len(p)], dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    verdicts = np.full(1, -1, dtype=np.int32)
    rc = pkg.lib().msbb_verify_batch(g.h, C.c_size_t(1), ncl.ctypes.data_as(bb.u64p), None, None, (bb.u8p * 1)(), lens.ctypes.data_as(bb.u64p),
                                     verdicts.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == -1 and verdicts[0] == -1
    buf = np.frombuffer(p, dtype=np.uint8)
    rc = pkg.lib().msbb_verify_batch(g.h, C.c_size_t(1), ncl.ctypes.data_as(bb.u64p), None, None, (bb.u8p * 1)(buf.ctypes.data_as(bb.u8p)),
                                     lens.ctypes.data_as(bb.u64p), None)
    assert rc == -1
    # a system created on another context verifies on its own context
    c2 = pkg.Context(0)
    with fe.field(fe.BABYBEAR):
        g2 = bb.System.new(c2, fe.test_params(), fe.mul_air_inputs(), K)
    assert g2.verify_batch([(c, p), (c, p[:-1]), (c, p)]) == [0, 3, 0]
    assert g.verify_batch([(c, p)]) == [0]


@pytest.mark.parametrize("total,num_queries,copies", [(255, 85, 3), (256, 64, 4), (257, 257, 1)])
def test_block_edge(ctx, total, num_queries, copies):
    """the batch's query count at the 256-thread block edge; the last query of the last proof is the one tampered with"""
    assert num_queries * copies == total
    params = fe.Params(1, 0, 0, 1, num_queries, 0, 0)
    g, c, p = _mul(ctx, "edge%d" % num_queries, params, 4)
    t = pc.parse(p, 4, 4)
    qp = t["opening_proof"]["query_proofs"][-1]
    qp["commit_phase_openings"][-1]["sibling_values"][0][0] = _bump(qp["commit_phase_openings"][-1]["sibling_values"][0][0])
    bad = pc.serialize(t, 4, 4)
    _check(g, [(c, p)] * copies, [0] * copies)
    _check(g, [(c, p)] * (copies - 1) + [(c, bad)], [0] * (copies - 1) + [2])
