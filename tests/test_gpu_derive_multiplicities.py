"""`-m gpu`: ms_witness_derive_multiplicities (csrc/multiplicity.hip) against the model of tests/multiplicity_model.py, which
tests/test_multiplicity_model.py pins to the witness builders' own counting. Every case is device against model: the derived
columns read back through w.trace(c), and every field of the report, compared exactly. The witnesses come from that module,
built once and left unchanged. Shapes: 16 additions are one workgroup block of messages, 128 additions (1 664 circuit messages +
128 claims) the smallest shape with more than one 1 024-message block, 4 096 the largest."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the library opens the device)

import multiplicity_model as mm
from test_multiplicity_model import cases, code2_inputs, garbage, model_of, system_of

pytestmark = pytest.mark.gpu
P = mm.P
_SYS, _PROOF = {}, {}


def system(pkg, fe, ctx, inputs):
    """the device system of a list of circuit inputs, built once"""
    key = id(inputs)
    if key not in _SYS:
        _SYS[key] = (pkg.System.new(ctx, fe.test_params(), inputs), inputs)
    return _SYS[key][0]


def upload(s, traces, packed, route):
    """held: ms_witness_create (from_stage_1 keeps lookup values); device: torch tensors through ms_witness_create_device"""
    if route == "held":
        return s.witness(traces, packed)
    tensors = [None if t is None or len(t) == 0 else torch.from_numpy(np.ascontiguousarray(t).view(np.int64)).cuda() for t in traces]
    return s.witness_from_device(tensors, packed)


def against_model(oracle, fe, s, inputs, traces, claims, targets, route="held", entries=64):
    """upload `traces`, derive on the device and in the model, compare the report and every trace -> (witness, report, model traces)"""
    osys, comp = system_of(oracle, fe, inputs)
    packed = fe.pack_claims(claims)
    want, m = mm.derive(osys, comp, traces, packed, targets, entries)
    w = upload(s, traces, packed, route)
    rep = w.derive_multiplicities(targets, entries=entries)
    assert rep.fields() == m.fields(), str(rep)
    assert rep.ok == m.ok
    for c, t in enumerate(want):
        if t is not None:
            assert np.array_equal(w.trace(c), t), "trace of circuit %d" % c
    return w, rep, want


@pytest.mark.parametrize("route", ["held", "device"])
@pytest.mark.parametrize("fill", [0, 7])
@pytest.mark.parametrize("n", [16, 128, 4096])
def test_byte_table_of_u32_add(pkg, fe, ctx, oracle, n, fill, route):
    name = "u32_%d" % n
    inputs, traces, claims, targets = cases(fe)[name]
    s = system(pkg, fe, ctx, inputs)
    _, comp = system_of(oracle, fe, inputs)
    packed = fe.pack_claims(claims)
    w = upload(s, garbage(traces, comp, targets, fill), packed, route)
    rep = w.derive_multiplicities(targets)
    _, m = model_of(oracle, fe, name)
    assert rep.fields() == m.fields() and rep.ok, str(rep)
    assert np.array_equal(w.trace(0), traces[0]) and np.array_equal(w.trace(1), traces[1])  # the builder's bincount trace
    assert w.lookup_balance().ok and w.check().verdict == 0
    if n not in _PROOF:
        _PROOF[n] = s.prove_multiple_claims(s.witness(traces, packed)).to_bytes()
    proof = s.prove_multiple_claims(w).to_bytes()
    assert proof == _PROOF[n] and s.verify_multiple_claims(packed, proof) == 0


def test_byte_operations_four_targets_demand_from_ragged_claims(pkg, fe, ctx, oracle):
    inputs, traces, claims, targets = cases(fe)["byte_ops"]
    s = system(pkg, fe, ctx, inputs)
    _, comp = system_of(oracle, fe, inputs)
    w = s.witness(garbage(traces, comp, targets), fe.pack_claims(claims))
    rep = w.derive_multiplicities(targets)
    _, m = model_of(oracle, fe, "byte_ops")
    assert rep.fields() == m.fields() and rep.ok and rep.duplicates == 0, str(rep)
    assert np.array_equal(w.trace(0), traces[0])  # byte_operations_witness
    assert w.lookup_balance().ok


def table_inputs(fe, pre):
    return fe.CircuitInputs(1, np.array(pre, dtype=np.uint64).reshape(-1, 1), [], [], [fe.Lookup.pull(fe.Expr.main(0), [fe.Expr.preprocessed(0)])])


def pusher_inputs(fe):
    """[value, multiplicity]: push(main(1), [main(0)])"""
    return fe.CircuitInputs(2, None, [], [], [fe.Lookup.push(fe.Expr.main(1), [fe.Expr.main(0)])])


def custom(fe, name):
    """circuit inputs of the hand-made systems, built once (the systems are cached by their identity)"""
    key = "custom_" + name
    made = cases(fe)
    if key not in made:
        E = fe.Expr
        made[key] = {
            "dup": lambda: [table_inputs(fe, [0, 1, 1, 2]), pusher_inputs(fe)],
            "push": lambda: [fe.CircuitInputs(1, np.array([[5], [6], [7], [8]], dtype=np.uint64), [], [], [fe.Lookup.push(E.main(0), [E.preprocessed(0)])]),
                             fe.CircuitInputs(2, None, [], [], [fe.Lookup.pull(E.main(1), [E.main(0)])])],
            "two": lambda: [table_inputs(fe, [0, 1, 2, 3]), table_inputs(fe, [0, 1, 2, 3]), pusher_inputs(fe)],
            "inactive": lambda: [fe.CircuitInputs(2, None, [], [], [fe.Lookup.pull(E.main(0), [E.main(1)])]), pusher_inputs(fe)],
            "code2": lambda: code2_inputs(fe),
        }[name]()
    return made[key]


def test_duplicate_table_rows(pkg, fe, ctx, oracle):
    inputs = custom(fe, "dup")
    traces = [np.full((4, 1), 9, dtype=np.uint64), np.array([[1, 1], [1, 1], [1, 1], [0, 0]], dtype=np.uint64)]
    w, rep, _ = against_model(oracle, fe, system(pkg, fe, ctx, inputs), inputs, traces, [], [(0, 0)])
    assert w.trace(0)[:, 0].tolist() == [0, 3, 0, 0]  # row 1 serves the three pushes of 1, row 2 repeats its tuple
    assert (rep.demand_messages, rep.demand_groups, rep.served, rep.unserved, rep.duplicates) == (3, 1, 1, 0, 1)
    assert w.lookup_balance().ok


def unserved_case(fe):
    """the 16-addition witness with the byte cell (row 5, column 2) set to 300; claim 5 follows the row's word, so that the
    u32 tuples of claim and row still cancel and the byte message (0, 300) is the one thing no table row serves"""
    inputs, traces, claims, targets = cases(fe)["u32_16"]
    traces = [t.copy() for t in traces]
    traces[1][5, 2] = 300
    claims = [list(c) for c in claims]
    claims[5][1] = sum(int(traces[1][5, k]) << (8 * k) for k in range(4))
    return inputs, traces, claims, targets


def test_unserved_demand_is_named(pkg, fe, ctx, oracle):
    inputs, traces, claims, targets = unserved_case(fe)
    s = system(pkg, fe, ctx, inputs)
    w, rep, want = against_model(oracle, fe, s, inputs, traces, claims, targets)
    assert rep.unserved == 1 and not rep.ok
    assert rep.entries[0].fields() == ((1, 5, 3), 1, 1, [0, 300])  # circuit 1, row 5, slot 3 = push(1, [0, main(2)])
    assert np.array_equal(w.trace(0), want[0]) and not w.lookup_balance().ok
    assert "unserved (0, 300): net 1 over 1 message, first at circuit 1 row 5 lookup 3" in str(rep)
    _, counts, _ = against_model(oracle, fe, s, inputs, traces, claims, targets, entries=0)
    assert counts.entries == [] and counts.fields()[:5] == rep.fields()[:5]


def test_push_signed_target_and_large_multiplicities(pkg, fe, ctx, oracle):
    inputs = custom(fe, "push")
    big = 1 << 40
    traces = [np.full((4, 1), 7, dtype=np.uint64), np.array([[5, 1], [6, P - 1], [7, big], [5, big]], dtype=np.uint64)]
    w, rep, _ = against_model(oracle, fe, system(pkg, fe, ctx, inputs), inputs, traces, [], [(0, 0)])
    # pulls of 1 + 2^40, of p - 1 (= a push of 1) and of 2^40; the provider pushes v = p - D
    assert w.trace(0)[:, 0].tolist() == [1 + big, P - 1, big, 0]
    assert (rep.demand_messages, rep.demand_groups, rep.served, rep.unserved, rep.duplicates) == (4, 3, 3, 0, 0)
    assert w.lookup_balance().ok and not (w.check().verdict & pkg.CHECK_LOOKUPS)
    assert s_mult(pkg, fe, ctx, inputs, 0, 0) == {"eligibility": 0, "column": 0, "pull": False}


def s_mult(pkg, fe, ctx, inputs, c, j):
    return system(pkg, fe, ctx, inputs).multiplicity_slot(c, j)


def test_two_tables_compete_for_the_same_tuples(pkg, fe, ctx, oracle):
    inputs = custom(fe, "two")
    traces = [np.full((4, 1), 7, dtype=np.uint64), np.full((4, 1), 7, dtype=np.uint64),
              np.array([[0, 2], [1, 1], [3, 5], [3, 1]], dtype=np.uint64)]
    w, rep, _ = against_model(oracle, fe, system(pkg, fe, ctx, inputs), inputs, traces, [], [(1, 0), (0, 0)])
    assert w.trace(0)[:, 0].tolist() == [2, 1, 0, 6] and w.trace(1)[:, 0].tolist() == [0, 0, 0, 0]
    assert (rep.served, rep.unserved, rep.duplicates) == (3, 0, 4) and w.lookup_balance().ok


def test_inactive_target_circuit_and_no_targets(pkg, fe, ctx, oracle):
    inputs = custom(fe, "inactive")
    traces = [None, np.array([[4, 1], [4, 1], [9, 2], [0, 0]], dtype=np.uint64)]
    w, rep, _ = against_model(oracle, fe, system(pkg, fe, ctx, inputs), inputs, traces, [], [(0, 0)])
    assert (rep.demand_messages, rep.demand_groups, rep.served, rep.unserved) == (3, 2, 0, 2) and w.trace(0).size == 0
    assert [e.fields() for e in rep.entries] == [((1, 0, 0), 2, 2, [4]), ((1, 2, 0), 2, 1, [9])]
    # no targets: a pure count; the table's own (garbage) messages are demand like any other, and nothing is written
    inputs, traces, claims, targets = cases(fe)["u32_16"]
    _, comp = system_of(oracle, fe, inputs)
    g = garbage(traces, comp, targets, 7)
    w, rep, _ = against_model(oracle, fe, system(pkg, fe, ctx, inputs), inputs, g, claims, [])
    assert rep.served == 0 and rep.unserved > 0 and np.array_equal(w.trace(0), g[0]) and np.array_equal(w.trace(1), g[1])


def test_idempotence_isolation_and_host_waits(pkg, fe, ctx, oracle):
    inputs, traces, claims, targets = cases(fe)["u32_128"]
    s = system(pkg, fe, ctx, inputs)
    _, comp = system_of(oracle, fe, inputs)
    packed = fe.pack_claims(claims)
    g = garbage(traces, comp, targets)
    w = s.witness(g, packed)
    bg = ((3, 5), (7, 11))
    claims_before = w.claims_accumulator(*bg)
    n0 = ctx.sync_count()
    first = w.derive_multiplicities(targets)
    assert ctx.sync_count() - n0 == 1  # nothing unserved: one host wait
    once = [w.trace(c) for c in range(2)]
    second = w.derive_multiplicities(targets)
    twice = [w.trace(c) for c in range(2)]
    assert first.fields() == second.fields() and all(np.array_equal(a, b) for a, b in zip(once, twice))
    assert np.array_equal(once[1], g[1]) and w.claims_accumulator(*bg) == claims_before  # the other trace and the claims
    # a witness the generator already filled is left as it is
    w = s.bench_witness_on_device(1 << 10)
    before = [w.trace(c) for c in range(2)]
    proof = s.prove_multiple_claims(w).to_bytes()
    rep = w.derive_multiplicities(targets)
    assert rep.ok and rep.fields() == model_of(oracle, fe, "u32_bench_1024")[1].fields()
    assert all(np.array_equal(a, w.trace(c)) for c, a in enumerate(before)) and s.prove_multiple_claims(w).to_bytes() == proof
    # unserved demand with room for entries: one more wait
    inputs, traces, claims, targets = unserved_case(fe)
    w = s.witness(traces, fe.pack_claims(claims))
    n0 = ctx.sync_count()
    assert w.derive_multiplicities(targets).unserved == 1 and ctx.sync_count() - n0 == 2
    n0 = ctx.sync_count()
    assert w.derive_multiplicities(targets, entries=0).unserved == 1 and ctx.sync_count() - n0 == 1


def test_long_probe_chains_give_the_same_report_and_bytes(pkg, fe, ctx, oracle, monkeypatch):
    inputs, traces, claims, targets = unserved_case(fe)
    s = system(pkg, fe, ctx, inputs)
    w, plain, want = against_model(oracle, fe, s, inputs, traces, claims, targets)
    monkeypatch.setenv("MSAMD_LB_HASH_BITS", "0")  # every probe sequence starts at slot 0
    w2, chained, _ = against_model(oracle, fe, s, inputs, traces, claims, targets)
    assert chained.fields() == plain.fields() and np.array_equal(w.trace(0), w2.trace(0))
    inputs = custom(fe, "two")  # target tuples nobody demands meet in one chain too
    traces = [np.full((4, 1), 7, dtype=np.uint64), np.full((4, 1), 7, dtype=np.uint64), np.array([[0, 2], [1, 1], [3, 5], [3, 1]], dtype=np.uint64)]
    _, rep, _ = against_model(oracle, fe, system(pkg, fe, ctx, inputs), inputs, traces, [], [(0, 0), (1, 0)])
    assert rep.duplicates == 4


def test_multiplicity_slot_agrees_with_the_model(pkg, fe, ctx, oracle):
    for inputs in (cases(fe)["u32_16"][0], cases(fe)["squares_16"][0], custom(fe, "code2")):
        s = system(pkg, fe, ctx, inputs)
        _, comp = system_of(oracle, fe, inputs)
        for c, cc in enumerate(comp):
            for j in range(len(cc.lookups)):
                code, col, pull = mm.classify(cc, j)
                assert s.multiplicity_slot(c, j) == {"eligibility": code, "column": col, "pull": pull}, (c, j)
    with pytest.raises(pkg.MstarkError, match="out of range"):
        s.multiplicity_slot(0, 99)


def test_misuse_is_an_error_and_the_context_stays_usable(pkg, fe, ctx, oracle):
    inputs, traces, claims, targets = cases(fe)["u32_16"]
    s = system(pkg, fe, ctx, inputs)
    packed = fe.pack_claims(claims)
    with pytest.raises(pkg.MstarkError, match="device-resident"):
        s.host_witness(traces, packed).derive_multiplicities(targets)
    w = s.witness(traces, packed)
    for bad, text in (([(1, 1)], "not eligible"), ([(0, 0), (0, 0)], "shares the derived column"), ([(2, 0)], "out of range"),
                      ([(0, 1)], "out of range")):
        with pytest.raises(pkg.MstarkError, match=text):
            w.derive_multiplicities(bad)
        assert np.array_equal(w.trace(0), traces[0])  # refused before anything was written
    L = pkg.lib()
    u64p = C.POINTER(C.c_uint64)
    summary = np.zeros(6, dtype=np.uint64)
    tg = (pkg.MultTarget * 1)(pkg.MultTarget(0, 0))
    sp = summary.ctypes.data_as(u64p)
    assert L.ms_witness_derive_multiplicities(None, tg, C.c_size_t(1), sp, None, C.c_size_t(0), None, C.c_size_t(0)) == -1
    assert L.ms_witness_derive_multiplicities(w.h, tg, C.c_size_t(1), None, None, C.c_size_t(0), None, C.c_size_t(0)) == -1
    assert L.ms_witness_derive_multiplicities(w.h, None, C.c_size_t(1), sp, None, C.c_size_t(0), None, C.c_size_t(0)) == -1
    assert L.ms_witness_derive_multiplicities(w.h, tg, C.c_size_t(1), sp, None, C.c_size_t(4), None, C.c_size_t(0)) == -1
    assert "null" in L.ms_last_error().decode()
    with pytest.raises(pkg.MstarkError, match="another rank"):
        s.witness(traces, packed, remote_heights={1: 16}).derive_multiplicities(targets)
    assert L.ms_witness_derive_multiplicities(w.h, tg, C.c_size_t(1), sp, None, C.c_size_t(0), None, C.c_size_t(0)) == 0
    assert w.derive_multiplicities(targets).ok and w.lookup_balance().ok and np.array_equal(w.trace(0), traces[0])
