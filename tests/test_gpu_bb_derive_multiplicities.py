"""`-m gpu`: msbb_witness_derive_multiplicities and msbb_witness_trace (csrc/bb_multiplicity.hip, csrc/bb_prover.hip) against the
model of tests/multiplicity_model_bb.py, which tests/test_bb_multiplicity_model.py pins to the witness builders' own counting.
Every case is device against model: the traces read back through w.trace(c), and every field of the report, compared exactly.
The witnesses come from that module, built once and left unchanged. Shapes: 16 additions are one workgroup block of 1024
messages; 128 additions (1 664 circuit messages + 128 claims + 256 table rows) the smallest shape with more than one block; the
2^16-row byte table x 4 targets has many blocks of target rows and a sparse table; the 4-row tables are a partial block. The
counterpart of test_gpu_derive_multiplicities.py."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the library opens the device)

import multiplicity_model_bb as mm
from test_bb_multiplicity_model import P, bb, cases, compiled_of, fe, garbage, model_of, pack, pkg, wrap_traces
from test_gpu_bb_lookup_balance import _SYS, ctx  # noqa: F401  (the module-scoped context with the permutation set; the system cache)

pytestmark = pytest.mark.gpu
u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
_PROOF, _CUSTOM = {}, {}


def system(ctx, inputs):
    """the device system of a list of circuit inputs, built once"""
    key = id(inputs)
    if key not in _SYS:
        blob, comp, _ = compiled_of(inputs)
        _SYS[key] = bb.System(ctx, blob, len(comp))
    return _SYS[key]


def upload(s, traces, packed, route):
    """host: msbb_witness_create; device: int32 torch tensors through msbb_witness_create_device"""
    if route == "host":
        return s.witness([np.zeros((0, 1), dtype=np.uint64) if t is None else t for t in traces], packed)
    tensors = [None if t is None or len(t) == 0 else torch.from_numpy(np.ascontiguousarray(t).astype(np.uint32).view(np.int32)).cuda() for t in traces]
    return s.witness_from_device(tensors, packed)


def same(got, want):
    return got.shape == want.shape and np.array_equal(got.astype(np.uint64), np.asarray(want, dtype=np.uint64))


def against_model(s, inputs, traces, claims, targets, route="host", entries=64):
    """upload `traces`, derive on the device and in the model, compare the report and every trace -> (witness, report, model traces)"""
    _, comp, osys = compiled_of(inputs)
    packed = pack(claims)
    want, m = mm.derive(osys, comp, traces, packed, targets, entries)
    w = upload(s, traces, packed, route)
    rep = w.derive_multiplicities(targets, entries=entries)
    assert rep.fields() == m.fields(), str(rep)
    assert rep.ok == m.ok
    for c, t in enumerate(want):
        if t is not None:
            assert same(w.trace(c), t), "trace of circuit %d" % c
    return w, rep, want


@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("fill", [0, None])
@pytest.mark.parametrize("n", [16, 128])
def test_byte_table_of_u32_add(ctx, n, fill, route):
    name = "u32_%d" % n
    inputs, traces, claims, targets = cases()[name]
    s = system(ctx, inputs)
    _, comp, _ = compiled_of(inputs)
    packed = pack(claims)
    w = upload(s, garbage(traces, comp, targets, fill), packed, route)
    rep = w.derive_multiplicities(targets)
    _, m = model_of(name)
    assert rep.fields() == m.fields() and rep.ok, str(rep)
    assert same(w.trace(0), traces[0]) and same(w.trace(1), traces[1])  # the builder's bincount trace
    assert w.lookup_balance().ok and w.check().verdict == 0
    if n not in _PROOF:
        _PROOF[n] = s.prove_multiple_claims(s.witness(traces, packed)).to_bytes()
    proof = s.prove_multiple_claims(w).to_bytes()
    assert proof == _PROOF[n] and s.verify_multiple_claims(packed, proof) == 0


def test_byte_operations_four_targets_demand_from_ragged_claims(ctx):
    inputs, traces, claims, targets = cases()["byte_ops"]
    s = system(ctx, inputs)
    _, comp, _ = compiled_of(inputs)
    w = s.witness(garbage(traces, comp, targets), pack(claims))
    rep = w.derive_multiplicities(targets)
    _, m = model_of("byte_ops")
    assert rep.fields() == m.fields() and rep.ok and rep.duplicates == 0, str(rep)
    assert same(w.trace(0), traces[0])  # byte_operations_witness
    assert w.lookup_balance().ok


def table_inputs(pre):
    return fe.CircuitInputs(1, np.array(pre, dtype=np.uint64).reshape(-1, 1), [], [], [fe.Lookup.pull(fe.Expr.main(0), [fe.Expr.preprocessed(0)])])


def pusher_inputs():
    """[value, multiplicity]: push(main(1), [main(0)])"""
    return fe.CircuitInputs(2, None, [], [], [fe.Lookup.push(fe.Expr.main(1), [fe.Expr.main(0)])])


def custom(name):
    """circuit inputs of the hand-made systems, built once (the systems are cached by their identity)"""
    if name not in _CUSTOM:
        E = fe.Expr
        _CUSTOM[name] = {
            "dup": lambda: [table_inputs([0, 1, 1, 2]), pusher_inputs()],
            "push": lambda: [fe.CircuitInputs(1, np.array([[5], [6], [7], [8]], dtype=np.uint64), [], [], [fe.Lookup.push(E.main(0), [E.preprocessed(0)])]),
                             fe.CircuitInputs(2, None, [], [], [fe.Lookup.pull(E.main(1), [E.main(0)])])],
            "two": lambda: [table_inputs([0, 1, 2, 3]), table_inputs([0, 1, 2, 3]), pusher_inputs()],
            "inactive": lambda: [fe.CircuitInputs(2, None, [], [], [fe.Lookup.pull(E.main(0), [E.main(1)])]), pusher_inputs()],
        }[name]()
    return _CUSTOM[name]


def test_a_sum_that_wraps_p_and_a_repeated_row(ctx):
    inputs, traces, claims, targets = cases()["wrap"]
    w, rep, _ = against_model(system(ctx, inputs), inputs, traces, claims, targets)
    assert w.trace(0)[:, 0].tolist() == [0, 3, 0, P - 2]  # 7: net 0 across one wrap of p; 9: row 1 serves, row 2 repeats it
    assert rep.fields()[:5] == (6, 3, 2, 0, 1)
    assert same(w.trace(1), wrap_traces()[1]) and w.lookup_balance().ok


def test_push_signed_target_and_multiplicities_up_to_p_minus_1(ctx):
    inputs = custom("push")
    traces = [np.full((4, 1), 7, dtype=np.uint64), np.array([[5, 1], [6, P - 1], [7, P - 1], [5, P - 1]], dtype=np.uint64)]
    s = system(ctx, inputs)
    w, rep, _ = against_model(s, inputs, traces, [], [(0, 0)])
    # pulls of 1 + (p - 1) = 0 on 5, of p - 1 (= a push of 1, D = 1) on 6 and on 7; the provider pushes v = p - D
    assert w.trace(0)[:, 0].tolist() == [0, P - 1, P - 1, 0]
    assert (rep.demand_messages, rep.demand_groups, rep.served, rep.unserved, rep.duplicates) == (4, 3, 2, 0, 0)
    assert w.lookup_balance().ok and not (w.check().verdict & pkg.CHECK_LOOKUPS)
    assert s.multiplicity_slot(0, 0) == {"eligibility": 0, "column": 0, "pull": False}
    traces[1][3] = [5, 3]  # a repeated tuple that does not cancel: pulled 1 + 3 times, D = p - 4, so the table pushes v = p - D = 4
    w, rep, _ = against_model(s, inputs, traces, [], [(0, 0)], route="device")
    assert w.trace(0)[:, 0].tolist() == [4, P - 1, P - 1, 0] and rep.served == 3 and w.lookup_balance().ok


def test_duplicate_table_rows(ctx):
    inputs = custom("dup")
    traces = [np.full((4, 1), 9, dtype=np.uint64), np.array([[1, 1], [1, 1], [1, 1], [0, 0]], dtype=np.uint64)]
    w, rep, _ = against_model(system(ctx, inputs), inputs, traces, [], [(0, 0)])
    assert w.trace(0)[:, 0].tolist() == [0, 3, 0, 0]  # row 1 serves the three pushes of 1, row 2 repeats its tuple
    assert (rep.demand_messages, rep.demand_groups, rep.served, rep.unserved, rep.duplicates) == (3, 1, 1, 0, 1)
    assert w.lookup_balance().ok


TWO = [np.full((4, 1), 7, dtype=np.uint64), np.full((4, 1), 7, dtype=np.uint64), np.array([[0, 2], [1, 1], [3, 5], [3, 1]], dtype=np.uint64)]


@pytest.mark.parametrize("targets", [[(1, 0), (0, 0)], [(0, 0), (1, 0)]])
def test_two_tables_compete_for_the_same_tuples(ctx, targets):
    inputs = custom("two")
    w, rep, _ = against_model(system(ctx, inputs), inputs, TWO, [], targets)
    assert w.trace(0)[:, 0].tolist() == [2, 1, 0, 6] and w.trace(1)[:, 0].tolist() == [0, 0, 0, 0]  # origins decide, not the order named
    assert (rep.served, rep.unserved, rep.duplicates) == (3, 0, 4) and w.lookup_balance().ok


def test_inactive_target_circuit_and_no_targets(ctx):
    inputs = custom("inactive")
    traces = [None, np.array([[4, 1], [4, 1], [9, 2], [0, 0]], dtype=np.uint64)]
    w, rep, _ = against_model(system(ctx, inputs), inputs, traces, [], [(0, 0)])
    assert (rep.demand_messages, rep.demand_groups, rep.served, rep.unserved) == (3, 2, 0, 2) and w.trace(0).size == 0
    assert [e.fields() for e in rep.entries] == [((1, 0, 0), 2, 2, [4]), ((1, 2, 0), 2, 1, [9])]
    # no targets: a pure count; the table's own (garbage) messages are demand like any other, and nothing is written
    inputs, traces, claims, targets = cases()["u32_16"]
    _, comp, _ = compiled_of(inputs)
    g = garbage(traces, comp, targets, 7)
    w, rep, _ = against_model(system(ctx, inputs), inputs, g, claims, [])
    assert rep.served == 0 and rep.unserved > 0 and same(w.trace(0), g[0]) and same(w.trace(1), g[1])


def unserved_case():
    """the 16-addition witness with the byte cell (row 5, column 2) set to 300; claim 5 follows the row's word, so that the
    u32 tuples of claim and row still cancel and the byte message (0, 300) is the one thing no table row serves"""
    inputs, traces, claims, targets = cases()["u32_16"]
    traces = [t.copy() for t in traces]
    traces[1][5, 2] = 300
    claims = [list(c) for c in claims]
    claims[5][1] = sum(int(traces[1][5, k]) << (8 * k) for k in range(4)) % P
    return inputs, traces, claims, targets


def test_unserved_demand_is_named(ctx):
    inputs, traces, claims, targets = unserved_case()
    s = system(ctx, inputs)
    w, rep, want = against_model(s, inputs, traces, claims, targets)
    assert rep.unserved == 1 and not rep.ok
    assert rep.entries[0].fields() == ((1, 5, 3), 1, 1, [0, 300])  # circuit 1, row 5, slot 3 = push(1, [0, main(2)])
    assert same(w.trace(0), want[0]) and not w.lookup_balance().ok
    assert "unserved (0, 300): net 1 over 1 message, first at circuit 1 row 5 lookup 3" in str(rep)
    _, counts, _ = against_model(s, inputs, traces, claims, targets, entries=0)
    assert counts.entries == [] and counts.fields()[:5] == rep.fields()[:5]


def test_idempotence_isolation_and_host_waits(ctx):
    inputs, traces, claims, targets = cases()["u32_128"]
    s = system(ctx, inputs)
    _, comp, _ = compiled_of(inputs)
    g = garbage(traces, comp, targets)
    w = s.witness(g, pack(claims))
    bg = ((3, 5, 7, 11), (13, 17, 19, 23))
    claims_before = bb.claims_accumulator(w, *bg)
    n0 = ctx.sync_count()
    first = w.derive_multiplicities(targets)
    assert ctx.sync_count() - n0 == 1  # nothing unserved: one host wait
    once = [w.trace(c) for c in range(2)]
    second = w.derive_multiplicities(targets)
    twice = [w.trace(c) for c in range(2)]
    assert first.fields() == second.fields() and all(np.array_equal(a, b) for a, b in zip(once, twice))
    assert same(once[1], g[1]) and bb.claims_accumulator(w, *bg) == claims_before  # the other trace and the claims
    # unserved demand with room for entries: one more wait
    inputs, traces, claims, targets = unserved_case()
    w = s.witness(traces, pack(claims))
    n0 = ctx.sync_count()
    assert w.derive_multiplicities(targets).unserved == 1 and ctx.sync_count() - n0 == 2
    n0 = ctx.sync_count()
    assert w.derive_multiplicities(targets, entries=0).unserved == 1 and ctx.sync_count() - n0 == 1


def test_long_probe_chains_give_the_same_report_and_bytes(ctx, monkeypatch):
    inputs, traces, claims, targets = unserved_case()
    s = system(ctx, inputs)
    w, plain, _ = against_model(s, inputs, traces, claims, targets)
    monkeypatch.setenv("MSAMD_LB_HASH_BITS", "0")  # every probe sequence starts at slot 0
    w2, chained, _ = against_model(s, inputs, traces, claims, targets)
    assert chained.fields() == plain.fields() and np.array_equal(w.trace(0), w2.trace(0))
    inputs = custom("two")  # target tuples nobody demands meet in one chain too
    _, rep, _ = against_model(system(ctx, inputs), inputs, TWO, [], [(0, 0), (1, 0)])
    assert rep.duplicates == 4


def test_multiplicity_slot_agrees_with_the_model(ctx):
    for inputs in (cases()["u32_16"][0], cases()["squares_16"][0], cases()["wrap"][0]):
        s = system(ctx, inputs)
        _, comp, _ = compiled_of(inputs)
        for c, cc in enumerate(comp):
            for j in range(len(cc.lookups)):
                code, col, pull = mm.classify(cc, j)
                assert s.multiplicity_slot(c, j) == {"eligibility": code, "column": col, "pull": pull}, (c, j)
    with pytest.raises(pkg.MstarkError, match="out of range"):
        s.multiplicity_slot(0, 99)


def test_witness_trace_round_trip_and_buffer_contract(ctx):
    inputs = custom("inactive")
    s = system(ctx, inputs)
    tr = np.array([[0, 1], [P - 1, 0], [1, P - 1], [P - 1, P - 1]], dtype=np.uint64)
    w = s.witness([np.zeros((0, 2), dtype=np.uint64), tr], pack([]))
    got = w.trace(1)
    assert got.dtype == np.uint32 and same(got, tr)
    L = pkg.lib()
    need, out = C.c_size_t(99), np.zeros(8, dtype=np.uint32)
    assert L.msbb_witness_trace(w.h, C.c_size_t(1), out.ctypes.data_as(u32p), C.c_size_t(7), C.byref(need)) == -3 and need.value == 8  # MS_ERR_BUFFER
    assert not out.any()
    assert L.msbb_witness_trace(w.h, C.c_size_t(1), out.ctypes.data_as(u32p), C.c_size_t(8), C.byref(need)) == 0 and same(out.reshape(4, 2), tr)
    assert L.msbb_witness_trace(w.h, C.c_size_t(0), None, C.c_size_t(0), C.byref(need)) == 0 and need.value == 0  # inactive
    assert w.trace(0).shape == (0, 2)
    assert L.msbb_witness_trace(w.h, C.c_size_t(2), None, C.c_size_t(0), C.byref(need)) == -1 and "no such circuit" in L.ms_last_error().decode()
    with pytest.raises(pkg.MstarkError, match="host-resident"):
        s.host_witness([np.zeros((0, 2), dtype=np.uint64), tr], pack([])).trace(1)
    w = upload(s, [None, tr], pack([]), "device")
    assert same(w.trace(1), tr)


def test_misuse_is_an_error_and_the_context_stays_usable(ctx):
    inputs, traces, claims, targets = cases()["u32_16"]
    s = system(ctx, inputs)
    packed = pack(claims)
    with pytest.raises(pkg.MstarkError, match="device-resident"):
        s.host_witness(traces, packed).derive_multiplicities(targets)
    w = s.witness(traces, packed)
    for bad, text in (([(1, 1)], "not eligible"), ([(0, 0), (0, 0)], "shares the derived column"), ([(2, 0)], "out of range"),
                      ([(0, 1)], "out of range")):
        with pytest.raises(pkg.MstarkError, match=text):
            w.derive_multiplicities(bad)
        assert same(w.trace(0), traces[0])  # refused before anything was written
    L = pkg.lib()
    summary = np.zeros(6, dtype=np.uint64)
    tg = (pkg.MultTarget * 1)(pkg.MultTarget(0, 0))
    sp, one, zero = summary.ctypes.data_as(u64p), C.c_size_t(1), C.c_size_t(0)
    assert L.msbb_witness_derive_multiplicities(None, tg, one, sp, None, zero, None, zero) == -1
    assert L.msbb_witness_derive_multiplicities(w.h, tg, one, None, None, zero, None, zero) == -1
    assert L.msbb_witness_derive_multiplicities(w.h, None, one, sp, None, zero, None, zero) == -1
    assert L.msbb_witness_derive_multiplicities(w.h, tg, one, sp, None, C.c_size_t(4), None, zero) == -1
    assert "null" in L.ms_last_error().decode()
    assert L.msbb_witness_derive_multiplicities(w.h, tg, one, sp, None, zero, None, C.c_size_t(4)) == -1
    ctx.debug_fail_alloc(1)  # the call's first allocation (a circuit's lookup values): the error names the bytes
    try:
        with pytest.raises(pkg.MstarkError, match=r"msbb_witness_derive_multiplicities: cannot allocate the \d+ bytes of "):
            w.derive_multiplicities(targets)
    finally:
        ctx.debug_fail_alloc(0)
    assert same(w.trace(0), traces[0])
    assert L.msbb_witness_derive_multiplicities(w.h, tg, one, sp, None, zero, None, zero) == 0
    assert w.derive_multiplicities(targets).ok and w.lookup_balance().ok and same(w.trace(0), traces[0])
