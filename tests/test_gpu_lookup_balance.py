"""`-m gpu`: ms_witness_lookup_balance (csrc/balance.hip) against the model of tests/lookup_balance_model.py, which
tests/test_lookup_balance_model.py anchors to the oracle. Every figure of the report is deterministic and compared exactly.
Witnesses and model reports come from that module, computed once per case and left unchanged. Shapes are the smallest that
reach the code named: 2^13 rows are 8 (one slot) or 16 (two slots) workgroups of 1024 messages."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the library opens the device: test_witness_from_torch_tensors)

from test_lookup_balance_model import b3, cases, model_of  # noqa: F401 (b3 is a fixture)

pytestmark = pytest.mark.gpu
P = (1 << 64) - (1 << 32) + 1
_SYS = {}


def system(pkg, fe, ctx, b3, name, params=None):
    """the device system of a case (one per set of circuit inputs), with its compiled circuits"""
    inputs = cases(fe, b3)[name][0]
    key = (id(inputs), params is not None)
    if key not in _SYS:
        comp = [fe.compile_circuit(ci) for ci in inputs]
        p = params or fe.test_params()
        s = pkg.System(ctx, fe.system_blob(p, comp), len(comp))
        s.params = p
        _SYS[key] = s
    return _SYS[key]


def both(pkg, fe, ctx, oracle, b3, name, entries=64, witness=None):
    """device report (of `witness`, default: the case's traces uploaded) and model report, compared in every field"""
    _, traces, claims, balanced = cases(fe, b3)[name]
    s = system(pkg, fe, ctx, b3, name)
    w = witness or s.witness(traces, fe.pack_claims(claims))
    rep = w.lookup_balance(entries=entries)
    m, _, _ = model_of(oracle, fe, b3, name, entries)
    assert rep.fields() == m.fields(), (name, str(rep))
    assert rep.ok == balanced
    return rep, w


@pytest.mark.parametrize("name", ["even_odd", "even_odd_wrong_claim", "even_odd_no_claim"])
def test_even_odd(pkg, fe, ctx, oracle, b3, name):
    rep, w = both(pkg, fe, ctx, oracle, b3, name)
    assert (rep.unbalanced == 0) == (not (w.check().verdict & pkg.CHECK_LOOKUPS))
    if name == "even_odd":
        assert rep.entries == [] and str(rep) == "lookups balanced (%d messages in %d groups)" % (rep.messages, rep.groups)
    elif name == "even_odd_wrong_claim":
        assert [(e.origin, e.net, e.args) for e in rep.entries] == [(("claims", 0, 0), 1, [0, 4]), ((0, 0, 0), P - 1, [0, 4, 1])]
        named = str(w.lookup_balance(names=["Even", "Odd"]))
        assert "(0, 4, 1): net -1 over 1 message, first at circuit 0 (Even) row 0 lookup 0" in named and "(0, 4): net 1 over 1 message, first at claim 0" in named
    else:
        assert rep.unbalanced == 1 and (rep.entries[0].origin, rep.entries[0].net, rep.entries[0].args) == ((0, 0, 0), P - 1, [0, 4, 1])


@pytest.mark.parametrize("name", ["trailing_zero_row", "empty_claim", "trailing_zero_row_longer_claim", "zero_row_longer_claim"])
def test_trailing_zeros_do_not_tell_tuples_apart(pkg, fe, ctx, oracle, b3, name):
    rep, _ = both(pkg, fe, ctx, oracle, b3, name)
    assert (rep.messages, rep.groups) == ((2, 1) if rep.ok else (2, 2))


def test_multiplicities_large_negative_and_zero(pkg, fe, ctx, oracle, b3):
    rep, _ = both(pkg, fe, ctx, oracle, b3, "multiplicities")
    assert (rep.messages, rep.groups, rep.unbalanced) == (6, 2, 0)


def test_hot_tuple_over_several_workgroups(pkg, fe, ctx, oracle, b3):
    rep, _ = both(pkg, fe, ctx, oracle, b3, "hot")
    assert (rep.messages, rep.groups) == (8193, 1)
    rep, _ = both(pkg, fe, ctx, oracle, b3, "hot_one_short")
    e = rep.entries[0]
    assert (e.origin, e.net, e.members, e.args) == ((0, 0, 0), 1, 8193, [3, 4]) and rep.slot_counts == [[8192, 1]]


def test_all_distinct_fills_every_table_and_entries_keep_origin_order(pkg, fe, ctx, oracle, b3):
    rep, w = both(pkg, fe, ctx, oracle, b3, "distinct", entries=16)
    assert rep.unbalanced == 8192 and [e.origin for e in rep.entries] == [(0, r, 0) for r in range(16)]
    assert [e.args for e in rep.entries] == [[r + 1, 5] for r in range(16)] and rep.slot_counts == [[8192, 0]]
    # more room than offenders, no room at all, and an args buffer too short for all tuples (raw call)
    both(pkg, fe, ctx, oracle, b3, "distinct", entries=9000, witness=w)
    assert w.lookup_balance(entries=0).fields()[:4] == (8192, 8192, 8192, [])
    summary, ent, args = np.zeros(4, dtype=np.uint64), np.zeros((4, 8), dtype=np.uint64), np.zeros(5, dtype=np.uint64)
    u64p = C.POINTER(C.c_uint64)
    rc = pkg.lib().ms_witness_lookup_balance(w.h, summary.ctypes.data_as(u64p), ent.ctypes.data_as(u64p), C.c_size_t(4), args.ctypes.data_as(u64p),
                                             C.c_size_t(5), None, C.c_size_t(0))
    assert rc == 0 and [int(x) for x in summary] == [8192, 8192, 8192, 4]
    assert [int(x) for x in ent[:, 6]] == [0, 2, (1 << 64) - 1, (1 << 64) - 1] and [int(x) for x in args] == [1, 5, 2, 5, 0]
    assert [int(x) for x in ent[:, 1]] == [0, 1, 2, 3] and not ent[:, 7].any()


def test_long_probe_chains_give_the_same_report(pkg, fe, ctx, oracle, b3, monkeypatch):
    plain, w = both(pkg, fe, ctx, oracle, b3, "distinct_256", entries=300)
    monkeypatch.setenv("MSAMD_LB_HASH_BITS", "0")  # every tuple starts at slot 0: 256-long chains, compared tuple by tuple
    chained, _ = both(pkg, fe, ctx, oracle, b3, "distinct_256", entries=300, witness=w)
    assert chained.fields() == plain.fields() and plain.unbalanced == 256


def test_u32_add_clean_and_one_cell_off(pkg, fe, ctx, oracle, b3):
    rep, _ = both(pkg, fe, ctx, oracle, b3, "u32")
    assert rep.ok and rep.claims_count == 0
    rep, _ = both(pkg, fe, ctx, oracle, b3, "u32_one_cell")
    assert rep.unbalanced == 4 and rep.claims_count == 1
    # the claim's u32 tuple, the table's two bytes, the row's u32 tuple - claim and row 5 disagree
    assert [e.origin[0] for e in rep.entries] == ["claims", 0, 0, 1] and rep.entries[0].origin == ("claims", 5, 0) and rep.entries[3].origin == (1, 5, 0)
    assert rep.entries[0].args[2:] == rep.entries[3].args[2:] and rep.entries[0].args[1] ^ rep.entries[3].args[1] == 1
    assert rep.slot_counts[1][0] == 1 and sum(rep.slot_counts[1][1:]) > 0  # the slots named: the row's u32 pull and its byte pushes
    assert "claims: 1 messages in unbalanced groups" in str(rep)


def test_bench_witness_generated_on_the_device(pkg, fe, ctx, oracle, b3):
    s = system(pkg, fe, ctx, b3, "bench_4096", fe.bench_params())
    rep, _ = both(pkg, fe, ctx, oracle, b3, "bench_4096", witness=s.bench_witness_on_device(1 << 12))  # ready-made lookup values
    assert rep.ok and rep.messages > 13 * 4096


def test_blake3_witness_generated_on_the_device(pkg, fe, ctx, oracle, b3, monkeypatch):
    monkeypatch.setenv("MSAMD_NO_JIT", "1")  # (the call runs no generated kernel; this spares the test their compilation)
    claims = cases(fe, b3)["blake3_nine"][2]
    states = np.array([c[1:33] for c in claims], dtype=np.uint32)
    rep, _ = both(pkg, fe, ctx, oracle, b3, "blake3_nine", witness=system(pkg, fe, ctx, b3, "blake3_nine").blake3_witness_on_device(states))
    assert rep.ok


@pytest.mark.parametrize("name", ["u32", "u32_one_cell"])
def test_witness_from_torch_tensors(pkg, fe, ctx, oracle, b3, name):
    """ms_witness_create_device keeps no lookup values for circuits whose stage 2 reads the trace: the call computes its own"""
    _, traces, claims, _ = cases(fe, b3)[name]
    s = system(pkg, fe, ctx, b3, name)
    tensors = [torch.from_numpy(np.ascontiguousarray(t).view(np.int64)).cuda() for t in traces]
    w = s.witness_from_device(tensors, fe.pack_claims(claims))
    rep, _ = both(pkg, fe, ctx, oracle, b3, name, witness=w)
    assert rep.fields() == s.witness(traces, fe.pack_claims(claims)).lookup_balance().fields()


def test_the_witness_is_not_changed_and_host_waits(pkg, fe, ctx, oracle, b3):
    _, traces, claims, _ = cases(fe, b3)["u32"]
    s = system(pkg, fe, ctx, b3, "u32")
    packed = fe.pack_claims(claims)
    w = s.witness(traces, packed)
    before = s.prove_multiple_claims(w).to_bytes()
    n0 = ctx.sync_count()
    assert w.lookup_balance().ok
    assert ctx.sync_count() - n0 == 1  # balanced: one host wait
    after = s.prove_multiple_claims(w).to_bytes()
    assert before == after and s.verify_multiple_claims(packed, after) == 0
    _, traces, claims, _ = cases(fe, b3)["u32_one_cell"]
    w = s.witness(traces, fe.pack_claims(claims))
    n0 = ctx.sync_count()
    assert w.lookup_balance().unbalanced == 4
    assert ctx.sync_count() - n0 == 2  # ... and one more for the entries


def test_no_lookups_no_claims(pkg, fe, ctx, oracle, b3):
    rep, _ = both(pkg, fe, ctx, oracle, b3, "pythagorean")
    assert rep.fields() == (0, 0, 0, [], [[]], 0) and rep.ok


def test_misuse_is_an_error_and_the_context_stays_usable(pkg, fe, ctx, oracle, b3):
    _, traces, claims, _ = cases(fe, b3)["even_odd"]
    s = system(pkg, fe, ctx, b3, "even_odd")
    packed = fe.pack_claims(claims)
    with pytest.raises(pkg.MstarkError, match="device-resident"):
        s.host_witness(traces, packed).lookup_balance()
    with pytest.raises(pkg.MstarkError, match="another rank"):
        s.witness(traces, packed, remote_heights={1: 4}).lookup_balance()
    w = s.witness(traces, packed)
    u64p = C.POINTER(C.c_uint64)
    summary, counts = np.zeros(4, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
    L = pkg.lib()
    total = sum(s.circuit_info(i)["num_lookups"] for i in range(s.n_circuits))
    rc = L.ms_witness_lookup_balance(w.h, summary.ctypes.data_as(u64p), None, C.c_size_t(0), None, C.c_size_t(0), counts.ctypes.data_as(u64p), C.c_size_t(total))
    assert rc == -3  # MS_ERR_BUFFER: one word short
    assert L.ms_witness_lookup_balance(None, summary.ctypes.data_as(u64p), None, C.c_size_t(0), None, C.c_size_t(0), None, C.c_size_t(0)) == -1
    assert L.ms_witness_lookup_balance(w.h, None, None, C.c_size_t(0), None, C.c_size_t(0), None, C.c_size_t(0)) == -1
    assert L.ms_witness_lookup_balance(w.h, summary.ctypes.data_as(u64p), None, C.c_size_t(4), None, C.c_size_t(0), None, C.c_size_t(0)) == -1
    assert "null" in L.ms_last_error().decode()
    ctx.debug_fail_alloc(1)  # the call's first allocation (its table, or lookup values the witness does not hold): the error names the bytes
    try:
        with pytest.raises(pkg.MstarkError, match=r"cannot allocate the \d+ bytes of "):
            w.lookup_balance()
    finally:
        ctx.debug_fail_alloc(0)
    assert w.lookup_balance().ok and both(pkg, fe, ctx, oracle, b3, "even_odd_wrong_claim")[0].unbalanced == 2
