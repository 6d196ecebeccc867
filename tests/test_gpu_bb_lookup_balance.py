"""`-m gpu`: msbb_witness_lookup_balance (csrc/bb_balance.hip) against the model of tests/lookup_balance_model_bb.py, which
tests/test_bb_lookup_balance_model.py anchors to the BabyBear oracle. Every figure of the report is deterministic and compared
exactly. Witnesses and model reports come from that module, computed once per case and left unchanged. Shapes are the smallest
that reach the code named: 2^13 rows x 2 slots are 16 workgroups of 1024 messages; the largest is the byte table's 2^16 rows x
4 slots. The counterpart of test_gpu_lookup_balance.py."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the library opens the device: test_witness_from_torch_tensors)

import oracle_bb as ob
from test_bb_lookup_balance_model import K, P, bb, cases, compiled_of, model_of, pack, pkg

pytestmark = pytest.mark.gpu
u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
_SYS = {}


@pytest.fixture(scope="module")
def ctx():
    c = pkg.Context(0)
    bb.set_poseidon2(c, K)
    ob.set_poseidon2(K)
    return c


def system(ctx, name):
    """the device system of a case (one per set of circuit inputs)"""
    key = id(cases()[name][0])
    if key not in _SYS:
        blob, comp, _ = compiled_of(name)
        _SYS[key] = bb.System(ctx, blob, len(comp))
    return _SYS[key]


def both(ctx, name, entries=64, witness=None):
    """device report (of `witness`, default: the case's traces uploaded) and model report, compared in every field"""
    _, traces, claims, balanced = cases()[name]
    w = witness or system(ctx, name).witness(traces, pack(claims))
    rep = w.lookup_balance(entries=entries)
    m = model_of(name, entries)
    assert rep.fields() == m.fields(), (name, str(rep))
    assert rep.ok == balanced
    return rep, w


@pytest.mark.parametrize("name", ["even_odd", "even_odd_wrong_claim", "even_odd_no_claim"])
def test_even_odd(ctx, name):
    rep, w = both(ctx, name)
    assert (rep.unbalanced == 0) == (not (w.check().verdict & pkg.CHECK_LOOKUPS))
    if name == "even_odd":
        assert (rep.messages, rep.groups, rep.unbalanced) == (10, 5, 0)
        assert rep.entries == [] and str(rep) == "lookups balanced (10 messages in 5 groups)"
    elif name == "even_odd_wrong_claim":
        assert (rep.messages, rep.groups, rep.unbalanced) == (10, 6, 2)
        assert [(e.origin, e.net, e.args) for e in rep.entries] == [(("claims", 0, 0), 1, [0, 4]), ((0, 0, 0), P - 1, [0, 4, 1])]
        named = str(w.lookup_balance(names=["Even", "Odd"]))
        assert "(0, 4, 1): net -1 over 1 message, first at circuit 0 (Even) row 0 lookup 0" in named and "(0, 4): net 1 over 1 message, first at claim 0" in named
    else:
        assert rep.unbalanced == 1 and (rep.entries[0].origin, rep.entries[0].net, rep.entries[0].args) == ((0, 0, 0), P - 1, [0, 4, 1])


@pytest.mark.parametrize("name", ["trailing_zero_row", "empty_claim", "trailing_zero_row_longer_claim", "zero_row_longer_claim"])
def test_trailing_zeros_do_not_tell_tuples_apart(ctx, name):
    rep, _ = both(ctx, name)
    assert (rep.messages, rep.groups, rep.unbalanced) == ((2, 1, 0) if rep.ok else (2, 2, 2))


def test_multiplicities_wrapping_negative_and_zero(ctx):
    rep, _ = both(ctx, "multiplicities")
    assert (rep.messages, rep.groups, rep.unbalanced) == (6, 2, 0)


def test_hot_tuple_over_several_workgroups(ctx):
    """2^13 rows x 2 slots = 16 workgroups on one tuple: the LDS flush and the cross-workgroup adds both run"""
    rep, _ = both(ctx, "hot")
    assert (rep.messages, rep.groups) == (8193, 1)
    rep, _ = both(ctx, "hot_one_short")
    e = rep.entries[0]
    assert (e.origin, e.net, e.members, e.args) == ((0, 0, 0), 1, 8193, [3, 4]) and rep.slot_counts == [[8192, 1]]


def test_all_distinct_fills_every_table_and_entries_keep_origin_order(ctx):
    rep, w = both(ctx, "distinct", entries=16)
    assert rep.unbalanced == 8192 and [e.origin for e in rep.entries] == [(0, r, 0) for r in range(16)]
    assert [e.args for e in rep.entries] == [[r + 1, 5] for r in range(16)] and rep.slot_counts == [[8192, 0]]
    # more room than offenders, no room at all, and an args buffer too short for all tuples (raw call)
    both(ctx, "distinct", entries=9000, witness=w)
    assert w.lookup_balance(entries=0).fields()[:4] == (8192, 8192, 8192, [])
    summary, ent, args = np.zeros(4, dtype=np.uint64), np.zeros((4, 8), dtype=np.uint64), np.zeros(5, dtype=np.uint32)
    rc = pkg.lib().msbb_witness_lookup_balance(w.h, summary.ctypes.data_as(u64p), ent.ctypes.data_as(u64p), C.c_size_t(4), args.ctypes.data_as(u32p),
                                               C.c_size_t(5), None, C.c_size_t(0))
    assert rc == 0 and [int(x) for x in summary] == [8192, 8192, 8192, 4]
    assert [int(x) for x in ent[:, 6]] == [0, 2, (1 << 64) - 1, (1 << 64) - 1] and [int(x) for x in args] == [1, 5, 2, 5, 0]
    assert [int(x) for x in ent[:, 1]] == [0, 1, 2, 3] and not ent[:, 7].any()


def test_long_probe_chains_give_the_same_report(ctx, monkeypatch):
    plain, w = both(ctx, "distinct_256", entries=300)
    monkeypatch.setenv("MSAMD_LB_HASH_BITS", "0")  # every tuple starts at slot 0: 256-long chains, compared tuple by tuple
    chained, _ = both(ctx, "distinct_256", entries=300, witness=w)
    assert chained.fields() == plain.fields() and plain.unbalanced == 256


def test_mul_air_balances_whatever_the_cells_hold(ctx):
    rep, _ = both(ctx, "mul_air")
    assert (rep.messages, rep.groups, rep.unbalanced) == (16384, 8192, 0)
    # one cell off: push and pull read the same cells, so the lookups still cancel - the constraint a b = c does not hold, which
    # only check() sees. That is why a witness needs both calls.
    rep, w = both(ctx, "mul_air_one_cell")
    assert rep.ok and (rep.messages, rep.groups) == (16384, 8192)
    assert w.check().verdict == pkg.CHECK_CONSTRAINT


def test_one_argument_lookups_and_a_preprocessed_argument(ctx):
    rep, _ = both(ctx, "squares")
    assert (rep.messages, rep.groups, rep.unbalanced) == (48, 16, 0)


def test_byte_operations_ragged_claims_and_a_large_sparse_table(ctx):
    """2^16 rows x 4 slots = 262144 candidate messages, of which 4 + 5 exist; constant arguments, claims of two lengths"""
    rep, _ = both(ctx, "byte_ops")
    assert (rep.messages, rep.groups, rep.unbalanced) == (9, 4, 0)
    rep, _ = both(ctx, "byte_ops_one_cell")
    e = rep.entries[0]
    assert rep.unbalanced == 1 and (e.origin, e.net, e.members, e.args) == (("claims", 0, 0), P - 1, 3, [0, 3, 5, 6])
    assert rep.slot_counts == [[1, 0, 0, 0]] and rep.claims_count == 2


def test_u32_add_clean_and_one_cell_off(ctx):
    rep, _ = both(ctx, "u32")
    assert (rep.messages, rep.groups, rep.unbalanced) == (14592, 1280, 0) and rep.claims_count == 0
    rep, _ = both(ctx, "u32_one_cell")
    assert rep.unbalanced == 4 and rep.claims_count == 1
    # the claim's u32 tuple, the table's two bytes, the row's u32 tuple - claim and row 5 disagree
    assert [e.origin[0] for e in rep.entries] == ["claims", 0, 0, 1] and rep.entries[0].origin == ("claims", 5, 0) and rep.entries[3].origin == (1, 5, 0)
    assert rep.entries[0].args[2:] == rep.entries[3].args[2:] and rep.entries[0].args[1] != rep.entries[3].args[1]
    assert rep.slot_counts[1][0] == 1 and sum(rep.slot_counts[1][1:]) > 0  # the slots named: the row's u32 pull and its byte pushes
    assert "claims: 1 messages in unbalanced groups" in str(rep)


@pytest.mark.parametrize("name", ["u32", "u32_one_cell"])
def test_witness_from_torch_tensors(ctx, name):
    _, traces, claims, _ = cases()[name]
    s = system(ctx, name)
    tensors = [torch.from_numpy(np.ascontiguousarray(t).astype(np.uint32).view(np.int32)).cuda() for t in traces]
    w = s.witness_from_device(tensors, pack(claims))
    rep, _ = both(ctx, name, witness=w)
    assert rep.fields() == s.witness(traces, pack(claims)).lookup_balance().fields()


def test_the_witness_is_not_changed_and_host_waits(ctx):
    _, traces, claims, _ = cases()["even_odd"]
    s = system(ctx, "even_odd")
    packed = pack(claims)
    w = s.witness(traces, packed)
    before = s.prove_multiple_claims(w).to_bytes()
    n0 = ctx.sync_count()
    assert w.lookup_balance().ok
    assert ctx.sync_count() - n0 == 1  # balanced: one host wait
    after = s.prove_multiple_claims(w).to_bytes()
    assert before == after and s.verify_multiple_claims(packed, after) == 0
    w = s.witness(traces, pack(cases()["even_odd_wrong_claim"][2]))
    n0 = ctx.sync_count()
    assert w.lookup_balance().unbalanced == 2
    assert ctx.sync_count() - n0 == 2  # ... and one more for the entries
    n0 = ctx.sync_count()
    assert w.lookup_balance(entries=0).unbalanced == 2
    assert ctx.sync_count() - n0 == 1  # nothing to fetch: no second wait


def test_no_lookups_no_claims(ctx):
    rep, _ = both(ctx, "pythagorean")
    assert rep.fields() == (0, 0, 0, [], [[]], 0) and rep.ok


def test_misuse_is_an_error_and_the_context_stays_usable(ctx):
    _, traces, claims, _ = cases()["even_odd"]
    s = system(ctx, "even_odd")
    packed = pack(claims)
    with pytest.raises(pkg.MstarkError, match="device-resident"):
        s.host_witness(traces, packed).lookup_balance()
    w = s.witness(traces, packed)
    summary, counts = np.zeros(4, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
    L = pkg.lib()
    total = sum(s.circuit_info(i)["num_lookups"] for i in range(s.n_circuits))
    sp, zero = summary.ctypes.data_as(u64p), C.c_size_t(0)
    assert L.msbb_witness_lookup_balance(w.h, sp, None, zero, None, zero, counts.ctypes.data_as(u64p), C.c_size_t(total)) == -3  # MS_ERR_BUFFER: one word short
    assert L.msbb_witness_lookup_balance(w.h, sp, None, zero, None, zero, counts.ctypes.data_as(u64p), C.c_size_t(total + 1)) == 0
    assert L.msbb_witness_lookup_balance(None, sp, None, zero, None, zero, None, zero) == -1
    assert L.msbb_witness_lookup_balance(w.h, None, None, zero, None, zero, None, zero) == -1
    assert L.msbb_witness_lookup_balance(w.h, sp, None, C.c_size_t(4), None, zero, None, zero) == -1
    assert "null" in L.ms_last_error().decode()
    assert L.msbb_witness_lookup_balance(w.h, sp, None, zero, None, C.c_size_t(4), None, zero) == -1
    ctx.debug_fail_alloc(1)  # the call's first allocation (a circuit's lookup values): the error names the bytes
    try:
        with pytest.raises(pkg.MstarkError, match=r"cannot allocate the \d+ bytes of "):
            w.lookup_balance()
    finally:
        ctx.debug_fail_alloc(0)
    assert w.lookup_balance().ok and both(ctx, "even_odd_wrong_claim")[0].unbalanced == 2
