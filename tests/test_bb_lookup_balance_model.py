"""CPU tests: the model of msbb_witness_lookup_balance (tests/lookup_balance_model_bb.py) anchored to the BabyBear oracle. On every
witness the GPU test (test_gpu_bb_lookup_balance.py) uses, the model finds no unbalanced group exactly when the oracle's chained
accumulator is zero under two pairs of challenges: the one CPU-checkable tie between the exact definition and the protocol, so
that the device is not compared with a model nobody has checked. The witnesses are built here, once, and shared with the GPU
test. Plus the additive pieces that need no device. The counterpart of test_lookup_balance_model.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lookup_balance_model_bb as lm
import oracle_bb as ob
from test_bb_witness_check_model import BG, BG2, K, bb, compile_system, fe, pack, pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = lm.P
_CACHE = {}


@pytest.fixture(autouse=True)
def _perm():
    ob.set_poseidon2(K)


def tuple_inputs():
    """one circuit, one slot: pull(main(2), [main(0), main(1)])"""
    E = fe.Expr
    return [fe.CircuitInputs(3, None, [], [], [fe.Lookup.pull(E.main(2), [E.main(0), E.main(1)])])]


def mult_inputs():
    """one circuit, one slot whose multiplicity is a column as it stands: push(main(0), [main(1)])"""
    E = fe.Expr
    return [fe.CircuitInputs(2, None, [], [], [fe.Lookup.push(E.main(0), [E.main(1)])])]


def push_pull_inputs():
    """one circuit, two slots over the same tuple: push(main(0), [main(1), main(2)]) and pull(main(3), [main(1), main(2)])"""
    E = fe.Expr
    args = [E.main(1), E.main(2)]
    return [fe.CircuitInputs(4, None, [], [], [fe.Lookup.push(E.main(0), args), fe.Lookup.pull(E.main(3), args)])]


def tuple_trace(a, b):
    tr = np.zeros((4, 3), dtype=np.uint64)
    tr[0] = [a, b, 1]
    return tr


def mult_trace():
    """(p - 1) / 2 and (p + 1) / 2 on one tuple (a sum that wraps p exactly once), p - 1 three times and 3 once on another (p - 1
    is "-1"), and a tuple whose only member has multiplicity 0"""
    rows = [[(P - 1) // 2, 7], [(P + 1) // 2, 7], [P - 1, 9], [P - 1, 9], [P - 1, 9], [3, 9], [0, 11], [0, 0]]
    return np.array(rows, dtype=np.uint64)


def hot_trace(pulled):
    """2^13 rows push (3, 4) once each; row 0 also pulls it `pulled` times"""
    n = 1 << 13
    tr = np.zeros((n, 4), dtype=np.uint64)
    tr[:, 0], tr[:, 1], tr[:, 2] = 1, 3, 4
    tr[0, 3] = pulled
    return tr


def distinct_trace(n):
    """n rows push n different tuples (r + 1, 5); nothing pulls"""
    tr = np.zeros((n, 4), dtype=np.uint64)
    tr[:, 0], tr[:, 1], tr[:, 2] = 1, np.arange(1, n + 1, dtype=np.uint64), 5
    return tr


def mul_air_traces(corrupt):
    with fe.field(fe.BABYBEAR):
        tr = fe.mul_air_trace(1 << 13)
    if corrupt:
        tr[5, 0] = (int(tr[5, 0]) + 1) % P  # a of row 5: push and pull read the same cells, so the lookups still cancel
    return [tr]


BYTE_CALLS = [(0, 3, 5), (1, 255, 254), (2, 0, 0), (3, 7, 9), (0, 3, 5)]


def byte_traces(corrupt):
    with fe.field(fe.BABYBEAR):
        traces, claims = fe.byte_operations_witness(BYTE_CALLS)
    if corrupt:
        traces[0][256 * 3 + 5, 0] += np.uint64(1)  # one xor pulled once more than it is claimed
    return traces, claims


def u32_traces(corrupt):
    """the bench witness of the Goldilocks configuration; u32 words above p are congruent to their reductions, which is what the
    claims carry"""
    with fe.field(fe.BABYBEAR):
        traces, claims = fe.u32_add_bench_witness(1 << 10)
    traces = [t.copy() for t in traces]
    if corrupt:
        traces[1][5, 0] ^= np.uint64(1)  # one byte of x in row 5: the byte's two tuples and the u32 tuple of claim and row
    return traces, [list(int(v) % P for v in c) for c in claims]


def cases():
    """name -> (circuit inputs, traces, claims, balanced): every witness of test_gpu_bb_lookup_balance.py"""
    if "cases" not in _CACHE:
        with fe.field(fe.BABYBEAR):
            eo, eot = fe.even_odd_inputs(), fe.even_odd_traces()
            tu, mu, pp = tuple_inputs(), mult_inputs(), push_pull_inputs()
            ma, sq, by, u32, py = fe.mul_air_inputs(), fe.squares_inputs(), fe.byte_operations_inputs(), fe.u32_add_system_inputs(), fe.pythagorean_inputs()
            sqt, pyt = fe.squares_traces(16), [fe.pythagorean_trace(4)]
        _CACHE["cases"] = {
            "even_odd": (eo, eot, [[0, 4, 1]], True),
            "even_odd_wrong_claim": (eo, eot, [[0, 4, 0]], False),
            "even_odd_no_claim": (eo, eot, [], False),
            "trailing_zero_row": (tu, [tuple_trace(5, 0)], [[5]], True),
            "empty_claim": (tu, [tuple_trace(0, 0)], [[]], True),
            "trailing_zero_row_longer_claim": (tu, [tuple_trace(5, 0)], [[5, 1]], False),
            "zero_row_longer_claim": (tu, [tuple_trace(0, 0)], [[5, 1]], False),
            "multiplicities": (mu, [mult_trace()], [], True),
            "hot": (pp, [hot_trace(1 << 13)], [], True),
            "hot_one_short": (pp, [hot_trace((1 << 13) - 1)], [], False),
            "distinct": (pp, [distinct_trace(1 << 13)], [], False),
            "distinct_256": (pp, [distinct_trace(256)], [], False),
            "mul_air": (ma, mul_air_traces(False), [], True),
            "mul_air_one_cell": (ma, mul_air_traces(True), [], True),
            "squares": (sq, sqt, [], True),
            "byte_ops": (by,) + byte_traces(False) + (True,),
            "byte_ops_one_cell": (by,) + byte_traces(True) + (False,),
            "u32": (u32,) + u32_traces(False) + (True,),
            "u32_one_cell": (u32,) + u32_traces(True) + (False,),
            "pythagorean": (py, pyt, [], True),
        }
    return _CACHE["cases"]


def compiled_of(name):
    """(blob, compiled circuits, oracle system) of a case's system, one per set of circuit inputs"""
    inputs = cases()[name][0]
    key = ("sys", id(inputs))
    if key not in _CACHE:
        blob, comp, _ = compile_system(inputs)
        _CACHE[key] = (blob, comp, ob.System(blob))
    return _CACHE[key]


def model_of(name, entries=64):
    """the model report of a case, computed once with every entry and cut to `entries`"""
    key = ("model", name)
    if key not in _CACHE:
        _, traces, claims, _ = cases()[name]
        _, comp, osys = compiled_of(name)
        _CACHE[key] = lm.balance(osys, comp, traces, pack(claims), 1 << 30)
    full = _CACHE[key]
    return lm.Report(full.messages, full.groups, full.unbalanced, full.entries[:entries], full.slot_counts, full.claims_count)


NAMES = ["even_odd", "even_odd_wrong_claim", "even_odd_no_claim", "trailing_zero_row", "empty_claim", "trailing_zero_row_longer_claim",
         "zero_row_longer_claim", "multiplicities", "hot", "hot_one_short", "distinct", "distinct_256", "mul_air", "mul_air_one_cell", "squares",
         "byte_ops", "byte_ops_one_cell", "u32", "u32_one_cell", "pythagorean"]


@pytest.mark.parametrize("name", NAMES)
def test_model_agrees_with_the_oracles_accumulator(name):
    _, traces, claims, balanced = cases()[name]
    _, comp, osys = compiled_of(name)
    m = model_of(name)
    assert (m.unbalanced == 0) == balanced and m.ok == balanced
    packed = pack(claims)
    for bg in (BG, BG2):
        assert lm.accumulator_is_zero(ob, osys, comp, traces, packed, *bg) == (m.unbalanced == 0), (name, bg)


def test_model_figures_on_the_small_cases():
    def figures(name):
        m = model_of(name)
        return (m.messages, m.groups, m.unbalanced)

    assert figures("even_odd") == (10, 5, 0)
    m = model_of("even_odd_wrong_claim")
    assert figures("even_odd_wrong_claim") == (10, 6, 2)
    assert m.entries == [(("claims", 0, 0), 1, 1, [0, 4]), ((0, 0, 0), P - 1, 1, [0, 4, 1])]
    assert m.claims_count == 1 and m.slot_counts[0][0] == 1
    m = model_of("even_odd_no_claim")
    assert m.unbalanced == 1 and m.entries[0][:2] == ((0, 0, 0), P - 1)
    assert figures("trailing_zero_row") == (2, 1, 0) and figures("empty_claim") == (2, 1, 0)
    assert figures("trailing_zero_row_longer_claim") == (2, 2, 2) and figures("zero_row_longer_claim") == (2, 2, 2)
    assert figures("multiplicities") == (6, 2, 0)
    assert figures("hot") == (8193, 1, 0)
    m = model_of("hot_one_short")
    assert m.entries == [((0, 0, 0), 1, 8193, [3, 4])] and m.groups == 1 and m.slot_counts == [[8192, 1]]
    m = model_of("distinct", entries=16)
    assert m.unbalanced == 8192 and [e[0] for e in m.entries] == [(0, r, 0) for r in range(16)]
    assert figures("mul_air") == (16384, 8192, 0) and figures("mul_air_one_cell") == (16384, 8192, 0)
    assert figures("squares") == (48, 16, 0)
    assert figures("byte_ops") == (9, 4, 0)
    m = model_of("byte_ops_one_cell")
    assert m.unbalanced == 1 and m.entries == [(("claims", 0, 0), P - 1, 3, [0, 3, 5, 6])] and m.slot_counts == [[1, 0, 0, 0]]
    assert figures("u32") == (14592, 1280, 0)
    m = model_of("u32_one_cell")
    assert m.unbalanced == 4 and m.claims_count == 1 and sum(map(sum, m.slot_counts)) > 3
    assert model_of("pythagorean").fields() == (0, 0, 0, [], [[]], 0)


def test_report_text_uses_the_fields_modulus():
    e = pkg.BalanceEntry((0, 0, 0), P - 1, 1, [0, 4, 1], p=P)
    assert e.line(["Even", "Odd"]) == "(0, 4, 1): net -1 over 1 message, first at circuit 0 (Even) row 0 lookup 0"
    gl = (1 << 64) - (1 << 32) + 1
    assert "net -1 " in pkg.BalanceEntry((0, 0, 0), gl - 1, 1, [1]).line() and "net %d " % (P - 1) in pkg.BalanceEntry((0, 0, 0), P - 1, 1, [1]).line()
    assert pkg.LookupBalanceReport(1, 1, 0, [], [[]], 0).p == gl and pkg.LookupBalanceReport(1, 1, 0, [], [[]], 0, p=P).p == P


def test_new_symbol_in_header_export_list_and_rust():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mstark_bb.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "mstark_sys.rs")).read()
    sym = "msbb_witness_lookup_balance"
    assert re.search(r"\b%s\s*\(" % sym, header) and sym in bb.exported_symbols() and ("pub fn %s(" % sym) in rust
    assert '#include "mstark.h"' in header and "MS_LB_ENTRY_WORDS" not in header  # (reused from mstark.h, not defined again)
    assert hasattr(bb.Witness, "lookup_balance")


def test_null_arguments_are_refused_before_any_device_work():
    L = pkg.lib()
    u64p = C.POINTER(C.c_uint64)
    summary = (C.c_uint64 * 4)()
    zero = C.c_size_t(0)
    assert L.msbb_witness_lookup_balance(None, summary, None, zero, None, zero, None, zero) == -1
    assert b"null argument" in L.ms_last_error()
    not_a_witness = (C.c_uint64 * 4)()  # any non-null address: a null summary is refused before the witness is looked at
    assert L.msbb_witness_lookup_balance(C.cast(not_a_witness, C.c_void_p), C.cast(None, u64p), None, zero, None, zero, None, zero) == -1
    assert b"null argument" in L.ms_last_error()
