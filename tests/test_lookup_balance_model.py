"""CPU tests: the model of ms_witness_lookup_balance (tests/lookup_balance_model.py) anchored to the oracle. On every witness the
GPU test (test_gpu_lookup_balance.py) uses, the model finds no unbalanced group exactly when the oracle's chained accumulator
is zero under two pairs of challenges: the one CPU-checkable tie between the exact definition and the protocol, so that the
device is not compared with a model nobody has checked. The witnesses are built here, once, and shared with the GPU test."""
import importlib
import os
import re

import numpy as np
import pytest

import lookup_balance_model as lm
from test_witness_check_model import BG, BG2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = lm.P
_CACHE = {}


def tuple_inputs(fe):
    """one circuit, one slot: pull(main(2), [main(0), main(1)])"""
    E = fe.Expr
    return [fe.CircuitInputs(3, None, [], [], [fe.Lookup.pull(E.main(2), [E.main(0), E.main(1)])])]


def mult_inputs(fe):
    """one circuit, one slot whose multiplicity is a column as it stands: push(main(0), [main(1)])"""
    E = fe.Expr
    return [fe.CircuitInputs(2, None, [], [], [fe.Lookup.push(E.main(0), [E.main(1)])])]


def push_pull_inputs(fe):
    """one circuit, two slots over the same tuple: push(main(0), [main(1), main(2)]) and pull(main(3), [main(1), main(2)])"""
    E = fe.Expr
    args = [E.main(1), E.main(2)]
    return [fe.CircuitInputs(4, None, [], [], [fe.Lookup.push(E.main(0), args), fe.Lookup.pull(E.main(3), args)])]


def tuple_trace(a, b):
    tr = np.zeros((4, 3), dtype=np.uint64)
    tr[0] = [a, b, 1]
    return tr


def mult_trace():
    """2^63 and p - 2^63 on one tuple (neither small nor small negative), p - 1 three times and 3 once on another, and a tuple
    whose only member has multiplicity 0"""
    rows = [[1 << 63, 7], [P - (1 << 63), 7], [P - 1, 9], [P - 1, 9], [3, 9], [P - 1, 9], [0, 11], [0, 0]]
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


def u32_traces(fe, corrupt):
    traces, claims = fe.u32_add_bench_witness(1 << 10)
    traces = [t.copy() for t in traces]
    if corrupt:
        traces[1][5, 0] ^= np.uint64(1)  # one byte of x in row 5: the byte's two tuples and the u32 tuple of claim and row
    return traces, [list(int(v) for v in c) for c in claims]


def blake3_nine(b3):
    """the nine compressions of the existing check test"""
    claims = [b3.compression_claim(i) for i in b3.blake3_compressions(bytes(range(256)) * 2 + b"tail")[0]]
    assert len(claims) == 9
    return claims


def cases(fe, b3):
    """name -> (circuit inputs, traces, claims, balanced): every witness of test_gpu_lookup_balance.py"""
    if "cases" not in _CACHE:
        eo, tu, mu, pp, u32 = fe.even_odd_inputs(), tuple_inputs(fe), mult_inputs(fe), push_pull_inputs(fe), fe.u32_add_system_inputs()
        bt, bc = fe.u32_add_bench_witness(1 << 12)
        b3c = blake3_nine(b3)
        _CACHE["cases"] = {
            "even_odd": (eo, fe.even_odd_traces(), [[0, 4, 1]], True),
            "even_odd_wrong_claim": (eo, fe.even_odd_traces(), [[0, 4, 0]], False),
            "even_odd_no_claim": (eo, fe.even_odd_traces(), [], False),
            "trailing_zero_row": (tu, [tuple_trace(5, 0)], [[5]], True),
            "empty_claim": (tu, [tuple_trace(0, 0)], [[]], True),
            "trailing_zero_row_longer_claim": (tu, [tuple_trace(5, 0)], [[5, 1]], False),
            "zero_row_longer_claim": (tu, [tuple_trace(0, 0)], [[5, 1]], False),
            "multiplicities": (mu, [mult_trace()], [], True),
            "hot": (pp, [hot_trace(1 << 13)], [], True),
            "hot_one_short": (pp, [hot_trace((1 << 13) - 1)], [], False),
            "distinct": (pp, [distinct_trace(1 << 13)], [], False),
            "distinct_256": (pp, [distinct_trace(256)], [], False),
            "u32": (u32,) + u32_traces(fe, False) + (True,),
            "u32_one_cell": (u32,) + u32_traces(fe, True) + (False,),
            "bench_4096": (u32, bt, [list(int(v) for v in c) for c in bc], True),
            "blake3_nine": (b3.blake3_system_inputs(), b3.blake3_witness(b3c), b3c, True),
            "pythagorean": (fe.pythagorean_inputs(), [fe.pythagorean_trace(4)], [], True),
        }
    return _CACHE["cases"]


def model_of(oracle, fe, b3, name, entries=64):
    """(model report, oracle system, compiled circuits) of a case; the report for entries = 64 is computed once"""
    key = ("model", name)
    if key not in _CACHE:
        inputs, traces, claims, _ = cases(fe, b3)[name]
        comp = [fe.compile_circuit(ci) for ci in inputs]
        osys = oracle.System(fe.system_blob(fe.test_params(), comp))
        _CACHE[key] = (lm.balance(osys, comp, traces, fe.pack_claims(claims), 1 << 30), osys, comp)
    full, osys, comp = _CACHE[key]
    return lm.Report(full.messages, full.groups, full.unbalanced, full.entries[:entries], full.slot_counts, full.claims_count), osys, comp


@pytest.fixture(scope="module")
def b3(pkg):
    return importlib.import_module("multi_stark_amd.blake3_circuit")


NAMES = ["even_odd", "even_odd_wrong_claim", "even_odd_no_claim", "trailing_zero_row", "empty_claim", "trailing_zero_row_longer_claim",
         "zero_row_longer_claim", "multiplicities", "hot", "hot_one_short", "distinct", "distinct_256", "u32", "u32_one_cell", "bench_4096",
         "blake3_nine", "pythagorean"]


@pytest.mark.parametrize("name", NAMES)
def test_model_agrees_with_the_oracles_accumulator(oracle, fe, b3, name):
    inputs, traces, claims, balanced = cases(fe, b3)[name]
    m, osys, comp = model_of(oracle, fe, b3, name)
    assert (m.unbalanced == 0) == balanced and m.ok == balanced
    packed = fe.pack_claims(claims)
    for bg in (BG, BG2):
        assert lm.accumulator_is_zero(oracle, osys, comp, traces, packed, *bg) == (m.unbalanced == 0), (name, bg)


def test_model_figures_on_the_small_cases(oracle, fe, b3):
    m, _, _ = model_of(oracle, fe, b3, "even_odd_wrong_claim")
    assert m.unbalanced == 2 and m.entries == [(("claims", 0, 0), 1, 1, [0, 4]), ((0, 0, 0), P - 1, 1, [0, 4, 1])]
    assert m.claims_count == 1 and m.slot_counts[0][0] == 1
    m, _, _ = model_of(oracle, fe, b3, "even_odd_no_claim")
    assert m.unbalanced == 1 and m.entries[0][0] == (0, 0, 0)
    m, _, _ = model_of(oracle, fe, b3, "multiplicities")
    assert (m.messages, m.groups, m.unbalanced) == (6, 2, 0)
    m, _, _ = model_of(oracle, fe, b3, "hot_one_short")
    assert m.entries == [((0, 0, 0), 1, 8193, [3, 4])] and m.groups == 1
    m, _, _ = model_of(oracle, fe, b3, "distinct", entries=16)
    assert m.unbalanced == 8192 and [e[0] for e in m.entries] == [(0, r, 0) for r in range(16)]
    m, _, _ = model_of(oracle, fe, b3, "u32_one_cell")
    assert m.unbalanced == 4 and m.claims_count == 1 and sum(map(sum, m.slot_counts)) > 3
    m, _, _ = model_of(oracle, fe, b3, "pythagorean")
    assert m.fields() == (0, 0, 0, [], [[]], 0)


def test_new_symbol_in_header_export_list_and_rust(pkg):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mstark.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "mstark_sys.rs")).read()
    sym = "ms_witness_lookup_balance"
    assert re.search(r"\b%s\s*\(" % sym, header) and sym in pkg.exported_symbols() and ("pub fn %s(" % sym) in rust
    assert "#define MS_LB_ENTRY_WORDS 8" in header and "MS_LB_ENTRY_WORDS: usize = 8" in rust and pkg.LB_ENTRY_WORDS == 8
    assert hasattr(pkg.SystemWitness, "lookup_balance")
