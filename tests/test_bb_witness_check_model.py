"""CPU tests: the model of msbb_witness_check (tests/witness_check_model_bb.py) anchored to the BabyBear oracle - a witness the
oracle's prover and verifier accept is model-clean, one they reject is model-dirty - so that the GPU test
(test_gpu_bb_witness_check.py) does not compare the device with a model nobody has checked. Plus the additive pieces that need
no device: the new symbols in the header, the export list and the Rust declarations. The counterpart of
test_witness_check_model.py."""
import os
import re

import numpy as np
import pytest

import oracle_bb as ob
import witness_check_model_bb as wm
from __graft_entry__ import load_package

pkg = load_package()
fe = pkg.frontend
bb = pkg.babybear
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = wm.P
K = fe.poseidon2_constants()
BG = (bb.CHECK_BETA, bb.CHECK_GAMMA)
BG2 = ((5, 7, 11, 13), (17, 19, 23, 29))


@pytest.fixture(autouse=True)
def _perm():
    ob.set_poseidon2(K)


def compile_system(inputs, params=None):
    """(blob, CompiledCircuits, params) of a system authored over BabyBear"""
    with fe.field(fe.BABYBEAR):
        params = params or fe.test_params()
        comp = [fe.compile_circuit(ci) for ci in inputs]
        return fe.system_blob(params, comp, K), comp, params


def pack(claims):
    with fe.field(fe.BABYBEAR):
        return fe.pack_claims(claims)


def _model(inputs, traces, claims, bg=BG):
    blob, comp, _ = compile_system(inputs)
    osys = ob.System(blob)
    return wm.check(ob, osys, comp, traces, pack(claims), *bg), osys


def selector_inputs():
    """three columns pinned to the three selectors"""
    E = fe.Expr
    return [fe.CircuitInputs(3, None, [E.main(0) - fe.IS_FIRST_ROW, E.main(1) - fe.IS_LAST_ROW, E.main(2) - fe.IS_TRANSITION], [], [])]


def selector_trace(n, polynomial):
    first, last, trans = wm.selector_values(n)
    if not polynomial:  # the 0 / 1 flags a reader of the names might expect
        first, last, trans = [int(r == 0) for r in range(n)], [int(r == n - 1) for r in range(n)], [int(r != n - 1) for r in range(n)]
    return np.array([[int(first[r]), int(last[r]), int(trans[r])] for r in range(n)], dtype=np.uint64)


def bb_traces(which, rows=None):
    """the front-end's example traces computed over BabyBear (their inverses and reductions are the field's)"""
    with fe.field(fe.BABYBEAR):
        if which == "mul_air":
            return [fe.mul_air_smoke_trace() if rows is None else fe.mul_air_trace(rows)]
        if which == "even_odd":
            return fe.even_odd_traces()
        return [fe.pythagorean_trace(rows)]


def test_generator_is_the_fields():
    assert wm.generator(27) == 0x1A427A41 == pow(31, (P - 1) >> 27, P) and wm.generator(1) == P - 1 and wm.generator(0) == 1
    assert int(ob.lib().mso_gl_two_adic_generator(5)) == wm.generator(5)


def test_valid_witnesses_are_clean():
    with fe.field(fe.BABYBEAR):
        cases = [
            (fe.mul_air_inputs(), bb_traces("mul_air"), []),          # the reference's four rows
            (fe.mul_air_inputs(), bb_traces("mul_air", 16), []),
            (fe.even_odd_inputs(), bb_traces("even_odd"), [[0, 4, 1]]),
            (fe.pythagorean_inputs(), bb_traces("pythagorean", 8), []),
        ]
    for inputs, traces, claims in cases:
        packed = pack(claims)
        for bg in (BG, BG2):
            m, osys = _model(inputs, traces, claims, bg)
            assert m.verdict == 0, [c.fields() for c in m.circuits]
            assert all(c.failing_rows == 0 and c.first_failure is None and not any(c.root_counts) for c in m.circuits)
            assert [c.height for c in m.circuits] == [t.shape[0] for t in traces] and m.final_accumulator == (0, 0, 0, 0)
        assert osys.verify(packed, osys.prove(traces, packed)) == 0


@pytest.mark.parametrize("n", [4, 8, 32])
def test_selectors_are_polynomial_values_not_flags(n):
    packed = pack([])
    good, bad = selector_trace(n, True), selector_trace(n, False)
    m, osys = _model(selector_inputs(), [good], [])
    assert m.verdict == 0
    assert osys.verify(packed, osys.prove([good], packed)) == 0
    m, _ = _model(selector_inputs(), [bad], [])
    assert m.verdict == 1
    c = m.circuits[0]
    # is_first: only row 0 differs (1 against n); is_last: only row n - 1; is_transition: w^r - w^-1 is 1 nowhere but by accident
    assert c.root_counts[0] == 1 and c.root_first[0] == 0 and c.root_counts[1] == 1 and c.root_first[1] == n - 1
    assert c.root_counts[2] >= n - 1 and c.first_failure == (0, 0, (1 - n) % P)
    assert osys.verify(packed, osys.prove([bad], packed)) != 0


def test_one_corrupted_cell():
    with fe.field(fe.BABYBEAR):
        inputs = fe.mul_air_inputs()
    tr = bb_traces("mul_air", 16)[0]
    tr[5, 1] += 1  # b of row 5: (a, c) - all that the self-cancelling lookups read - stay as they are
    m, osys = _model(inputs, [tr], [])
    c = m.circuits[0]
    assert m.verdict == 1 and c.failing_rows == 1 and c.root_counts == [1] and c.root_first == [5]
    assert c.first_failure == (5, 0, (6 * 8 - 6 * 7) % P)
    packed = pack([])
    assert osys.verify(packed, osys.prove([tr], packed)) != 0


def test_unbalanced_lookups_only_set_bit_1():
    with fe.field(fe.BABYBEAR):
        inputs = fe.even_odd_inputs()
    for claims in ([[0, 4, 0]], []):
        m, _ = _model(inputs, bb_traces("even_odd"), claims)
        assert m.verdict == 2 and not any(any(c.root_counts) for c in m.circuits) and m.final_accumulator != (0, 0, 0, 0)


def test_default_challenges_are_canonical_and_distinct():
    words = bb.CHECK_BETA + bb.CHECK_GAMMA
    assert len(bb.CHECK_BETA) == len(bb.CHECK_GAMMA) == 4 and all(1 < x < P for x in words) and len(set(words)) == 8


def test_null_arguments_are_refused_before_any_device_work():
    import ctypes as C

    L = pkg.lib()
    out4, v = (C.c_uint64 * 4)(), C.c_uint32()
    assert L.msbb_witness_check(None, None, None, C.byref(v), None, None, None, C.c_size_t(0)) == -1
    assert b"null argument" in L.ms_last_error()
    assert L.msbb_system_check_info(None, C.c_size_t(0), out4) == -1 and b"null argument" in L.ms_last_error()


def test_new_symbols_in_header_export_list_and_rust():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mstark_bb.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "mstark_sys.rs")).read()
    for sym in ("msbb_witness_check", "msbb_system_check_info"):
        assert re.search(r"\b%s\s*\(" % sym, header) and sym in bb.exported_symbols() and ("pub fn %s(" % sym) in rust
    assert re.search(r"#define\s+MSBB_CHECK_CIRCUIT_WORDS\s+12\b", header) and "MSBB_CHECK_CIRCUIT_WORDS: usize = 12" in rust
    assert hasattr(bb.Witness, "check") and hasattr(bb.System, "check_info") and bb.CHECK_CIRCUIT_WORDS == 12
