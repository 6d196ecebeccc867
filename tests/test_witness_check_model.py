"""CPU tests: the model of ms_witness_check (tests/witness_check_model.py) anchored to the oracle - a witness the oracle's
prover and verifier accept is model-clean, one they reject is model-dirty - so that the GPU test (test_gpu_witness_check.py)
does not compare the device with a model nobody has checked. Plus the additive pieces that need no device: zero_origins of
the front-end and the new symbols in the header, the export list and the Rust declarations."""
import importlib
import os
import re

import numpy as np
import pytest

import witness_check_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BG = ((0x243F6A8885A308D3, 0x13198A2E03707344), (0xA4093822299F31D0, 0x082EFA98EC4E6C89))
BG2 = ((5, 7), (11, 13))


def _sys(oracle, fe, inputs, params=None):
    comp = [fe.compile_circuit(ci) for ci in inputs]
    return oracle.System(fe.system_blob(params or fe.test_params(), comp)), comp


def _model(oracle, fe, inputs, traces, claims, bg=BG):
    osys, comp = _sys(oracle, fe, inputs)
    return wm.check(oracle, osys, comp, traces, fe.pack_claims(claims), *bg), osys


def selector_inputs(fe):
    """three columns pinned to the three selectors"""
    E = fe.Expr
    return [fe.CircuitInputs(3, None, [E.main(0) - fe.IS_FIRST_ROW, E.main(1) - fe.IS_LAST_ROW, E.main(2) - fe.IS_TRANSITION], [], [])]


def selector_trace(n, polynomial):
    first, last, trans = wm.selector_values(n)
    if not polynomial:  # the 0 / 1 flags a reader of the names might expect
        first, last, trans = [int(r == 0) for r in range(n)], [int(r == n - 1) for r in range(n)], [int(r != n - 1) for r in range(n)]
    return np.array([[int(first[r]), int(last[r]), int(trans[r])] for r in range(n)], dtype=np.uint64)


def test_valid_witnesses_are_clean(oracle, fe):
    cases = [
        (fe.pythagorean_inputs(), [fe.pythagorean_trace(8)], []),
        (fe.u32_add_system_inputs(),) + tuple(fe.u32_add_witness([(10, 5), (30, 20), (100, 100), (8000, 10000)])),
        (fe.even_odd_inputs(), fe.even_odd_traces(), [[0, 4, 1]]),
        (fe.byte_operations_inputs(),) + tuple(fe.byte_operations_witness([(0, 10, 5), (1, 30, 20), (2, 100, 40), (3, 200, 100)])),
        (fe.squares_inputs(), fe.squares_traces(16), []),
        (fe.verifier_test_inputs(), fe.verifier_test_traces(), []),
    ]
    for inputs, traces, claims in cases:
        claims = [list(c) for c in np.asarray(claims, dtype=object)] if not isinstance(claims, list) else claims
        for bg in (BG, BG2):
            m, _ = _model(oracle, fe, inputs, traces, claims, bg)
            assert m.verdict == 0, [c.fields() for c in m.circuits]
            assert all(c.failing_rows == 0 and c.first_failure is None and not any(c.root_counts) for c in m.circuits)
            assert [c.height for c in m.circuits] == [t.shape[0] for t in traces]


def test_blake3_system_one_short_hash_is_clean(oracle, fe, pkg):
    b3 = importlib.import_module("multi_stark_amd.blake3_circuit")
    claims = [b3.compression_claim(i) for i in b3.blake3_compressions(b"abc")[0]]
    traces = b3.blake3_witness(claims)
    m, _ = _model(oracle, fe, b3.blake3_system_inputs(), traces, claims)
    assert m.verdict == 0, [(i, c.failing_rows, c.first_failure) for i, c in enumerate(m.circuits)]
    assert sum(c.roots for c in m.circuits) > 100  # the compression circuit's roots were evaluated


@pytest.mark.parametrize("n", [4, 8, 32])
def test_selectors_are_polynomial_values_not_flags(oracle, fe, n):
    packed = fe.pack_claims([])
    good, bad = selector_trace(n, True), selector_trace(n, False)
    m, osys = _model(oracle, fe, selector_inputs(fe), [good], [])
    assert m.verdict == 0
    assert osys.verify(packed, osys.prove([good], packed)) == 0
    m, _ = _model(oracle, fe, selector_inputs(fe), [bad], [])
    assert m.verdict == 1
    c = m.circuits[0]
    # is_first: only row 0 differs (1 against n); is_last: only row n - 1; is_transition: w^r - w^-1 is 1 nowhere but by accident
    assert c.root_counts[0] == 1 and c.root_first[0] == 0 and c.root_counts[1] == 1 and c.root_first[1] == n - 1
    assert c.root_counts[2] >= n - 1 and c.first_failure[:2] == (0, 0) and c.first_failure[2] == (1 - n) % wm.P
    assert osys.verify(packed, osys.prove([bad], packed)) != 0


def test_one_corrupted_cell(oracle, fe):
    tr = fe.pythagorean_trace(8)
    tr[3, 2] += 1
    m, osys = _model(oracle, fe, fe.pythagorean_inputs(), [tr], [])
    c = m.circuits[0]
    assert m.verdict == 1 and c.failing_rows == 1 and c.root_counts == [1] and c.root_first == [3]
    assert c.first_failure == (3, 0, (7 * 7 + 24 * 24 - 26 * 26) % wm.P)
    packed = fe.pack_claims([])
    assert osys.verify(packed, osys.prove([tr], packed)) != 0


def test_unbalanced_lookups_only_set_bit_1(oracle, fe):
    for claims in ([[0, 4, 0]], []):
        m, _ = _model(oracle, fe, fe.even_odd_inputs(), fe.even_odd_traces(), claims)
        assert m.verdict == 2 and not any(any(c.root_counts) for c in m.circuits)


def test_zero_origins_cover_every_authored_constraint(fe, pkg):
    b3 = importlib.import_module("multi_stark_amd.blake3_circuit")
    E, X = fe.Expr, fe.ExtExpr
    ext = fe.CircuitInputs(2, None, [E.main(0) * E.main(1) - E.main(1) * E.main(0), E.main(0) - E.main(1), E.main(0) - E.main(1)],
                           [X.coords([E.var(2, 0, 0), E.var(2, 0, 1)]) * X.base(E.main(0)) - X.coords([E.public(4), E.public(5)])], [])
    systems = [fe.pythagorean_inputs(), fe.u32_add_system_inputs(), fe.even_odd_inputs(), fe.squares_inputs(), fe.verifier_test_inputs(),
               b3.blake3_system_inputs(), [ext]]
    for inputs in systems:
        for ci in inputs:
            cc = fe.compile_circuit(ci)
            assert len(cc.zero_origins) == len(cc.zeros) and all(cc.zero_origins)
            seen = sorted(o for os_ in cc.zero_origins for o in os_)
            assert len(seen) == len(set(seen))
            # every authored constraint appears, except those that fold to the constant zero
            it = fe._Interner()
            spec = {"main_width": ci.main_width, "preprocessed_width": 0 if ci.preprocessed is None else int(ci.preprocessed.shape[1]),
                    "stage2_width": max(len(ci.lookups), 1) * 2, "num_publics": 8}
            for lk in ci.lookups:  # (the interner numbers nodes in compile order: lookups first)
                it.compile_expr(lk.multiplicity, spec, False)
                [it.compile_expr(a, spec, False) for a in lk.args]
            want = []
            for i, c in enumerate(ci.constraints):
                if it.as_const(it.compile_expr(c, spec, False)) is None:
                    want.append(("constraint", i))
            for i, c in enumerate(ci.ext_constraints):
                for k, root in enumerate(it.expand_ext(c, spec, 2, 7, True)):
                    if it.as_const(root) is None:
                        want.append(("ext", i, k))
            assert seen == sorted(want)
    cc = fe.compile_circuit(ext)
    assert [("constraint", 1), ("constraint", 2)] in cc.zero_origins  # two authored constraints, one root
    assert not any(("constraint", 0) in o for o in cc.zero_origins)   # a b - b a folds to zero


def test_new_symbols_in_header_export_list_and_rust(pkg):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mstark.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "mstark_sys.rs")).read()
    for sym in ("ms_witness_check", "ms_system_check_info"):
        assert re.search(r"\b%s\s*\(" % sym, header) and sym in pkg.exported_symbols() and ("pub fn %s(" % sym) in rust
    assert hasattr(pkg.SystemWitness, "check") and "witness_check" in [pkg.lib().ms_kernel_name(i).decode() for i in range(pkg.lib().ms_kernel_count())]
