"""CPU tests: the model of ms_witness_derive_multiplicities (tests/multiplicity_model.py) pinned against counting it did not do
itself. The witness builders of frontend.py fill their tables' multiplicity columns with np.bincount (or += 1 per call); the
model, given those witnesses with the derived columns overwritten by garbage, must return exactly the builders' columns and find
nothing unserved - so that the device (test_gpu_derive_multiplicities.py, which shares the cases built here) is not compared with
a model nobody has checked. Also the eligibility classification on compiled circuits."""
import os
import re

import numpy as np
import pytest

import multiplicity_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = mm.P
_CACHE = {}


def byte_calls():
    """about 300 calls of the byte operations: random ones, repeats of some of them, and the all-zero calls whose tuples strip
    to length 0 ((0, 0, 0): xor gives (0, 0, 0, 0)) or 1 ((1, 0, 0), (3, 0, 0))"""
    rng = np.random.default_rng(20240607)
    calls = [(int(op), int(x), int(y)) for op, x, y in zip(rng.integers(0, 4, 260), rng.integers(0, 256, 260), rng.integers(0, 256, 260))]
    calls += calls[:30] + calls[5:10] * 2
    calls += [(0, 0, 0), (1, 0, 0), (3, 0, 0), (0, 0, 0), (2, 255, 255), (0, 77, 77)]
    return calls


def u32_pairs(n):
    rng = np.random.default_rng(n)
    return [(int(x), int(y)) for x, y in zip(rng.integers(0, 1 << 32, n), rng.integers(0, 1 << 32, n))]


def claim_lists(claims):
    return [[int(v) for v in c] for c in claims]


def cases(fe):
    """name -> (circuit inputs, the builder's traces, claims, targets)"""
    if "cases" not in _CACHE:
        u32 = fe.u32_add_system_inputs()
        out = {}
        for n in (16, 128, 4096):
            traces, claims = fe.u32_add_witness(u32_pairs(n))
            out["u32_%d" % n] = (u32, traces, claim_lists(claims), [(0, 0)])
        traces, claims = fe.u32_add_bench_witness(1 << 10)
        out["u32_bench_1024"] = (u32, traces, claim_lists(claims), [(0, 0)])
        out["squares_16"] = (fe.squares_inputs(), fe.squares_traces(16), [], [(0, 0)])
        traces, claims = fe.byte_operations_witness(byte_calls())
        out["byte_ops"] = (fe.byte_operations_inputs(), traces, claims, [(0, 0), (0, 1), (0, 2), (0, 3)])
        _CACHE["cases"] = out
    return _CACHE["cases"]


def system_of(oracle, fe, inputs):
    """(oracle system, compiled circuits) of a list of circuit inputs, built once"""
    key = ("sys", id(inputs))
    if key not in _CACHE:
        comp = [fe.compile_circuit(ci) for ci in inputs]
        _CACHE[key] = (oracle.System(fe.system_blob(fe.test_params(), comp)), comp, inputs)  # (inputs: keeps the id alive)
    return _CACHE[key][:2]


def garbage(traces, compiled, targets, fill=None):
    """copies of the traces with every derived column overwritten: by `fill`, or by arbitrary canonical values"""
    out = [np.array(t, dtype=np.uint64) for t in traces]
    rng = np.random.default_rng(99)
    for c, j in targets:
        col = mm.classify(compiled[c], j)[1]
        out[c][:, col] = rng.integers(0, P, len(out[c]), dtype=np.uint64) if fill is None else fill
    return out


def model_of(oracle, fe, name, entries=64):
    """(derived traces, report) of the model on a case's witness with garbage in the derived columns; computed once"""
    key = ("model", name)
    if key not in _CACHE:
        inputs, traces, claims, targets = cases(fe)[name]
        osys, comp = system_of(oracle, fe, inputs)
        _CACHE[key] = mm.derive(osys, comp, garbage(traces, comp, targets), fe.pack_claims(claims), targets, 1 << 30)
    derived, full = _CACHE[key]
    return derived, mm.Report(full.demand_messages, full.demand_groups, full.served, full.unserved, full.duplicates, full.entries[:entries])


@pytest.mark.parametrize("name", ["u32_16", "u32_128", "u32_bench_1024", "squares_16", "byte_ops"])
def test_model_returns_the_builders_columns(oracle, fe, name):
    _, traces, _, targets = cases(fe)[name]
    derived, rep = model_of(oracle, fe, name)
    assert rep.unserved == 0 and rep.ok and rep.entries == []
    for got, want in zip(derived, traces):
        assert np.array_equal(got, np.asarray(want, dtype=np.uint64)), name
    assert rep.served > 0 and rep.demand_groups >= rep.served


def test_model_figures(oracle, fe):
    _, rep = model_of(oracle, fe, "u32_16")
    # 16 claims + 16 u32 pulls on 16 tuples of net 0, 12 x 16 byte pushes on the bytes that occur
    traces = cases(fe)["u32_16"][1]
    occurring = int(np.count_nonzero(traces[0][:, 0]))
    assert (rep.demand_messages, rep.demand_groups, rep.served, rep.duplicates) == (16 * 14, 16 + occurring, occurring, 0)
    _, rep = model_of(oracle, fe, "byte_ops")
    calls = byte_calls()
    assert rep.demand_messages == len(calls) and rep.served == rep.demand_groups == len(set(calls)) and rep.duplicates == 0


def test_eligibility_on_the_u32_add_system(fe):
    comp = [fe.compile_circuit(ci) for ci in fe.u32_add_system_inputs()]
    assert mm.classify(comp[0], 0) == (0, 0, True)  # ByteTable: pull(main(0), ...)
    assert mm.classify(comp[1], 0) == (0, 13, True)  # U32Add: pull(main(13), ...)
    for j in range(1, 13):
        assert mm.classify(comp[1], j)[0] == 1  # push(1, ...): a constant multiplicity
    sq = [fe.compile_circuit(ci) for ci in fe.squares_inputs()]
    assert mm.classify(sq[0], 0) == (0, 0, True)
    assert mm.classify(sq[1], 0)[0] == 2 and mm.classify(sq[1], 1)[0] == 2  # both slots push main(4): each reads the other's column


def code2_inputs(fe):
    """slot 0's column is an argument of slot 1; slot 2's multiplicity is a product; slot 3 reads the next row"""
    E = fe.Expr
    lookups = [fe.Lookup.pull(E.main(0), [E.main(1)]), fe.Lookup.push(E.const(1), [E.main(0) * E.const(2) + E.main(1)]),
               fe.Lookup.push(E.main(2) * E.main(1), [E.main(1)]), fe.Lookup.push(E.main_next(3), [E.main(1)]), fe.Lookup.push(E.main(3), [E.main(1)])]
    return [fe.CircuitInputs(4, None, [], [], lookups)]


def test_eligibility_codes_follow_the_node_program(fe):
    cc = fe.compile_circuit(code2_inputs(fe)[0])
    assert mm.classify(cc, 0) == (2, 0, True)  # read inside another slot's argument
    assert mm.classify(cc, 1)[0] == 1 and mm.classify(cc, 2)[0] == 1 and mm.classify(cc, 3)[0] == 1
    assert mm.classify(cc, 4) == (2, 3, False)  # slot 3's multiplicity reads column 3 at the next row
    # -(-x) folds to x: the authoring form says pull of a negation, the node program says push
    E = fe.Expr
    cc = fe.compile_circuit(fe.CircuitInputs(2, None, [], [], [fe.Lookup.pull(-E.main(0), [E.main(1)])]))
    assert mm.classify(cc, 0) == (0, 0, False)


def test_model_refuses_misuse(oracle, fe):
    inputs, traces, claims, _ = cases(fe)["u32_16"]
    osys, comp = system_of(oracle, fe, inputs)
    packed = fe.pack_claims(claims)
    for bad in ([(1, 1)], [(0, 0), (0, 0)], [(2, 0)], [(0, 1)]):
        with pytest.raises(mm.Misuse):
            mm.derive(osys, comp, traces, packed, bad)


def test_new_symbols_in_header_export_list_and_rust(pkg):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mstark.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "mstark_sys.rs")).read()
    for sym in ("ms_witness_derive_multiplicities", "ms_system_multiplicity_slot"):
        assert re.search(r"\b%s\s*\(" % sym, header) and sym in pkg.exported_symbols() and ("pub fn %s(" % sym) in rust
    assert "#define MS_DM_SUMMARY_WORDS 6" in header and "MS_DM_SUMMARY_WORDS: usize = 6" in rust and pkg.DM_SUMMARY_WORDS == 6
    assert "pub struct ms_mult_target" in rust and hasattr(pkg.SystemWitness, "derive_multiplicities") and hasattr(pkg.System, "multiplicity_slot")
