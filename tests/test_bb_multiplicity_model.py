"""CPU tests: the model of msbb_witness_derive_multiplicities (tests/multiplicity_model_bb.py) pinned against counting it did not
do itself. The witness builders of frontend.py fill their tables' multiplicity columns with np.bincount (or += 1 per call); the
model, given those witnesses built over BabyBear with the derived columns overwritten by garbage, must return exactly the
builders' columns and find nothing unserved - so that the device (test_gpu_bb_derive_multiplicities.py, which shares the cases
built here) is not compared with a model nobody has checked. Also the eligibility classification on circuits compiled over
BabyBear, and the additive pieces that need no device. The counterpart of test_multiplicity_model.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import multiplicity_model_bb as mm
import oracle_bb as ob
from test_bb_witness_check_model import K, bb, compile_system, fe, pack, pkg
from test_multiplicity_model import byte_calls, claim_lists, code2_inputs, u32_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = mm.P
_CACHE = {}


@pytest.fixture(autouse=True)
def _perm():
    ob.set_poseidon2(K)


def wrap_inputs():
    """a four-row table pulled by its multiplicity column, and a pusher [value, multiplicity]: push(main(1), [main(0)])"""
    E = fe.Expr
    table = fe.CircuitInputs(1, np.array([[7], [9], [9], [11]], dtype=np.uint64), [], [], [fe.Lookup.pull(E.main(0), [E.preprocessed(0)])])
    return [table, fe.CircuitInputs(2, None, [], [], [fe.Lookup.push(E.main(1), [E.main(0)])])]


def wrap_traces():
    """7 is pushed (p - 1) / 2 + (p + 1) / 2 = p times: one wrap of p, net 0. 9 is pushed 2 (p - 1) + 5 = 3 times (mod p), and
    two table rows hold it. 11 is pushed p - 2 times and once with multiplicity 0, a message that does not exist"""
    rows = [[7, (P - 1) // 2], [7, (P + 1) // 2], [9, P - 1], [9, P - 1], [9, 5], [11, P - 2], [11, 0], [0, 0]]
    return [np.full((4, 1), 12345, dtype=np.uint64), np.array(rows, dtype=np.uint64)]


def cases():
    """name -> (circuit inputs, the builder's traces, claims reduced mod p, targets)"""
    if "cases" not in _CACHE:
        with fe.field(fe.BABYBEAR):
            u32, sq, by = fe.u32_add_system_inputs(), fe.squares_inputs(), fe.byte_operations_inputs()
            out = {}
            for n in (16, 128):
                traces, claims = fe.u32_add_witness(u32_pairs(n))
                out["u32_%d" % n] = (u32, traces, [[v % P for v in c] for c in claim_lists(claims)], [(0, 0)])
            out["squares_16"] = (sq, fe.squares_traces(16), [], [(0, 0)])
            traces, claims = fe.byte_operations_witness(byte_calls())
            out["byte_ops"] = (by, traces, [[int(v) % P for v in c] for c in claims], [(0, 0), (0, 1), (0, 2), (0, 3)])
            out["wrap"] = (wrap_inputs(), wrap_traces(), [], [(0, 0)])
        _CACHE["cases"] = out
    return _CACHE["cases"]


def compiled_of(inputs):
    """(blob, compiled circuits, oracle system) of a list of circuit inputs, built once"""
    key = ("sys", id(inputs))
    if key not in _CACHE:
        blob, comp, _ = compile_system(inputs)
        _CACHE[key] = (blob, comp, ob.System(blob), inputs)  # (inputs: keeps the id alive)
    return _CACHE[key][:3]


def garbage(traces, compiled, targets, fill=None):
    """copies of the traces with every derived column overwritten: by `fill`, or by arbitrary values below the BabyBear p"""
    out = [np.array(t, dtype=np.uint64) for t in traces]
    rng = np.random.default_rng(99)
    for c, j in targets:
        col = mm.classify(compiled[c], j)[1]
        out[c][:, col] = rng.integers(0, P, len(out[c]), dtype=np.uint64) if fill is None else fill
    return out


def model_of(name, entries=64):
    """(derived traces, report) of the model on a case's witness with garbage in the derived columns; computed once"""
    key = ("model", name)
    if key not in _CACHE:
        inputs, traces, claims, targets = cases()[name]
        _, comp, osys = compiled_of(inputs)
        _CACHE[key] = mm.derive(osys, comp, garbage(traces, comp, targets), pack(claims), targets, 1 << 30)
    derived, full = _CACHE[key]
    return derived, mm.Report(full.demand_messages, full.demand_groups, full.served, full.unserved, full.duplicates, full.entries[:entries])


# (demand messages, groups, served, unserved, duplicates): a BabyBear copy of the model run on these inputs by hand
FIGURES = {"u32_16": (224, 163, 147, 0, 0), "u32_128": (1792, 382, 254, 0, 0), "byte_ops": (306, 265, 265, 0, 0), "squares_16": (32, 16, 16, 0, 0)}


@pytest.mark.parametrize("name", ["u32_16", "u32_128", "byte_ops", "squares_16"])
def test_model_returns_the_builders_columns(name):
    _, traces, _, _ = cases()[name]
    derived, rep = model_of(name)
    assert rep.unserved == 0 and rep.ok and rep.entries == []
    for got, want in zip(derived, traces):
        assert np.array_equal(got, np.asarray(want, dtype=np.uint64)), name
    assert rep.fields()[:5] == FIGURES[name]


def test_a_sum_that_wraps_p_is_no_demand_and_a_repeated_row_is_a_duplicate():
    derived, rep = model_of("wrap")
    assert derived[0][:, 0].tolist() == [0, 3, 0, P - 2]
    assert rep.fields()[:5] == (6, 3, 2, 0, 1) and rep.ok  # the group of 7 nets to zero: a group, but not a served one
    assert np.array_equal(derived[1], cases()["wrap"][1][1])


def test_eligibility_does_not_depend_on_the_field():
    comp = compile_system(fe.u32_add_system_inputs())[1]
    assert mm.classify(comp[0], 0) == (0, 0, True)  # ByteTable: pull(main(0), ...)
    assert mm.classify(comp[1], 0) == (0, 13, True)  # U32Add: pull(main(13), ...)
    for j in range(1, 13):
        assert mm.classify(comp[1], j)[0] == 1  # push(1, ...): a constant multiplicity
    sq = compile_system(fe.squares_inputs())[1]
    assert mm.classify(sq[0], 0) == (0, 0, True)
    assert mm.classify(sq[1], 0)[0] == 2 and mm.classify(sq[1], 1)[0] == 2  # both slots push main(4): each reads the other's column
    cc = compile_system(code2_inputs(fe))[1][0]
    assert mm.classify(cc, 0) == (2, 0, True)  # read inside another slot's argument
    assert mm.classify(cc, 1)[0] == 1 and mm.classify(cc, 2)[0] == 1 and mm.classify(cc, 3)[0] == 1
    assert mm.classify(cc, 4) == (2, 3, False)  # slot 3's multiplicity reads column 3 at the next row


def test_model_refuses_misuse():
    inputs, traces, claims, _ = cases()["u32_16"]
    _, comp, osys = compiled_of(inputs)
    for bad in ([(1, 1)], [(0, 0), (0, 0)], [(2, 0)], [(0, 1)]):
        with pytest.raises(mm.Misuse):
            mm.derive(osys, comp, traces, pack(claims), bad)


SYMBOLS = ("msbb_system_multiplicity_slot", "msbb_witness_derive_multiplicities", "msbb_witness_trace")


def test_new_symbols_in_header_export_list_and_rust():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mstark_bb.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "mstark_sys.rs")).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header) and sym in bb.exported_symbols() and ("pub fn %s(" % sym) in rust, sym
    # reused from mstark.h, not defined again
    assert '#include "mstark.h"' in header and "define MS_DM_SUMMARY_WORDS" not in header and not re.search(r"struct\s+ms_mult_target", header)
    assert hasattr(bb.Witness, "derive_multiplicities") and hasattr(bb.Witness, "trace") and hasattr(bb.System, "multiplicity_slot")


def test_null_arguments_are_refused_before_any_device_work():
    L = pkg.lib()
    u64p = C.POINTER(C.c_uint64)
    summary = (C.c_uint64 * 6)()
    zero = C.c_size_t(0)
    tg = (pkg.MultTarget * 1)(pkg.MultTarget(0, 0))
    assert L.msbb_witness_derive_multiplicities(None, tg, C.c_size_t(1), summary, None, zero, None, zero) == -1
    assert b"null" in L.ms_last_error()
    not_a_witness = (C.c_uint64 * 4)()  # any non-null address: a null summary is refused before the witness is looked at
    assert L.msbb_witness_derive_multiplicities(C.cast(not_a_witness, C.c_void_p), tg, C.c_size_t(1), C.cast(None, u64p), None, zero, None, zero) == -1
    assert b"null" in L.ms_last_error()
    assert L.msbb_witness_trace(None, zero, None, zero, None) == -1 and b"null" in L.ms_last_error()
    assert L.msbb_system_multiplicity_slot(None, zero, zero, summary) == -1 and b"null" in L.ms_last_error()
