"""CPU tests of fill programs over BabyBear (`-m "not gpu"`): the model of tests/fill_model_bb.py pinned against the witness
builder, the operator edges of the definition in the model, what compile_fill promises under field(BABYBEAR), and
msbb_fill_program_info - host code of the library that checks a program and describes how msbb_witness_fill would run it,
without a device. The counterpart of test_fill_model.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fill_model as fm_gl
import fill_model_bb as fm
from test_fill_model import SEQ_OLD, SEQ_WANT, sequential_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = fm.P


def halves(xs, ys):
    """n x 4: (x_lo, x_hi, y_lo, y_hi), 16 bits each"""
    xs, ys = np.asarray(xs, dtype=np.uint64), np.asarray(ys, dtype=np.uint64)
    m, s = np.uint64(0xFFFF), np.uint64(16)
    return np.stack([xs & m, xs >> s, ys & m, ys >> s], axis=1)


def one_cell(fe, make, n_inputs=0, inputs=None, rows=1):
    """the value(s) column 0 takes under the one-step program (0, make()), compiled over BabyBear"""
    with fe.field(fe.BABYBEAR):
        prog = fe.compile_fill(1, 0, n_inputs, [(0, make())])
    ins = None if inputs is None else np.array(inputs, dtype=np.uint64).reshape(rows, n_inputs)
    return [int(v) for v in fm.run(prog.blob, np.zeros((rows, 1), dtype=np.uint64), None, ins)[:, 0]]


@pytest.mark.parametrize("n", [1, 5, 128])
def test_model_reproduces_the_u32_add_builder_from_halves(fe, n):
    with fe.field(fe.BABYBEAR):
        (_, add), _ = fe.u32_add_bench_witness(n)
        prog = fe.u32_add_halves_fill_program(n)
    garbage = np.full(add.shape, 7, dtype=np.uint64)  # every column is assigned: what the trace held does not matter
    got = fm.run(prog.blob, garbage, None, halves(*fe.xorshift_pairs(n)))
    assert got.shape == add.shape == (max(1, 1 << (n - 1).bit_length()), 14)
    assert np.array_equal(got, add)  # all 14 columns, padding rows included
    assert len(prog.nodes) == 24


def test_the_halves_program_means_the_same_over_goldilocks(fe):
    (_, add), _ = fe.u32_add_bench_witness(5)
    prog = fe.u32_add_halves_fill_program(5)
    got = fm_gl.run(prog.blob, np.full(add.shape, 7, dtype=np.uint64), None, halves(*fe.xorshift_pairs(5)))
    assert np.array_equal(got, add)


def test_inv0(fe):
    E = fe.Expr
    assert one_cell(fe, lambda: fe.inv0(E.input(0)), 1, [0]) == [0]
    for x in (1, 2, P - 1):
        assert one_cell(fe, lambda: E.input(0) * fe.inv0(E.input(0)), 1, [x]) == [1]
    assert one_cell(fe, lambda: fe.inv0(E.input(0)), 1, [2]) == [(P + 1) // 2]


def test_lt(fe):
    E = fe.Expr
    lt = lambda: fe.lt(E.input(0), E.input(1))  # noqa: E731
    assert one_cell(fe, lt, 2, [5, 5]) == [0]  # equal operands
    assert one_cell(fe, lt, 2, [P - 1, 0]) == [0] and one_cell(fe, lt, 2, [0, P - 1]) == [1]  # integers, not field distance
    assert one_cell(fe, lt, 2, [P - 1, P - 1]) == [0]
    assert one_cell(fe, lambda: fe.lt(E.row(), 2), rows=4) == [1, 1, 0, 0]


def test_bit_xor_reduces_and_bit_and(fe):
    E = fe.Expr
    a, b = 0x40000000, 0x3FFFFFFF
    assert a < P and b < P and (a ^ b) == 0x7FFFFFFF >= P
    assert one_cell(fe, lambda: fe.bit_xor(E.input(0), E.input(1)), 2, [a, b]) == [0x7FFFFFFF - P] == [0x07FFFFFE]
    assert one_cell(fe, lambda: fe.bit_and(E.input(0), E.input(1)), 2, [a, P - 1]) == [a & (P - 1)]
    assert one_cell(fe, lambda: fe.bit_and(E.input(0), E.input(1)), 2, [0x3FFFFFFF, P - 1]) == [0x3FFFFFFF & (P - 1)] == [0x38000000]


def test_bits_edges(fe):
    E = fe.Expr
    x = P - 1  # 0x78000000
    assert one_cell(fe, lambda: fe.bits(E.input(0), 0, 32), 1, [x]) == [x]
    assert one_cell(fe, lambda: fe.bits(E.input(0), 30, 1), 1, [x]) == [1]
    assert one_cell(fe, lambda: fe.bits(E.input(0), 31, 1), 1, [x]) == [0]
    assert one_cell(fe, lambda: fe.bits(E.input(0), 0, 1), 1, [3]) == [1]
    with fe.field(fe.BABYBEAR):
        for lo, length in ((1, 32), (32, 1), (0, 0)):
            with pytest.raises(fe.CompileError, match="BadBitsFields"):
                fe.bits(E.input(0), lo, length)
    fe.bits(E.input(0), 1, 32)  # outside field(BABYBEAR) the limit is today's 64
    with pytest.raises(fe.CompileError):
        fe.bits(E.input(0), 1, 64)


def test_sequential_semantics_in_the_model(fe):
    with fe.field(fe.BABYBEAR):
        prog = sequential_program(fe)
    assert fm.run(prog.blob, np.array(SEQ_OLD, dtype=np.uint64)).tolist() == SEQ_WANT


def test_compile_fill_emits_the_magic_of_the_active_field(fe):
    E = fe.Expr
    before = fe.FILL_MAGIC
    assert before == fm_gl.FILL_MAGIC == 0x31304C4C49464D00 and fe.FILL_BITS == 64
    with fe.field(fe.BABYBEAR):
        bb_prog = fe.compile_fill(1, 0, 1, [(0, E.input(0) + (P + 2))])  # folded modulo the active P: the constant 2
        assert fe.FILL_MAGIC == fm.FILL_MAGIC == 0x3130424C49464D00 and fe.FILL_BITS == 32
    gl_prog = fe.compile_fill(1, 0, 1, [(0, E.input(0) + 2)])
    assert fe.FILL_MAGIC == before and fe.FILL_BITS == 64
    assert int(np.frombuffer(bb_prog.blob, dtype="<u8")[0]) == fm.FILL_MAGIC and bytes(bb_prog.blob[:8]) == b"\0MFILB01"
    assert int(np.frombuffer(gl_prog.blob, dtype="<u8")[0]) == fm_gl.FILL_MAGIC
    assert bb_prog.nodes == gl_prog.nodes and bb_prog.blob[8:] == gl_prog.blob[8:]
    fm.parse(bb_prog.blob)
    with pytest.raises(fm.FillError):
        fm.parse(gl_prog.blob)
    with pytest.raises(fm_gl.FillError):
        fm_gl.parse(bb_prog.blob)


# ---------------------------------------------------------------- msbb_fill_program_info: host code of the library
def info(pkg, blob, call="msbb_fill_program_info"):
    """(status, out4, error text)"""
    L = pkg.lib()
    a = np.frombuffer(bytes(blob), dtype=np.uint8)
    out = np.zeros(4, dtype=np.uint64)
    rc = getattr(L, call)(a.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_size_t(a.size), out.ctypes.data_as(C.POINTER(C.c_uint64)))
    return rc, [int(x) for x in out], L.ms_last_error().decode()


def test_program_info_of_the_halves_program(pkg, fe):
    with fe.field(fe.BABYBEAR):
        prog = fe.u32_add_halves_fill_program(100)
    rc, out, _ = info(pkg, prog.blob)
    # four inputs, s_lo, its carry, two adds for s_hi, 12 bytes, the carry, row, the constant 100, lt: 24 instructions, one per node
    assert rc == 0 and len(prog.nodes) == 24
    assert out[0] == 24 and out[3] == 14 and 14 <= out[1] <= 20
    assert out[1] * 256 * 4 <= 64 * 1024 and out[2] == 256
    assert pkg.babybear.fill_program_info(prog) == {"instructions": 24, "slots": out[1], "lds_lanes": 256, "assigned_columns": 14}


def test_program_info_linearises_steps(pkg, fe):
    E = fe.Expr
    with fe.field(fe.BABYBEAR):
        # step 1 reads what step 0 assigned: one shared instance, no load of main(0); the overwritten first value of column 2 is dropped
        prog = fe.compile_fill(3, 0, 1, [(0, E.input(0) + 1), (2, fe.inv0(E.input(0))), (1, E.main(0) * E.main(0)), (2, E.main(0))])
        n = 300
        wide = fe.compile_fill(n, 0, 1, [(n - 1 - k, fe.bits(E.input(0) + k, k % 25, 8)) for k in range(n)])
        mid = fe.compile_fill(100, 0, 1, [(k, E.input(0) + k) for k in range(100)])
        small = fe.compile_fill(40, 0, 1, [(k, E.input(0) + k) for k in range(40)])
    rc, out, _ = info(pkg, prog.blob)
    assert rc == 0 and out[0] == 4 and out[3] == 3  # input, 1, add, mul
    # a few hundred leaves consumed in reverse order are all live at once: no LDS form (more than 256 four-byte slots)
    rc, out, _ = info(pkg, wide.blob)
    assert rc == 0 and out[1] >= n and out[2] == 0 and out[3] == n
    # 100 live outputs: past 64 slots, within 128; 40: within 64 (a four-byte slot file, so twice the lanes of Goldilocks)
    assert info(pkg, mid.blob)[1][2] == 128 and info(pkg, small.blob)[1][2] == 256


def refusal_blobs(fe):
    """(what, blob, a word the error text must contain) for every refusal that needs no witness; call under field(BABYBEAR)"""
    N = fe
    assert fe.FILL_MAGIC == fm.FILL_MAGIC
    ok_nodes = [(N.N_VAR, N.SRC_INPUT, 0, 0, 0), (N.N_CONST, 0, 0, 3, 0), (N.N_ADD, 0, 0, 0, 1)]
    good = fe.fill_blob(2, 1, 1, ok_nodes, [(0, 2)])
    words = np.frombuffer(good, dtype="<u8").copy()
    bad_magic, gl_magic = words.copy(), words.copy()
    bad_magic[0] = fe.BLOB_MAGIC
    gl_magic[0] = fm_gl.FILL_MAGIC
    cases = [("bad magic", bad_magic.tobytes(), "magic"),
             ("the Goldilocks magic", gl_magic.tobytes(), "magic"),
             ("truncated", good[:-8], "truncated"),
             ("truncated header", good[:40], "truncated"),
             ("not whole words", good + b"\0", "truncated"),
             ("dst", fe.fill_blob(2, 1, 1, ok_nodes, [(2, 2)]), "dst"),
             ("root", fe.fill_blob(2, 1, 1, ok_nodes, [(0, 3)]), "root"),
             ("forward operand", fe.fill_blob(2, 1, 1, [ok_nodes[0], (N.N_ADD, 0, 0, 0, 2), ok_nodes[1]], [(0, 1)]), "forward"),
             ("self operand", fe.fill_blob(2, 1, 1, [ok_nodes[0], (N.N_NEG, 0, 0, 1, 0)], [(0, 1)]), "forward"),
             ("bits beyond 32", fe.fill_blob(2, 1, 1, [ok_nodes[0], (N.N_BITS, 0, 0, 0, 28 | (5 << 8))], [(0, 1)]), "bits"),
             ("bits of the other field", fe.fill_blob(2, 1, 1, [ok_nodes[0], (N.N_BITS, 0, 0, 0, 32 | (1 << 8))], [(0, 1)]), "bits"),
             ("bits of length 0", fe.fill_blob(2, 1, 1, [ok_nodes[0], (N.N_BITS, 0, 0, 0, 3)], [(0, 1)]), "bits"),
             ("selector", fe.fill_blob(2, 1, 1, [(N.N_IS_FIRST, 0, 0, 0, 0)], [(0, 0)]), "selector"),
             ("selector", fe.fill_blob(2, 1, 1, [(N.N_IS_LAST, 0, 0, 0, 0)], [(0, 0)]), "selector"),
             ("selector", fe.fill_blob(2, 1, 1, [(N.N_IS_TRANS, 0, 0, 0, 0)], [(0, 0)]), "selector"),
             ("public", fe.fill_blob(2, 1, 1, [(N.N_PUBLIC, 0, 0, 0, 0)], [(0, 0)]), "public"),
             ("stage 2", fe.fill_blob(2, 1, 1, [(N.N_VAR, N.SRC_STAGE2, 0, 0, 0)], [(0, 0)]), "stage-2"),
             ("unknown kind", fe.fill_blob(2, 1, 1, [(12, 0, 0, 0, 0)], [(0, 0)]), "kind"),
             ("main variable", fe.fill_blob(2, 1, 1, [(N.N_VAR, N.SRC_MAIN, 0, 2, 0)], [(0, 0)]), "out of range"),
             ("input variable", fe.fill_blob(2, 1, 1, [(N.N_VAR, N.SRC_INPUT, 0, 1, 0)], [(0, 0)]), "out of range"),
             ("preprocessed variable", fe.fill_blob(2, 1, 1, [(N.N_VAR, N.SRC_PRE, 1, 1, 0)], [(0, 0)]), "out of range"),
             ("offset 2", fe.fill_blob(2, 1, 1, [(N.N_VAR, N.SRC_MAIN, 2, 0, 0)], [(1, 0)]), "offset"),
             ("constant p", fe.fill_blob(2, 1, 1, [(N.N_CONST, 0, 0, P, 0)], [(0, 0)]), "constant"),
             ("next row of an assigned column", fe.fill_blob(2, 1, 1, [(N.N_VAR, N.SRC_MAIN, 1, 1, 0), ok_nodes[1]], [(0, 0), (1, 1)]), "offset-1")]
    return good, cases


def test_program_info_refusals(pkg, fe):
    with fe.field(fe.BABYBEAR):
        good, cases = refusal_blobs(fe)
        edge = [fe.fill_blob(2, 1, 1, [(fe.N_VAR, fe.SRC_MAIN, 1, 1, 0)], [(0, 0)]),  # the next row of a column no step assigns
                fe.fill_blob(2, 1, 1, [(fe.N_CONST, 0, 0, P - 1, 0)], [(0, 0)]),
                fe.fill_blob(2, 1, 1, [(fe.N_VAR, fe.SRC_INPUT, 0, 0, 0), (fe.N_BITS, 0, 0, 0, 31 | (1 << 8))], [(0, 1)])]
    assert info(pkg, good)[0] == 0
    fm.parse(good)
    for what, blob, word in cases:
        rc, _, text = info(pkg, blob)
        assert rc == -1 and text.startswith("msbb_fill_program_info: ") and word in text, (what, rc, text)
        with pytest.raises(fm.FillError):  # the model refuses the same programs
            fm.parse(blob)
    for blob in edge:
        assert info(pkg, blob)[0] == 0
        fm.parse(blob)
    # the other direction of the magic: a program authored over BabyBear is no program of the Goldilocks call
    rc, _, text = info(pkg, good, "ms_fill_program_info")
    assert rc == -1 and text.startswith("ms_fill_program_info: ") and "magic" in text
    with pytest.raises(fm_gl.FillError):
        fm_gl.parse(good)


SYMBOLS = ("msbb_witness_fill", "msbb_fill_program_info")


def test_new_symbols_in_header_export_list_library_and_rust(pkg):
    bb = pkg.babybear
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mstark_bb.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "mstark_sys.rs")).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header) and sym in bb.exported_symbols() and ("pub fn %s(" % sym) in rust, sym
        assert getattr(pkg.lib(), sym)  # (ctypes raises AttributeError for a symbol the library does not export)
    assert hasattr(bb.Witness, "fill") and hasattr(bb, "fill_program_info")


def test_null_arguments_are_refused_before_any_device_work(pkg):
    L = pkg.lib()
    u64p, u8p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
    summary = (C.c_uint64 * 4)()
    blob = (C.c_uint8 * 48)()
    zero, n48 = C.c_size_t(0), C.c_size_t(48)
    not_a_witness = C.cast((C.c_uint64 * 4)(), C.c_void_p)  # any non-null address: the nulls are refused before the witness is looked at
    assert L.msbb_witness_fill(None, zero, blob, n48, None, None, summary) == -1
    assert L.ms_last_error().decode() == "msbb_witness_fill: null argument"
    assert L.msbb_witness_fill(not_a_witness, zero, C.cast(None, u8p), n48, None, None, summary) == -1 and b"null" in L.ms_last_error()
    assert L.msbb_witness_fill(not_a_witness, zero, blob, n48, None, None, C.cast(None, u64p)) == -1 and b"null" in L.ms_last_error()
    assert L.msbb_fill_program_info(C.cast(None, u8p), n48, summary) == -1 and b"null" in L.ms_last_error()
    assert L.msbb_fill_program_info(blob, n48, C.cast(None, u64p)) == -1
    assert L.ms_last_error().decode() == "msbb_fill_program_info: null argument"
