"""CPU tests of fill programs (`-m "not gpu"`): the model of tests/fill_model.py pinned against the witness builders, the
operator edges of the definition in the model, what compile_fill and compile_circuit promise, and ms_fill_program_info - host
code of the library that checks a program and describes how ms_witness_fill would run it, without a device."""
import ctypes as C

import numpy as np
import pytest

import fill_model as fm

P = fm.P


def one_cell(fe, expr, n_inputs=0, inputs=None, rows=1):
    """the value(s) column 0 takes under the one-step program (0, expr)"""
    prog = fe.compile_fill(1, 0, n_inputs, [(0, expr)])
    ins = None if inputs is None else np.array(inputs, dtype=np.uint64).reshape(rows, n_inputs)
    return [int(v) for v in fm.run(prog.blob, np.zeros((rows, 1), dtype=np.uint64), None, ins)[:, 0]]


@pytest.mark.parametrize("n", [1, 5, 128])
def test_model_reproduces_the_u32_add_builder(fe, n):
    (_, add), _ = fe.u32_add_bench_witness(n)
    xs, ys = fe.xorshift_pairs(n)
    prog = fe.u32_add_fill_program(n)
    garbage = np.full(add.shape, 7, dtype=np.uint64)  # every column is assigned: what the trace held does not matter
    got = fm.run(prog.blob, garbage, None, np.stack([xs, ys], axis=1))
    assert got.shape == add.shape == (max(1, 1 << (n - 1).bit_length()), 14)
    assert np.array_equal(got, add)  # all 14 columns, padding rows included


def test_inv0(fe):
    E = fe.Expr
    assert one_cell(fe, fe.inv0(E.input(0)), 1, [0]) == [0]
    for x in (1, 2, P - 1):
        assert one_cell(fe, E.input(0) * fe.inv0(E.input(0)), 1, [x]) == [1]
    assert one_cell(fe, fe.inv0(E.input(0)), 1, [2]) == [(P + 1) // 2]


def test_lt(fe):
    E = fe.Expr
    lt = fe.lt(E.input(0), E.input(1))
    assert one_cell(fe, lt, 2, [5, 5]) == [0]  # equal operands
    assert one_cell(fe, lt, 2, [P - 1, 0]) == [0] and one_cell(fe, lt, 2, [0, P - 1]) == [1]  # integers, not field distance
    assert one_cell(fe, lt, 2, [P - 1, P - 1]) == [0]
    assert one_cell(fe, fe.lt(E.row(), 2), rows=4) == [1, 1, 0, 0]


def test_bit_xor_reduces_and_bit_and(fe):
    E = fe.Expr
    a, b = 0xFFFFFFFF00000000, 0x00000000FFFFFFFF
    assert a < P and (a ^ b) >= P
    assert one_cell(fe, fe.bit_xor(E.input(0), E.input(1)), 2, [a, b]) == [(a ^ b) - P]
    assert one_cell(fe, fe.bit_and(E.input(0), E.input(1)), 2, [a, P - 1]) == [a & (P - 1)]


def test_bits_edges(fe):
    E = fe.Expr
    x = P - 1  # 0xFFFFFFFF00000000
    assert one_cell(fe, fe.bits(E.input(0), 0, 64), 1, [x]) == [x]
    assert one_cell(fe, fe.bits(E.input(0), 63, 1), 1, [x]) == [1]
    assert one_cell(fe, fe.bits(E.input(0), 0, 1), 1, [x]) == [0]
    assert one_cell(fe, fe.bits(E.input(0), 0, 1), 1, [3]) == [1]
    for lo, length in ((0, 0), (1, 64), (64, 1)):
        with pytest.raises(fe.CompileError):
            fe.bits(E.input(0), lo, length)


SEQ_OLD = [[10, 20, 30, 40], [11, 21, 31, 41]]
# column 0 = old column 1 + 1; column 1 sees the NEW column 0 and the OLD column 2 (assigned only later); column 2 sees the next
# row of column 3 (never assigned) and the new column 0; column 0 is assigned again and keeps the last value; column 3 stays
SEQ_WANT = [[9, 2 * 21 + 30, 41 + 21, 40], [9, 2 * 22 + 31, 40 + 22, 41]]


def sequential_program(fe):
    E = fe.Expr
    return fe.compile_fill(4, 0, 0, [(0, E.main(1) + 1), (1, E.main(0) * 2 + E.main(2)), (2, E.main_next(3) + E.main(0)), (0, E.const(9))])


def test_sequential_semantics_in_the_model(fe):
    E = fe.Expr
    prog = sequential_program(fe)
    got = fm.run(prog.blob, np.array(SEQ_OLD, dtype=np.uint64))
    assert got.tolist() == SEQ_WANT


def test_compile_fill_shares_subexpressions_and_folds_constants(fe):
    E = fe.Expr
    x, y = E.input(0), E.input(1)
    prog = fe.compile_fill(3, 0, 2, [(0, fe.bits(x + y, 0, 8)), (1, fe.bits(x + y, 8, 8)), (2, fe.bits(y + x, 0, 8))])
    kinds = [n[0] for n in prog.nodes]
    assert kinds.count(fe.N_ADD) == 1 and kinds.count(fe.N_BITS) == 2  # x + y once (either order), bits(.., 0, 8) once
    assert prog.steps[0][1] == prog.steps[2][1] != prog.steps[1][1]
    folded = fe.compile_fill(1, 0, 0, [(0, fe.bits(E.const(0x1234), 4, 8) + fe.lt(3, 4) + fe.inv0(2) * 2 + fe.bit_xor(5, 3) + fe.bit_and(6, 3))])
    assert folded.nodes[folded.steps[0][1]] == (fe.N_CONST, 0, 0, 0x23 + 1 + 1 + 6 + 2, 0)
    assert all(n[0] == fe.N_CONST for n in folded.nodes)  # (the interner keeps the folded operands; nothing refers to them)
    words = np.frombuffer(prog.blob, dtype="<u8")
    assert [int(w) for w in words[:6]] == [fe.FILL_MAGIC, 3, 0, 2, len(prog.nodes), 3] and len(words) == 6 + 3 * len(prog.nodes) + 6
    assert fm.parse(prog.blob)[3:] == (prog.nodes, prog.steps)


def test_compile_fill_refusals(fe):
    E = fe.Expr
    for steps in ([(2, E.const(1))],                               # dst out of range
                  [(0, E.main(2))], [(0, E.input(1))], [(0, E.preprocessed(0))],  # variables out of range
                  [(0, E.public(0))], [(0, fe.IS_FIRST_ROW)], [(0, fe.IS_LAST_ROW + 1)], [(0, fe.IS_TRANSITION)],
                  [(0, E.var(fe.SRC_STAGE2, 0, 0))],
                  [(0, E.main_next(1)), (1, E.const(1))],          # next row of an assigned column
                  [(0, E.main_next(0))]):
        with pytest.raises(fe.CompileError):
            fe.compile_fill(2, 0, 1, steps)
    fe.compile_fill(2, 0, 1, [(0, E.main_next(1) + E.input_next(0))])  # next row of a column nobody assigns: fine


def new_kind_exprs(fe):
    E = fe.Expr
    return [E.input(0), E.input_next(0), E.row(), fe.bits(E.main(0), 0, 8), fe.inv0(E.main(0)), fe.lt(E.main(0), E.main(1)),
            fe.bit_xor(E.main(0), E.main(1)), fe.bit_and(E.main(0), E.main(1))]


def test_compile_circuit_rejects_the_witness_only_nodes(fe):
    E = fe.Expr
    for e in new_kind_exprs(fe):
        with pytest.raises(fe.CompileError):
            fe.compile_circuit(fe.CircuitInputs(2, None, [E.main(0) * (e + 1)], [], []))
        with pytest.raises(fe.CompileError):
            fe.compile_circuit(fe.CircuitInputs(2, None, [], [], [fe.Lookup.push(e, [E.main(0)])]))
        with pytest.raises(fe.CompileError):
            fe.compile_circuit(fe.CircuitInputs(2, None, [], [], [fe.Lookup.push(1, [E.main(0), e - E.main(1)])]))


# ---------------------------------------------------------------- ms_fill_program_info: host code of the library
def info(pkg, blob):
    """(status, out4, error text)"""
    L = pkg.lib()
    a = np.frombuffer(bytes(blob), dtype=np.uint8)
    out = np.zeros(4, dtype=np.uint64)
    rc = L.ms_fill_program_info(a.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_size_t(a.size), out.ctypes.data_as(C.POINTER(C.c_uint64)))
    return rc, [int(x) for x in out], L.ms_last_error().decode()


def test_program_info_of_the_u32_add_program(pkg, fe):
    prog = fe.u32_add_fill_program(100)
    rc, out, _ = info(pkg, prog.blob)
    # x, y, x + y, 12 bytes, the carry, row, the constant 100, lt: 19 instructions, one per node of the program; the 14 outputs
    # stay live to the end next to x + y while its last bits are taken (x and y have been freed by then)
    assert rc == 0 and len(prog.nodes) == 19
    assert out[0] == 19 and out[3] == 14 and 14 <= out[1] <= 17 and out[2] == 256
    assert pkg.fill_program_info(prog) == {"instructions": 19, "slots": out[1], "lds_lanes": 256, "assigned_columns": 14}


def test_program_info_linearises_steps(pkg, fe):
    E = fe.Expr
    # step 1 reads what step 0 assigned: one shared instance, no load of main(0); the overwritten first value of column 2 is dropped
    prog = fe.compile_fill(3, 0, 1, [(0, E.input(0) + 1), (2, fe.inv0(E.input(0))), (1, E.main(0) * E.main(0)), (2, E.main(0))])
    rc, out, _ = info(pkg, prog.blob)
    assert rc == 0 and out[0] == 4 and out[3] == 3  # input, 1, add, mul
    # a few hundred leaves consumed in reverse order are all live at once: no LDS form
    n = 300
    wide = fe.compile_fill(n, 0, 1, [(n - 1 - k, fe.bits(E.input(0) + k, k % 57, 8)) for k in range(n)])
    rc, out, _ = info(pkg, wide.blob)
    assert rc == 0 and out[1] >= n and out[2] == 0 and out[3] == n
    mid = fe.compile_fill(40, 0, 1, [(k, E.input(0) + k) for k in range(40)])
    assert info(pkg, mid.blob)[1][2] == 128


def refusal_blobs(fe):
    """(what, blob, a word the error text must contain) for every refusal that needs no witness"""
    N = fe
    ok_nodes = [(N.N_VAR, N.SRC_INPUT, 0, 0, 0), (N.N_CONST, 0, 0, 3, 0), (N.N_ADD, 0, 0, 0, 1)]
    good = fe.fill_blob(2, 1, 1, ok_nodes, [(0, 2)])
    words = np.frombuffer(good, dtype="<u8").copy()
    bad_magic = words.copy()
    bad_magic[0] = fe.BLOB_MAGIC
    cases = [("bad magic", bad_magic.tobytes(), "magic"),
             ("truncated", good[:-8], "truncated"),
             ("truncated header", good[:40], "truncated"),
             ("not whole words", good + b"\0", "truncated"),
             ("dst", fe.fill_blob(2, 1, 1, ok_nodes, [(2, 2)]), "dst"),
             ("root", fe.fill_blob(2, 1, 1, ok_nodes, [(0, 3)]), "root"),
             ("forward operand", fe.fill_blob(2, 1, 1, [ok_nodes[0], (N.N_ADD, 0, 0, 0, 2), ok_nodes[1]], [(0, 1)]), "forward"),
             ("self operand", fe.fill_blob(2, 1, 1, [ok_nodes[0], (N.N_NEG, 0, 0, 1, 0)], [(0, 1)]), "forward"),
             ("bits beyond 64", fe.fill_blob(2, 1, 1, [ok_nodes[0], (N.N_BITS, 0, 0, 0, 60 | (5 << 8))], [(0, 1)]), "bits"),
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
             ("constant", fe.fill_blob(2, 1, 1, [(N.N_CONST, 0, 0, P, 0)], [(0, 0)]), "constant"),
             ("next row of an assigned column", fe.fill_blob(2, 1, 1, [(N.N_VAR, N.SRC_MAIN, 1, 1, 0), ok_nodes[1]], [(0, 0), (1, 1)]), "offset-1")]
    return good, cases


def test_program_info_refusals(pkg, fe):
    good, cases = refusal_blobs(fe)
    assert info(pkg, good)[0] == 0
    fm.parse(good)
    for what, blob, word in cases:
        rc, _, text = info(pkg, blob)
        assert rc == -1 and text.startswith("ms_fill_program_info: ") and word in text, (what, rc, text)
        with pytest.raises(fm.FillError):  # the model refuses the same programs
            fm.parse(blob)
    # the next row of a column no step assigns is fine
    assert info(pkg, fe.fill_blob(2, 1, 1, [(fe.N_VAR, fe.SRC_MAIN, 1, 1, 0)], [(0, 0)]))[0] == 0
