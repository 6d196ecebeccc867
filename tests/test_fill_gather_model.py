"""CPU tests of the indexed reads of fill programs (include/mstark.h, "INDEXED READS"): that the model of
tests/fill_gather_model.py equals the three older models on programs without the node, the blob word for word in both fields,
the definition in the model with hand-computed expectations, every refusal - from compile_fill, from the model and from the
library's host code (ms_fill_program_info, ms_fill_scan_info, msbb_fill_program_info) - and the info words."""
import ctypes as C

import numpy as np
import pytest

import fill_gather_model as gm
import fill_model as fm
import fill_model_bb as fmb
import fill_scan_model as fsm
from test_fill_model import SEQ_OLD, SEQ_WANT, sequential_program

P, PB = gm.GOLDILOCKS_P, gm.BABYBEAR_P
GL_CALLS = ["ms_fill_program_info", "ms_fill_scan_info"]
CALLS = GL_CALLS + ["msbb_fill_program_info"]


def words_of(blob):
    return [int(x) for x in np.frombuffer(blob, dtype="<u8")]


def info(pkg, blob, call="ms_fill_program_info"):
    """(status, out4, error text)"""
    L = pkg.lib()
    a = np.frombuffer(bytes(blob), dtype=np.uint8)
    out = np.zeros(4, dtype=np.uint64)
    rc = getattr(L, call)(a.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_size_t(a.size), out.ctypes.data_as(C.POINTER(C.c_uint64)))
    return rc, [int(x) for x in out], L.ms_last_error().decode()


def u64(rows):
    return np.array(rows, dtype=np.uint64)


# ---------------------------------------------------------------- the model equals the older ones where there is no `at`
def test_model_equals_the_older_models_without_indexed_reads(fe):
    E = fe.Expr
    rng = np.random.default_rng(5)
    n = 16
    xs, ys = fe.xorshift_pairs(n)
    pairs = np.stack([xs, ys], axis=1).astype(np.uint64)
    prog = fe.u32_add_fill_program(n - 3)
    old = rng.integers(0, P, size=(n, 14), dtype=np.uint64)
    want = fm.run(prog.blob, old, None, pairs)
    assert np.array_equal(gm.run(prog.blob, old, None, pairs), want) and np.array_equal(fsm.run(prog.blob, old, None, pairs), want)
    assert np.array_equal(gm.run(prog.blob, old, None, pairs[:9]), fm.run(prog.blob, old, None, pairs[:9]))  # short inputs read 0
    seq = sequential_program(fe)
    assert gm.run(seq.blob, u64(SEQ_OLD)).tolist() == SEQ_WANT == fm.run(seq.blob, u64(SEQ_OLD)).tolist()
    assert gm.parse(seq.blob)[1:6] == fm.parse(seq.blob)
    # the three-group scan program of test_fill_scan_model
    x = E.input(0)
    three = fe.compile_fill(3, 0, 1, [(0, x + 1), (1, fe.scan(x, E.main(0), init=2)), (2, E.main_next(1) - E.main(1))])
    old3 = rng.integers(0, P, size=(n, 3), dtype=np.uint64)
    inp = rng.integers(0, P, size=(n, 1), dtype=np.uint64)
    assert np.array_equal(gm.run(three.blob, old3, None, inp), fsm.run(three.blob, old3, None, inp))
    assert gm.parse(three.blob)[1:] == fsm.parse(three.blob)
    # BabyBear: the halves program and the sequential program
    m16 = np.uint64(0xFFFF)
    halves = np.stack([xs & m16, xs >> np.uint64(16), ys & m16, ys >> np.uint64(16)], axis=1)
    with fe.field(fe.BABYBEAR):
        hprog, bseq = fe.u32_add_halves_fill_program(n - 3), sequential_program(fe)
    oldb = rng.integers(0, PB, size=(n, 14), dtype=np.uint64)
    assert np.array_equal(gm.run(hprog.blob, oldb, None, halves), fmb.run(hprog.blob, oldb, None, halves))
    assert np.array_equal(gm.run(hprog.blob, oldb, None, halves[:5]), fmb.run(hprog.blob, oldb, None, halves[:5]))
    assert gm.run(bseq.blob, u64(SEQ_OLD)).tolist() == fmb.run(bseq.blob, u64(SEQ_OLD)).tolist() == SEQ_WANT
    assert gm.parse(hprog.blob)[0] == PB and gm.parse(hprog.blob)[1:6] == fmb.parse(hprog.blob)


# ---------------------------------------------------------------- the blob
def small_program(fe):
    E = fe.Expr
    return fe.compile_fill(3, 1, 1, [(0, E.input_at(0, E.row())), (1, E.pre_at(0, E.main_at(2, 5)))])


@pytest.mark.parametrize("bb", [False, True])
def test_blob_word_for_word(fe, bb):
    if bb:
        with fe.field(fe.BABYBEAR):
            prog, magic = small_program(fe), fe.FILL_MAGIC
        assert prog.blob[:8] == b"\0MFILB01"
    else:
        prog, magic = small_program(fe), fe.FILL_MAGIC
        assert prog.blob[:8] == b"\0MFILL01"
    A, I, M, R = fe.N_AT, fe.SRC_INPUT, fe.SRC_MAIN, fe.SRC_PRE
    assert A == 22
    # nodes operands first: row, input column 0 at it; the constant 5 (a constant row stays a node), main column 2 at it,
    # preprocessed column 0 at that
    assert prog.nodes == [(fe.N_ROW, 0, 0, 0, 0), (A, I, 0, 0, 0), (fe.N_CONST, 0, 0, 5, 0), (A, M, 0, 2, 2), (A, R, 0, 0, 3)]
    assert prog.steps == [(0, 1), (1, 4)] and prog.scans == []
    assert words_of(prog.blob) == [
        magic, 3, 1, 1, 5, 2,                                                                  # magic, widths, n_nodes, n_steps
        fe.N_ROW, 0, 0, A | (I << 8), 0, 0, fe.N_CONST, 5, 0, A | (M << 8), 2, 2, A | (R << 8), 0, 3,  # [22 | source << 8, column, row node]
        0, 1, 1, 4]                                                                            # steps [dst, root]
    assert gm.parse(prog.blob)[1:] == (3, 1, 1, prog.nodes, prog.steps, {})
    for older in ((fmb,) if bb else (fm, fsm)):  # the older models do not know the node
        with pytest.raises(older.FillError):
            older.parse(prog.blob)


def test_a_program_without_indexed_reads_keeps_its_blob(fe):
    E = fe.Expr
    for prog in (fe.u32_add_fill_program(100), sequential_program(fe), fe.compile_fill(2, 1, 1, [(0, E.input(0) + 3)])):
        assert all(kind != fe.N_AT for kind, _, _, _, _ in prog.nodes) and prog.blob[:8] == b"\0MFILL01"
        assert prog.blob == fe.fill_blob(prog.main_width, prog.preprocessed_width, prog.n_inputs, prog.nodes, prog.steps)
    # pinned: the blob of the sequential program, as it was before the node existed
    V, M = fe.N_VAR, fe.SRC_MAIN
    want = [0x31304C4C49464D00, 4, 0, 0, 11, 4]
    got = words_of(sequential_program(fe).blob)
    assert got[:6] == want and len(got) == 6 + 3 * 11 + 2 * 4 and got[6:9] == [V | (M << 8), 1, 0] and got[-8:] == [0, 2, 1, 7, 2, 9, 0, 10]
    three = fe.compile_fill(3, 0, 1, [(0, E.input(0) + 1), (1, fe.scan(E.input(0), E.main(0), init=2))])
    assert three.blob[:8] == b"\0MFILL02"


def test_equal_reads_are_one_node_and_constant_rows_are_not_folded(fe):
    E = fe.Expr
    prog = fe.compile_fill(2, 0, 1, [(0, E.input_at(0, E.row()) + E.input_at(0, E.row())), (1, E.input_at(0, 3))])
    kinds = [k for k, _, _, _, _ in prog.nodes]
    assert kinds.count(fe.N_AT) == 2 and kinds.count(fe.N_ROW) == 1 and (fe.N_CONST, 0, 0, 3, 0) in prog.nodes


# ---------------------------------------------------------------- the definition, in the model
def test_semantics_in_the_model_goldilocks(fe):
    E = fe.Expr
    n, h_in = 8, 5
    idx = [0, n - 1, n, h_in - 1, h_in, P - 1, 1 << 32, (1 << 32) + 1]
    old = u64([[99, 98, idx[r], 100 + r] for r in range(n)])
    inputs = u64([[50 + r] for r in range(h_in)])
    pre = u64([[200 + r] for r in range(n)])
    prog = fe.compile_fill(4, 1, 1, [(0, E.main_at(3, E.main(2))), (1, E.input_at(0, E.main(2)) + E.pre_at(0, E.main(2)) * 1000)])
    got = gm.run(prog.blob, old, pre, inputs)
    # rows n, p - 1, 2^32 and 2^32 + 1 read 0: no reduction modulo n, no truncation to 32 bits
    assert got[:, 0].tolist() == [100, 107, 0, 104, 105, 0, 0, 0]
    assert got[:, 1].tolist() == [50 + 200000, 0 + 207000, 0, 54 + 204000, 0 + 205000, 0, 0, 0]
    assert np.array_equal(got[:, 2:], old[:, 2:])


def test_semantics_in_the_model_babybear(fe):
    E = fe.Expr
    n, h_in = 8, 5
    idx = [0, n - 1, n, h_in - 1, h_in, PB - 1, 1, 2]
    old = u64([[99, 98, idx[r], 100 + r] for r in range(n)])
    inputs = u64([[50 + r] for r in range(h_in)])
    with fe.field(fe.BABYBEAR):
        prog = fe.compile_fill(4, 0, 1, [(0, E.main_at(3, E.main(2))), (1, E.input_at(0, E.main(2)))])
    got = gm.run(prog.blob, old, None, inputs)
    assert got[:, 0].tolist() == [100, 107, 0, 104, 105, 0, 101, 102]
    assert got[:, 1].tolist() == [50, 0, 0, 54, 0, 0, 51, 52]


def test_finished_scan_column_and_unassigned_column_in_the_model(fe):
    E = fe.Expr
    n = 8
    # column 0: 1, 3, 5, ... (a scan); column 1, a later group: column 0 at row 2 (r & 3), plus column 2 - which no step assigns -
    # read backwards
    prog = fe.compile_fill(3, 0, 0, [(0, fe.running_sum(2, init=1)), (1, E.main_at(0, fe.bits(E.row(), 0, 2) * 2) + E.main_at(2, 7 - E.row()))])
    old = u64([[77, 66, 10 * r] for r in range(n)])
    got = gm.run(prog.blob, old)
    assert got[:, 0].tolist() == [1 + 2 * r for r in range(n)]
    assert got[:, 1].tolist() == [1 + 4 * (r & 3) + 10 * (7 - r) for r in range(n)]
    assert got[:, 2].tolist() == [10 * r for r in range(n)]


# ---------------------------------------------------------------- refusals of compile_fill
def test_compile_fill_refusals(fe):
    E = fe.Expr
    x, row = E.input(0), E.row()
    cases = [("IndexedReadOfAssignedColumn column=0 step=1", [(0, x), (1, E.main_at(0, row))]),                     # the same group, first format
             ("IndexedReadOfAssignedColumn column=1 step=0", [(0, E.main_at(1, row)), (1, x)]),                     # assigned later in the group
             ("IndexedReadOfAssignedColumn column=0 step=1", [(0, x), (1, E.main_at(0, row)), (2, fe.running_sum(x))]),  # the same group, second format
             ("IndexedReadOfAssignedColumn column=0 step=0", [(1, E.main_at(0, row)), (0, fe.running_sum(x))]),     # a later group assigns
             ("IndexedReadOfAssignedColumn column=0 step=0", [(0, fe.scan(E.main_at(0, row), x))]),                 # a scan's own dst, mul root
             ("IndexedReadOfAssignedColumn column=0 step=0", [(0, fe.running_sum(E.input_at(0, E.main_at(0, 3))))]),  # and under another read
             ("ColumnOutOfRange", [(0, E.main_at(3, row))]),
             ("ColumnOutOfRange", [(0, E.input_at(1, row))]),
             ("ColumnOutOfRange", [(0, E.pre_at(0, row))]),
             ("Stage2InFillProgram", [(0, E.at(fe.SRC_STAGE2, 0, row))])]
    for name, steps in cases:
        with pytest.raises(fe.CompileError) as e:
            fe.compile_fill(3, 0, 1, steps)
        assert str(e.value).startswith(name), (name, str(e.value))
    # accepted: a finished scan column read by a later group; a column no step assigns
    ok = fe.compile_fill(3, 0, 1, [(0, fe.running_sum(x)), (1, E.main_at(0, row)), (1, E.main_at(2, E.main(1)))])
    assert len(ok.scans) == 1 and gm.parse(ok.blob)[6].keys() == {0}


def test_constraint_compilers_refuse_the_node(fe):
    E = fe.Expr
    for e in (E.main_at(0, E.main(1)), E.pre_at(0, 1), E.input_at(0, 1), E.main(0) * E.main_at(1, 0) - 1):
        with pytest.raises(fe.CompileError):
            fe.compile_circuit(fe.CircuitInputs(2, None, [e], [], []))
        with pytest.raises(fe.CompileError):
            fe.compile_circuit(fe.CircuitInputs(2, None, [E.main(0)], [], [fe.Lookup.push(1, [e])]))
        with pytest.raises(fe.CompileError):
            fe.compile_circuit(fe.CircuitInputs(2, None, [], [fe.ExtExpr.coords([e, E.main(0)])], []))


# ---------------------------------------------------------------- refusals of the blob: the model and the library's host code
def gather_refusal_blobs(fe):
    """-> (good, cases (what, blob, a word the error text must contain), accepted) of the first format, widths 3 / 1 / 1, under
    the field the front end stands in; scan_cases and scan_accepted: the second format (Goldilocks)"""
    N = fe
    A, M = N.N_AT, N.SRC_MAIN
    row, three = (N.N_ROW, 0, 0, 0, 0), (N.N_CONST, 0, 0, 3, 0)
    blob = lambda nodes, steps, scans=None: fe.fill_blob(3, 1, 1, nodes, steps, scans)
    good = blob([row, (A, M, 0, 2, 0), (A, N.SRC_INPUT, 0, 0, 1), (A, N.SRC_PRE, 0, 0, 2)], [(0, 3)])
    cases = [("the same group assigns the column", blob([row, (A, M, 0, 0, 0)], [(0, 0), (1, 1)]), "indexed read of main column 0"),
             ("its own column", blob([row, (A, M, 0, 1, 0)], [(1, 1)]), "indexed read of main column 1"),
             ("main column out of range", blob([row, (A, M, 0, 3, 0)], [(0, 1)]), "out of range"),
             ("preprocessed column out of range", blob([row, (A, N.SRC_PRE, 0, 1, 0)], [(0, 1)]), "out of range"),
             ("input column out of range", blob([row, (A, N.SRC_INPUT, 0, 1, 0)], [(0, 1)]), "out of range"),
             ("column 2^20", blob([row, (A, M, 0, 1 << 20, 0)], [(0, 1)]), "out of range"),
             ("a stage-2 source", blob([row, (A, N.SRC_STAGE2, 0, 0, 0)], [(0, 1)]), "stage-2"),
             ("unknown source", blob([row, (A, 7, 0, 0, 0)], [(0, 1)]), "unknown source"),
             ("non-zero offset field", blob([row, (A, M, 1, 2, 0)], [(0, 1)]), "offset field"),
             ("forward row operand", blob([(A, M, 0, 2, 1), row], [(0, 0)]), "forward"),
             ("its own row operand", blob([row, (A, M, 0, 2, 1)], [(0, 1)]), "forward"),
             ("row operand beyond the nodes", blob([row, (A, M, 0, 2, 1 << 40)], [(0, 1)]), "forward")]
    x = (N.N_VAR, N.SRC_INPUT, 0, 0, 0)
    scan_cases = [("the same group, second format", blob([row, (A, M, 0, 0, 0), x, three], [(0, 0), (1, 1), (2, 2)], [(2, 3, 0)]), "indexed read of main column 0"),
                  ("a later group assigns", blob([row, (A, M, 0, 0, 0), x, three], [(1, 1), (0, 2)], [(1, 3, 0)]), "step group 1 assigns"),
                  ("a scan's own dst, add root", blob([row, (A, M, 0, 0, 0), three], [(0, 1)], [(0, 2, 0)]), "indexed read of main column 0"),
                  ("a scan's own dst, mul root", blob([row, (A, M, 0, 0, 0), three], [(0, 2)], [(0, 1, 0)]), "indexed read of main column 0")]
    scan_accepted = [("a finished scan column", blob([row, (A, M, 0, 0, 0), x, three], [(0, 2), (1, 1)], [(0, 3, 0)])),
                     ("a column no step assigns", blob([row, (A, M, 0, 2, 0), x, three], [(0, 2), (1, 1)], [(0, 3, 0)])),
                     ("a scan's coefficients index an earlier group's column", blob([row, (A, M, 0, 0, 0), x, three], [(0, 2), (1, 1)], [(1, 3, 0)]))]
    return good, cases, scan_cases, scan_accepted


@pytest.mark.parametrize("call", CALLS)
def test_blob_refusals(pkg, fe, call):
    if call.startswith("msbb"):
        with fe.field(fe.BABYBEAR):
            good, cases, scan_cases, scan_accepted = gather_refusal_blobs(fe)
        scan_cases, scan_accepted = [], []  # the second format is the other configuration's
    else:
        good, cases, scan_cases, scan_accepted = gather_refusal_blobs(fe)
    assert info(pkg, good, call)[0] == 0, info(pkg, good, call)[2]
    gm.parse(good)
    for what, blob, word in cases + scan_cases:
        rc, _, text = info(pkg, blob, call)
        assert rc == -1 and text.startswith(call + ": ") and word in text, (what, rc, text)
        with pytest.raises(gm.FillError):  # the model refuses the same programs
            gm.parse(blob)
    for what, blob in scan_accepted:
        assert info(pkg, blob, call)[0] == 0, (what, info(pkg, blob, call)[2])
        gm.parse(blob)


def test_the_group_message_names_node_column_and_both_groups(pkg, fe):
    _, _, scan_cases, _ = gather_refusal_blobs(fe)
    text = info(pkg, scan_cases[1][1])[2]
    assert "node 1" in text and "main column 0" in text and "step group 0" in text and "step group 1 assigns" in text


# ---------------------------------------------------------------- the info words
def test_info_words(pkg, fe):
    E = fe.Expr
    one = fe.compile_fill(2, 0, 1, [(0, E.input_at(0, E.row()))])
    assert pkg.fill_program_info(one)["instructions"] == 2  # row, the read
    twice = fe.compile_fill(2, 0, 1, [(0, E.input_at(0, E.row())), (1, E.input_at(0, E.row()) + 1)])
    assert pkg.fill_program_info(twice)["instructions"] == 4  # row, the read once, the constant, the sum
    # by hand in the blob too: two equal nodes are one instruction
    row, at = (fe.N_ROW, 0, 0, 0, 0), (fe.N_AT, fe.SRC_INPUT, 0, 0, 0)
    rc, out, text = info(pkg, fe.fill_blob(2, 0, 1, [row, at, at], [(0, 1), (1, 2)]))
    assert rc == 0 and out[0] == 2 and out[3] == 2, text
    # three nodes in a chain: every instruction has one operand, which dies there, so one value is live at a time; 2 allows for
    # a compiler that does not give the operand's slot to the result
    chain = fe.compile_fill(2, 0, 1, [(0, E.main_at(1, E.input_at(0, E.row())))])
    got = pkg.fill_program_info(chain)
    assert got["instructions"] == 3 and 1 <= got["slots"] <= 2 and got["lds_lanes"] == 256 and got["assigned_columns"] == 1
    with fe.field(fe.BABYBEAR):
        chain_bb = fe.compile_fill(2, 0, 1, [(0, E.main_at(1, E.input_at(0, E.row())))])
    got = pkg.babybear.fill_program_info(chain_bb)
    assert got["instructions"] == 3 and 1 <= got["slots"] <= 2
    # a read in a scan's coefficients is an instruction of the coefficient pass; reads in two groups are issued in both
    x = E.input(0)
    sc = fe.compile_fill(3, 0, 1, [(0, fe.running_sum(E.input_at(0, E.row()))), (1, E.main_at(0, x) + E.input_at(0, E.row()))])
    assert pkg.fill_program_info(sc)["instructions"] == 2 + 5 and pkg.fill_scan_info(sc)[:3] == (1, 2, 1)
