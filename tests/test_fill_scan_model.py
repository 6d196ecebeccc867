"""CPU tests of the scan steps of fill programs (include/mstark.h, "SCAN STEPS"): the blob of the second format word for
word, that a scan-free program keeps the first format byte for byte, the definition in the model of tests/fill_scan_model.py,
every refusal - from compile_fill, from the model and from the library's host code (ms_fill_program_info, ms_fill_scan_info) -
the group rule for offset-1 reads in both directions, and the info words of a three-group program."""
import ctypes as C

import numpy as np
import pytest

import fill_model as fm
import fill_scan_model as fsm
from test_fill_model import SEQ_OLD, SEQ_WANT, sequential_program

P = fm.P
SCAN_MAGIC = 0x32304C4C49464D00


def words_of(blob):
    return [int(x) for x in np.frombuffer(blob, dtype="<u8")]


def info(pkg, blob, call="ms_fill_program_info"):
    """(status, out4, error text)"""
    L = pkg.lib()
    a = np.frombuffer(bytes(blob), dtype=np.uint8)
    out = np.zeros(4, dtype=np.uint64)
    rc = getattr(L, call)(a.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_size_t(a.size), out.ctypes.data_as(C.POINTER(C.c_uint64)))
    return rc, [int(x) for x in out], L.ms_last_error().decode()


# ---------------------------------------------------------------- the blob
def test_blob_of_the_second_format_word_for_word(fe):
    E = fe.Expr
    prog = fe.compile_fill(3, 0, 1, [(0, E.input(0)), (1, fe.scan(E.main(0), E.input(0), init=7)), (2, fe.running_sum(E.main(1)))])
    V, I, M = fe.N_VAR, fe.SRC_INPUT, fe.SRC_MAIN
    # nodes in the order the steps reach them: input 0; main 0 (the mul root of step 1); the constant 1 (the mul root of step 2);
    # main 1
    assert prog.nodes == [(V, I, 0, 0, 0), (V, M, 0, 0, 0), (fe.N_CONST, 0, 0, 1, 0), (V, M, 0, 1, 0)]
    assert prog.steps == [(0, 0), (1, 0), (2, 3)] and prog.scans == [(1, 1, 7), (2, 2, 0)]
    assert words_of(prog.blob) == [
        SCAN_MAGIC, 3, 0, 1, 4, 3, 2,                                                   # magic, widths, n_nodes, n_steps, n_scans
        V | (I << 8), 0, 0, V | (M << 8), 0, 0, fe.N_CONST, 1, 0, V | (M << 8), 1, 0,   # nodes [kind | source << 8 | offset << 16, a, b]
        0, 0, 1, 0, 2, 3,                                                               # steps [dst, root]; a scan step's root is its add root
        1, 1, 7, 2, 2, 0]                                                               # scans [step index, mul root, init]
    assert prog.blob[:8] == b"\0MFILL02" and fe.FILL_SCAN_MAGIC == SCAN_MAGIC
    assert fsm.parse(prog.blob) == (3, 0, 1, prog.nodes, prog.steps, {1: (1, 7), 2: (2, 0)})


def test_a_scan_free_program_keeps_the_first_format(fe):
    E = fe.Expr
    for prog in (fe.u32_add_fill_program(100), sequential_program(fe), fe.compile_fill(2, 1, 1, [(0, E.input(0) + 3)]), fe.compile_fill(2, 0, 0, [])):
        assert prog.scans == [] and prog.blob[:8] == b"\0MFILL01"
        words = [fe.FILL_MAGIC, prog.main_width, prog.preprocessed_width, prog.n_inputs, len(prog.nodes), len(prog.steps)]
        for kind, source, offset, a, b in prog.nodes:
            words += [kind | (source << 8) | (offset << 16), a, b]
        for dst, root in prog.steps:
            words += [dst, root]
        assert prog.blob == np.asarray(words, dtype=np.uint64).tobytes()
        assert prog.blob == fe.fill_blob(prog.main_width, prog.preprocessed_width, prog.n_inputs, prog.nodes, prog.steps)
    # and the model of the second format reads it as fill_model does
    old = np.array(SEQ_OLD, dtype=np.uint64)
    assert fsm.run(sequential_program(fe).blob, old).tolist() == SEQ_WANT == fm.run(sequential_program(fe).blob, old).tolist()


# ---------------------------------------------------------------- the definition, in the model
def test_scan_semantics_in_the_model(fe):
    E = fe.Expr
    # column 0: a running sum of the inputs from 5; column 1: Horner, acc' = acc * 3 + input; column 2: the next row of column 0
    # minus column 0 (row n - 1 reads row 0); column 3: a running product of column 2 + 1
    prog = fe.compile_fill(4, 0, 1, [(0, fe.running_sum(E.input(0), init=5)), (1, fe.scan(3, E.input(0))),
                                     (2, E.main_next(0) - E.main(0)), (3, fe.running_product(E.main(2) + 1))])
    x = [2, P - 1, 10, 1000]  # the last input is never used by a scan: no wrap-around
    got = fsm.run(prog.blob, np.full((4, 4), 99, dtype=np.uint64), None, np.array(x, dtype=np.uint64).reshape(4, 1))
    s = [5, 7, 6, 16]
    h = [0, 2, (3 * 2 + P - 1) % P, (3 * (3 * 2 + P - 1) + 10) % P]
    d = [2, P - 1, 10, (5 - 16) % P]
    q = [1, 3, 0, 0]
    assert got.tolist() == [[s[r], h[r], d[r], q[r]] for r in range(4)]
    # one row: only init is written
    one = fsm.run(prog.blob, np.full((1, 4), 99, dtype=np.uint64), None, np.array([[4]], dtype=np.uint64))
    assert one.tolist() == [[5, 0, 0, 1]]
    # an input matrix shorter than the circuit reads 0 from its height on
    short = fsm.run(prog.blob, np.zeros((4, 4), dtype=np.uint64), None, np.array([[2]], dtype=np.uint64))
    assert short[:, 0].tolist() == [5, 7, 7, 7]


# ---------------------------------------------------------------- refusals of compile_fill
def test_compile_fill_refusals(fe):
    E = fe.Expr
    x = E.input(0)
    cases = [("ScanReadsOwnColumn", [(0, fe.scan(x, E.main(0)))]),                    # the add root reads dst at offset 0
             ("ScanReadsOwnColumn", [(0, fe.scan(E.main(0) + 1, x))]),                # the mul root does
             ("ScanReadsOwnColumn", [(0, fe.scan(x, E.main_next(0)))]),               # offset 1
             ("ScanReadsOwnColumn", [(0, fe.running_product(fe.inv0(E.main_next(0)) * x))]),
             ("ScanInitOutOfRange", [(0, fe.scan(x, x, init=P))]),
             ("ScanInitOutOfRange", [(0, fe.running_sum(x, init=-1))]),
             ("NextRowOfAssignedColumn", [(1, x), (0, E.main_next(1)), (2, fe.running_sum(x))]),            # the same ordinary group
             ("NextRowOfAssignedColumn", [(0, E.main_next(2)), (2, fe.running_sum(x))]),                    # an earlier group reads
             ("NextRowOfAssignedColumn", [(0, fe.scan(E.main_next(2), x)), (2, x)]),                        # a scan reads, a later group assigns
             ("NextRowOfAssignedColumn", [(2, fe.running_sum(x)), (0, E.main_next(2)), (1, fe.running_sum(x)), (2, x)]),  # assigned again later
             ("DstOutOfRange", [(3, fe.running_sum(x))]),
             ("ColumnOutOfRange", [(0, fe.scan(E.main(3), x))])]
    for name, steps in cases:
        with pytest.raises(fe.CompileError) as e:
            fe.compile_fill(3, 0, 1, steps)
        assert str(e.value).startswith(name), (name, str(e.value))
    # the other direction: a LATER group may read the next row of a finished scan column
    ok = fe.compile_fill(3, 0, 1, [(2, fe.running_sum(x)), (0, E.main_next(2) - E.main(2)), (1, fe.scan(E.main_next(2), E.main_next(0)))])
    assert len(ok.scans) == 2 and fsm.parse(ok.blob)[5].keys() == {0, 2}
    with fe.field(fe.BABYBEAR):
        with pytest.raises(fe.CompileError, match="scan steps: Goldilocks configuration only"):
            fe.compile_fill(3, 0, 1, [(0, fe.running_sum(E.input(0)))])
    # a scan marker is the right-hand side of a step and nothing else
    with pytest.raises((TypeError, AttributeError, fe.CompileError)):
        fe.compile_fill(3, 0, 1, [(0, fe.running_sum(x) + 1)])


# ---------------------------------------------------------------- refusals of the blob: the model and the library's host code
def scan_refusal_blobs(fe):
    """(what, blob, a word the error text must contain)"""
    N = fe
    nodes = [(N.N_VAR, N.SRC_INPUT, 0, 0, 0), (N.N_CONST, 0, 0, 3, 0), (N.N_ADD, 0, 0, 0, 1), (N.N_VAR, N.SRC_MAIN, 0, 1, 0),
             (N.N_VAR, N.SRC_MAIN, 1, 1, 0), (N.N_ADD, 0, 0, 3, 1), (N.N_NEG, 0, 0, 4, 0)]
    blob = lambda steps, scans, nd=nodes: fe.fill_blob(2, 1, 1, nd, steps, scans)
    good = blob([(0, 2)], [(0, 1, 5)])
    w = np.frombuffer(good, dtype="<u8").copy()
    more_scans, fewer_scans = w.copy(), w.copy()
    more_scans[6], fewer_scans[6] = 2, 0
    cases = [("truncated", good[:-8], "truncated"),
             ("a word too many", good + bytes(8), "truncated"),
             ("header of six words", good[:48], "truncated"),
             ("not whole words", good + b"\0", "truncated"),
             ("n_scans above the records", more_scans.tobytes(), "truncated"),
             ("n_scans below the records", fewer_scans.tobytes(), "truncated"),
             ("step index out of range", blob([(0, 2)], [(1, 1, 5)]), "step index"),
             ("step indices descending", blob([(0, 2), (1, 2)], [(1, 1, 5), (0, 1, 5)]), "ascending"),
             ("step index twice", blob([(0, 2), (1, 2)], [(1, 1, 5), (1, 1, 5)]), "ascending"),
             ("mul root out of range", blob([(0, 2)], [(0, len(nodes), 5)]), "mul root"),
             ("add root out of range", blob([(0, len(nodes))], [(0, 1, 5)]), "root"),
             ("dst out of range", blob([(2, 2)], [(0, 1, 5)]), "dst"),
             ("init = p", blob([(0, 2)], [(0, 1, P)]), "init"),
             ("init = 2^64 - 1", blob([(0, 2)], [(0, 1, (1 << 64) - 1)]), "init"),
             ("the add root reads dst", blob([(1, 5)], [(0, 1, 0)]), "own dst"),
             ("the mul root reads dst", blob([(1, 2)], [(0, 5, 0)]), "own dst"),
             ("dst at offset 1", blob([(1, 6)], [(0, 1, 0)]), "own dst"),
             ("next row, assigned by the same group", blob([(1, 2), (0, 6), (0, 2)], [(2, 1, 0)]), "offset-1"),
             ("next row, assigned by a later group", blob([(0, 6), (1, 2)], [(1, 1, 0)]), "offset-1"),
             ("next row read by a scan, assigned by a later group", blob([(0, 2), (1, 2)], [(0, 4, 0)]), "offset-1"),
             ("forward operand", blob([(0, 1)], [(0, 0, 0)], [nodes[0], (N.N_ADD, 0, 0, 0, 2), nodes[1]]), "forward"),
             ("constant", blob([(0, 0)], [(0, 0, 0)], [(N.N_CONST, 0, 0, P, 0)]), "constant")]
    accepted = [("next row of a scan column read by a later group", blob([(1, 2), (0, 6)], [(0, 1, 0)])),
                ("next row of a column no step assigns", blob([(0, 6)], [(0, 1, 0)])),
                ("no scan record: one group", fewer_scans[: len(w) - 3].tobytes())]
    return good, cases, accepted


@pytest.mark.parametrize("call", ["ms_fill_program_info", "ms_fill_scan_info"])
def test_blob_refusals(pkg, fe, call):
    good, cases, accepted = scan_refusal_blobs(fe)
    assert info(pkg, good, call)[0] == 0
    fsm.parse(good)
    for what, blob, word in cases:
        rc, _, text = info(pkg, blob, call)
        assert rc == -1 and text.startswith(call + ": ") and word in text, (what, rc, text)
        with pytest.raises(fm.FillError):  # the model refuses the same programs
            fsm.parse(blob)
    for what, blob in accepted:
        assert info(pkg, blob, call)[0] == 0, (what, info(pkg, blob, call)[2])
        fsm.parse(blob)


def test_the_other_configuration_refuses_the_blob_by_its_magic(pkg, fe):
    good = scan_refusal_blobs(fe)[0]
    rc, _, text = info(pkg, good, "msbb_fill_program_info")
    assert rc == -1 and text.startswith("msbb_fill_program_info: ") and "magic" in text
    with pytest.raises(fm.FillError):
        fm.parse(good)  # the model of the first format does not know it either


# ---------------------------------------------------------------- the info words
def test_info_words_of_a_three_group_program(pkg, fe):
    E = fe.Expr
    x = E.input(0)
    affine = fe.compile_fill(3, 0, 1, [(0, x + 1), (1, fe.scan(x, E.main(0), init=2)), (2, E.main_next(1) - E.main(1))])
    T = pkg.fill_scan_info(affine)[3]
    assert T >= 256 and T % 64 == 0
    # launches of the fill kernel: the group of step 0, the coefficient pass of the scan, the group of step 2
    assert pkg.fill_scan_info(affine) == (1, 3, 0, T)
    rc, out, _ = info(pkg, affine.blob)
    # [x, 1, x + 1] + [x, main 0: a load of the trace, group 0 has finished] + [main 1 at the next row, main 1, their difference]
    assert rc == 0 and out[0] == 3 + 2 + 3 and 2 <= out[1] <= 3 and out[2] == 256 and out[3] == 3
    assert pkg.fill_program_info(affine) == {"instructions": 8, "slots": out[1], "lds_lanes": 256, "assigned_columns": 3}
    # the multiplier authored as the constant 1: the additive form, whose pass computes the add root alone
    additive = fe.compile_fill(3, 0, 1, [(0, x + 1), (1, fe.running_sum(E.main(0), init=2)), (2, E.main_next(1) - E.main(1))])
    assert pkg.fill_scan_info(additive) == (1, 3, 1, T) and info(pkg, additive.blob)[1][0] == 3 + 1 + 3
    # two scans in a row are two groups; steps behind the last scan are one more; the same dst twice counts once
    four = fe.compile_fill(3, 0, 1, [(0, fe.running_sum(x)), (1, fe.running_product(x)), (2, E.main(0)), (2, E.main(1) + E.main(0))])
    assert pkg.fill_scan_info(four) == (2, 3, 1, T) and info(pkg, four.blob)[1][3] == 3
    # a wide coefficient pass leaves LDS: the smallest lanes figure is reported
    wide = x
    leaves = [fe.bits(x + k, k % 57, 8) for k in range(300)]
    wide = leaves[-1]
    for leaf in reversed(leaves[:-1]):
        wide = leaf - wide
    lanes0 = fe.compile_fill(3, 0, 1, [(0, x + 1), (1, fe.scan(x, wide))])
    assert info(pkg, lanes0.blob)[1][2] == 0 and pkg.fill_program_info(lanes0)["slots"] >= 300
    # a program of the first format: no scans, one launch (none without steps)
    assert pkg.fill_scan_info(fe.u32_add_fill_program(100)) == (0, 1, 0, T)
    assert pkg.fill_scan_info(fe.compile_fill(2, 0, 0, [])) == (0, 0, 0, T)


def test_scan_info_is_part_of_the_interface(pkg):
    assert "ms_fill_scan_info" in pkg.exported_symbols() and hasattr(pkg, "fill_scan_info")
    L = pkg.lib()
    u8p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
    blob = (C.c_uint8 * 56)()
    out = (C.c_uint64 * 4)()
    assert L.ms_fill_scan_info(C.cast(None, u8p), C.c_size_t(56), out) == -1
    assert L.ms_last_error().decode() == "ms_fill_scan_info: null argument"
    assert L.ms_fill_scan_info(blob, C.c_size_t(56), C.cast(None, u64p)) == -1 and b"null" in L.ms_last_error()
    assert L.ms_fill_scan_info(blob, C.c_size_t(56), out) == -1 and b"magic" in L.ms_last_error()
