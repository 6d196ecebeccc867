"""CPU tests of the scan steps of fill programs over BabyBear (include/mstark_bb.h, "SCAN STEPS"): the definition in the model
of tests/fill_scan_model_bb.py pinned to hand-computed columns, the front end (the `scans` keyword of compile_fill,
babybear.compile_fill, the blob of the second format "\\0MFILB02"), every refusal - from compile_fill, from the model and from
the library's host code (msbb_fill_program_info, msbb_fill_scan_info) - the four magics against the four info calls, and the
info words of a three-group program."""
import ctypes as C

import numpy as np
import pytest

import fill_gather_model as gm
import fill_model_bb as fmb
import fill_scan_model_bb as bsm
from test_fill_gather_model import gather_refusal_blobs
from test_fill_model import SEQ_OLD, SEQ_WANT, sequential_program
from test_fill_scan_model import info, scan_refusal_blobs, words_of

P = bsm.P
BB_CALLS = ["msbb_fill_program_info", "msbb_fill_scan_info"]
GL_CALLS = ["ms_fill_program_info", "ms_fill_scan_info"]


def u64(rows):
    return np.array(rows, dtype=np.uint64)


# ---------------------------------------------------------------- the definition, in the model
def test_scan_semantics_in_the_model(pkg, fe):
    E, bb = fe.Expr, pkg.babybear
    # column 0: a running sum of the inputs from 5; column 1: Horner, acc' = acc * 3 + input; column 2: the next row of column 0
    # minus column 0 (row n - 1 reads row 0); column 3: a running product of column 2 + 1
    prog = bb.compile_fill(4, 0, 1, [(0, fe.running_sum(E.input(0), init=5)), (1, fe.scan(3, E.input(0))),
                                     (2, E.main_next(0) - E.main(0)), (3, fe.running_product(E.main(2) + 1))])
    x = [2, P - 1, 10, 1000]  # the last input is never used by a scan: no wrap-around
    got = bsm.run(prog.blob, np.full((4, 4), 99, dtype=np.uint64), None, u64(x).reshape(4, 1))
    s = [5, 7, 6, 16]
    h = [0, 2, (3 * 2 + P - 1) % P, (3 * (3 * 2 + P - 1) + 10) % P]
    d = [2, P - 1, 10, (5 - 16) % P]
    q = [1, 3, 0, 0]  # (P - 1) + 1 = 0: the product stays 0 from there
    assert got.tolist() == [[s[r], h[r], d[r], q[r]] for r in range(4)]
    assert h[2] == 5 and h[3] == 25 and d[3] == P - 11  # by hand
    # one row: only init is written
    one = bsm.run(prog.blob, np.full((1, 4), 99, dtype=np.uint64), None, u64([[4]]))
    assert one.tolist() == [[5, 0, 0, 1]]
    # an input matrix shorter than the circuit reads 0 from its height on
    short = bsm.run(prog.blob, np.zeros((4, 4), dtype=np.uint64), None, u64([[2]]))
    assert short[:, 0].tolist() == [5, 7, 7, 7]


def test_restart_where_the_multiplier_is_zero_and_products_wrap_modulo_this_p(pkg, fe):
    E, bb = fe.Expr, pkg.babybear
    prog = bb.compile_fill(2, 0, 2, [(0, fe.scan(E.input(0), E.input(1), init=9)), (1, fe.running_product(E.input(0), init=1 << 30))])
    a = [2, 0, 3, 1 << 28, 1, 7]
    b = [1, 4, 0, 5, P - 1, 7]
    got = bsm.run(prog.blob, np.zeros((6, 2), dtype=np.uint64), None, u64([[a[r], b[r]] for r in range(6)]))
    # 9; 2 * 9 + 1; A = 0: the chain restarts at B = 4; 3 * 4; 2^28 * 12 + 5 = 3 * 2^30 + 5 = p + (2^30 + 2^27 - 1) + 5; that - 1
    big = (1 << 30) + (1 << 27) + 4
    assert big == 12 * (1 << 28) + 5 - P and big < P
    assert got[:, 0].tolist() == [9, 19, 4, 12, big, big - 1]
    # 2^30, 2^31 mod p = 2^27 - 1, 0 and 0 from there
    assert got[:, 1].tolist() == [1 << 30, (1 << 27) - 1, 0, 0, 0, 0]


def test_a_later_group_reads_the_scan_at_offsets_0_and_1_and_through_at(pkg, fe):
    E, bb = fe.Expr, pkg.babybear
    n = 8
    # column 0: 1, 3, 5, ... (a scan); column 1, a later group: column 0 at row 2 (r & 3), plus column 2 - which no step assigns -
    # read backwards; column 3: the scan's next row minus the scan (row n - 1 reads row 0)
    prog = bb.compile_fill(4, 0, 0, [(0, fe.running_sum(2, init=1)), (1, E.main_at(0, fe.bits(E.row(), 0, 2) * 2) + E.main_at(2, 7 - E.row())),
                                     (3, E.main_next(0) - E.main(0))])
    assert prog.blob[:8] == b"\0MFILB02"
    old = u64([[77, 66, 10 * r, 55] for r in range(n)])
    got = bsm.run(prog.blob, old)
    assert got[:, 0].tolist() == [1 + 2 * r for r in range(n)]
    assert got[:, 1].tolist() == [1 + 4 * (r & 3) + 10 * (7 - r) for r in range(n)]
    assert got[:, 2].tolist() == [10 * r for r in range(n)]
    assert got[:, 3].tolist() == [2] * (n - 1) + [P - 14]
    # an index from the height on reads 0, p - 1 among them
    far = bb.compile_fill(2, 0, 1, [(0, fe.running_sum(1, init=3)), (1, E.main_at(0, E.input(0)))])
    got = bsm.run(far.blob, np.zeros((4, 2), dtype=np.uint64), None, u64([[3], [4], [P - 1], [0]]))
    assert got[:, 1].tolist() == [6, 0, 0, 3]


def test_the_model_equals_the_older_models_on_the_first_format(pkg, fe):
    rng = np.random.default_rng(6)
    n = 16
    xs, ys = fe.xorshift_pairs(n)
    m16 = np.uint64(0xFFFF)
    halves = np.stack([xs & m16, xs >> np.uint64(16), ys & m16, ys >> np.uint64(16)], axis=1)
    with fe.field(fe.BABYBEAR):
        hprog, bseq = fe.u32_add_halves_fill_program(n - 3), sequential_program(fe)
    old = rng.integers(0, P, size=(n, 14), dtype=np.uint64)
    assert np.array_equal(bsm.run(hprog.blob, old, None, halves), fmb.run(hprog.blob, old, None, halves))
    assert np.array_equal(bsm.run(hprog.blob, old, None, halves[:5]), gm.run(hprog.blob, old, None, halves[:5]))
    assert bsm.run(bseq.blob, u64(SEQ_OLD)).tolist() == SEQ_WANT
    assert bsm.parse(hprog.blob)[:5] == fmb.parse(hprog.blob) and bsm.parse(hprog.blob)[5] == {}


# ---------------------------------------------------------------- the front end
def test_the_keyword_and_the_blob_of_the_second_format(pkg, fe):
    E, bb = fe.Expr, pkg.babybear
    steps = [(0, E.input(0)), (1, fe.scan(E.main(0), E.input(0), init=7)), (2, fe.running_sum(E.main(1)))]
    with fe.field(fe.BABYBEAR):
        with pytest.raises(fe.CompileError) as e:  # no keyword: today's refusal, verbatim
            fe.compile_fill(3, 0, 1, steps)
        assert str(e.value).startswith("ScanStepInThisField step=1: scan steps: Goldilocks configuration only")
        with pytest.raises(fe.CompileError, match="ScanStepInThisField"):
            fe.compile_fill(3, 0, 1, steps, scans=None)
        keyword = fe.compile_fill(3, 0, 1, steps, scans=True)
        assert fe.FILL_SCAN_MAGIC == bsm.SCAN_MAGIC == fe.BABYBEAR["FILL_SCAN_MAGIC"]
    assert fe.FILL_SCAN_MAGIC == 0x32304C4C49464D00 == fe.GOLDILOCKS["FILL_SCAN_MAGIC"]  # and the field is left again
    prog = bb.compile_fill(3, 0, 1, steps)
    assert prog.blob == keyword.blob and prog.blob[:8] == b"\0MFILB02"
    V, I, M = fe.N_VAR, fe.SRC_INPUT, fe.SRC_MAIN
    assert prog.nodes == [(V, I, 0, 0, 0), (V, M, 0, 0, 0), (fe.N_CONST, 0, 0, 1, 0), (V, M, 0, 1, 0)]
    assert prog.steps == [(0, 0), (1, 0), (2, 3)] and prog.scans == [(1, 1, 7), (2, 2, 0)]
    assert words_of(prog.blob) == [
        0x3230424C49464D00, 3, 0, 1, 4, 3, 2,                                           # magic, widths, n_nodes, n_steps, n_scans
        V | (I << 8), 0, 0, V | (M << 8), 0, 0, fe.N_CONST, 1, 0, V | (M << 8), 1, 0,   # nodes [kind | source << 8 | offset << 16, a, b]
        0, 0, 1, 0, 2, 3,                                                               # steps [dst, root]; a scan step's root is its add root
        1, 1, 7, 2, 2, 0]                                                               # scans [step index, mul root, init]
    assert bsm.parse(prog.blob) == (3, 0, 1, prog.nodes, prog.steps, {1: (1, 7), 2: (2, 0)})
    # the keyword changes nothing under Goldilocks
    assert fe.compile_fill(3, 0, 1, steps, scans=True).blob == fe.compile_fill(3, 0, 1, steps).blob
    assert fe.compile_fill(3, 0, 1, steps).blob[:8] == b"\0MFILL02"
    # fill_blob follows the field
    with fe.field(fe.BABYBEAR):
        assert fe.fill_blob(3, 0, 1, prog.nodes, prog.steps, prog.scans) == prog.blob
        assert fe.fill_blob(3, 0, 1, prog.nodes, prog.steps)[:8] == b"\0MFILB01"


def test_a_scan_free_program_keeps_the_first_format(pkg, fe):
    E, bb = fe.Expr, pkg.babybear
    with fe.field(fe.BABYBEAR):
        x3 = E.input(0) + 3
        plain = [fe.u32_add_halves_fill_program(100), sequential_program(fe), fe.compile_fill(2, 1, 1, [(0, x3)]), fe.compile_fill(2, 0, 0, [])]
        keyed = [fe.compile_fill(p.main_width, p.preprocessed_width, p.n_inputs, [], scans=True) for p in plain[3:]]
    keyed += [bb.compile_fill(2, 1, 1, [(0, x3)])]
    assert keyed[0].blob == plain[3].blob and keyed[1].blob == plain[2].blob
    for prog in plain + keyed:
        assert prog.scans == [] and prog.blob[:8] == b"\0MFILB01"
        words = [0x3130424C49464D00, prog.main_width, prog.preprocessed_width, prog.n_inputs, len(prog.nodes), len(prog.steps)]
        for kind, source, offset, a, b in prog.nodes:
            words += [kind | (source << 8) | (offset << 16), a, b]
        for dst, root in prog.steps:
            words += [dst, root]
        assert prog.blob == np.asarray(words, dtype=np.uint64).tobytes()


def test_compile_fill_refusals_hold_under_babybear(pkg, fe):
    E, bb = fe.Expr, pkg.babybear
    x, row = E.input(0), E.row()
    cases = [("ScanReadsOwnColumn", [(0, fe.scan(x, E.main(0)))]),
             ("ScanReadsOwnColumn", [(0, fe.scan(E.main(0) + 1, x))]),
             ("ScanReadsOwnColumn", [(0, fe.scan(x, E.main_next(0)))]),
             ("ScanInitOutOfRange", [(0, fe.scan(x, x, init=P))]),
             ("ScanInitOutOfRange", [(0, fe.running_sum(x, init=-1))]),
             ("ScanInitOutOfRange", [(0, fe.running_sum(x, init=(1 << 64) - (1 << 32)))]),  # canonical over the other field only
             ("NextRowOfAssignedColumn", [(1, x), (0, E.main_next(1)), (2, fe.running_sum(x))]),            # the same ordinary group
             ("NextRowOfAssignedColumn", [(0, E.main_next(2)), (2, fe.running_sum(x))]),                    # an earlier group reads
             ("NextRowOfAssignedColumn", [(0, fe.scan(E.main_next(2), x)), (2, x)]),                        # a scan reads, a later group assigns
             ("IndexedReadOfAssignedColumn column=0 step=1", [(0, x), (1, E.main_at(0, row)), (2, fe.running_sum(x))]),  # the same group
             ("IndexedReadOfAssignedColumn column=0 step=0", [(1, E.main_at(0, row)), (0, fe.running_sum(x))]),     # a later group assigns
             ("IndexedReadOfAssignedColumn column=0 step=0", [(0, fe.scan(E.main_at(0, row), x))]),                 # a scan's own dst
             ("DstOutOfRange", [(3, fe.running_sum(x))])]
    for name, steps in cases:
        with pytest.raises(fe.CompileError) as e:
            bb.compile_fill(3, 0, 1, steps)
        assert str(e.value).startswith(name), (name, str(e.value))
    assert bb.compile_fill(3, 0, 1, [(0, fe.running_sum(x, init=P - 1))]).scans[0][2] == P - 1
    # the other direction: a LATER group may read the next row of a finished scan column, and index it
    ok = bb.compile_fill(3, 0, 1, [(2, fe.running_sum(x)), (0, E.main_next(2) - E.main_at(2, row)), (1, fe.scan(E.main_next(2), E.main_next(0)))])
    assert len(ok.scans) == 2 and bsm.parse(ok.blob)[5].keys() == {0, 2}


# ---------------------------------------------------------------- refusals of the blob: the model and the library's host code
def bb_refusal_blobs(fe):
    """scan_refusal_blobs and the scan cases of gather_refusal_blobs rebuilt under BabyBear -> (good, cases (what, blob, a word
    the error text must contain), accepted (what, blob)); init = p and the constant = p are this field's p"""
    N = fe
    with fe.field(fe.BABYBEAR):
        assert fe.P == P
        good, cases, accepted = scan_refusal_blobs(fe)  # (it reads P of its own module for two cases: replaced below)
        nodes = [(N.N_VAR, N.SRC_INPUT, 0, 0, 0), (N.N_CONST, 0, 0, 3, 0), (N.N_ADD, 0, 0, 0, 1)]
        cases = [c for c in cases if c[0] not in ("init = p", "constant")]
        cases += [("init = p", fe.fill_blob(2, 1, 1, nodes, [(0, 2)], [(0, 1, P)]), "init"),
                  ("init = p + 1", fe.fill_blob(2, 1, 1, nodes, [(0, 2)], [(0, 1, P + 1)]), "init"),
                  ("constant = p", fe.fill_blob(2, 1, 1, [(N.N_CONST, 0, 0, P, 0)], [(0, 0)], [(0, 0, 0)]), "constant")]
        accepted = accepted + [("init = p - 1", fe.fill_blob(2, 1, 1, nodes, [(0, 2)], [(0, 1, P - 1)])),
                               ("constant = p - 1", fe.fill_blob(2, 1, 1, [(N.N_CONST, 0, 0, P - 1, 0)], [(0, 0)], [(0, 0, 0)]))]
        _, _, g_cases, g_accepted = gather_refusal_blobs(fe)
    assert any(c[0] == "init = 2^64 - 1" for c in cases) and len(g_cases) == 4 and len(g_accepted) == 3
    return good, cases + g_cases, accepted + g_accepted


@pytest.mark.parametrize("call", BB_CALLS)
def test_blob_refusals(pkg, fe, call):
    good, cases, accepted = bb_refusal_blobs(fe)
    assert good[:8] == b"\0MFILB02" and all(b[:7] == b"\0MFILB0" for _, b, _ in cases if len(b) >= 8)
    assert info(pkg, good, call)[0] == 0, info(pkg, good, call)[2]
    bsm.parse(good)
    for what, blob, word in cases:
        rc, _, text = info(pkg, blob, call)
        assert rc == -1 and text.startswith(call + ": ") and word in text, (what, rc, text)
        with pytest.raises(bsm.FillError):  # the model refuses the same programs
            bsm.parse(blob)
    for what, blob in accepted:
        assert info(pkg, blob, call)[0] == 0, (what, info(pkg, blob, call)[2])
        bsm.parse(blob)


def test_four_magics_against_four_info_calls(pkg, fe):
    E = fe.Expr
    steps = [(0, E.input(0) + 1), (1, fe.running_sum(E.main(0)))]
    blobs = {"\0MFILL01": fe.compile_fill(2, 0, 1, steps[:1]).blob, "\0MFILL02": fe.compile_fill(2, 0, 1, steps).blob,
             "\0MFILB01": pkg.babybear.compile_fill(2, 0, 1, steps[:1]).blob, "\0MFILB02": pkg.babybear.compile_fill(2, 0, 1, steps).blob}
    for magic, blob in blobs.items():
        assert blob[:8] == magic.encode()
        for call in GL_CALLS + BB_CALLS:
            rc, _, text = info(pkg, blob, call)
            if (magic[5] == "B") == call.startswith("msbb"):
                assert rc == 0, (magic, call, text)
            else:
                assert rc == -1 and text.startswith(call + ": ") and "magic" in text, (magic, call, text)
    for magic, blob in blobs.items():  # the model of this field: its own two, not the other's
        if magic[5] == "B":
            bsm.parse(blob)
        else:
            with pytest.raises(bsm.FillError):
                bsm.parse(blob)


# ---------------------------------------------------------------- the info words
def test_info_words_of_a_three_group_program(pkg, fe):
    E, bb = fe.Expr, pkg.babybear
    x = E.input(0)
    affine = bb.compile_fill(3, 0, 1, [(0, x + 1), (1, fe.scan(x, E.main(0), init=2)), (2, E.main_next(1) - E.main(1))])
    T = bb.fill_scan_info(affine)[3]
    assert T >= 256 and T % 64 == 0
    # launches of the fill kernel: the group of step 0, the coefficient pass of the scan, the group of step 2
    assert bb.fill_scan_info(affine) == (1, 3, 0, T)
    rc, out, _ = info(pkg, affine.blob, "msbb_fill_program_info")
    # [x, 1, x + 1] + [x, main 0: a load of the trace, group 0 has finished] + [main 1 at the next row, main 1, their difference]
    assert rc == 0 and out[0] == 3 + 2 + 3 and 2 <= out[1] <= 3 and out[2] == 256 and out[3] == 3
    assert bb.fill_program_info(affine) == {"instructions": 8, "slots": out[1], "lds_lanes": 256, "assigned_columns": 3}
    # the multiplier authored as the constant 1: the additive form, whose pass computes the add root alone
    additive = bb.compile_fill(3, 0, 1, [(0, x + 1), (1, fe.running_sum(E.main(0), init=2)), (2, E.main_next(1) - E.main(1))])
    assert bb.fill_scan_info(additive) == (1, 3, 1, T) and info(pkg, additive.blob, "msbb_fill_program_info")[1][0] == 3 + 1 + 3
    # two scans in a row are two groups; steps behind the last scan are one more; the same dst twice counts once
    four = bb.compile_fill(3, 0, 1, [(0, fe.running_sum(x)), (1, fe.running_product(x)), (2, E.main(0)), (2, E.main(1) + E.main(0))])
    assert bb.fill_scan_info(four) == (2, 3, 1, T) and info(pkg, four.blob, "msbb_fill_program_info")[1][3] == 3
    # a wide coefficient pass leaves LDS: the smallest lanes figure is reported
    with fe.field(fe.BABYBEAR):
        leaves = [fe.bits(x + k, k % 25, 7) for k in range(300)]
    wide = leaves[-1]
    for leaf in reversed(leaves[:-1]):
        wide = leaf - wide
    lanes0 = bb.compile_fill(3, 0, 1, [(0, x + 1), (1, fe.scan(x, wide))])
    assert info(pkg, lanes0.blob, "msbb_fill_program_info")[1][2] == 0 and bb.fill_program_info(lanes0)["slots"] >= 300
    # a program of the first format: no scans, one launch (none without steps)
    with fe.field(fe.BABYBEAR):
        assert bb.fill_scan_info(fe.u32_add_halves_fill_program(100)) == (0, 1, 0, T)
    assert bb.fill_scan_info(bb.compile_fill(2, 0, 0, [])) == (0, 0, 0, T)


def test_scan_info_is_part_of_the_interface(pkg):
    bb = pkg.babybear
    assert "msbb_fill_scan_info" in bb.exported_symbols() and hasattr(bb, "fill_scan_info") and hasattr(bb, "compile_fill")
    L = pkg.lib()
    u8p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
    blob = (C.c_uint8 * 56)()
    out = (C.c_uint64 * 4)()
    assert L.msbb_fill_scan_info(C.cast(None, u8p), C.c_size_t(56), out) == -1
    assert L.ms_last_error().decode() == "msbb_fill_scan_info: null argument"
    assert L.msbb_fill_scan_info(blob, C.c_size_t(56), C.cast(None, u64p)) == -1 and b"null" in L.ms_last_error()
    assert L.msbb_fill_scan_info(blob, C.c_size_t(56), out) == -1 and b"magic" in L.ms_last_error()
