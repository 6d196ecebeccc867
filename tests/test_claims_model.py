"""CPU: claim programs (include/mstark.h, "CLAIM PROGRAMS") - the blob that frontend.compile_claims emits, word by word; the
model of tests/claims_model.py against expectations written out by hand; every refusal of the front end; every refusal of a
blob, through ms_claims_program_info (host code, no device) and through the model; and the three entry points in the header,
the exported-symbol list and the Rust declarations."""
import os
import re

import numpy as np
import pytest

import claims_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = cm.P
NONE = (1 << 64) - 1


def words(blob):
    return [int(x) for x in np.frombuffer(blob, dtype="<u8")]


def blob_of(ws):
    return np.asarray(ws, dtype=np.uint64).tobytes()


def hand_blob(nodes, roots, keep=NONE, mw=3, pw=2, ni=1, magic=cm.MAGIC, n_nodes=None, width=None):
    ws = [magic, mw, pw, ni, len(nodes) if n_nodes is None else n_nodes, len(roots) if width is None else width, keep]
    for (kind, src, off, a, b) in nodes:
        ws += [kind | (src << 8) | (off << 16), a, b]
    return blob_of(ws + list(roots))


def test_blob_word_by_word(fe):
    E = fe.Expr
    prog = fe.compile_claims(3, 2, 1, [E.const(7), E.main(0) + E.main_next(1), E.pre_at(1, E.input(0)), E.main(0) + E.main_next(1)],
                             keep=fe.lt(E.row(), 5))
    assert (prog.width, prog.has_keep, prog.main_width, prog.preprocessed_width, prog.n_inputs) == (4, True, 3, 2, 1)
    assert words(prog.blob) == [
        0x314D49414C434D00, 3, 2, 1, 9, 4, 8,  # magic, widths, inputs, nodes, W, keep root
        0, 7, 0,                               # 0: const 7
        1 | 1 << 8, 0, 0,                      # 1: main(0)
        1 | 1 << 8 | 1 << 16, 1, 0,            # 2: main_next(1)
        6, 1, 2,                               # 3: add
        1 | 3 << 8, 0, 0,                      # 4: input(0)
        22 | 0 << 8, 1, 4,                     # 5: pre_at(1, node 4)
        16, 0, 0,                              # 6: row
        0, 5, 0,                               # 7: const 5
        19, 6, 7,                              # 8: lt
        0, 3, 5, 3]                            # the element roots: equal expressions share a node
    assert prog.blob[:8] == b"\0MCLAIM1"
    assert cm.parse(prog.blob) == (3, 2, 1, prog.nodes, prog.roots, 8)
    bare = fe.compile_claims(1, 0, 0, [E.main(0)])
    assert words(bare.blob) == [0x314D49414C434D00, 1, 0, 0, 1, 1, NONE, 1 | 1 << 8, 0, 0, 0] and not bare.has_keep
    # the U32Add claims: [1, x, y, z] with the words from their bytes
    u = fe.u32_add_claims_program()
    t = np.zeros((2, 14), dtype=np.uint64)
    t[0, :12] = [0x78, 0x56, 0x34, 0x12, 0xF0, 0xDE, 0xBC, 0x9A, 0x68, 0x35, 0xF1, 0xAC]
    assert cm.run(u.blob, t, rows=1) == [[1, 0x12345678, 0x9ABCDEF0, 0xACF13568]] and (u.width, u.has_keep) == (4, False)


def test_model_against_hand_written_expectations(fe):
    E = fe.Expr
    trace = np.array([[1, 10, 100], [2, 20, 200], [3, 30, 300], [4, 40, P - 1]], dtype=np.uint64)
    pre = np.array([[5, 50], [6, 60], [7, 70], [8, 80]], dtype=np.uint64)
    inputs = np.array([[3], [9]], dtype=np.uint64)  # two rows: rows 2 and 3 read 0; the index 9 is beyond every height
    prog = fe.compile_claims(3, 2, 1, [E.main(0) + E.main_next(1), E.pre_at(1, E.input(0)), E.main(2) * 2, E.input_next(0), E.main_at(1, E.row() + 2)])
    assert cm.run(prog.blob, trace, pre, inputs) == [
        [1 + 20, 80, 200, 9, 30],
        [2 + 30, 0, 400, 0, 40],        # pre_at(1, 9): from the height on, 0; input_next at row 1 is input row 2: 0
        [3 + 40, 50, 600, 0, 0],        # input(0) = 0 from the input height on, so pre row 0; main_at(1, 4) = 0
        [4 + 10, 50, P - 2, 3, 0]]      # the next row of the last row is row 0, for the trace and for the inputs
    assert cm.run(prog.blob, trace, pre, inputs, rows=2) == [[21, 80, 200, 9, 30], [32, 0, 400, 0, 40]]
    assert cm.run(prog.blob, trace, pre, inputs, rows=0) == []
    # rows = 3 of n = 4: row 2's next row is row 3, not row 0 - the wrap is the trace's, not the call's
    assert cm.run(prog.blob, trace, pre, inputs, rows=3)[2][0] == 3 + 40
    # keep: the rows where it is non-zero, in row order; any non-zero value keeps
    kept = fe.compile_claims(3, 2, 1, [E.main(0), E.row()], keep=E.main(0) - 2)
    assert cm.run(kept.blob, trace, pre, inputs) == [[1, 0], [3, 2], [4, 3]]
    assert cm.run(fe.compile_claims(3, 2, 1, [E.main(0)], keep=E.const(0)).blob, trace, pre, inputs) == []
    offs, data = cm.claims(kept.blob, trace, pre, inputs, before=(np.array([0, 0, 3], dtype=np.uint64), np.array([7, 8, 9], dtype=np.uint64)))
    assert offs.tolist() == [0, 0, 3, 5, 7, 9] and data.tolist() == [7, 8, 9, 1, 0, 3, 2, 4, 3]
    offs, data = cm.claims(kept.blob, trace, pre, inputs, rows=1)
    assert offs.tolist() == [0, 2] and data.tolist() == [1, 0]
    # the witness-only operators
    ops = fe.compile_claims(3, 2, 1, [fe.bits(E.main(2), 3, 4), fe.inv0(E.main(0) - 1), fe.bit_xor(E.main(1), E.main(0)), fe.bit_and(E.main(1), 24), -E.main(0)])
    got = cm.run(ops.blob, trace, pre, inputs)
    assert got[0] == [(100 >> 3) & 15, 0, 10 ^ 1, 10 & 24, P - 1] and got[1][1] == 1 and got[2][1] == pow(2, P - 2, P)


def test_front_end_refusals(fe):
    E = fe.Expr
    ok = [E.main(0)]
    cases = [
        ("PeerReadInClaimProgram", lambda: fe.compile_claims(3, 0, 0, [E.peer(1, 0)])),
        ("PeerReadInClaimProgram", lambda: fe.compile_claims(3, 0, 0, ok, keep=E.peer_pre_at(2, 0, E.row()))),
        ("ScanInClaimProgram", lambda: fe.compile_claims(3, 0, 0, [fe.running_sum(E.main(0))])),
        ("ScanInClaimProgram", lambda: fe.compile_claims(3, 0, 0, ok, keep=fe.scan(1, 1))),
        ("NotAllowedInFillProgram kind=2", lambda: fe.compile_claims(3, 0, 0, [E.main(0) + E.public(0)])),
        ("NotAllowedInFillProgram kind=3", lambda: fe.compile_claims(3, 0, 0, [fe.IS_FIRST_ROW])),
        ("NotAllowedInFillProgram kind=4", lambda: fe.compile_claims(3, 0, 0, [fe.IS_LAST_ROW])),
        ("NotAllowedInFillProgram kind=5", lambda: fe.compile_claims(3, 0, 0, ok, keep=fe.IS_TRANSITION)),
        ("Stage2InFillProgram", lambda: fe.compile_claims(3, 0, 0, [E.var(fe.SRC_STAGE2, 0, 0)])),
        ("Stage2InFillProgram", lambda: fe.compile_claims(3, 0, 0, [E.at(fe.SRC_STAGE2, 0, E.row())])),
        ("ColumnOutOfRange", lambda: fe.compile_claims(3, 0, 0, [E.main(3)])),
        ("ColumnOutOfRange", lambda: fe.compile_claims(3, 0, 0, [E.preprocessed(0)])),
        ("ColumnOutOfRange", lambda: fe.compile_claims(3, 1, 0, [E.input(0)])),
        ("ColumnOutOfRange", lambda: fe.compile_claims(3, 1, 2, [E.input_at(2, E.row())])),
        ("RowOffsetOutOfRange", lambda: fe.compile_claims(3, 0, 0, [E.var(fe.SRC_MAIN, 2, 0)])),
        ("UnknownNodeKind", lambda: fe.compile_claims(3, 0, 0, [E(12, E.main(0), E.main(1))])),
        ("ClaimWidthOutOfRange width=0", lambda: fe.compile_claims(3, 0, 0, [])),
        ("ClaimWidthOutOfRange width=65537", lambda: fe.compile_claims(3, 0, 0, [E.main(0)] * 65537)),
    ]
    for text, call in cases:
        with pytest.raises(fe.CompileError, match=re.escape(text)):
            call()
    # the text names the element
    with pytest.raises(fe.CompileError, match=r"element 2 of the claim program"):
        fe.compile_claims(3, 0, 0, [E.main(0), E.main(1), E.public(0)])
    with pytest.raises(fe.CompileError, match=r"keep of the claim program"):
        fe.compile_claims(3, 0, 0, ok, keep=E.main(9))
    # what a fill program may not do and a claim program may: nothing is assigned
    free = fe.compile_claims(3, 0, 0, [E.main_next(0), E.main_at(1, E.main(2)), E.main(0)])
    assert free.width == 3 and len(fe.compile_claims(3, 0, 0, [E.main(0)] * 65536).roots) == 65536


VAR_MAIN0 = (1, 1, 0, 0, 0)


def blob_refusals(fe):
    """[(what, blob, text of ms_claims_program_info, text of the model)]"""
    E = fe.Expr
    good = fe.compile_claims(3, 2, 1, [E.main(0) + E.main_next(1), E.pre_at(1, E.input(0))], keep=E.main(2))
    ws = words(good.blob)
    fill = fe.compile_fill(3, 2, 1, [(0, E.main(1))])
    scan = fe.compile_fill(3, 2, 1, [(0, fe.running_sum(E.main(1)))])
    peers = fe.compile_fill(3, 2, 1, [(0, E.peer(1, 0))], peers={1: (2, 0)})
    assert fill.blob[:8] == b"\0MFILL01" and scan.blob[:8] == b"\0MFILL02" and peers.blob[:8] == b"\0MFILL03"
    out = [
        ("one word short", blob_of(ws[:-1]), "truncated program blob", "truncated"),
        ("one word long", blob_of(ws + [0]), "truncated program blob", "truncated"),
        ("half a word", good.blob + b"\0\0\0\0", "truncated program blob", "truncated"),
        ("a header alone, short", blob_of(ws[:6]), "truncated program blob", "truncated"),
        ("W = 0", hand_blob([VAR_MAIN0], []), "a claim has 1 to 2^16 elements, this program 0", "width"),
        ("W = 2^16 + 1", hand_blob([VAR_MAIN0], [0] * 65537), "a claim has 1 to 2^16 elements, this program 65537", "width"),
        ("a root out of range", hand_blob([VAR_MAIN0], [0, 1]), "element 1: root 1 is out of range", "element root 1"),
        ("a keep root out of range", hand_blob([VAR_MAIN0], [0], keep=1), "keep: root 1 is out of range", "keep root"),
        ("a keep root far out of range", hand_blob([VAR_MAIN0], [0], keep=NONE - 1), "keep: root", "keep root"),
        ("a peer source", hand_blob([(1, 4, 0, 0, 0)], [0]), "node 0: peer reads are not allowed in a claim program", "peer source"),
        ("a peer source in an indexed read", hand_blob([VAR_MAIN0, (22, 11, 0, 0, 0)], [1]), "node 1: peer reads are not allowed in a claim program", "peer source"),
        ("a source beyond the peers", hand_blob([(1, 12, 0, 0, 0)], [0]), "node 0: unknown variable source", "unknown source"),
        ("a scan magic", scan.blob, "a fill program, not a claim program", "a fill program"),
        ("a fill magic", fill.blob, "a fill program, not a claim program", "a fill program"),
        ("a peer magic", peers.blob, "a fill program, not a claim program", "a fill program"),
        ("a fill magic on a claim body", blob_of([0x31304C4C49464D00] + ws[1:]), "a fill program, not a claim program", "a fill program"),
        ("another magic", blob_of([0x324D49414C434D00] + ws[1:]), "not a claim program (wrong magic)", "magic"),
        ("a public", hand_blob([(2, 0, 0, 0, 0)], [0]), "node 0: publics are not allowed in a claim program", "public"),
        ("a stage-2 variable", hand_blob([(1, 2, 0, 0, 0)], [0]), "node 0: stage-2 variables are not allowed in a claim program", "stage 2"),
        ("a stage-2 indexed read", hand_blob([VAR_MAIN0, (22, 2, 0, 0, 0)], [1]), "node 1: stage-2 columns are not allowed in a claim program", "stage 2"),
        ("a column out of range", hand_blob([(1, 1, 0, 3, 0)], [0]), "node 0: variable 3 of source 1 is out of range (width 3)", "column"),
        ("an indexed column out of range", hand_blob([VAR_MAIN0, (22, 0, 0, 2, 0)], [1]), "node 1: indexed read of column 2 of source 0", "column"),
        ("a row offset of 2", hand_blob([(1, 1, 2, 0, 0)], [0]), "node 0: row offset out of range", "row offset"),
        ("an offset on an indexed read", hand_blob([VAR_MAIN0, (22, 1, 1, 0, 0)], [1]), "node 1: the offset field of an indexed read must be 0", "offset field"),
        ("a forward row operand", hand_blob([(22, 1, 0, 0, 0)], [0]), "node 0: forward row operand", "forward row operand"),
        ("a forward operand", hand_blob([VAR_MAIN0, (6, 0, 0, 0, 1)], [1]), "node 1: forward operand", "forward operand"),
        ("bad bits fields", hand_blob([VAR_MAIN0, (17, 0, 0, 0, 60 | 5 << 8)], [1]), "node 1: bad bits fields", "bits"),
        ("a non-canonical constant", hand_blob([(0, 0, 0, P, 0)], [0]), "node 0: non-canonical constant", "constant"),
        ("a malformed head word", blob_of(ws[:7] + [ws[7] | 1 << 24] + ws[8:]), "node 0: malformed head word", "head word"),
        ("more nodes than words", hand_blob([VAR_MAIN0], [0], n_nodes=1 << 40), "truncated program blob", "truncated"),
    ]
    for kind in (3, 4, 5):
        out.append(("selector %d" % kind, hand_blob([(kind, 0, 0, 0, 0)], [0]), "node 0: selector nodes are not allowed in a claim program", "selector"))
    for kind in list(range(10, 16)) + [23, 24, 255]:
        out.append(("node kind %d" % kind, hand_blob([VAR_MAIN0, (kind, 0, 0, 0, 0)], [1]), "node 1: unknown node kind %d" % kind, "node kind %d" % kind))
    return good, out


def test_blob_refusals(pkg, fe):
    good, cases = blob_refusals(fe)
    info = pkg.claims_program_info(good)
    assert (info["width"], info["has_keep"], info["lds_lanes"]) == (2, True, 256) and info["instructions"] == 6 and 1 <= info["slots"] <= 6
    assert cm.parse(good.blob)[5] == good.keep
    for what, blob, text, model_text in cases:
        with pytest.raises(pkg.MstarkError, match=re.escape(text)) as e:
            pkg.claims_program_info(blob)
        assert str(e.value).startswith("ms_claims_program_info: "), what
        with pytest.raises(cm.ClaimError, match=re.escape(model_text)):
            cm.parse(blob)
    # a claim program is no fill program
    with pytest.raises(pkg.MstarkError, match=re.escape("ms_fill_program_info: not a fill program (wrong magic)")):
        pkg.fill_program_info(good)
    with pytest.raises(pkg.MstarkError, match=re.escape("ms_fill_scan_info: not a fill program (wrong magic)")):
        pkg.fill_scan_info(good)
    # what the info call tells: shared subexpressions once, the outputs live to the end
    E = fe.Expr
    wide = fe.compile_claims(14, 0, 0, [E.main(k % 14) * (k + 2) for k in range(49)])
    assert pkg.claims_program_info(wide) == {"instructions": 14 + 49 + 49, "slots": pkg.claims_program_info(wide)["slots"], "lds_lanes": 128, "width": 49, "has_keep": False}
    assert 49 <= pkg.claims_program_info(wide)["slots"] <= 64
    same = fe.compile_claims(14, 0, 0, [E.main(0)] * 5)
    assert pkg.claims_program_info(same)["instructions"] == 1


def test_symbols_in_header_exports_and_rust(pkg):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mstark.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "mstark_sys.rs")).read()
    for sym in ("ms_witness_claims_fill", "ms_claims_program_info", "ms_witness_claims"):
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in pkg.exported_symbols(), sym
        assert re.search(r"pub fn %s\(" % sym, rust), sym
        assert hasattr(pkg.lib(), sym), sym
    assert re.search(r"#define MS_CLAIMS_REPLACE 0\b", header) and re.search(r"#define MS_CLAIMS_APPEND 1\b", header)
    assert (pkg.CLAIMS_REPLACE, pkg.CLAIMS_APPEND) == (0, 1)
