"""CPU: BabyBear claim programs (include/mstark_bb.h, "Claim programs") - the blob that frontend.compile_claims emits under
field(BABYBEAR), word by word; the model of tests/claims_model_bb.py against expectations written out by hand; every refusal of
a blob, through msbb_claims_program_info (host code, no device) and through the model; the two configurations refusing each
other's magics; the lanes the info call reports; and the three entry points in the header, the library, the Rust declarations and
babybear.py."""
import os
import re

import numpy as np
import pytest

import claims_model_bb as cb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = cb.P
NONE = (1 << 64) - 1
MAGIC = 0x314249414C434D00
GL_FILL, GL_SCAN, GL_CLAIM = 0x31304C4C49464D00, 0x32304C4C49464D00, 0x314D49414C434D00
VAR_MAIN0 = (1, 1, 0, 0, 0)


@pytest.fixture(scope="module")
def bb(pkg):
    return pkg.babybear


def words(blob):
    return [int(x) for x in np.frombuffer(blob, dtype="<u8")]


def blob_of(ws):
    return np.asarray(ws, dtype=np.uint64).tobytes()


def hand_blob(nodes, roots, keep=NONE, mw=3, pw=2, ni=1, magic=MAGIC, n_nodes=None, width=None):
    ws = [magic, mw, pw, ni, len(nodes) if n_nodes is None else n_nodes, len(roots) if width is None else width, keep]
    for (kind, src, off, a, b) in nodes:
        ws += [kind | (src << 8) | (off << 16), a, b]
    return blob_of(ws + list(roots))


def test_blob_word_by_word(fe, bb):
    E = fe.Expr
    with fe.field(fe.BABYBEAR):
        prog = fe.compile_claims(3, 2, 1, [E.const(P + 7), E.main(0) + E.main_next(1), E.pre_at(1, E.input(0)), E.main(0) + E.main_next(1)],
                                 keep=fe.lt(E.row(), 5))
        folded = fe.compile_claims(1, 0, 0, [E.main(0) * E.const(256 ** 4)])
    assert (prog.width, prog.has_keep, prog.main_width, prog.preprocessed_width, prog.n_inputs) == (4, True, 3, 2, 1)
    assert words(prog.blob) == [
        MAGIC, 3, 2, 1, 9, 4, 8,               # magic, widths, inputs, nodes, W, keep root
        0, 7, 0,                               # 0: const p + 7, folded modulo p
        1 | 1 << 8, 0, 0,                      # 1: main(0)
        1 | 1 << 8 | 1 << 16, 1, 0,            # 2: main_next(1)
        6, 1, 2,                               # 3: add
        1 | 3 << 8, 0, 0,                      # 4: input(0)
        22 | 0 << 8, 1, 4,                     # 5: pre_at(1, node 4)
        16, 0, 0,                              # 6: row
        0, 5, 0,                               # 7: const 5
        19, 6, 7,                              # 8: lt
        0, 3, 5, 3]                            # the element roots: equal expressions share a node
    assert prog.blob[:8] == b"\0MCLAIB1" and MAGIC == cb.MAGIC
    assert cb.parse(prog.blob) == (3, 2, 1, prog.nodes, prog.roots, 8)
    assert (0, 0, 0, 256 ** 4 % P, 0) in folded.nodes
    # babybear.compile_claims is the same compile, and outside the block the front end is back at Goldilocks
    same = bb.compile_claims(3, 2, 1, [E.const(7), E.main(0) + E.main_next(1), E.pre_at(1, E.input(0)), E.main(0) + E.main_next(1)], keep=fe.lt(E.row(), 5))
    assert same.blob == prog.blob
    assert fe.compile_claims(1, 0, 0, [E.main(0)]).blob[:8] == b"\0MCLAIM1"
    bare = bb.compile_claims(1, 0, 0, [E.main(0)])
    assert words(bare.blob) == [MAGIC, 1, 0, 0, 1, 1, NONE, 1 | 1 << 8, 0, 0, 0] and not bare.has_keep
    # the U32Add claims: [1, x, y, z] with the words from their bytes, modulo p
    with fe.field(fe.BABYBEAR):
        u = fe.u32_add_claims_program()
    t = np.zeros((2, 14), dtype=np.uint64)
    t[0, :12] = [0x78, 0x56, 0x34, 0x12, 0xF0, 0xDE, 0xBC, 0x9A, 0x68, 0x35, 0xF1, 0xAC]
    assert cb.run(u.blob, t, rows=1) == [[1, 0x12345678, 0x9ABCDEF0 % P, 0xACF13568 % P]] and (u.width, u.has_keep) == (4, False)
    assert bb.claims_program_info(u)["lds_lanes"] == 256


def test_model_against_hand_written_expectations(fe, bb):
    E = fe.Expr
    trace = np.array([[1, 10, 100], [2, 20, 200], [3, 30, 300], [4, 40, P - 1]], dtype=np.uint64)
    pre = np.array([[5, 50], [6, 60], [7, 70], [8, 80]], dtype=np.uint64)
    inputs = np.array([[3], [9]], dtype=np.uint64)  # two rows: rows 2 and 3 read 0; the index 9 is beyond every height
    prog = bb.compile_claims(3, 2, 1, [E.main(0) + E.main_next(1), E.pre_at(1, E.input(0)), E.main(2) * 2, E.input_next(0), E.main_at(1, E.row() + 2)])
    assert cb.run(prog.blob, trace, pre, inputs) == [
        [1 + 20, 80, 200, 9, 30],
        [2 + 30, 0, 400, 0, 40],        # pre_at(1, 9): from the height on, 0; input_next at row 1 is input row 2: 0
        [3 + 40, 50, 600, 0, 0],        # input(0) = 0 from the input height on, so pre row 0; main_at(1, 4) = 0
        [4 + 10, 50, P - 2, 3, 0]]      # the next row of the last row is row 0, for the trace and for the inputs
    assert cb.run(prog.blob, trace, pre, inputs, rows=2) == [[21, 80, 200, 9, 30], [32, 0, 400, 0, 40]]
    assert cb.run(prog.blob, trace, pre, inputs, rows=0) == []
    # rows = 3 of n = 4: row 2's next row is row 3, not row 0 - the wrap is the trace's, not the call's
    assert cb.run(prog.blob, trace, pre, inputs, rows=3)[2][0] == 3 + 40
    # keep: the rows where it is non-zero, in row order; any non-zero value keeps
    kept = bb.compile_claims(3, 2, 1, [E.main(0), E.row()], keep=E.main(0) - 2)
    assert cb.run(kept.blob, trace, pre, inputs) == [[1, 0], [3, 2], [4, 3]]
    assert cb.run(bb.compile_claims(3, 2, 1, [E.main(0)], keep=E.const(0)).blob, trace, pre, inputs) == []
    offs, data = cb.claims(kept.blob, trace, pre, inputs, before=(np.array([0, 0, 3], dtype=np.uint64), np.array([7, 8, 9], dtype=np.uint32)))
    assert offs.tolist() == [0, 0, 3, 5, 7, 9] and data.tolist() == [7, 8, 9, 1, 0, 3, 2, 4, 3] and data.dtype == np.uint32
    offs, data = cb.claims(kept.blob, trace, pre, inputs, rows=1)
    assert offs.tolist() == [0, 2] and data.tolist() == [1, 0]
    # the witness-only operators over this p: xor folds once, bits reach bit 31, products and inverses are modulo p
    big = np.array([[0x40000000, 0x3FFFFFFF, P - 1]], dtype=np.uint64)
    with fe.field(fe.BABYBEAR):
        ops = fe.compile_claims(3, 0, 0, [fe.bit_xor(E.main(0), E.main(1)), fe.bits(E.main(2), 27, 5), fe.bits(E.main(2), 0, 32), E.main(2) * E.main(2),
                                          fe.inv0(E.main(0)) * E.main(0), fe.inv0(E.main(0) - 0x40000000), -E.main(1), fe.bit_and(E.main(0), E.main(2)),
                                          fe.lt(E.main(1), E.main(0)), E.main(2) + 2])
    assert cb.run(ops.blob, big) == [[0x7FFFFFFF - P, (P - 1) >> 27, P - 1, 1, 1, 0, P - 0x3FFFFFFF, 0x40000000, 1, 1]]


def blob_refusals(fe, bb):
    """[(what, blob, text of msbb_claims_program_info, text of the model)]"""
    E = fe.Expr
    good = bb.compile_claims(3, 2, 1, [E.main(0) + E.main_next(1), E.pre_at(1, E.input(0))], keep=E.main(2))
    ws = words(good.blob)
    fill = bb.compile_fill(3, 2, 1, [(0, E.main(1))])
    scan = bb.compile_fill(3, 2, 1, [(0, fe.running_sum(E.main(1)))])
    assert fill.blob[:8] == b"\0MFILB01" and scan.blob[:8] == b"\0MFILB02"
    wrong, a_fill = "not a claim program (wrong magic)", "a fill program, not a claim program"
    out = [
        ("the Goldilocks fill magic", blob_of([GL_FILL] + ws[1:]), wrong, "magic"),
        ("the Goldilocks scan magic", blob_of([GL_SCAN] + ws[1:]), wrong, "magic"),
        ("the Goldilocks claim magic", blob_of([GL_CLAIM] + ws[1:]), wrong, "magic"),
        ("a Goldilocks claim program", fe.compile_claims(3, 2, 1, [E.main(0)]).blob, wrong, "magic"),
        ("another magic", blob_of([MAGIC + (1 << 56)] + ws[1:]), wrong, "magic"),
        ("a fill program", fill.blob, a_fill, "a fill program"),
        ("a program with scan steps", scan.blob, a_fill, "a fill program"),
        ("a fill magic on a claim body", blob_of([0x3130424C49464D00] + ws[1:]), a_fill, "a fill program"),
        ("a scan magic on a claim body", blob_of([0x3230424C49464D00] + ws[1:]), a_fill, "a fill program"),
        ("one word short", blob_of(ws[:-1]), "truncated program blob", "truncated"),
        ("one word long", blob_of(ws + [0]), "truncated program blob", "truncated"),
        ("half a word", good.blob + b"\0\0\0\0", "truncated program blob", "truncated"),
        ("a header alone, short", blob_of(ws[:6]), "truncated program blob", "truncated"),
        ("more nodes than words", hand_blob([VAR_MAIN0], [0], n_nodes=1 << 40), "truncated program blob", "truncated"),
        ("W = 0", hand_blob([VAR_MAIN0], []), "a claim has 1 to 2^16 elements, this program 0", "width"),
        ("W = 2^16 + 1", hand_blob([VAR_MAIN0], [0] * 65537), "a claim has 1 to 2^16 elements, this program 65537", "width"),
        ("a root out of range", hand_blob([VAR_MAIN0], [0, 1]), "element 1: root 1 is out of range", "element root 1"),
        ("a keep root out of range", hand_blob([VAR_MAIN0], [0], keep=1), "keep: root 1 is out of range", "keep root"),
        ("a peer source", hand_blob([(1, 4, 0, 0, 0)], [0]), "node 0: peer reads are not allowed in a claim program", "peer source"),
        ("a peer source in an indexed read", hand_blob([VAR_MAIN0, (22, 11, 0, 0, 0)], [1]), "node 1: peer reads are not allowed in a claim program", "peer source"),
        ("a public", hand_blob([(2, 0, 0, 0, 0)], [0]), "node 0: publics are not allowed in a claim program", "public"),
        ("a stage-2 variable", hand_blob([(1, 2, 0, 0, 0)], [0]), "node 0: stage-2 variables are not allowed in a claim program", "stage 2"),
        ("a stage-2 indexed read", hand_blob([VAR_MAIN0, (22, 2, 0, 0, 0)], [1]), "node 1: stage-2 columns are not allowed in a claim program", "stage 2"),
        ("the constant p", hand_blob([(0, 0, 0, P, 0)], [0]), "node 0: non-canonical constant", "constant"),
        ("a Goldilocks constant", hand_blob([(0, 0, 0, 1 << 32, 0)], [0]), "node 0: non-canonical constant", "constant"),
        ("bits with lo + length = 33", hand_blob([VAR_MAIN0, (17, 0, 0, 0, 1 | 32 << 8)], [1]), "node 1: bad bits fields", "bits"),
        ("bits with lo + length = 33, lo 28", hand_blob([VAR_MAIN0, (17, 0, 0, 0, 28 | 5 << 8)], [1]), "node 1: bad bits fields", "bits"),
        ("a column out of range", hand_blob([(1, 1, 0, 3, 0)], [0]), "node 0: variable 3 of source 1 is out of range (width 3)", "column"),
        ("a forward operand", hand_blob([VAR_MAIN0, (6, 0, 0, 0, 1)], [1]), "node 1: forward operand", "forward operand"),
    ]
    for kind in (3, 4, 5):
        out.append(("selector %d" % kind, hand_blob([(kind, 0, 0, 0, 0)], [0]), "node 0: selector nodes are not allowed in a claim program", "selector"))
    return good, out


def test_blob_refusals(pkg, fe, bb):
    good, cases = blob_refusals(fe, bb)
    info = bb.claims_program_info(good)
    assert (info["width"], info["has_keep"], info["lds_lanes"]) == (2, True, 256) and info["instructions"] == 6 and 1 <= info["slots"] <= 6
    assert cb.parse(good.blob)[5] == good.keep
    for what, blob, text, model_text in cases:
        with pytest.raises(pkg.MstarkError, match=re.escape(text)) as e:
            bb.claims_program_info(blob)
        assert str(e.value).startswith("msbb_claims_program_info: "), what
        with pytest.raises(cb.ClaimError, match=re.escape(model_text)):
            cb.parse(blob)
    # accepted at the edge: bits with lo + length = 32, the constant p - 1
    assert bb.claims_program_info(hand_blob([VAR_MAIN0, (17, 0, 0, 0, 0 | 32 << 8), (0, 0, 0, P - 1, 0)], [1, 2]))["width"] == 2
    # the other configuration refuses the new magic as a wrong magic, and its own answers stand
    for blob in (good.blob, blob_of([MAGIC] + words(fe.compile_claims(3, 2, 1, [fe.Expr.main(0)]).blob)[1:])):
        with pytest.raises(pkg.MstarkError, match=re.escape("ms_claims_program_info: not a claim program (wrong magic)")):
            pkg.claims_program_info(blob)
    E = fe.Expr
    gl = fe.compile_claims(3, 2, 1, [E.main(0) + E.main_next(1), E.pre_at(1, E.input(0))], keep=E.main(2))
    assert pkg.claims_program_info(gl) == {"instructions": 6, "slots": pkg.claims_program_info(gl)["slots"], "lds_lanes": 256, "width": 2, "has_keep": True}
    # a claim program is no fill program, in this configuration either
    with pytest.raises(pkg.MstarkError, match=re.escape("msbb_fill_program_info: not a fill program (wrong magic)")):
        bb.fill_program_info(good)
    with pytest.raises(pkg.MstarkError, match=re.escape("msbb_fill_scan_info: not a fill program (wrong magic)")):
        bb.fill_scan_info(good)


def wide_elements(fe, width):
    """W distinct elements over few columns: every element stays live to the end of the row, so the program needs at least W slots"""
    E = fe.Expr
    return [E.main(k % 3) * (k + 2) + E.main_next(3 + k % 2) for k in range(width)]


# 4-byte slots: the slot file fits 64 KB at 256 lanes up to 64 live slots, at 128 up to 128, at 64 up to 256
LANE_CASES = [(1, 256), (4, 256), (49, 256), (100, 128), (200, 64), (300, 0)]


@pytest.mark.parametrize("width,lanes", LANE_CASES)
def test_reported_lanes(fe, bb, width, lanes):
    E = fe.Expr
    for keep in (None, E.main(9)):
        info = bb.claims_program_info(bb.compile_claims(14, 0, 0, wide_elements(fe, width), keep=keep))
        assert info["width"] == width and info["has_keep"] == (keep is not None)
        assert info["lds_lanes"] == lanes, info
        assert info["slots"] >= width
        assert lanes == next((t for t in (256, 128, 64) if info["slots"] * t * 4 <= 64 * 1024), 0)


def test_symbols_in_header_library_rust_and_python(pkg, bb):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mstark_bb.h")).read(), flags=re.S)
    text = open(os.path.join(ROOT, "include", "mstark_bb.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "mstark_sys.rs")).read()
    for sym in ("msbb_witness_claims_fill", "msbb_claims_program_info", "msbb_witness_claims"):
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in bb.exported_symbols(), sym
        assert re.search(r"pub fn %s\(" % sym, rust), sym
        assert hasattr(pkg.lib(), sym), sym
    assert "Goldilocks alone so" not in text and "0x314249414C434D00" in text
    for name in ("compile_claims", "claims_program_info"):
        assert callable(getattr(bb, name)), name
    for name in ("fill_claims", "claims"):
        assert callable(getattr(bb.Witness, name)), name
