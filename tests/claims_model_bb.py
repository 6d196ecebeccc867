"""msbb_witness_claims_fill restated (include/mstark_bb.h; "CLAIM PROGRAMS" of include/mstark.h read over p = 2^31 - 2^27 + 1):
integers and numpy. It reads the program's blob and nothing else of the library - no import of the package, none of its compiled
code, none of the other models: its own parse, its own run. The counterpart of fill_model_bb.py for claims.

parse(blob) -> (main_width, pre_width, n_inputs, nodes, roots, keep root or None)
run(blob, trace, pre, inputs, rows) -> the list of emitted claims, each a list of W Python integers in [0, p), in row order
claims(blob, trace, pre, inputs, rows, before=None) -> (offsets uint64, data uint32) behind the claims `before` = (offsets, data)

Blob: [magic "\\0MCLAIB1", main_width, pre_width, n_inputs, n_nodes, W, keep root (all ones: none)], n_nodes x [kind | source << 8
| offset << 16, a, b], W roots. For every row r < rows with keep(r) != 0 (every row without keep) one claim [e_0(r) .. e_{W-1}(r)].
The next row of row n - 1 is row 0; an input row from the input height on reads 0; an index from the source's height on reads 0.
Values are the canonical integers: bits needs lo + length <= 32, xor is folded once, row is r."""
import numpy as np

P = (1 << 31) - (1 << 27) + 1
MAGIC = 0x314249414C434D00                               # "\0MCLAIB1"
FILL_MAGICS = (0x3130424C49464D00, 0x3230424C49464D00)   # "\0MFILB01", "\0MFILB02": named as fill programs
VALUE_BITS = 32
NONE = (1 << 64) - 1
MAX_WIDTH = 1 << 16
CONST, VAR, PUBLIC, IS_FIRST, IS_LAST, IS_TRANS, ADD, SUB, MUL, NEG = range(10)
ROW, BITS, INV0, LT, XOR, AND, AT = range(16, 23)
SRC_PRE, SRC_MAIN, SRC_STAGE2, SRC_INPUT, SRC_PEER0, N_PEERS = 0, 1, 2, 3, 4, 8
UNARY, BINARY = (NEG, INV0, BITS), (ADD, SUB, MUL, LT, XOR, AND)


class ClaimError(Exception):
    pass


def parse(blob):
    """refuses what the definition refuses of a program on its own; the text says which rule"""
    if len(blob) % 8 or len(blob) < 7 * 8:
        raise ClaimError("truncated")
    w = np.frombuffer(blob, dtype="<u8").tolist()
    if w[0] in FILL_MAGICS:
        raise ClaimError("a fill program")
    if w[0] != MAGIC:
        raise ClaimError("magic")
    mw, pw, ni, nn, W, keep = w[1:7]
    if W < 1 or W > MAX_WIDTH:
        raise ClaimError("width")
    if len(w) != 7 + 3 * nn + W:
        raise ClaimError("truncated")
    nodes = []
    for i in range(nn):
        head, a, b = w[7 + 3 * i: 10 + 3 * i]
        if head >> 24:
            raise ClaimError("head word")
        nodes.append((head & 0xFF, (head >> 8) & 0xFF, head >> 16, a, b))
    roots = w[7 + 3 * nn:]
    for e, root in enumerate(roots):
        if root >= nn:
            raise ClaimError("element root %d" % e)
    if keep != NONE and keep >= nn:
        raise ClaimError("keep root")
    widths = {SRC_PRE: pw, SRC_MAIN: mw, SRC_INPUT: ni}
    for i, (kind, src, off, a, b) in enumerate(nodes):
        if kind == VAR or kind == AT:
            if src == SRC_STAGE2:
                raise ClaimError("stage 2")
            if src not in widths:
                raise ClaimError("peer source" if src < SRC_PEER0 + N_PEERS else "unknown source")
            if a >= widths[src]:
                raise ClaimError("column")
            if kind == VAR and off > 1:
                raise ClaimError("row offset")
            if kind == AT and off:
                raise ClaimError("offset field of an indexed read")
            if kind == AT and b >= i:
                raise ClaimError("forward row operand")
        elif kind == CONST:
            if a >= P:
                raise ClaimError("constant")
        elif kind == PUBLIC:
            raise ClaimError("public")
        elif kind in (IS_FIRST, IS_LAST, IS_TRANS):
            raise ClaimError("selector")
        elif kind == ROW:
            pass
        elif kind in UNARY:
            if a >= i:
                raise ClaimError("forward operand")
            if kind == BITS and (b >> 16 or (b >> 8) < 1 or (b & 0xFF) + (b >> 8) > VALUE_BITS):
                raise ClaimError("bits")
        elif kind in BINARY:
            if a >= i or b >= i:
                raise ClaimError("forward operand")
        else:
            raise ClaimError("node kind %d" % kind)
    return mw, pw, ni, nodes, roots, None if keep == NONE else keep


def _rows_of(m, cols):
    """a matrix of canonical values as rows of Python integers"""
    if m is None or not cols:
        return []
    m = np.asarray(m, dtype=np.uint64)
    assert m.ndim == 2 and m.shape[1] == cols
    assert m.size == 0 or int(m.max()) < P
    return m.tolist()


def run(blob, trace, pre=None, inputs=None, rows=None):
    """trace: n x main_width; pre: n x pre_width or None; inputs: h_in x n_inputs with h_in <= n, or None; rows <= n (default n).
    One row at a time, every node of the row in index order (operands come first)."""
    mw, pw, ni, nodes, roots, keep = parse(blob)
    n = np.asarray(trace).shape[0]
    table = {SRC_MAIN: _rows_of(trace, mw), SRC_PRE: _rows_of(pre, pw), SRC_INPUT: _rows_of(inputs, ni)}
    height = {SRC_MAIN: n, SRC_PRE: n, SRC_INPUT: len(table[SRC_INPUT])}
    rows = n if rows is None else rows
    assert n >= 1 and rows <= n and height[SRC_INPUT] <= n and (not pw or len(table[SRC_PRE]) == n)
    emitted = []
    for r in range(rows):
        v = [0] * len(nodes)
        for i, (kind, src, off, a, b) in enumerate(nodes):
            if kind == CONST:
                x = a
            elif kind == VAR:
                at = r if not off else (r + 1 if r + 1 < n else 0)  # the trace's own next row, whatever `rows` is
                x = table[src][at][a] if at < height[src] else 0
            elif kind == AT:
                at = v[b]  # the canonical integer in [0, p), compared with the height before anything is addressed
                x = table[src][at][a] if at < height[src] else 0
            elif kind == ROW:
                x = r
            elif kind == ADD:
                x = (v[a] + v[b]) % P
            elif kind == SUB:
                x = (v[a] - v[b]) % P
            elif kind == MUL:
                x = v[a] * v[b] % P
            elif kind == NEG:
                x = (P - v[a]) % P
            elif kind == BITS:
                x = (v[a] >> (b & 0xFF)) % (1 << (b >> 8))
            elif kind == INV0:
                x = pow(v[a], P - 2, P)
            elif kind == LT:
                x = int(v[a] < v[b])
            elif kind == XOR:
                x = v[a] ^ v[b]  # < 2^31 < 2 p: one fold
                x = x - P if x >= P else x
            else:
                x = v[a] & v[b]
            assert 0 <= x < P
            v[i] = x
        if keep is None or v[keep]:
            emitted.append([v[root] for root in roots])
    return emitted


def claims(blob, trace, pre=None, inputs=None, rows=None, before=None):
    """(offsets, data) of the witness's claims after the call: the emitted claims behind `before` (append) or alone (replace)"""
    offs = [0] if before is None else [int(x) for x in before[0]]
    data = [] if before is None else [int(x) for x in before[1]]
    assert offs[0] == 0 and offs[-1] == len(data)
    for c in run(blob, trace, pre, inputs, rows):
        data += c
        offs.append(len(data))
    return np.array(offs, dtype=np.uint64), np.array(data, dtype=np.uint32)
