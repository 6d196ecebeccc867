"""Claim programs restated (include/mstark.h, "CLAIM PROGRAMS"): integers and numpy. It reads the program's blob and nothing else
of the library, and nothing of the other models: its own parse, its own run.

parse(blob) -> (main_width, pre_width, n_inputs, nodes, roots, keep root or None)
run(blob, trace, pre, inputs, rows) -> the list of emitted claims, each a list of W Python integers, in row order
claims(blob, trace, pre, inputs, rows, before=None) -> (offsets, data) as uint64 arrays, behind the claims `before` = (offsets, data)

Blob: [magic "\\0MCLAIM1", main_width, pre_width, n_inputs, n_nodes, W, keep root (all ones: none)], n_nodes x [kind | source << 8
| offset << 16, a, b], W roots. For every row r < rows with keep(r) != 0 (every row without keep) one claim [e_0(r) .. e_{W-1}(r)].
The next row of row n - 1 is row 0; an input row from the input height on reads 0; an index from the source's height on reads 0."""
import numpy as np

P = (1 << 64) - (1 << 32) + 1
MAGIC = 0x314D49414C434D00
FILL_MAGICS = (0x31304C4C49464D00, 0x32304C4C49464D00, 0x33304C4C49464D00)
NONE = (1 << 64) - 1
MAX_WIDTH = 1 << 16
CONST, VAR, PUBLIC, IS_FIRST, IS_LAST, IS_TRANS, ADD, SUB, MUL, NEG = range(10)
ROW, BITS, INV0, LT, XOR, AND, AT = range(16, 23)
PRE, MAIN, STAGE2, INPUT, PEER0 = 0, 1, 2, 3, 4


class ClaimError(Exception):
    pass


def parse(blob):
    """refuses what the definition refuses of a program on its own; the text says which rule"""
    if len(blob) % 8 or len(blob) < 56:
        raise ClaimError("truncated")
    w = [int(x) for x in np.frombuffer(blob, dtype="<u8")]
    if w[0] in FILL_MAGICS:
        raise ClaimError("a fill program")
    if w[0] != MAGIC:
        raise ClaimError("magic")
    mw, pw, ni, nn, W, keep = w[1:7]
    if not 1 <= W <= MAX_WIDTH:
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
    width_of = {PRE: pw, MAIN: mw, INPUT: ni}
    for i, (kind, src, off, a, b) in enumerate(nodes):
        if kind in (VAR, AT):
            if src == STAGE2:
                raise ClaimError("stage 2")
            if src >= PEER0:
                raise ClaimError("peer source" if src < PEER0 + 8 else "unknown source")
            if a >= width_of[src]:
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
        elif kind in (NEG, INV0, BITS):
            if a >= i:
                raise ClaimError("forward operand")
            if kind == BITS and (b >> 16 or (b >> 8) < 1 or (b & 0xFF) + (b >> 8) > 64):
                raise ClaimError("bits")
        elif kind in (ADD, SUB, MUL, LT, XOR, AND):
            if a >= i or b >= i:
                raise ClaimError("forward operand")
        else:
            raise ClaimError("node kind %d" % kind)
    return mw, pw, ni, nodes, roots, None if keep == NONE else keep


def _ints(m, cols):
    """a matrix of canonical values as rows of Python integers"""
    if m is None or not cols:
        return []
    m = np.asarray(m, dtype=np.uint64)
    assert m.ndim == 2 and m.shape[1] == cols
    out = [[int(x) for x in row] for row in m]
    assert all(x < P for row in out for x in row)
    return out


def run(blob, trace, pre=None, inputs=None, rows=None):
    """trace: n x main_width; pre: n x pre_width or None; inputs: h_in x n_inputs with h_in <= n, or None; rows <= n (default n).
    One row at a time, every node of the row in index order (operands come first)."""
    mw, pw, ni, nodes, roots, keep = parse(blob)
    main, pre_m, inp = _ints(trace, mw), _ints(pre, pw), _ints(inputs, ni)
    n = np.asarray(trace).shape[0]
    rows = n if rows is None else rows
    assert n >= 1 and rows <= n and len(inp) <= n and (not pw or len(pre_m) == n)
    matrix = {PRE: pre_m, MAIN: main, INPUT: inp}
    height = {PRE: n, MAIN: n, INPUT: len(inp)}
    out = []
    for r in range(rows):
        v = []
        for (kind, src, off, a, b) in nodes:
            if kind == CONST:
                x = a
            elif kind == VAR:
                at = (r + 1) % n if off else r  # n, not rows: the trace's own next row
                x = matrix[src][at][a] if at < height[src] else 0
            elif kind == AT:
                i = v[b]  # the canonical integer, neither reduced nor truncated
                x = matrix[src][i][a] if i < height[src] else 0
            elif kind == ROW:
                x = r
            elif kind == ADD:
                x = (v[a] + v[b]) % P
            elif kind == SUB:
                x = (v[a] - v[b]) % P
            elif kind == MUL:
                x = (v[a] * v[b]) % P
            elif kind == NEG:
                x = (-v[a]) % P
            elif kind == BITS:
                x = (v[a] >> (b & 0xFF)) & ((1 << (b >> 8)) - 1)
            elif kind == INV0:
                x = pow(v[a], P - 2, P)
            elif kind == LT:
                x = 1 if v[a] < v[b] else 0
            elif kind == XOR:
                x = (v[a] ^ v[b]) % P
            else:
                x = v[a] & v[b]
            v.append(x)
        if keep is None or v[keep] != 0:
            out.append([v[root] for root in roots])
    return out


def claims(blob, trace, pre=None, inputs=None, rows=None, before=None):
    """(offsets, data) of the witness's claims after the call: the emitted claims behind `before` (append) or alone (replace)"""
    emitted = run(blob, trace, pre, inputs, rows)
    offs = [0] if before is None else [int(x) for x in before[0]]
    data = [] if before is None else [int(x) for x in before[1]]
    assert offs[0] == 0 and offs[-1] == len(data)
    for c in emitted:
        data += c
        offs.append(len(data))
    return np.array(offs, dtype=np.uint64), np.array(data, dtype=np.uint64)
