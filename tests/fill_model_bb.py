"""msbb_witness_fill restated (include/mstark_bb.h, the definition of include/mstark.h read over p = 2^31 - 2^27 + 1): integers
and numpy, the steps one after the other, every step for all rows at once. It reads the program's blob and nothing else of the
library - no import of the package, none of its compiled code. The counterpart of fill_model.py.

run(blob, trace, pre, inputs) -> the trace after the call. Values are Python integers in object arrays, so that products and
shifts are exact; a column is one array over the rows."""
import numpy as np

P = (1 << 31) - (1 << 27) + 1
FILL_MAGIC = 0x3130424C49464D00  # "\0MFILB01"
VALUE_BITS = 32
CONST, VAR, PUBLIC, IS_FIRST, IS_LAST, IS_TRANS, ADD, SUB, MUL, NEG = range(10)
ROW, BITS, INV0, LT, XOR, AND = range(16, 22)
SRC_PRE, SRC_MAIN, SRC_STAGE2, SRC_INPUT = 0, 1, 2, 3


class FillError(Exception):
    pass


def parse(blob):
    """-> (main_width, pre_width, n_inputs, nodes [(kind, source, offset, a, b)], steps [(dst, root)]), refusing what the
    definition refuses of a program on its own"""
    if len(blob) % 8 or len(blob) < 48:
        raise FillError("truncated")
    w = [int(x) for x in np.frombuffer(blob, dtype="<u8")]
    if w[0] != FILL_MAGIC:
        raise FillError("magic")
    mw, pw, ni, nn, ns = w[1:6]
    if len(w) != 6 + 3 * nn + 2 * ns:
        raise FillError("truncated")
    nodes = [(w[6 + 3 * i] & 0xFF, (w[6 + 3 * i] >> 8) & 0xFF, w[6 + 3 * i] >> 16, w[7 + 3 * i], w[8 + 3 * i]) for i in range(nn)]
    base = 6 + 3 * nn
    steps = [(w[base + 2 * k], w[base + 2 * k + 1]) for k in range(ns)]
    assigned = {d for d, _ in steps}
    for d, root in steps:
        if d >= mw or root >= nn:
            raise FillError("step out of range")
    for i, (kind, src, off, a, b) in enumerate(nodes):
        if kind == CONST:
            if a >= P:
                raise FillError("constant")
        elif kind == VAR:
            width = {SRC_PRE: pw, SRC_MAIN: mw, SRC_INPUT: ni}.get(src)
            if width is None or off > 1 or a >= width:
                raise FillError("variable")
            if src == SRC_MAIN and off == 1 and a in assigned:
                raise FillError("next row of an assigned column")
        elif kind == ROW:
            pass
        elif kind in (NEG, INV0, BITS):
            if a >= i:
                raise FillError("forward operand")
            if kind == BITS and ((b >> 8) < 1 or (b & 0xFF) + (b >> 8) > VALUE_BITS or b >> 16):
                raise FillError("bits")
        elif kind in (ADD, SUB, MUL, LT, XOR, AND):
            if a >= i or b >= i:
                raise FillError("forward operand")
        else:
            raise FillError("node kind %d" % kind)
    return mw, pw, ni, nodes, steps


def _obj(a, rows, cols):
    """matrix of canonical values -> object matrix of Python integers, padded with zero rows to `rows`"""
    out = np.zeros((rows, cols), dtype=object)
    if a is not None and cols:
        a = np.asarray(a)
        assert a.ndim == 2 and a.shape[1] == cols and a.shape[0] <= rows
        assert a.size == 0 or int(a.max()) < P
        out[: a.shape[0]] = a.astype(np.uint64).astype(object)
    return out


def run(blob, trace, pre=None, inputs=None):
    """trace: n x main_width canonical values (what the witness held before); pre: n x pre_width; inputs: h_in x n_inputs,
    h_in <= n (rows from h_in on read 0). -> n x main_width uint64"""
    mw, pw, ni, nodes, steps = parse(blob)
    trace = np.asarray(trace, dtype=np.uint64)
    n = trace.shape[0]
    assert trace.shape == (n, mw)
    old = _obj(trace, n, mw)
    cur = old.copy()
    src0 = {SRC_PRE: _obj(pre, n, pw), SRC_INPUT: _obj(inputs, n, ni)}
    nxt = {k: np.roll(v, -1, axis=0) for k, v in src0.items()}  # row (r + 1) mod n
    old_next = np.roll(old, -1, axis=0)
    rows = np.arange(n).astype(object)
    inv = np.frompyfunc(lambda v: pow(v, P - 2, P), 1, 1)

    def value(i, memo):
        """node i for every row, under the columns as they stand now (iterative: programs may be deep)"""
        stack = [i]
        while stack:
            j = stack[-1]
            if j in memo:
                stack.pop()
                continue
            kind, src, off, a, b = nodes[j]
            ops = [a] if kind in (NEG, INV0, BITS) else [a, b] if kind in (ADD, SUB, MUL, LT, XOR, AND) else []
            todo = [o for o in ops if o not in memo]
            if todo:
                stack += todo
                continue
            if kind == CONST:
                v = np.full(n, a, dtype=object)
            elif kind == VAR:
                if src == SRC_MAIN:
                    v = (old_next if off else cur)[:, a].copy()
                else:
                    v = (nxt if off else src0)[src][:, a].copy()
            elif kind == ROW:
                v = rows.copy()
            elif kind == ADD:
                v = (memo[a] + memo[b]) % P
            elif kind == SUB:
                v = (memo[a] - memo[b]) % P
            elif kind == MUL:
                v = (memo[a] * memo[b]) % P
            elif kind == NEG:
                v = (-memo[a]) % P
            elif kind == BITS:
                v = (memo[a] >> (b & 0xFF)) & ((1 << (b >> 8)) - 1)
            elif kind == INV0:
                v = inv(memo[a])
            elif kind == LT:
                v = np.array([1 if x < y else 0 for x, y in zip(memo[a], memo[b])], dtype=object)
            elif kind == XOR:
                v = (memo[a] ^ memo[b]) % P
            else:
                v = memo[a] & memo[b]
            memo[j] = v
            stack.pop()
        return memo[i]

    for dst, root in steps:
        cur[:, dst] = value(root, {})  # nothing is remembered across steps: a column read may have changed
    return cur.astype(np.uint64)
