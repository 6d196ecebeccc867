"""ms_witness_fill with scan steps restated (include/mstark.h, "SCAN STEPS"): integers and numpy, column at a time - step k
computes its whole column before step k + 1 starts - and a plain sequential loop over the rows for a scan. It reads the
program's blob and nothing else of the library; the constants and the padding helper come from fill_model.

parse(blob) -> (main_width, pre_width, n_inputs, nodes, steps, scans {step index: (mul root, init)}), for both formats.
run(blob, trace, pre, inputs) -> the trace after the call."""
import numpy as np

from fill_model import (ADD, AND, BITS, CONST, FILL_MAGIC, INV0, LT, MUL, NEG, ROW, SRC_INPUT, SRC_MAIN, SRC_PRE, SUB, VAR, XOR, FillError, P, _obj)
import fill_model

SCAN_MAGIC = 0x32304C4C49464D00  # "\0MFILL02"
UNARY, BINARY = (NEG, INV0, BITS), (ADD, SUB, MUL, LT, XOR, AND)


def groups_of(n_steps, scans):
    """group index per step: every scan step is a group, every maximal run of ordinary steps between scans is one"""
    out, g = [], -1
    for k in range(n_steps):
        if k in scans or k == 0 or (k - 1) in scans:
            g += 1
        out.append(g)
    return out


def reachable(nodes, roots):
    seen, stack = set(), list(roots)
    while stack:
        i = stack.pop()
        if i in seen:
            continue
        seen.add(i)
        kind, _, _, a, b = nodes[i]
        if kind in UNARY or kind in BINARY:
            stack.append(a)
        if kind in BINARY:
            stack.append(b)
    return seen


def parse(blob):
    """refuses what the definition refuses of a program on its own; the first format is fill_model's"""
    if len(blob) % 8 or len(blob) < 48:
        raise FillError("truncated")
    w = [int(x) for x in np.frombuffer(blob, dtype="<u8")]
    if w[0] == FILL_MAGIC:
        return fill_model.parse(blob) + ({},)
    if w[0] != SCAN_MAGIC:
        raise FillError("magic")
    if len(w) < 7:
        raise FillError("truncated")
    mw, pw, ni, nn, ns, nsc = w[1:7]
    if len(w) != 7 + 3 * nn + 2 * ns + 3 * nsc:
        raise FillError("truncated")
    nodes = [(w[7 + 3 * i] & 0xFF, (w[7 + 3 * i] >> 8) & 0xFF, w[7 + 3 * i] >> 16, w[8 + 3 * i], w[9 + 3 * i]) for i in range(nn)]
    base = 7 + 3 * nn
    steps = [(w[base + 2 * k], w[base + 2 * k + 1]) for k in range(ns)]
    base += 2 * ns
    records = [(w[base + 3 * j], w[base + 3 * j + 1], w[base + 3 * j + 2]) for j in range(nsc)]
    for d, root in steps:
        if d >= mw or root >= nn:
            raise FillError("step out of range")
    scans, prev = {}, -1
    for step, mul, init in records:
        if step >= ns:
            raise FillError("scan: step index out of range")
        if step <= prev:
            raise FillError("scan: step indices not ascending")
        if mul >= nn:
            raise FillError("scan: mul root out of range")
        if init >= P:
            raise FillError("scan: init")
        scans[step], prev = (mul, init), step
    for i, (kind, src, off, a, b) in enumerate(nodes):
        if kind == CONST:
            if a >= P:
                raise FillError("constant")
        elif kind == VAR:
            width = {SRC_PRE: pw, SRC_MAIN: mw, SRC_INPUT: ni}.get(src)
            if width is None or off > 1 or a >= width:
                raise FillError("variable")
        elif kind == ROW:
            pass
        elif kind in UNARY:
            if a >= i:
                raise FillError("forward operand")
            if kind == BITS and ((b >> 8) < 1 or (b & 0xFF) + (b >> 8) > 64 or b >> 16):
                raise FillError("bits")
        elif kind in BINARY:
            if a >= i or b >= i:
                raise FillError("forward operand")
        else:
            raise FillError("node kind %d" % kind)
    group = groups_of(ns, scans)
    last_group = {}
    for k, (d, _) in enumerate(steps):
        last_group[d] = group[k]
    for k, (d, root) in enumerate(steps):
        for i in reachable(nodes, [root] + ([scans[k][0]] if k in scans else [])):
            kind, src, off, a, _ = nodes[i]
            if kind != VAR or src != SRC_MAIN:
                continue
            if k in scans and a == d:
                raise FillError("scan: the coefficients read its own dst")
            if off == 1 and last_group.get(a, -1) >= group[k]:
                raise FillError("next row of a column that the same or a later group assigns")
    return mw, pw, ni, nodes, steps, scans


def run(blob, trace, pre=None, inputs=None):
    """trace: n x main_width uint64 (what the witness held before); pre: n x pre_width; inputs: h_in x n_inputs, h_in <= n
    (rows from h_in on read 0). -> n x main_width uint64"""
    mw, pw, ni, nodes, steps, scans = parse(blob)
    trace = np.asarray(trace, dtype=np.uint64)
    n = trace.shape[0]
    assert trace.shape == (n, mw)
    cur = _obj(trace, n, mw)
    src0 = {SRC_PRE: _obj(pre, n, pw), SRC_INPUT: _obj(inputs, n, ni)}
    rows = np.arange(n).astype(object)
    inv = np.frompyfunc(lambda v: pow(v, P - 2, P), 1, 1)

    def value(root):
        """node `root` for every row, under the columns as they stand now (operands have smaller indices)"""
        memo = {}
        for j in sorted(reachable(nodes, [root])):
            kind, src, off, a, b = nodes[j]
            if kind == CONST:
                v = np.full(n, a, dtype=object)
            elif kind == VAR:
                col = (cur if src == SRC_MAIN else src0[src])[:, a]
                v = np.roll(col, -1) if off else col.copy()  # row (r + 1) mod n
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
        return memo[root]

    for k, (dst, root) in enumerate(steps):
        if k not in scans:
            cur[:, dst] = value(root)
            continue
        mul, s = scans[k]
        a, b = value(mul), value(root)
        col = np.zeros(n, dtype=object)
        for r in range(n):  # the sequential loop: A(n - 1) and B(n - 1) are not used
            col[r] = s
            s = (int(a[r]) * s + int(b[r])) % P
        cur[:, dst] = col
    return cur.astype(np.uint64)
