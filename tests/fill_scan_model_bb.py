"""msbb_witness_fill with scan steps restated (include/mstark_bb.h, "SCAN STEPS": the paragraph of include/mstark.h read over
p = 2^31 - 2^27 + 1): integers and numpy, column at a time - step k computes its whole column before step k + 1 starts - and a
plain sequential loop over the rows for a scan. Both formats of this configuration ("\\0MFILB01", "\\0MFILB02"), indexed reads
(node 22, `at`) and the group rule included. It reads the program's blob and nothing else of the library, and nothing of the
other models: its own parse, its own run.

parse(blob) -> (main_width, pre_width, n_inputs, nodes, steps, scans {step index: (mul root, init)}).
run(blob, trace, pre, inputs) -> the trace after the call."""
import numpy as np

P = (1 << 31) - (1 << 27) + 1
FILL_MAGIC, SCAN_MAGIC = 0x3130424C49464D00, 0x3230424C49464D00  # "\0MFILB01", "\0MFILB02"
VALUE_BITS = 32
CONST, VAR, PUBLIC, IS_FIRST, IS_LAST, IS_TRANS, ADD, SUB, MUL, NEG = range(10)
ROW, BITS, INV0, LT, XOR, AND, AT = range(16, 23)
SRC_PRE, SRC_MAIN, SRC_STAGE2, SRC_INPUT = 0, 1, 2, 3
UNARY, BINARY = (NEG, INV0, BITS), (ADD, SUB, MUL, LT, XOR, AND)


class FillError(Exception):
    pass


def operands(node):
    kind, _, _, a, b = node
    return [a] if kind in UNARY else [a, b] if kind in BINARY else [b] if kind == AT else []


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
        if i not in seen:
            seen.add(i)
            stack += operands(nodes[i])
    return seen


def parse(blob):
    """refuses what the definition refuses of a program on its own"""
    if len(blob) % 8 or len(blob) < 48:
        raise FillError("truncated")
    w = [int(x) for x in np.frombuffer(blob, dtype="<u8")]
    if w[0] not in (FILL_MAGIC, SCAN_MAGIC):
        raise FillError("magic")
    v2 = w[0] == SCAN_MAGIC
    hw = 7 if v2 else 6
    if len(w) < hw:
        raise FillError("truncated")
    mw, pw, ni, nn, ns = w[1:6]
    nsc = w[6] if v2 else 0
    if len(w) != hw + 3 * nn + 2 * ns + 3 * nsc:
        raise FillError("truncated")
    for head in w[hw:hw + 3 * nn:3]:
        if head >> 24:
            raise FillError("head word")
    nodes = [(w[hw + 3 * i] & 0xFF, (w[hw + 3 * i] >> 8) & 0xFF, w[hw + 3 * i] >> 16, w[hw + 1 + 3 * i], w[hw + 2 + 3 * i]) for i in range(nn)]
    base = hw + 3 * nn
    steps = [(w[base + 2 * k], w[base + 2 * k + 1]) for k in range(ns)]
    base += 2 * ns
    for d, root in steps:
        if d >= mw or root >= nn:
            raise FillError("step out of range")
    scans, prev = {}, -1
    for j in range(nsc):
        step, mul, init = w[base + 3 * j: base + 3 * j + 3]
        if step >= ns:
            raise FillError("scan: step index out of range")
        if step <= prev:
            raise FillError("scan: step indices not ascending")
        if mul >= nn:
            raise FillError("scan: mul root out of range")
        if init >= P:
            raise FillError("scan: init")
        scans[step], prev = (mul, init), step
    widths = {SRC_PRE: pw, SRC_MAIN: mw, SRC_INPUT: ni}
    assigned = {d for d, _ in steps}
    for i, (kind, src, off, a, b) in enumerate(nodes):
        if kind == CONST:
            if a >= P:
                raise FillError("constant")
        elif kind == VAR:
            if src not in widths or off > 1 or a >= widths[src]:
                raise FillError("variable")
            if not v2 and src == SRC_MAIN and off == 1 and a in assigned:
                raise FillError("next row of an assigned column")
        elif kind == AT:
            if src not in widths or off or a >= widths[src] or b >= i:
                raise FillError("indexed read")
            if not v2 and src == SRC_MAIN and a in assigned:
                raise FillError("indexed read of an assigned column")
        elif kind == ROW:
            pass
        elif kind in UNARY:
            if a >= i:
                raise FillError("forward operand")
            if kind == BITS and ((b >> 8) < 1 or (b & 0xFF) + (b >> 8) > VALUE_BITS or b >> 16):
                raise FillError("bits")
        elif kind in BINARY:
            if a >= i or b >= i:
                raise FillError("forward operand")
        else:
            raise FillError("node kind %d" % kind)
    if v2:  # the group rule, over what each group reaches
        group = groups_of(ns, scans)
        last_group = {}
        for k, (d, _) in enumerate(steps):
            last_group[d] = group[k]
        for k, (d, root) in enumerate(steps):
            for i in reachable(nodes, [root] + ([scans[k][0]] if k in scans else [])):
                kind, src, off, a, _ = nodes[i]
                if kind not in (VAR, AT) or src != SRC_MAIN:
                    continue
                if kind == VAR and k in scans and a == d:
                    raise FillError("scan: the coefficients read its own dst")
                if (kind == AT or off == 1) and last_group.get(a, -1) >= group[k]:
                    raise FillError("next row or computed row of a column that the same or a later group assigns")
    return mw, pw, ni, nodes, steps, scans


def _obj(a, cols):
    """matrix of canonical values -> object matrix of Python integers, at its own height"""
    if a is None or not cols:
        return np.zeros((0, cols), dtype=object)
    a = np.asarray(a)
    assert a.ndim == 2 and a.shape[1] == cols
    assert a.size == 0 or int(a.max()) < P
    return a.astype(np.uint64).astype(object)


def _padded(m, rows):
    out = np.zeros((rows, m.shape[1]), dtype=object)
    out[: m.shape[0]] = m
    return out


def run(blob, trace, pre=None, inputs=None):
    """trace: n x main_width canonical values (what the witness held before); pre: n x pre_width; inputs: h_in x n_inputs,
    h_in <= n (an offset-0 or offset-1 read from h_in on reads 0, and so does an indexed read). -> n x main_width uint64"""
    mw, pw, ni, nodes, steps, scans = parse(blob)
    trace = np.asarray(trace, dtype=np.uint64)
    n = trace.shape[0]
    assert trace.shape == (n, mw)
    cur = _obj(trace, mw) if mw else np.zeros((n, 0), dtype=object)
    pre_m, inp_m = _obj(pre, pw), _obj(inputs, ni)
    assert pre_m.shape[0] in (0, n) and inp_m.shape[0] <= n
    h_of = {SRC_PRE: pre_m.shape[0] if pw else n, SRC_MAIN: n, SRC_INPUT: inp_m.shape[0]}
    by_row = {SRC_PRE: _padded(pre_m, n), SRC_INPUT: _padded(inp_m, n)}
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
                col = (cur if src == SRC_MAIN else by_row[src])[:, a]
                v = np.roll(col, -1) if off else col.copy()  # row (r + 1) mod n
            elif kind == AT:
                m = cur if src == SRC_MAIN else pre_m if src == SRC_PRE else inp_m
                h = h_of[src]
                v = np.array([m[i, a] if i < h else 0 for i in memo[b]], dtype=object)  # i: a Python integer, never narrowed
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
