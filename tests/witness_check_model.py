"""Model of ms_witness_check (include/mstark.h) over the compiled node vector: helper for the tests, not a test.

For every active circuit and every row r the user constraint roots (`zeros`, in that order) are evaluated on numpy object arrays
(Python integers mod p), vectorised over the rows, on the values the quotient kernels see on the trace domain at x = w^r:
main / preprocessed columns at row r and (r + 1) mod n; the selector polynomials with their limits (is_first = n at row 0,
is_last = n w at row n - 1, is_transition = w^r - w^-1); the stage-2 columns and publics of the ORACLE's stage-2 trace
(oracle.stage2_trace on oracle lookup values, oracle.claims_accumulator) under the given (beta, gamma).
The report has the fields of the device's: see `CircuitModel.fields`."""
import numpy as np

P = (1 << 64) - (1 << 32) + 1
NONE = (1 << 64) - 1
K_CONST, K_VAR, K_PUBLIC, K_IS_FIRST, K_IS_LAST, K_IS_TRANS, K_ADD, K_SUB, K_MUL, K_NEG = range(10)
SRC_PRE, SRC_MAIN, SRC_STAGE2 = 0, 1, 2


def generator(log_n):
    """generator of the subgroup of order 2^log_n: 7^((p - 1) / n)"""
    return pow(7, (P - 1) >> log_n, P)


def selector_values(n):
    """(is_first, is_last, is_transition) on the trace domain: object arrays of n Python integers"""
    log_n = n.bit_length() - 1
    w = generator(log_n)
    w_inv = pow(w, P - 2, P)
    first, last, trans = np.zeros(n, dtype=object), np.zeros(n, dtype=object), np.zeros(n, dtype=object)
    first[0] = n % P
    last[n - 1] = n * w % P
    x = 1
    for r in range(n):
        trans[r] = (x - w_inv) % P
        x = x * w % P
    return first, last, trans


def _obj(a):
    return np.array([int(v) for v in np.asarray(a).reshape(-1)], dtype=object).reshape(np.asarray(a).shape)


def eval_roots(cc, trace, stage2, publics):
    """values of cc.zeros on every row: list of object arrays (n). trace: n x main_width; stage2: n x stage2_width (natural row
    order) or None; publics: 8 integers"""
    n = trace.shape[0]
    need = set()
    stack = list(cc.zeros)
    while stack:
        i = stack.pop()
        if i in need:
            continue
        need.add(i)
        k, _, _, a, b = cc.nodes[i]
        if k in (K_ADD, K_SUB, K_MUL):
            stack += [a, b]
        elif k == K_NEG:
            stack.append(a)
    main = _obj(trace)
    pre = _obj(cc.preprocessed) if cc.preprocessed is not None else None
    s2 = _obj(stage2) if stage2 is not None else None
    first, last, trans = selector_values(n)
    vals = {}
    for i in sorted(need):
        k, src, off, a, b = cc.nodes[i]
        if k == K_CONST:
            v = np.full(n, int(a) % P, dtype=object)
        elif k == K_VAR:
            m = {SRC_PRE: pre, SRC_MAIN: main, SRC_STAGE2: s2}[src]
            col = m[:, a]
            v = np.roll(col, -1) if off else col
        elif k == K_PUBLIC:
            v = np.full(n, int(publics[a]), dtype=object)
        elif k == K_IS_FIRST:
            v = first
        elif k == K_IS_LAST:
            v = last
        elif k == K_IS_TRANS:
            v = trans
        elif k == K_ADD:
            v = (vals[a] + vals[b]) % P
        elif k == K_SUB:
            v = (vals[a] - vals[b]) % P
        elif k == K_MUL:
            v = (vals[a] * vals[b]) % P
        else:
            v = (-vals[a]) % P
        vals[i] = v
    return [vals[z] for z in cc.zeros]


class CircuitModel:
    def __init__(self, height, roots):
        self.height, self.roots = height, roots
        self.failing_rows, self.first_failure, self.accumulator = 0, None, (0, 0)
        self.root_counts, self.root_first = [0] * roots, [NONE] * roots

    def fields(self):
        """the same tuple as multi_stark_amd.CircuitCheck.fields()"""
        return (self.height, self.failing_rows, self.first_failure, self.accumulator, self.roots, self.root_counts, self.root_first)


class Model:
    def __init__(self, verdict, circuits):
        self.verdict, self.circuits, self.ok = verdict, circuits, verdict == 0


def check(oracle, osys, compiled, traces, claims_packed, beta, gamma):
    """the report of ms_witness_check for the system `compiled` (CompiledCircuits; osys = oracle.System of its blob)"""
    beta, gamma = [int(x) for x in beta], [int(x) for x in gamma]
    acc = tuple(oracle.claims_accumulator(claims_packed, beta, gamma)) if len(claims_packed[0]) > 1 else (0, 0)
    out, verdict = [], 0
    for ci, cc in enumerate(compiled):
        tr = np.asarray(traces[ci], dtype=np.uint64) if traces[ci] is not None else np.zeros((0, 1), dtype=np.uint64)
        n = tr.shape[0]
        cm = CircuitModel(n, len(cc.zeros))
        out.append(cm)
        if n == 0:
            continue
        L = len(cc.lookups)
        acc_in = acc
        if L:
            mult, args = osys.compute_lookup_values(ci, tr)
            offs = np.cumsum([0] + [len(a) for _, a in cc.lookups]).astype(np.uint64)
            stage2, acc = oracle.stage2_trace(mult, offs, args, beta, gamma, acc_in)
        else:
            stage2 = np.zeros((n, 2), dtype=np.uint64)
        cm.accumulator = (int(acc[0]), int(acc[1]))
        if not cc.zeros:
            continue
        publics = beta + gamma + [int(x) for x in acc_in] + [int(x) for x in acc]
        roots = eval_roots(cc, tr, stage2, publics)
        nz = np.array([(col != 0).astype(bool) for col in roots], dtype=bool).reshape(len(roots), n)  # roots x rows
        cm.root_counts = [int(x) for x in nz.sum(axis=1)]
        cm.root_first = [int(np.argmax(row)) if row.any() else NONE for row in nz]
        bad_rows = nz.any(axis=0)
        cm.failing_rows = int(bad_rows.sum())
        if cm.failing_rows:
            r = int(np.argmax(bad_rows))
            k = int(np.argmax(nz[:, r]))
            cm.first_failure = (r, k, int(roots[k][r]))
            verdict |= 1
    if acc != (0, 0) and tuple(int(x) for x in acc) != (0, 0):
        verdict |= 2
    return Model(verdict, out)
