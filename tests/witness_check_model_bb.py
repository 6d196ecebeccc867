"""Model of msbb_witness_check (include/mstark_bb.h) over the compiled node vector: helper for the tests, not a test.
The counterpart of witness_check_model.py for p = 2^31 - 2^27 + 1.

For every active circuit and every row r the user constraint roots (`zeros`, in that order) are evaluated on numpy uint64 arrays
(every operand is below 2^31, so a product fits 64 bits and plain arithmetic mod p is exact), vectorised over the rows, on the
values the BabyBear quotient kernel would see on the trace domain at x = w^r, w = 0x1a427a41 squared 27 - log n times: main /
preprocessed columns at row r and (r + 1) mod n; the selector polynomials with their limits (is_first = n at row 0, is_last =
n w at row n - 1, is_transition = w^r - w^-1); the stage-2 columns and the 16 public coordinates of the ORACLE's stage-2 trace
(oracle_bb.stage2_trace on oracle lookup values, oracle_bb.claims_accumulator) under the given (beta, gamma).
The report has the fields of the device's: see `CircuitModel.fields`."""
import numpy as np

P = (1 << 31) - (1 << 27) + 1
NONE = (1 << 64) - 1
D = 4
K_CONST, K_VAR, K_PUBLIC, K_IS_FIRST, K_IS_LAST, K_IS_TRANS, K_ADD, K_SUB, K_MUL, K_NEG = range(10)
SRC_PRE, SRC_MAIN, SRC_STAGE2 = 0, 1, 2
_P = np.uint64(P)


def generator(log_n):
    """BabyBear::two_adic_generator(log_n): 0x1a427a41 has order 2^27"""
    g = 0x1A427A41
    for _ in range(27 - log_n):
        g = g * g % P
    return g


def selector_values(n):
    """(is_first, is_last, is_transition) on the trace domain: uint64 arrays of n values"""
    log_n = n.bit_length() - 1
    w = generator(log_n)
    w_inv = pow(w, P - 2, P)
    first, last, trans = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    first[0] = n % P
    last[n - 1] = n * w % P
    x = 1
    for r in range(n):
        trans[r] = (x - w_inv) % P
        x = x * w % P
    return first, last, trans


def eval_roots(cc, trace, stage2, publics):
    """values of cc.zeros on every row: list of uint64 arrays (n). trace: n x main_width; stage2: n x stage2_width (natural row
    order) or None; publics: 16 integers"""
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
    main = np.asarray(trace, dtype=np.uint64)
    pre = np.asarray(cc.preprocessed, dtype=np.uint64) if cc.preprocessed is not None else None
    s2 = np.asarray(stage2, dtype=np.uint64) if stage2 is not None else None
    assert int(main.max(initial=0)) < P
    first, last, trans = selector_values(n)
    vals = {}
    for i in sorted(need):
        k, src, off, a, b = cc.nodes[i]
        if k == K_CONST:
            v = np.full(n, int(a) % P, dtype=np.uint64)
        elif k == K_VAR:
            m = {SRC_PRE: pre, SRC_MAIN: main, SRC_STAGE2: s2}[src]
            col = m[:, a]
            v = np.roll(col, -1) if off else col
        elif k == K_PUBLIC:
            v = np.full(n, int(publics[a]), dtype=np.uint64)
        elif k == K_IS_FIRST:
            v = first
        elif k == K_IS_LAST:
            v = last
        elif k == K_IS_TRANS:
            v = trans
        elif k == K_ADD:
            v = (vals[a] + vals[b]) % _P
        elif k == K_SUB:
            v = (vals[a] + _P - vals[b]) % _P
        elif k == K_MUL:
            v = (vals[a] * vals[b]) % _P
        else:
            v = (_P - vals[a]) % _P
        vals[i] = v
    return [vals[z] for z in cc.zeros]


class CircuitModel:
    def __init__(self, height, roots):
        self.height, self.roots = height, roots
        self.failing_rows, self.first_failure, self.accumulator = 0, None, (0,) * D
        self.root_counts, self.root_first = [0] * roots, [NONE] * roots

    def fields(self):
        """the same tuple as multi_stark_amd.CircuitCheck.fields()"""
        return (self.height, self.failing_rows, self.first_failure, self.accumulator, self.roots, self.root_counts, self.root_first)


class Model:
    def __init__(self, verdict, circuits):
        self.verdict, self.circuits, self.ok = verdict, circuits, verdict == 0
        self.final_accumulator = next((c.accumulator for c in reversed(circuits) if c.height), (0,) * D)


def check(oracle_bb, osys, compiled, traces, claims_packed, beta, gamma):
    """the report of msbb_witness_check for the system `compiled` (CompiledCircuits; osys = oracle_bb.System of its blob)"""
    beta, gamma = [int(x) for x in beta], [int(x) for x in gamma]
    assert len(beta) == D and len(gamma) == D
    acc = tuple(oracle_bb.claims_accumulator(claims_packed, beta, gamma)) if len(claims_packed[0]) > 1 else (0,) * D
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
            stage2, acc = oracle_bb.stage2_trace(mult, offs, args, beta, gamma, acc_in)
        else:
            stage2 = np.zeros((n, D), dtype=np.uint64)
        acc = tuple(int(x) for x in acc)
        cm.accumulator = acc
        if not cc.zeros:
            continue
        publics = beta + gamma + [int(x) for x in acc_in] + list(acc)
        roots = eval_roots(cc, tr, stage2, publics)
        nz = np.array([col != 0 for col in roots], dtype=bool).reshape(len(roots), n)  # roots x rows
        cm.root_counts = [int(x) for x in nz.sum(axis=1)]
        cm.root_first = [int(np.argmax(row)) if row.any() else NONE for row in nz]
        bad_rows = nz.any(axis=0)
        cm.failing_rows = int(bad_rows.sum())
        if cm.failing_rows:
            r = int(np.argmax(bad_rows))
            k = int(np.argmax(nz[:, r]))
            cm.first_failure = (r, k, int(roots[k][r]))
            verdict |= 1
    if tuple(int(x) for x in acc) != (0,) * D:
        verdict |= 2
    return Model(verdict, out)
