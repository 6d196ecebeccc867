"""Circuit front-end: expression trees -> compiled node program -> system blob.

Host-side mirror of the reference's authoring path so that the node programs fed to the prover have the
same shape the reference would compile:
  * `Expr` operators with constant folding     -- /root/reference/src/expr.rs:179-227
  * hash-consing interner + `compile`            -- /root/reference/src/graph.rs:120-188, 213-507
  * recording AIR builder (`assert_zero`, `when`, `assert_bool`, ...) -- /root/reference/src/p3_adapter.rs:245-354
    (p3-air / p3-field default methods restated from Plonky3 0.5.1: assert_eq(x,y) = assert_zero(x-y),
     assert_bool(x) = assert_zero(x.bool_check()) with bool_check(x) = (1-x)*x, when(c).assert_zero(x) = c*x)
  * the bench / test circuits and their witnesses -- benches/multi_stark.rs:73-238, examples/simple_proof.rs,
    src/lookup.rs:868-1007 (even/odd), src/test_circuits/u32_add.rs:150-221

This is setup-time code (untimed in the reference's bench): pure Python + numpy, no GPU.
"""
import struct

import numpy as np

import contextlib

P = (1 << 64) - (1 << 32) + 1
EXT_D, EXT_W = 2, 7  # Challenge = BinomialExtensionField<Goldilocks, 2>, X^2 = 7

# node kinds (the system-blob encoding, see include/mstark.h)
N_CONST, N_VAR, N_PUBLIC, N_IS_FIRST, N_IS_LAST, N_IS_TRANS, N_ADD, N_SUB, N_MUL, N_NEG = range(10)
SRC_PRE, SRC_MAIN, SRC_STAGE2 = 0, 1, 2
BLOB_MAGIC = 0x31305359534D0000
# witness-only node kinds and the input source of fill programs (compile_fill, ms_witness_fill): never part of a constraint
N_ROW, N_BITS, N_INV0, N_LT, N_XOR, N_AND = range(16, 22)
N_AT = 22  # an indexed read: column a of `source` at the row that node b computes (Expr.main_at / pre_at / input_at)
SRC_INPUT = 3
FILL_MAGIC = 0x31304C4C49464D00  # "\0MFILL01"; over BabyBear "\0MFILB01": a fill program belongs to the field its constants were folded in
FILL_BITS = 64  # bits(x, lo, length) needs lo + length <= the width of a value: 64, over BabyBear 32
FILL_SCAN_MAGIC = 0x32304C4C49464D00  # "\0MFILL02": a program with scan steps; over BabyBear "\0MFILB02"
FILL_PEER_MAGIC = 0x33304C4C49464D00  # "\0MFILL03": a program with peer reads (Goldilocks alone)
CLAIM_MAGIC = 0x314D49414C434D00  # "\0MCLAIM1": a claim program (compile_claims, ms_witness_claims_fill); over BabyBear "\0MCLAIB1"
CLAIM_MAX_WIDTH = 1 << 16
SRC_PEER, FL_MAX_PEERS = 4, 8  # source byte 4 + k: peer record k of the program (include/mstark.h, "PEER READS")

# The two StarkGenericConfig instantiations of the reference: GoldilocksBlake3Config (src/types.rs:24-29,199-223) and
# the BabyBear / degree-4 extension / Poseidon2 test configuration (src/test_circuits/baby_bear_config.rs:28-38).
GOLDILOCKS = dict(name="goldilocks", P=P, EXT_D=2, EXT_W=7, BLOB_MAGIC=0x31305359534D0000, FILL_MAGIC=0x31304C4C49464D00, FILL_BITS=64,
                  FILL_SCAN_MAGIC=0x32304C4C49464D00, CLAIM_MAGIC=0x314D49414C434D00)
BABYBEAR = dict(name="babybear", P=(1 << 31) - (1 << 27) + 1, EXT_D=4, EXT_W=11, BLOB_MAGIC=0x31304259534D0000, FILL_MAGIC=0x3130424C49464D00,
                FILL_BITS=32, FILL_SCAN_MAGIC=0x3230424C49464D00, CLAIM_MAGIC=0x314249414C434D00)


@contextlib.contextmanager
def field(cfg):
    """Author circuits / witnesses / blobs over another configuration's field: `with frontend.field(frontend.BABYBEAR):`.
    (The reference picks the field through the SC type parameter; this front-end keeps it in module state.)"""
    g = globals()
    saved = {k: g[k] for k in ("P", "EXT_D", "EXT_W", "BLOB_MAGIC", "FILL_MAGIC", "FILL_BITS", "FILL_SCAN_MAGIC", "CLAIM_MAGIC")}
    g.update({k: cfg[k] for k in saved})
    try:
        yield cfg
    finally:
        g.update(saved)


class Expr:
    """Frontend base-field expression (src/expr.rs:38-51)."""

    __slots__ = ("kind", "a", "b", "source", "offset")

    def __init__(self, kind, a=None, b=None, source=0, offset=0):
        self.kind, self.a, self.b, self.source, self.offset = kind, a, b, source, offset

    # constructors
    @staticmethod
    def const(v):
        return Expr(N_CONST, int(v) % P)

    @staticmethod
    def var(source, offset, index):
        return Expr(N_VAR, int(index), None, source, offset)

    @staticmethod
    def main(i):
        return Expr.var(SRC_MAIN, 0, i)

    @staticmethod
    def main_next(i):
        return Expr.var(SRC_MAIN, 1, i)

    @staticmethod
    def preprocessed(i):
        return Expr.var(SRC_PRE, 0, i)

    @staticmethod
    def public(i):
        return Expr(N_PUBLIC, int(i))

    # witness-only leaves (fill programs)
    @staticmethod
    def input(i):
        return Expr.var(SRC_INPUT, 0, i)

    @staticmethod
    def input_next(i):
        return Expr.var(SRC_INPUT, 1, i)

    @staticmethod
    def row():
        return Expr(N_ROW)

    # indexed reads: column c at the row that `row` (a fill expression or an integer) computes; 0 from the source's height on
    @staticmethod
    def at(source, c, row):
        return Expr(N_AT, int(c), Expr.lift(row), source, 0)

    @staticmethod
    def main_at(c, row):
        return Expr.at(SRC_MAIN, c, row)

    @staticmethod
    def pre_at(c, row):
        return Expr.at(SRC_PRE, c, row)

    @staticmethod
    def input_at(c, row):
        return Expr.at(SRC_INPUT, c, row)

    # peer reads: the main / preprocessed trace of ANOTHER circuit of the witness; 0 from that trace's height on. Until
    # compile_fill numbers the peers a program reaches, the source of such a node is the triple ("peer", circuit, trace).
    @staticmethod
    def peer(circuit, col):
        return Expr.var(("peer", int(circuit), SRC_MAIN), 0, col)

    @staticmethod
    def peer_next(circuit, col):
        return Expr.var(("peer", int(circuit), SRC_MAIN), 1, col)

    @staticmethod
    def peer_at(circuit, col, row):
        return Expr.at(("peer", int(circuit), SRC_MAIN), col, row)

    @staticmethod
    def peer_pre(circuit, col):
        return Expr.var(("peer", int(circuit), SRC_PRE), 0, col)

    @staticmethod
    def peer_pre_next(circuit, col):
        return Expr.var(("peer", int(circuit), SRC_PRE), 1, col)

    @staticmethod
    def peer_pre_at(circuit, col, row):
        return Expr.at(("peer", int(circuit), SRC_PRE), col, row)

    def is_const(self, v=None):
        return self.kind == N_CONST and (v is None or self.a == v % P)

    @staticmethod
    def lift(x):
        return x if isinstance(x, Expr) else Expr.const(x)

    # operators, folding constants exactly like src/expr.rs:179-227
    def __add__(self, rhs):
        rhs = Expr.lift(rhs)
        if self.kind == N_CONST and rhs.kind == N_CONST:
            return Expr.const(self.a + rhs.a)
        if self.is_const(0):
            return rhs
        if rhs.is_const(0):
            return self
        return Expr(N_ADD, self, rhs)

    def __radd__(self, lhs):
        return Expr.lift(lhs) + self

    def __sub__(self, rhs):
        rhs = Expr.lift(rhs)
        if self.kind == N_CONST and rhs.kind == N_CONST:
            return Expr.const(self.a - rhs.a)
        if rhs.is_const(0):
            return self
        if self.is_const(0):
            return -rhs
        return Expr(N_SUB, self, rhs)

    def __rsub__(self, lhs):
        return Expr.lift(lhs) - self

    def __mul__(self, rhs):
        rhs = Expr.lift(rhs)
        if self.kind == N_CONST and rhs.kind == N_CONST:
            return Expr.const(self.a * rhs.a)
        if self.is_const(0) or rhs.is_const(0):
            return Expr.const(0)
        if self.is_const(1):
            return rhs
        if rhs.is_const(1):
            return self
        return Expr(N_MUL, self, rhs)

    def __rmul__(self, lhs):
        return Expr.lift(lhs) * self

    def __neg__(self):
        if self.kind == N_CONST:
            return Expr.const(-self.a)
        if self.kind == N_NEG:
            return self.a
        return Expr(N_NEG, self)


IS_FIRST_ROW = Expr(N_IS_FIRST)
IS_LAST_ROW = Expr(N_IS_LAST)
IS_TRANSITION = Expr(N_IS_TRANS)


class ExtExpr:
    """Frontend extension expression (src/expr.rs:55-66): kinds 'coords' | 'base' | 'add' | 'sub' | 'mul' | 'neg'."""

    def __init__(self, kind, a=None, b=None):
        self.kind, self.a, self.b = kind, a, b

    @staticmethod
    def coords(cs):
        return ExtExpr("coords", [Expr.lift(c) for c in cs])

    @staticmethod
    def base(e):
        return ExtExpr("base", Expr.lift(e))

    @staticmethod
    def lift(x):
        return x if isinstance(x, ExtExpr) else ExtExpr.base(x)

    def __add__(self, r):
        return ExtExpr("add", self, ExtExpr.lift(r))

    def __sub__(self, r):
        return ExtExpr("sub", self, ExtExpr.lift(r))

    def __mul__(self, r):
        return ExtExpr("mul", self, ExtExpr.lift(r))

    def __neg__(self):
        return ExtExpr("neg", self)

    def is_purely_base(self):
        if self.kind == "coords":
            return False
        if self.kind == "base":
            return True
        if self.kind == "neg":
            return self.a.is_purely_base()
        return self.a.is_purely_base() and self.b.is_purely_base()


class Lookup:
    """src/lookup.rs:38-74."""

    def __init__(self, multiplicity, args):
        self.multiplicity = Expr.lift(multiplicity)
        self.args = [Expr.lift(a) for a in args]

    @staticmethod
    def push(m, args):
        return Lookup(m, args)

    @staticmethod
    def pull(m, args):
        return Lookup(-Expr.lift(m), args)


class CompileError(Exception):
    pass


class _Interner:
    """Bottom-up hash-consing interner, src/graph.rs:213-324."""

    def __init__(self):
        self.nodes = []  # tuples (kind, source, offset, a, b)
        self.map = {}

    def intern(self, node):
        i = self.map.get(node)
        if i is None:
            i = len(self.nodes)
            self.nodes.append(node)
            self.map[node] = i
        return i

    def as_const(self, i):
        n = self.nodes[i]
        return n[3] if n[0] == N_CONST else None

    def constant(self, v):
        return self.intern((N_CONST, 0, 0, v % P, 0))

    def add(self, a, b):
        x, y = self.as_const(a), self.as_const(b)
        if x is not None and y is not None:
            return self.constant(x + y)
        if x == 0:
            return b
        if y == 0:
            return a
        if a > b:
            a, b = b, a
        return self.intern((N_ADD, 0, 0, a, b))

    def sub(self, a, b):
        if a == b:
            return self.constant(0)
        x, y = self.as_const(a), self.as_const(b)
        if x is not None and y is not None:
            return self.constant(x - y)
        if y == 0:
            return a
        if x == 0:
            return self.neg(b)
        return self.intern((N_SUB, 0, 0, a, b))

    def mul(self, a, b):
        x, y = self.as_const(a), self.as_const(b)
        if x is not None and y is not None:
            return self.constant(x * y)
        if x is not None:
            if x == 0:
                return a
            if x == 1:
                return b
        if y is not None:
            if y == 0:
                return b
            if y == 1:
                return a
        if a > b:
            a, b = b, a
        return self.intern((N_MUL, 0, 0, a, b))

    def neg(self, a):
        x = self.as_const(a)
        if x is not None:
            return self.constant(-x)
        n = self.nodes[a]
        if n[0] == N_NEG:
            return n[3]
        return self.intern((N_NEG, 0, 0, a, 0))

    def compile_expr(self, e, spec, allow_stage2):
        k = e.kind
        if k >= N_ROW or (k == N_VAR and (e.source == SRC_INPUT or isinstance(e.source, tuple))):
            raise CompileError("WitnessOnlyNode kind=%d: row, bits, inv0, lt, bit_xor, bit_and, indexed reads, inputs and peer reads belong to fill programs" % k)
        if k == N_CONST:
            return self.constant(e.a)
        if k == N_VAR:
            width = {SRC_PRE: spec["preprocessed_width"], SRC_MAIN: spec["main_width"], SRC_STAGE2: spec["stage2_width"]}[e.source]
            if e.source == SRC_STAGE2 and not allow_stage2:
                raise CompileError("Stage2InBaseContext")
            if e.a >= width:
                raise CompileError("ColumnOutOfRange source=%d index=%d width=%d" % (e.source, e.a, width))
            return self.intern((N_VAR, e.source, e.offset, e.a, 0))
        if k == N_PUBLIC:
            if e.a >= spec["num_publics"]:
                raise CompileError("PublicOutOfRange")
            return self.intern((N_PUBLIC, 0, 0, e.a, 0))
        if k in (N_IS_FIRST, N_IS_LAST, N_IS_TRANS):
            return self.intern((k, 0, 0, 0, 0))
        if k == N_NEG:
            return self.neg(self.compile_expr(e.a, spec, allow_stage2))
        a = self.compile_expr(e.a, spec, allow_stage2)
        b = self.compile_expr(e.b, spec, allow_stage2)
        return {N_ADD: self.add, N_SUB: self.sub, N_MUL: self.mul}[k](a, b)

    def is_scalar(self, coords):
        return all(self.as_const(c) == 0 for c in coords[1:])

    def ext_mul(self, a, b, d, w, karatsuba):
        # src/graph.rs:448-507
        if self.is_scalar(a):
            return [self.mul(a[0], bk) for bk in b]
        if self.is_scalar(b):
            return [self.mul(b[0], ak) for ak in a]
        if d == 2 and karatsuba:
            p0 = self.mul(a[0], b[0])
            p1 = self.mul(a[1], b[1])
            sa = self.add(a[0], a[1])
            sb = self.add(b[0], b[1])
            s = self.mul(sa, sb)
            wn = self.constant(w)
            wp1 = self.mul(wn, p1)
            c0 = self.add(p0, wp1)
            t = self.sub(s, p0)
            c1 = self.sub(t, p1)
            return [c0, c1]
        wn = self.constant(w)
        out = []
        for k in range(d):
            low = high = None
            for i, ai in enumerate(a):
                for j, bj in enumerate(b):
                    if i + j == k:
                        term = self.mul(ai, bj)
                        low = term if low is None else self.add(low, term)
                    elif i + j == k + d:
                        term = self.mul(ai, bj)
                        high = term if high is None else self.add(high, term)
            out.append(low if high is None else self.add(low, self.mul(wn, high)))
        return out

    def expand_ext(self, e, spec, d, w, karatsuba):
        k = e.kind
        if k == "coords":
            if len(e.a) != d:
                raise CompileError("CoordsLength")
            return [self.compile_expr(c, spec, True) for c in e.a]
        if k == "base":
            zero = self.constant(0)
            coords = [zero] * d
            coords[0] = self.compile_expr(e.a, spec, True)
            return coords
        if k == "neg":
            return [self.neg(c) for c in self.expand_ext(e.a, spec, d, w, karatsuba)]
        a = self.expand_ext(e.a, spec, d, w, karatsuba)
        b = self.expand_ext(e.b, spec, d, w, karatsuba)
        if k == "add":
            return [self.add(a[i], b[i]) for i in range(d)]
        if k == "sub":
            return [self.sub(a[i], b[i]) for i in range(d)]
        return self.ext_mul(a, b, d, w, karatsuba)


class CompiledCircuit:
    """What `graph::compile` returns (src/graph.rs:62-76) plus the widths System::new keeps."""

    def __init__(self, nodes, zeros, lookups, main_width, preprocessed):
        self.nodes, self.zeros, self.lookups = nodes, zeros, lookups
        self.main_width = main_width
        self.preprocessed = preprocessed  # None or np.ndarray (h, w) uint64
        self.lookup_prefix_len = 0
        # per entry of `zeros`: the authored constraints it came from, ("constraint", i) or ("ext", i, coordinate); several
        # may share a root (`zeros` is a sorted set), one folded to the constant zero appears nowhere
        self.zero_origins = [[] for _ in zeros]


class CircuitInputs:
    """src/system.rs:29-47."""

    def __init__(self, main_width=0, preprocessed=None, constraints=None, ext_constraints=None, lookups=None):
        self.main_width = main_width
        self.preprocessed = preprocessed
        self.constraints = list(constraints or [])
        self.ext_constraints = list(ext_constraints or [])
        self.lookups = list(lookups or [])


def compile_circuit(inputs, d=None, w=None):
    """`graph::compile` (src/graph.rs:120-188) on the spec System::new builds (src/system.rs:128-149)."""
    d = EXT_D if d is None else d
    w = EXT_W if w is None else w
    pre = inputs.preprocessed
    spec = {
        "main_width": inputs.main_width,
        "preprocessed_width": 0 if pre is None else int(pre.shape[1]),
        "stage2_width": max(len(inputs.lookups), 1) * d,
        "num_publics": 4 * d,
    }
    it = _Interner()
    lookups = []
    for lk in inputs.lookups:
        m = it.compile_expr(lk.multiplicity, spec, False)
        args = [it.compile_expr(a, spec, False) for a in lk.args]
        lookups.append((m, args))
    prefix = len(it.nodes)
    zeros = []
    authored = {}  # root -> the authored constraints that compiled to it (several may share one)

    def record(root, what, origin):
        c = it.as_const(root)
        if c is None:
            zeros.append(root)
            authored.setdefault(root, []).append(origin)
        elif c != 0:
            raise CompileError("UnsatisfiableConstant %s" % what)

    for i, c in enumerate(inputs.constraints):
        record(it.compile_expr(c, spec, False), "constraint %d" % i, ("constraint", i))
    for i, c in enumerate(inputs.ext_constraints):
        if c.is_purely_base():
            raise CompileError("PurelyBaseExtConstraint %d" % i)
        for k, root in enumerate(it.expand_ext(c, spec, d, w, d == 2)):
            record(root, "ext constraint %d coord %d" % (i, k), ("ext", i, k))
    zeros = sorted(set(zeros))
    cc = CompiledCircuit(it.nodes, zeros, lookups, inputs.main_width, pre)
    cc.lookup_prefix_len = prefix
    cc.zero_origins = [authored[z] for z in zeros]
    return cc


class AirBuilder:
    """Recording builder, src/p3_adapter.rs:245-288 (+ p3-air default methods)."""

    def __init__(self, main_width, preprocessed_width=0, _cond=None, _sink=None):
        self.main_width, self.preprocessed_width = main_width, preprocessed_width
        self.constraints = [] if _sink is None else _sink
        self._cond = _cond

    def main(self):
        return [Expr.main(i) for i in range(self.main_width)], [Expr.main_next(i) for i in range(self.main_width)]

    def preprocessed(self):
        return ([Expr.var(SRC_PRE, 0, i) for i in range(self.preprocessed_width)],
                [Expr.var(SRC_PRE, 1, i) for i in range(self.preprocessed_width)])

    def is_first_row(self):
        return IS_FIRST_ROW

    def is_last_row(self):
        return IS_LAST_ROW

    def is_transition(self):
        return IS_TRANSITION

    def assert_zero(self, x):
        x = Expr.lift(x)
        self.constraints.append(x if self._cond is None else self._cond * x)

    def assert_eq(self, x, y):
        self.assert_zero(Expr.lift(x) - Expr.lift(y))

    def assert_one(self, x):
        self.assert_zero(Expr.lift(x) - Expr.const(1))

    def assert_bool(self, x):
        x = Expr.lift(x)
        self.assert_zero((Expr.const(1) - x) * x)  # p3 bool_check = andn(self, self)

    def assert_bools(self, xs):
        for x in xs:
            self.assert_bool(x)

    def when(self, cond):
        cond = Expr.lift(cond)
        c = cond if self._cond is None else self._cond * cond
        return AirBuilder(self.main_width, self.preprocessed_width, c, self.constraints)

    def when_transition(self):
        return self.when(IS_TRANSITION)

    def when_first_row(self):
        return self.when(IS_FIRST_ROW)

    def when_last_row(self):
        return self.when(IS_LAST_ROW)


def lookup_air(main_width, eval_fn, lookups, preprocessed=None):
    """`LookupAir::new(air, lookups).into()` (src/p3_adapter.rs:295-354)."""
    pw = 0 if preprocessed is None else int(preprocessed.shape[1])
    b = AirBuilder(main_width, pw)
    if eval_fn is not None:
        eval_fn(b)
    return CircuitInputs(main_width, preprocessed, b.constraints, [], lookups)


class Params:
    """CommitmentParameters + FriParameters (src/types.rs:171-197)."""

    def __init__(self, log_blowup=1, cap_height=0, log_final_poly_len=0, max_log_arity=1, num_queries=64,
                 commit_proof_of_work_bits=0, query_proof_of_work_bits=0):
        self.log_blowup, self.cap_height = log_blowup, cap_height
        self.log_final_poly_len, self.max_log_arity, self.num_queries = log_final_poly_len, max_log_arity, num_queries
        self.commit_proof_of_work_bits, self.query_proof_of_work_bits = commit_proof_of_work_bits, query_proof_of_work_bits

    def words(self):
        return [self.log_blowup, self.cap_height, self.log_final_poly_len, self.max_log_arity, self.num_queries,
                self.commit_proof_of_work_bits, self.query_proof_of_work_bits]


def bench_params():
    """benches/multi_stark.rs:244-258."""
    return Params(2, 0, 0, 1, 100, 10, 10)


def test_params():
    """The parameters every in-tree test/example uses (e.g. src/test_circuits/u32_add.rs:195-207)."""
    return Params(1, 0, 0, 1, 64, 0, 0)


def system_blob(params, compiled, poseidon2=None):
    """Serialise (params, compiled circuits) into the little-endian u64-word blob both libraries parse. Under
    `field(BABYBEAR)` the parameters are followed by the 141 Poseidon2 round constants (8 x 16 external, 13 internal)."""
    words = [BLOB_MAGIC] + params.words()
    if BLOB_MAGIC == BABYBEAR["BLOB_MAGIC"]:
        k = np.asarray(poseidon2, dtype=np.uint64).reshape(-1)
        if k.size != 141 or int(k.max()) >= P:
            raise ValueError("the BabyBear configuration needs 141 canonical Poseidon2 round constants")
        words += [int(x) for x in k]
    words += [len(compiled)]
    chunks = []
    for c in compiled:
        pre = c.preprocessed
        pw = 0 if pre is None else int(pre.shape[1])
        ph = 0 if pre is None else int(pre.shape[0])
        words += [c.main_width, pw, ph, len(c.nodes), len(c.zeros), len(c.lookups)]
        for (kind, source, offset, a, b) in c.nodes:
            words += [kind | (source << 8) | (offset << 16), a, b]
        words += list(c.zeros)
        for (m, args) in c.lookups:
            words += [m, len(args)] + list(args)
        chunks.append(np.asarray(words, dtype=np.uint64).tobytes())
        words = []
        if pre is not None:
            chunks.append(np.ascontiguousarray(pre, dtype=np.uint64).tobytes())
    chunks.append(np.asarray(words, dtype=np.uint64).tobytes())
    return b"".join(chunks)


# --------------------------------------------------------------------------- fill programs (ms_witness_fill)
# How the dependent columns of one circuit follow from inputs and other columns: an ordered list of steps (dst_column, Expr)
# over the constraint algebra plus the witness-only leaves Expr.input / Expr.input_next / Expr.row, the indexed reads
# Expr.main_at / Expr.pre_at / Expr.input_at (a column at a computed row; 0 from the source's height on) and the operators below.
# The semantics are written down in include/mstark.h; operands are the canonical integers in [0, P).
def bits(x, lo, length):
    """(x >> lo) & (2^length - 1), 1 <= length, lo + length <= 64 (32 under field(BABYBEAR))"""
    lo, length = int(lo), int(length)
    if lo < 0 or length < 1 or lo + length > FILL_BITS:
        raise CompileError("BadBitsFields lo=%d length=%d" % (lo, length))
    return Expr(N_BITS, Expr.lift(x), lo | (length << 8))


def inv0(x):
    """x^-1 mod P, and 0 for x = 0"""
    return Expr(N_INV0, Expr.lift(x))


def lt(x, y):
    """1 if x < y as integers, else 0"""
    return Expr(N_LT, Expr.lift(x), Expr.lift(y))


def bit_xor(x, y):
    """(x ^ y) mod P"""
    return Expr(N_XOR, Expr.lift(x), Expr.lift(y))


def bit_and(x, y):
    """x & y"""
    return Expr(N_AND, Expr.lift(x), Expr.lift(y))


class _FillInterner(_Interner):
    """The interner of compile_circuit with the witness-only nodes: equal subexpressions are shared, constants folded."""

    def bits(self, a, f):
        x = self.as_const(a)
        if x is not None:
            return self.constant((x >> (f & 0xFF)) & ((1 << (f >> 8)) - 1))
        return self.intern((N_BITS, 0, 0, a, f))

    def inv0(self, a):
        x = self.as_const(a)
        if x is not None:
            return self.constant(pow(x, P - 2, P))
        return self.intern((N_INV0, 0, 0, a, 0))

    def lt(self, a, b):
        x, y = self.as_const(a), self.as_const(b)
        if x is not None and y is not None:
            return self.constant(1 if x < y else 0)
        return self.intern((N_LT, 0, 0, a, b))

    def xor(self, a, b):
        x, y = self.as_const(a), self.as_const(b)
        if x is not None and y is not None:
            return self.constant(x ^ y)
        return self.intern((N_XOR, 0, 0, min(a, b), max(a, b)))

    def and_(self, a, b):
        x, y = self.as_const(a), self.as_const(b)
        if x is not None and y is not None:
            return self.constant(x & y)
        return self.intern((N_AND, 0, 0, min(a, b), max(a, b)))

    @staticmethod
    def source_width(source, spec):
        """the width a column of `source` must stay below; a peer: from compile_fill's peers= ({circuit: (main, preprocessed)})"""
        if isinstance(source, tuple):
            _, circuit, trace = source
            if spec.get("claims"):
                raise CompileError("PeerReadInClaimProgram circuit=%d: a claim program reads the traces of its own circuit and the inputs" % circuit)
            if FILL_MAGIC != GOLDILOCKS["FILL_MAGIC"]:
                raise CompileError("PeerReadInThisField circuit=%d: peer reads: Goldilocks configuration only" % circuit)
            if circuit not in (spec["peers"] or {}):
                raise CompileError("UnknownPeer circuit=%d: not among compile_fill(..., peers=...), which names %s"
                                   % (circuit, sorted(spec["peers"]) if spec["peers"] else "none"))
            return int(spec["peers"][circuit][0 if trace == SRC_MAIN else 1])
        if source not in (SRC_PRE, SRC_MAIN, SRC_INPUT):
            raise CompileError("Stage2InFillProgram")
        return {SRC_PRE: spec["preprocessed_width"], SRC_MAIN: spec["main_width"], SRC_INPUT: spec["n_inputs"]}[source]

    def compile_fill_expr(self, e, spec):
        k = e.kind
        if k == N_CONST:
            return self.constant(e.a)
        if k == N_VAR:
            width = self.source_width(e.source, spec)
            if e.offset not in (0, 1):
                raise CompileError("RowOffsetOutOfRange offset=%d" % e.offset)
            if not 0 <= e.a < width:
                raise CompileError("ColumnOutOfRange source=%s index=%d width=%d" % (e.source, e.a, width))
            return self.intern((N_VAR, e.source, e.offset, e.a, 0))
        if k in (N_PUBLIC, N_IS_FIRST, N_IS_LAST, N_IS_TRANS):
            raise CompileError("NotAllowedInFillProgram kind=%d: publics and selector polynomials are no witness values "
                               "(flags come from row, lt and inv0)" % k)
        if k == N_ROW:
            return self.intern((N_ROW, 0, 0, 0, 0))
        if k == N_AT:
            width = self.source_width(e.source, spec)
            if e.offset:
                raise CompileError("RowOffsetOutOfRange offset=%d: an indexed read has no row offset" % e.offset)
            if not 0 <= e.a < width:
                raise CompileError("ColumnOutOfRange source=%s index=%d width=%d" % (e.source, e.a, width))
            return self.intern((N_AT, e.source, 0, e.a, self.compile_fill_expr(e.b, spec)))  # (a constant row stays a node)
        if k not in (N_ADD, N_SUB, N_MUL, N_NEG, N_BITS, N_INV0, N_LT, N_XOR, N_AND):
            raise CompileError("UnknownNodeKind kind=%d" % k)
        a = self.compile_fill_expr(e.a, spec)
        if k == N_NEG:
            return self.neg(a)
        if k == N_INV0:
            return self.inv0(a)
        if k == N_BITS:
            return self.bits(a, e.b)
        b = self.compile_fill_expr(e.b, spec)
        return {N_ADD: self.add, N_SUB: self.sub, N_MUL: self.mul, N_LT: self.lt, N_XOR: self.xor, N_AND: self.and_}[k](a, b)


class Scan:
    """The right-hand side of a scan step (scan, running_sum, running_product): dst[0] = init, dst[r + 1] = mul(r) * dst[r] + add(r)"""

    __slots__ = ("mul", "add", "init")

    def __init__(self, mul, add, init):
        self.mul, self.add, self.init = Expr.lift(mul), Expr.lift(add), int(init)


def scan(mul, add, init=0):
    """A column that follows its previous row, usable only as the right-hand side of a step of compile_fill: the column starts
    at init (an integer in [0, P)) and row r + 1 is mul * previous + add with both expressions taken at row r (no wrap-around:
    their values at the last row are not used). The expressions may not read the column itself."""
    return Scan(mul, add, init)


def running_sum(add, init=0):
    """scan(1, add, init): the additive form on the device, no multiplications"""
    return Scan(1, add, init)


def running_product(mul, init=1):
    return Scan(mul, 0, init)


def fill_blob(main_width, preprocessed_width, n_inputs, nodes, steps, scans=None, peers=None):
    """The little-endian u64-word blob of a fill program, unchecked: magic, main_width, pre_width, n_inputs, n_nodes, n_steps,
    the nodes as [kind | source << 8 | offset << 16, a, b], the steps as [dst, root]. With scans (a non-empty list of
    (step index, mul root, init)): the magic of the second format, n_scans as a seventh header word, and the scan records
    behind the steps; the root of a scan step is its add root. With peers (a non-empty list of (circuit, trace, width)): the
    magic of the third format, n_scans (0 allowed) and n_peers as seventh and eighth header word, and the peer records last."""
    words = [FILL_MAGIC, main_width, preprocessed_width, n_inputs, len(nodes), len(steps)]
    if peers:
        words[0] = FILL_PEER_MAGIC
        words += [len(scans or []), len(peers)]
    elif scans:
        words[0] = FILL_SCAN_MAGIC
        words.append(len(scans))
    for (kind, source, offset, a, b) in nodes:
        words += [kind | (source << 8) | (offset << 16), a, b]
    for (dst, root) in steps:
        words += [dst, root]
    for (step, mul, init) in scans or []:
        words += [step, mul, init]
    for (circuit, trace, width) in peers or []:
        words += [circuit, trace, width]
    return np.asarray(words, dtype=np.uint64).tobytes()


class FillProgram:
    """What compile_fill returns: .nodes (kind, source, offset, a, b), .steps (dst, root; a scan step's root is its add root),
    .scans (step index, mul root, init), .peers (circuit, trace, width; source 4 + k of a node names .peers[k]), the widths
    and .blob"""

    def __init__(self, main_width, preprocessed_width, n_inputs, nodes, steps, scans=(), peers=()):
        self.main_width, self.preprocessed_width, self.n_inputs = main_width, preprocessed_width, n_inputs
        self.nodes, self.steps, self.scans, self.peers = nodes, steps, list(scans), list(peers)
        self.blob = fill_blob(main_width, preprocessed_width, n_inputs, nodes, steps, self.scans, self.peers)


def _main_reads(nodes):
    """per node: the main columns it reads, directly or through operands, as (at offset 0, at offset 1, at a computed row);
    for the group rule an indexed read counts as an offset-1 read, and it is kept apart only for the error's name"""
    none = frozenset()
    reads = []
    for (kind, source, offset, a, b) in nodes:
        if kind == N_VAR:
            cols = frozenset([a]) if source == SRC_MAIN else none
            reads.append((none, cols, none) if offset else (cols, none, none))
        elif kind == N_AT:
            r = reads[b]
            reads.append((r[0], r[1], r[2] | frozenset([a])) if source == SRC_MAIN else r)
        elif kind in (N_NEG, N_INV0, N_BITS):
            reads.append(reads[a])
        elif kind in (N_ADD, N_SUB, N_MUL, N_LT, N_XOR, N_AND):
            reads.append(tuple(reads[a][t] | reads[b][t] for t in range(3)))
        else:
            reads.append((none, none, none))
    return reads


def _number_peers(nodes, roots, spec):
    """The ("peer", circuit, trace) sources of the nodes that `roots` reach -> (nodes with source bytes 4 + k, the records
    (circuit, trace, width) in ascending order). A peer read that constant folding left unreached becomes the constant 0: it
    stands in the blob like every node, and names no record."""
    reached, stack = set(), list(roots)
    while stack:
        i = stack.pop()
        if i in reached:
            continue
        reached.add(i)
        kind, _, _, a, b = nodes[i]
        if kind in (N_NEG, N_INV0, N_BITS):
            stack.append(a)
        elif kind in (N_ADD, N_SUB, N_MUL, N_LT, N_XOR, N_AND):
            stack += [a, b]
        elif kind == N_AT:
            stack.append(b)
    pairs = sorted({n[1][1:] for i, n in enumerate(nodes) if i in reached and isinstance(n[1], tuple)})
    if len(pairs) > FL_MAX_PEERS:
        raise CompileError("TooManyPeers %d: a fill program reads at most %d (circuit, trace) pairs: %s" % (len(pairs), FL_MAX_PEERS, pairs))
    out = []
    for i, n in enumerate(nodes):
        if isinstance(n[1], tuple):
            n = (n[0], SRC_PEER + pairs.index(n[1][1:]), n[2], n[3], n[4]) if i in reached else (N_CONST, 0, 0, 0, 0)
        out.append(n)
    return out, [(c, t, int(spec["peers"][c][0 if t == SRC_MAIN else 1])) for (c, t) in pairs]


def compile_fill(main_width, preprocessed_width, n_inputs, steps, scans=None, peers=None):
    """steps: [(dst_column, Expr or scan(...))], run in order, each for every row (include/mstark.h, ms_witness_fill).
    Every scan step is a group of its own and every run of ordinary steps between scans is one; the next row of a main column
    may be read only where no step of the same or a later group assigns it. scans: None - scan steps are accepted under the
    Goldilocks field alone; True - under either field (babybear.compile_fill passes it). peers: {circuit: (main_width,
    preprocessed_width)} of the OTHER circuits of the witness that Expr.peer / peer_next / peer_at and their peer_pre
    counterparts may read (System.fill_peers() gives it for a whole system); a program that reads none keeps its blob byte for
    byte, one that does is emitted in the third format with a record per (circuit, trace) pair reached. -> FillProgram"""
    spec = {"main_width": int(main_width), "preprocessed_width": int(preprocessed_width), "n_inputs": int(n_inputs), "peers": peers}
    it = _FillInterner()
    any_field, out, scans = bool(scans), [], []
    for k, (dst, e) in enumerate(steps):
        dst = int(dst)
        if not 0 <= dst < spec["main_width"]:
            raise CompileError("DstOutOfRange step=%d dst=%d main_width=%d" % (k, dst, spec["main_width"]))
        if isinstance(e, Scan):
            if FILL_MAGIC != GOLDILOCKS["FILL_MAGIC"] and not any_field:
                raise CompileError("ScanStepInThisField step=%d: scan steps: Goldilocks configuration only "
                                   "(unless compile_fill(..., scans=True), as babybear.compile_fill passes)" % k)
            if not 0 <= e.init < P:
                raise CompileError("ScanInitOutOfRange step=%d init=%d: the first value of a scan column is an integer in [0, P)" % (k, e.init))
            scans.append((k, it.compile_fill_expr(e.mul, spec), e.init))
            e = e.add
        out.append((dst, it.compile_fill_expr(Expr.lift(e), spec)))
    records = []
    if any(isinstance(n[1], tuple) for n in it.nodes):
        it.nodes, records = _number_peers(it.nodes, [root for _, root in out] + [mul for _, mul, _ in scans], spec)
    if not scans:
        assigned = {dst for dst, _ in out}
        for (kind, source, offset, a, _) in it.nodes:
            if kind == N_VAR and source == SRC_MAIN and offset == 1 and a in assigned:
                raise CompileError("NextRowOfAssignedColumn column=%d: a fill program may read the next row only of columns it does not assign" % a)
        if any(kind == N_AT for (kind, _, _, _, _) in it.nodes):
            reads = _main_reads(it.nodes)
            for k, (_, root) in enumerate(out):
                for m in sorted(reads[root][2] & assigned):
                    raise CompileError("IndexedReadOfAssignedColumn column=%d step=%d: a computed row may be read only of columns that no step "
                                       "of the same or a later group assigns (a program without scan steps is one group)" % (m, k))
        return FillProgram(spec["main_width"], spec["preprocessed_width"], spec["n_inputs"], it.nodes, out, peers=records)
    # groups: a scan step is one, a run of ordinary steps between scans is one
    mul_of = {k: mul for k, mul, _ in scans}
    group, g = [], -1
    for k in range(len(out)):
        if k in mul_of or k == 0 or (k - 1) in mul_of:
            g += 1
        group.append(g)
    last_group = {}
    for k, (dst, _) in enumerate(out):
        last_group[dst] = group[k]
    reads = _main_reads(it.nodes)
    for k, (dst, root) in enumerate(out):
        roots = [root] + ([mul_of[k]] if k in mul_of else [])
        at0 = frozenset().union(*(reads[r][0] for r in roots))
        at1 = frozenset().union(*(reads[r][1] for r in roots))
        if k in mul_of and dst in at0 | at1:
            raise CompileError("ScanReadsOwnColumn step=%d column=%d: the coefficients of a scan step may not read its own column "
                               "(the previous row's value enters through the recurrence alone)" % (k, dst))
        for m in sorted(at1):
            if last_group.get(m, -1) >= group[k]:
                raise CompileError("NextRowOfAssignedColumn column=%d step=%d: the next row may be read only of columns that no step of "
                                   "the same or a later group assigns (group %d reads, group %d assigns)" % (m, k, group[k], last_group[m]))
        for m in sorted(frozenset().union(*(reads[r][2] for r in roots))):  # (a scan's own dst is such a column)
            if last_group.get(m, -1) >= group[k]:
                raise CompileError("IndexedReadOfAssignedColumn column=%d step=%d: a computed row may be read only of columns that no step of "
                                   "the same or a later group assigns (group %d reads, group %d assigns)" % (m, k, group[k], last_group[m]))
    return FillProgram(spec["main_width"], spec["preprocessed_width"], spec["n_inputs"], it.nodes, out, scans, records)


def u32_add_fill_program(num_adds):
    """The 14 columns of the U32Add circuit (u32_add_system_inputs) from inputs (x, y), one pair per row: the byte decompositions
    of x, y and the low word of x + y, the carry, and the row's activity flag; rows from num_adds on come out as zeros."""
    x, y = Expr.input(0), Expr.input(1)
    s = x + y
    steps = [(k, bits(x, 8 * k, 8)) for k in range(4)] + [(4 + k, bits(y, 8 * k, 8)) for k in range(4)]
    steps += [(8 + k, bits(s, 8 * k, 8)) for k in range(4)]
    steps += [(12, bits(s, 32, 1)), (13, lt(Expr.row(), num_adds))]
    return compile_fill(14, 0, 2, steps)


def u32_add_halves_fill_program(num_adds):
    """The 14 columns of the U32Add circuit from inputs (x_lo, x_hi, y_lo, y_hi), the 16-bit halves of one pair per row. No
    intermediate value reaches 2^18, so the program means the same over both fields (u32_add_fill_program reads bit 32 of x + y,
    which a field below 2^31 cannot hold): s_lo = x_lo + y_lo, s_hi = x_hi + y_hi + its carry, the bytes of the six halves, the
    carry of s_hi, and the row's activity flag; rows from num_adds on come out as zeros."""
    x_lo, x_hi, y_lo, y_hi = (Expr.input(k) for k in range(4))
    s_lo = x_lo + y_lo
    s_hi = x_hi + y_hi + bits(s_lo, 16, 1)
    steps = []
    for base, (lo, hi) in ((0, (x_lo, x_hi)), (4, (y_lo, y_hi)), (8, (s_lo, s_hi))):
        steps += [(base, bits(lo, 0, 8)), (base + 1, bits(lo, 8, 8)), (base + 2, bits(hi, 0, 8)), (base + 3, bits(hi, 8, 8))]
    steps += [(12, bits(s_hi, 16, 1)), (13, lt(Expr.row(), num_adds))]
    return compile_fill(14, 0, 4, steps)


def rows_per_item_fill_program(k):
    """A circuit that spends k rows on every item (k a power of two, at most 256): row r belongs to item r >> log2(k) and holds
    limb r & (k - 1) of it. The input matrix has one row per item and max(k / 2, 1) columns of 16-bit words, two 8-bit limbs
    each (limb j is byte j & 1 of word j >> 1), so the program means the same over both fields. Columns: 0 the item's number,
    1 the limb's number, 2 the limb - every row of an item reads the item's input row, Expr.input_at(c, item), and the limb is
    selected by the bits of the limb's number. Rows behind the last item read 0 (an index from the height on)."""
    k = int(k)
    log_k = k.bit_length() - 1
    if k < 1 or k != 1 << log_k or k > 256:
        raise CompileError("RowsPerItem k=%d: a power of two between 1 and 256" % k)
    row = Expr.row()
    item = bits(row, log_k, 32 - log_k)
    which = bits(row, 0, log_k) if log_k else Expr.const(0)
    bit = [bits(row, t, 1) for t in range(log_k)]
    limb = Expr.const(0)
    for j in range(k):
        sel = Expr.const(1)
        for t in range(log_k):
            sel = sel * (bit[t] if (j >> t) & 1 else 1 - bit[t])
        limb = limb + sel * bits(Expr.input_at(j >> 1, item), 8 * (j & 1), 8)
    return compile_fill(3, 0, max(k // 2, 1), [(0, item), (1, which), (2, limb)])


# --------------------------------------------------------------------------- claim programs (ms_witness_claims_fill)
# The claims of a witness as a function of one circuit's rows: W expressions, the elements of a claim, and optionally `keep`; one
# claim per row of the first `rows` whose keep is non-zero, in row order. The algebra is that of fill programs without peer reads
# and scans; nothing is assigned, so any main column may be read at the next row or at a computed row (include/mstark.h,
# "CLAIM PROGRAMS").
def claims_blob(main_width, preprocessed_width, n_inputs, nodes, roots, keep=None):
    """The little-endian u64-word blob of a claim program, unchecked: magic, main_width, pre_width, n_inputs, n_nodes, W, the keep
    root (all ones: none), the nodes as in fill_blob, the W element roots."""
    words = [CLAIM_MAGIC, main_width, preprocessed_width, n_inputs, len(nodes), len(roots), (1 << 64) - 1 if keep is None else keep]
    for (kind, source, offset, a, b) in nodes:
        words += [kind | (source << 8) | (offset << 16), a, b]
    words += list(roots)
    return np.asarray(words, dtype=np.uint64).tobytes()


class ClaimProgram:
    """What compile_claims returns: .nodes (kind, source, offset, a, b), .roots (one per element), .keep (a root or None), the
    widths, .width (W), .has_keep and .blob"""

    def __init__(self, main_width, preprocessed_width, n_inputs, nodes, roots, keep=None):
        self.main_width, self.preprocessed_width, self.n_inputs = main_width, preprocessed_width, n_inputs
        self.nodes, self.roots, self.keep = nodes, list(roots), keep
        self.width, self.has_keep = len(self.roots), keep is not None
        self.blob = claims_blob(main_width, preprocessed_width, n_inputs, nodes, self.roots, keep)


def compile_claims(main_width, preprocessed_width, n_inputs, elements, keep=None):
    """elements: the W expressions of one claim, 1 <= W <= 2^16; keep: None (every row emits a claim) or an expression (the rows
    where it is non-zero do). The program belongs to the field in force (`field(BABYBEAR)`: the magic "\\0MCLAIB1", constants
    folded modulo that p, bits up to 32). -> ClaimProgram"""
    spec = {"main_width": int(main_width), "preprocessed_width": int(preprocessed_width), "n_inputs": int(n_inputs), "peers": None, "claims": True}
    elements = list(elements)
    if not 1 <= len(elements) <= CLAIM_MAX_WIDTH:
        raise CompileError("ClaimWidthOutOfRange width=%d: a claim has 1 to 2^16 elements" % len(elements))
    it = _FillInterner()

    def root(e, what):
        if isinstance(e, Scan):
            raise CompileError("ScanInClaimProgram %s: a claim is a function of one row's reads, scan steps belong to fill programs" % what)
        try:
            return it.compile_fill_expr(Expr.lift(e), spec)
        except CompileError as err:
            raise CompileError("%s (%s of the claim program)" % (err, what)) from None

    roots = [root(e, "element %d" % k) for k, e in enumerate(elements)]
    keep_root = None if keep is None else root(keep, "keep")
    return ClaimProgram(spec["main_width"], spec["preprocessed_width"], spec["n_inputs"], it.nodes, roots, keep_root)


def u32_add_claims_program():
    """The claims of the U32Add circuit (u32_add_system_inputs) from its filled trace, [1, x, y, z] per addition with the words
    put together from their byte columns: call it with rows = the number of additions. Under `field(BABYBEAR)` the words are
    taken modulo p, as frontend.u32_add_bench_witness's claims are there."""
    def word(i):
        return sum((Expr.main(i + k) * Expr.const(256 ** k) for k in range(1, 4)), Expr.main(i))

    return compile_claims(14, 0, 0, [Expr.const(1), word(0), word(4), word(8)])


# --------------------------------------------------------------------------- circuits
def u32_add_system_inputs():
    """[ByteTable, U32Add] -- benches/multi_stark.rs:73-165,260-267 (same as src/test_circuits/u32_add.rs)."""
    byte_index, u32_index = Expr.const(0), Expr.const(1)
    var = Expr.main
    byte_pre = np.arange(256, dtype=np.uint64).reshape(256, 1)
    byte_table = lookup_air(1, None, [Lookup.pull(var(0), [byte_index, Expr.preprocessed(0)])], byte_pre)

    def eval_add(b):
        local, _ = b.main()
        x, y, z, carry = local[0:4], local[4:8], local[8:12], local[12]
        b.assert_bool(carry)
        e1 = (x[0] + x[1] * Expr.const(256) + x[2] * Expr.const(256 ** 2) + x[3] * Expr.const(256 ** 3)
              + y[0] + y[1] * Expr.const(256) + y[2] * Expr.const(256 ** 2) + y[3] * Expr.const(256 ** 3))
        e2 = (z[0] + z[1] * Expr.const(256) + z[2] * Expr.const(256 ** 2) + z[3] * Expr.const(256 ** 3)
              + carry * Expr.const(256 ** 4))
        b.assert_eq(e1, e2)

    def word(i):
        return (var(i) + var(i + 1) * Expr.const(256) + var(i + 2) * Expr.const(256 ** 2)
                + var(i + 3) * Expr.const(256 ** 3))

    lookups = [Lookup.pull(var(13), [u32_index, word(0), word(4), word(8)])]
    lookups += [Lookup.push(Expr.const(1), [byte_index, var(i)]) for i in range(12)]
    u32_add = lookup_air(14, eval_add, lookups)
    return [byte_table, u32_add]


def u32_add_witness(pairs, height=None):
    """Traces for explicit (x, y) calls: src/test_circuits/u32_add.rs:150-190."""
    n = len(pairs)
    h = height or max(1, 1 << (n - 1).bit_length())
    x = np.array([p[0] for p in pairs], dtype=np.uint64)
    y = np.array([p[1] for p in pairs], dtype=np.uint64)
    return _u32_add_traces(x, y, h)


def _u32_add_traces(x, y, h):
    n = len(x)
    s = x + y
    z = s & np.uint64(0xFFFFFFFF)
    carry = s >> np.uint64(32)
    add = np.zeros((h, 14), dtype=np.uint64)
    for k in range(4):
        sh = np.uint64(8 * k)
        add[:n, k] = (x >> sh) & np.uint64(0xFF)
        add[:n, 4 + k] = (y >> sh) & np.uint64(0xFF)
        add[:n, 8 + k] = (z >> sh) & np.uint64(0xFF)
    add[:n, 12] = carry
    add[:n, 13] = 1
    counts = np.bincount(add[:n, :12].astype(np.int64).ravel(), minlength=256).astype(np.uint64)
    byte = counts.reshape(256, 1)
    claims = np.stack([np.ones(n, dtype=np.uint64), x, y, z], axis=1)
    return [byte, add], claims


def xorshift_pairs(num_adds, a0=0xDEADBEEF, b0=0xCAFEBABE):
    """benches/multi_stark.rs:180-192: two independent xorshift32 streams."""
    xs = np.empty(num_adds, dtype=np.uint64)
    ys = np.empty(num_adds, dtype=np.uint64)
    a, b, M = a0, b0, 0xFFFFFFFF
    for i in range(num_adds):
        a ^= (a << 13) & M
        a ^= a >> 17
        a ^= (a << 5) & M
        b ^= (b << 13) & M
        b ^= b >> 17
        b ^= (b << 5) & M
        xs[i] = a
        ys[i] = b
    return xs, ys


def u32_add_bench_witness(num_adds, a0=0xDEADBEEF, b0=0xCAFEBABE):
    """build_witness + build_claims (benches/multi_stark.rs:171-238): returns ([byte_trace, add_trace], claims)."""
    xs, ys = xorshift_pairs(num_adds, a0, b0)
    h = max(1, 1 << (num_adds - 1).bit_length())
    return _u32_add_traces(xs, ys, h)


def multi_u32_add_system_inputs(k):
    """[ByteTable, U32Add x k]: SURVEY §8d config 3 as ONE system (all AIRs in one proof)."""
    base = u32_add_system_inputs()
    return [base[0]] + [u32_add_system_inputs()[1] for _ in range(k)]


def multi_u32_add_witness(k, num_adds):
    """Per-AIR xorshift seeds a0 ^ (i * 0x9e3779b9), b0 ^ (i * 0x85ebca6b); byte multiplicities summed; all claims."""
    byte = np.zeros((256, 1), dtype=np.uint64)
    traces, claims = [None], []
    for i in range(k):
        a0 = 0xDEADBEEF ^ ((i * 0x9E3779B9) & 0xFFFFFFFF)
        b0 = 0xCAFEBABE ^ ((i * 0x85EBCA6B) & 0xFFFFFFFF)
        (bt, add), cl = u32_add_bench_witness(num_adds, a0, b0)
        byte += bt
        traces.append(add)
        claims.append(cl)
    traces[0] = byte
    return traces, np.concatenate(claims, axis=0)


def byte_operations_inputs():
    """ByteCS of src/test_circuits/byte_operations.rs:12-103: a 2^16-row preprocessed table [A, B, A^B, A&B, A|B], four
    multiplicity columns, no AIR constraints, four pull lookups (xor / and / or with 4 arguments, the pair range check
    with 3)."""
    a = np.repeat(np.arange(256, dtype=np.uint64), 256)
    b = np.tile(np.arange(256, dtype=np.uint64), 256)
    pre = np.stack([a, b, a ^ b, a & b, a | b], axis=1)
    var, pvar = Expr.main, Expr.preprocessed
    lookups = [Lookup.pull(var(i), [Expr.const(i), pvar(0), pvar(1), pvar(2 + i)]) for i in range(3)]
    lookups.append(Lookup.pull(var(3), [Expr.const(3), pvar(0), pvar(1)]))
    return [lookup_air(4, None, lookups, pre)]


def byte_operations_witness(calls):
    """ByteCalls::witness (src/test_circuits/byte_operations.rs:106-122): calls = [(op, x, y)], op 0 xor / 1 and / 2 or /
    3 pair range check. Returns ([trace], claims) with the claims of byte_test (:148-154), of ragged lengths."""
    trace = np.zeros((65536, 4), dtype=np.uint64)
    claims = []
    for (op, x, y) in calls:
        trace[256 * x + y, op] += 1
        claims.append([op, x, y] + ([x ^ y, x & y, x | y][op:op + 1] if op < 3 else []))
    return [trace], claims


def squares_inputs():
    """[RangeTable, Squares] of examples/preprocessed_proof.rs:27-88: a byte table pulled by its multiplicity column
    (one-argument lookups, no circuit index) and a squaring circuit [x, x^2, low, high, mult] pushing both bytes."""
    var = Expr.main
    pre = np.arange(256, dtype=np.uint64).reshape(256, 1)
    table = lookup_air(1, None, [Lookup.pull(var(0), [Expr.preprocessed(0)])], pre)

    def ev(b):
        local, _ = b.main()
        x, sq, low, high = local[0], local[1], local[2], local[3]
        b.assert_eq(sq, x * x)
        b.assert_eq(sq, low + high * Expr.const(256))

    squares = lookup_air(5, ev, [Lookup.push(var(4), [var(2)]), Lookup.push(var(4), [var(3)])])
    return [table, squares]


def squares_traces(n=16):
    """examples/preprocessed_proof.rs:108-127: squares of 0..n (n a power of two, n <= 256 so x^2 fits two bytes)."""
    x = np.arange(n, dtype=np.uint64)
    sq = x * x
    low, high = sq & np.uint64(0xFF), (sq >> np.uint64(8)) & np.uint64(0xFF)
    mult = np.bincount(np.concatenate([low, high]).astype(np.int64), minlength=256).astype(np.uint64).reshape(256, 1)
    return [mult, np.stack([x, sq, low, high, np.ones(n, dtype=np.uint64)], axis=1)]


def pythagorean_inputs():
    """examples/simple_proof.rs:21-44."""

    def ev(b):
        local, _ = b.main()
        b.assert_eq(local[0] * local[0] + local[1] * local[1], local[2] * local[2])

    return [lookup_air(3, ev, [])]


def pythagorean_trace(rows):
    """examples/simple_proof.rs:64-83, the 4 triples cycled to `rows` rows."""
    base = np.array([[3, 4, 5], [5, 12, 13], [8, 15, 17], [7, 24, 25]], dtype=np.uint64)
    reps = (rows + 3) // 4
    return np.tile(base, (reps, 1))[:rows].copy()


def verifier_test_inputs():
    """[CS::Pythagorean, CS::Complex] of the verifier's own tests, src/verifier.rs:718-782: a (a^2 + b^2) = a c^2 (the extra
    factor raises the constraint degree to 3) and the complex product (a + ib)(c + id) = e + if; no lookups."""
    def pyth(b):
        local, _ = b.main()
        b.assert_eq(local[0] * (local[0] * local[0] + local[1] * local[1]), local[0] * (local[2] * local[2]))

    def cplx(b):
        local, _ = b.main()
        b.assert_eq(local[0] * local[2] - local[1] * local[3], local[4])
        b.assert_eq(local[0] * local[3] + local[1] * local[2], local[5])

    return [lookup_air(3, pyth, []), lookup_air(6, cplx, [])]


def verifier_test_traces(doublings=0):
    """src/verifier.rs:787-797 (4 + 2 rows); `doublings` = 4 gives the 16-row traces of :806-813 (one row repeated)"""
    if doublings:
        py, cx = [3, 4, 5], [4, 2, 3, 1, 10, 10]
        for _ in range(doublings):
            py, cx = py + py, cx + cx
        return [np.array(py, dtype=np.uint64).reshape(-1, 3), np.array(cx, dtype=np.uint64).reshape(-1, 6)]
    return [np.array([3, 4, 5, 5, 12, 13, 8, 15, 17, 7, 24, 25], dtype=np.uint64).reshape(4, 3),
            np.array([4, 2, 3, 1, 10, 10, 3, 2, 5, 1, 13, 13], dtype=np.uint64).reshape(2, 6)]


def even_odd_inputs(with_dead=False):
    """src/lookup.rs:868-947 (Even / Odd / Dead circuits)."""
    var = Expr.main

    def ev(b):
        local, _ = b.main()
        mult, inp, inp_inv, is_zero, not_zero = local[0], local[1], local[2], local[3], local[4]
        b.assert_bools([is_zero, not_zero])
        b.when(mult).assert_one(is_zero + not_zero)
        b.when(is_zero).assert_zero(inp)
        b.when(not_zero).assert_one(inp * inp_inv)

    mult, inp, is_zero, not_zero, rec = var(0), var(1), var(3), var(4), var(5)
    even_i, odd_i, one = Expr.const(0), Expr.const(1), Expr.const(1)
    even = [Lookup.pull(mult, [even_i, inp, not_zero * rec + is_zero]), Lookup.push(not_zero, [odd_i, inp - one, rec])]
    odd = [Lookup.pull(mult, [odd_i, inp, not_zero * rec]), Lookup.push(not_zero, [even_i, inp - one, rec])]
    out = [lookup_air(6, ev, even), lookup_air(6, ev, odd)]
    if with_dead:
        out.append(lookup_air(6, ev, [Lookup.pull(mult, [Expr.const(2), inp])]))
    return out


def even_odd_traces():
    """src/lookup.rs:975-1007; claim is [0, 4, 1]."""
    inv = lambda v: pow(v, P - 2, P)  # noqa: E731
    even = np.array([[1, 4, inv(4), 0, 1, 1], [1, 2, inv(2), 0, 1, 1], [1, 0, 0, 1, 0, 0], [0, 0, 0, 0, 0, 0]], dtype=np.uint64)
    odd = np.array([[1, 3, inv(3), 0, 1, 1], [1, 1, inv(1), 0, 1, 1], [0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]], dtype=np.uint64)
    return [even, odd]


# --------------------------------------------------------------------------- BabyBear / Poseidon2 configuration
def poseidon2_constants_stand_in(seed=42):
    """141 uniform values below p from numpy's PCG64: the stand-in constants of rounds 1-3 (kept for the fuzzers, which want many
    different permutations, and as the second instantiation the parity tests run under)."""
    return np.random.default_rng(seed).integers(0, BABYBEAR["P"], 141, dtype=np.uint64)


class SmallRngXoshiro:
    """rand's `SmallRng` on a 64-bit target = Xoshiro256++, seeded by `seed_from_u64` through SplitMix64, `next_u32` = the HIGH half
    of `next_u64` [UPSTREAM-RECALL: rand 0.9 `rngs::xoshiro256plusplus`; the reference pins rand 0.10.2 (Cargo.lock:864-865), whose
    SmallRng is assumed unchanged - the pinning kit's 141 dumped constants settle it, tests/test_reference_pins.py]. The
    generator itself is the published xoshiro256++ 1.0 (Blackman / Vigna), checked against its reference vector in
    tests/test_frontend.py."""

    MASK = (1 << 64) - 1

    def __init__(self, seed_u64):
        s, st = [], seed_u64 & self.MASK
        for _ in range(4):  # SplitMix64: one output per 8 seed bytes, little-endian words = the state words in order
            st = (st + 0x9E3779B97F4A7C15) & self.MASK
            z = st
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & self.MASK
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & self.MASK
            s.append(z ^ (z >> 31))
        self.s = s

    @staticmethod
    def _rotl(x, k):
        return ((x << k) | (x >> (64 - k))) & SmallRngXoshiro.MASK

    def next_u64(self):
        s = self.s
        result = (self._rotl((s[0] + s[3]) & self.MASK, 23) + s[0]) & self.MASK
        t = (s[1] << 17) & self.MASK
        s[2] ^= s[0]
        s[3] ^= s[1]
        s[1] ^= s[2]
        s[0] ^= s[3]
        s[2] ^= t
        s[3] = self._rotl(s[3], 45)
        return result

    def next_u32(self):
        return self.next_u64() >> 32


def poseidon2_constants_small_rng(seed=42):
    """The reference's own instantiation, restated: `Perm::new_from_rng_128(&mut SmallRng::seed_from_u64(42))`
    (src/test_circuits/baby_bear_config.rs:54-55) [UPSTREAM-RECALL for everything below; nothing in the reference's tree pins it]:
      * p3-poseidon2 `Poseidon2::new_from_rng_128` -> round numbers for BabyBear, width 16, S-box degree 7: 8 full rounds, 13
        partial ones; `ExternalLayerConstants::new_from_rng` draws the 4 initial rounds' [F; 16] arrays, then the 4 terminal
        ones, element by element, and the 13 internal constants follow;
      * p3-monty-31 `Distribution<MontyField31> for StandardUniform`: `loop { let x = rng.next_u32() >> 1; if x < P { return
        MontyField31::new_monty(x) } }` - the 31-bit value is taken AS the Montgomery word, so the field element is x * 2^-32.
    Returned as canonical values in the front-end's order (initial, terminal, internal), which is what the ABI takes."""
    p = BABYBEAR["P"]
    rng = SmallRngXoshiro(seed)
    r_inv = pow(1 << 32, -1, p)
    out = []
    while len(out) < 141:
        x = rng.next_u32() >> 1
        if x < p:
            out.append(x * r_inv % p)
    return np.array(out, dtype=np.uint64)


def poseidon2_constants(seed=42):
    """141 round constants for Poseidon2BabyBear<16> (8 x 16 external: initial then terminal; then 13 internal), canonical values.
    Default = the restatement of the reference's instantiation (poseidon2_constants_small_rng: SmallRng::seed_from_u64(42) ->
    new_from_rng_128, labelled UPSTREAM-RECALL and checked by the pinning kit's dumped constants when they arrive); they remain
    INPUTS of the library (msbb_system_create takes them), so any other instantiation works the same."""
    return poseidon2_constants_small_rng(seed)


def mul_air_inputs():
    """MulAir + its self-cancelling push/pull pair, src/test_circuits/baby_bear_config.rs:129-157: a * b = c per row,
    lookups push(1, [a, c]) and pull(1, [a, c]). Use under `field(BABYBEAR)`."""
    def ev(b):
        local, _ = b.main()
        b.assert_eq(local[0] * local[1], local[2])

    one = Expr.const(1)
    return [lookup_air(3, ev, [Lookup.push(one, [Expr.main(0), Expr.main(2)]), Lookup.pull(one, [Expr.main(0), Expr.main(2)])])]


def mul_air_trace(rows):
    """rows (r + 1, r + 2, product mod p): BASELINE config 4's scaling of the reference's 4-row trace
    (baby_bear_config.rs:176-192 uses (2,3,6), (4,5,20), (7,8,56), (0,0,0))."""
    r = np.arange(rows, dtype=np.uint64)
    a, b = (r + 1) % P, (r + 2) % P
    return np.stack([a, b, (a * b) % P], axis=1).astype(np.uint64)


def mul_air_smoke_trace():
    """the reference's own 4 rows, baby_bear_config.rs:176-192"""
    return np.array([[2, 3, 6], [4, 5, 20], [7, 8, 56], [0, 0, 0]], dtype=np.uint64)


def pack_claims(claims):
    """list of sequences (or 2-D array) -> (offsets uint64[n+1], data uint64[total])."""
    if isinstance(claims, np.ndarray) and claims.ndim == 2:
        n, w = claims.shape
        return np.arange(0, (n + 1) * w, w, dtype=np.uint64), np.ascontiguousarray(claims.astype(np.uint64) % np.uint64(P)).ravel()
    offs = np.zeros(len(claims) + 1, dtype=np.uint64)
    for i, c in enumerate(claims):
        offs[i + 1] = offs[i] + len(c)
    data = np.array([int(x) % P for c in claims for x in c], dtype=np.uint64)
    return offs, data
