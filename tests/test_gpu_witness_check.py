"""`-m gpu`: ms_witness_check (csrc/check.hip over csrc/check_dev.h) against the model of tests/witness_check_model.py, which
tests/test_witness_check_model.py anchors to the oracle. Every figure of the report is deterministic and compared exactly.
References (model reports, traces) are computed once per case and left unchanged."""
import importlib
import re

import numpy as np
import pytest
import torch  # (before the library opens the device: test_witness_from_a_torch_tensor)

import witness_check_model as wm
from test_witness_check_model import BG, BG2, selector_inputs, selector_trace

pytestmark = pytest.mark.gpu
P = wm.P


class Sys:
    """one system on the device and in the oracle"""

    def __init__(self, pkg, fe, ctx, oracle, inputs, params=None):
        self.comp = [fe.compile_circuit(ci) for ci in inputs]
        self.params = params or fe.test_params()
        blob = fe.system_blob(self.params, self.comp)
        self.dev = pkg.System(ctx, blob, len(self.comp))
        self.dev.params = self.params
        self.osys = oracle.System(blob)
        self.oracle, self.fe = oracle, fe

    def model(self, traces, claims, bg=BG):
        return wm.check(self.oracle, self.osys, self.comp, traces, self.fe.pack_claims(claims), *bg)

    def both(self, traces, claims, bg=BG, witness=None):
        """device report (of `witness`, default: the uploaded traces) and model report, compared in every field"""
        w = witness or self.dev.witness(traces, self.fe.pack_claims(claims))
        rep = w.check(*bg)
        m = self.model(traces, claims, bg)
        assert rep.verdict == m.verdict, (rep.verdict, m.verdict, str(rep))
        assert rep.ok == m.ok
        for i, (d, c) in enumerate(zip(rep.circuits, m.circuits)):
            assert d.fields() == c.fields(), ("circuit %d" % i, d.fields(), c.fields())
        return rep, w


def fib_inputs(fe):
    """a circuit with a next-row window: is_first (m0 - 1), is_transition (n0 - m1), is_transition (n1 - m0 - m1), and - with no
    selector, so that the last row reads row 0 - n2 - m2"""
    E = fe.Expr
    return [fe.CircuitInputs(3, None, [fe.IS_FIRST_ROW * (E.main(0) - 1), fe.IS_TRANSITION * (E.main_next(0) - E.main(1)),
                                       fe.IS_TRANSITION * (E.main_next(1) - E.main(0) - E.main(1)), E.main_next(2) - E.main(2)], [], [])]


_FIB = {}


def fib_trace(n):
    if n not in _FIB:
        a, b, rows = 1, 1, []
        for _ in range(n):
            rows.append([a, b, 77])
            a, b = b, (a + b) % P
        _FIB[n] = np.array(rows, dtype=np.uint64)
    return _FIB[n].copy()


@pytest.fixture(scope="module")
def fib(pkg, fe, ctx, oracle):
    return Sys(pkg, fe, ctx, oracle, fib_inputs(fe))


@pytest.fixture(scope="module")
def b3(pkg):
    return importlib.import_module("multi_stark_amd.blake3_circuit")


@pytest.fixture(scope="module")
def b3sys(pkg, fe, ctx, oracle, b3):
    return Sys(pkg, fe, ctx, oracle, b3.blake3_system_inputs())


# ---------------------------------------------------------------- clean witnesses
@pytest.mark.parametrize("rows", [4, 1])  # 1: the smallest height ms_witness_create accepts (a power of two)
def test_clean_pythagorean(pkg, fe, ctx, oracle, rows):
    s = Sys(pkg, fe, ctx, oracle, fe.pythagorean_inputs())
    rep, _ = s.both([fe.pythagorean_trace(rows)], [])
    assert rep.ok and rep.verdict == 0 and rep.circuits[0].height == rows and "satisfies" in str(rep)


def test_clean_u32_add(pkg, fe, ctx, oracle):
    s = Sys(pkg, fe, ctx, oracle, fe.u32_add_system_inputs())
    traces, claims = fe.u32_add_bench_witness(1 << 10)
    for bg in (BG, BG2):
        rep, _ = s.both(traces, [list(c) for c in claims], bg)
        assert rep.verdict == 0 and [c.height for c in rep.circuits] == [256, 1024]


def test_clean_blake3_one_chunk_hash(fe, b3, b3sys):
    claims = [b3.compression_claim(i) for i in b3.blake3_compressions(bytes(range(200)))[0]]  # four compressions of one chunk
    rep, _ = b3sys.both(b3.blake3_witness(claims), claims)
    assert rep.verdict == 0 and rep.circuits[8].height == 4
    assert rep.circuits[8].kernel == 2  # the compression circuit's thousands of slots: one wave per row


def test_device_generated_witnesses_are_clean(pkg, fe, ctx, oracle, b3, b3sys):
    s = Sys(pkg, fe, ctx, oracle, fe.u32_add_system_inputs(), fe.bench_params())
    rep = s.dev.bench_witness_on_device(1 << 12).check()
    assert rep.verdict == 0 and [c.height for c in rep.circuits] == [256, 4096] and not any(c.failing_rows for c in rep.circuits), str(rep)
    # witness_gen.hip against the constraints themselves, not against another generator
    states = np.array([b3.compression_claim(i)[1:33] for i in b3.blake3_compressions(bytes(range(256)) * 2 + b"tail")[0]], dtype=np.uint32)
    assert len(states) == 9
    rep = b3sys.dev.blake3_witness_on_device(states).check()
    assert rep.verdict == 0 and rep.circuits[8].height == 16 and not any(c.failing_rows for c in rep.circuits), str(rep)


# ---------------------------------------------------------------- one cell off
@pytest.mark.parametrize("row,col", [(0, 0), (0, 2), ((1 << 13) - 1, 1), ((1 << 13) - 1, 2), (4100, 1)],
                         ids=["row0", "row0_wrap_column", "last_row", "last_row_wrap_column", "middle"])
def test_one_cell_off(fe, fib, row, col):
    n = 1 << 13  # 32 workgroups of 256 rows
    tr = fib_trace(n)
    tr[row, col] = (int(tr[row, col]) + 5) % P
    rep, w = fib.both([tr], [])
    c = rep.circuits[0]
    assert rep.verdict == 1 and 1 <= c.failing_rows <= 2 and c.first_failure is not None
    if col == 2:  # the column without a selector: the row in front reads the cell as its next row - for row 0 that is row n - 1
        assert sorted(int(x) for x in c.root_first if x != wm.NONE) == [min(row, (row - 1) % n)] and c.failing_rows == 2
    packed = fe.pack_claims([])
    assert fib.dev.verify_multiple_claims(packed, fib.dev.prove_multiple_claims(w)) != 0
    text = str(rep)
    assert re.search(r"circuit 0: constraint root \d+ non-zero on \d+ rows, first at row %d \(value 0x[0-9a-f]{16}\)" % c.first_failure[0], text), text


def test_clean_fib_proves_and_check_does_not_change_the_proof(fe, fib):
    tr = fib_trace(1 << 13)
    w = fib.dev.witness([tr], fe.pack_claims([]))
    before = fib.dev.prove_multiple_claims(w).to_bytes()
    rep, _ = fib.both([tr], [], witness=w)
    assert rep.verdict == 0
    after = fib.dev.prove_multiple_claims(w).to_bytes()
    assert before == after and fib.dev.verify_multiple_claims(fe.pack_claims([]), after) == 0


def test_named_report(fe, fib):
    tr = fib_trace(16)
    tr[3, 1] += 1
    rep = fib.dev.witness([tr], fe.pack_claims([])).check(names=["Fib"], origins=[fib.comp[0].zero_origins])
    assert re.search(r"circuit 0 \(Fib\): constraint \d \(root \d\) non-zero on 2 rows, first at row 2 \(value 0x", str(rep)), str(rep)


def test_every_row_fails(fe, fib):
    """two columns of garbage (the one the last row reads through the wrap among them): 2^13 failing rows in 32 workgroups, all
    reduced onto the same few counters"""
    n = 1 << 13
    tr = fib_trace(n)
    tr[:, 1:] = np.random.default_rng(7).integers(0, P, (n, 2), dtype=np.uint64)
    rep, _ = fib.both([tr], [])
    c = rep.circuits[0]
    assert c.failing_rows == n and c.first_failure[0] == 0 and max(int(x) for x in c.root_counts) >= n - 1


# ---------------------------------------------------------------- selectors
@pytest.mark.parametrize("n", [4, 32])
def test_selector_polynomials(pkg, fe, ctx, oracle, n):
    s = Sys(pkg, fe, ctx, oracle, selector_inputs(fe))
    rep, _ = s.both([selector_trace(n, True)], [])
    assert rep.verdict == 0
    rep, _ = s.both([selector_trace(n, False)], [])
    c = rep.circuits[0]
    assert rep.verdict == 1 and c.first_failure == (0, 0, (1 - n) % P) and int(c.root_first[1]) == n - 1


# ---------------------------------------------------------------- lookups
def test_lookup_balance(pkg, fe, ctx, oracle):
    s = Sys(pkg, fe, ctx, oracle, fe.even_odd_inputs())
    for bg in (BG, BG2):
        rep, _ = s.both(fe.even_odd_traces(), [[0, 4, 1]], bg)
        assert rep.verdict == 0 and rep.final_accumulator == (0, 0)
        for claims in ([[0, 4, 0]], []):
            rep, _ = s.both(fe.even_odd_traces(), claims, bg)
            assert rep.verdict == pkg.CHECK_LOOKUPS and "lookups unbalanced" in str(rep)
            assert not any(c.failing_rows or any(int(x) for x in c.root_counts) for c in rep.circuits)


def ext_inputs(fe):
    """the logUp step written again as a user's extension constraint, with the multiplicity read from ANOTHER column (m2):
    is_transition ((S' - S)(beta + m1) - m2), S = stage-2 columns 0, 1 (this and the next row), beta = publics 0, 1"""
    E, X = fe.Expr, fe.ExtExpr
    s_cur, s_next = X.coords([E.var(2, 0, 0), E.var(2, 0, 1)]), X.coords([E.var(2, 1, 0), E.var(2, 1, 1)])
    beta = X.coords([E.public(0), E.public(1)])
    c = X.base(fe.IS_TRANSITION) * ((s_next - s_cur) * (beta + X.base(E.main(1))) - X.base(E.main(2)))
    return [fe.CircuitInputs(3, None, [], [c], [fe.Lookup.push(E.main(0), [E.main(1)])])]


def test_ext_constraint_reads_stage2_and_publics(pkg, fe, ctx, oracle):
    s = Sys(pkg, fe, ctx, oracle, ext_inputs(fe))
    assert any(nd[0] == wm.K_VAR and nd[1] == wm.SRC_STAGE2 for nd in s.comp[0].nodes) and any(nd[0] == wm.K_PUBLIC for nd in s.comp[0].nodes)
    n = 16
    rng = np.random.default_rng(3)
    args = np.repeat(rng.integers(1, 1 << 20, n // 2, dtype=np.uint64), 2)
    mult = np.array([1, P - 1] * (n // 2), dtype=np.uint64)  # every push is taken back: the channel balances
    good = np.stack([mult, args, mult], axis=1)
    bad = good.copy()
    bad[5, 2] = 3
    for bg in (BG, BG2):
        rep, _ = s.both([good], [], bg)
        assert rep.verdict == 0
        rep, _ = s.both([bad], [], bg)
        assert rep.verdict == 1 and rep.circuits[0].failing_rows == 1 and rep.circuits[0].first_failure[0] == 5


# ---------------------------------------------------------------- slot-file tiers
def chain_inputs(fe, k, extra=0, width=40):
    """k products of column pairs, all compiled before the first sum node (a right-nested sum), so that k values are live at
    once; constraint: their sum equals column `width`. extra: that many further roots z (m_i + m_j) over the all-zero column
    z = width + 1 - nodes and live roots without depth"""
    E = fe.Expr
    pairs = [(i, j) for i in range(width) for j in range(i, width)]
    assert len(pairs) >= max(k, extra)
    s = None
    for i, j in reversed(pairs[:k]):
        p = E.main(i) * E.main(j)
        s = p if s is None else p + s
    more = [E.main(width + 1) * (E.main(i) + E.main(j)) for i, j in pairs[:extra]]
    return [fe.CircuitInputs(width + 2, None, [s - E.main(width)] + more, [], [])], pairs[:k]


_CHAIN = {}


def chain_trace(pairs, n, width=40):
    key = (len(pairs), n)
    if key not in _CHAIN:
        rng = np.random.default_rng(len(pairs) + n)
        tr = rng.integers(0, 1 << 31, (n, width + 2), dtype=np.uint64)
        tot = np.zeros(n, dtype=object)
        for i, j in pairs:
            tot = (tot + tr[:, i].astype(object) * tr[:, j].astype(object)) % P
        tr[:, width] = np.array([int(v) for v in tot], dtype=np.uint64)
        tr[:, width + 1] = 0
        _CHAIN[key] = tr
    return _CHAIN[key].copy()


# check_dev.h over check.hip's 8-byte words: a slot file of s slots runs with slots in LDS at the largest of 256 / 128 / 64 lanes with (s * lanes + 24) * 8 <= 64 KB:
# 256 lanes up to s = 31, 128 up to 63, 64 up to 127. Above that: a program with a wave schedule (>= 1024 needed nodes, at most
# 160 KB of positions - a sum chain of depth 600 has none) and <= 16384 rows takes the wave-per-row form; else <= 8192 rows
# (256 workgroups of 32 lanes) with (s * 32 + 24) * 8 <= 160 KB, s <= 639, take the few-lanes form; the rest the global scratch.
@pytest.mark.parametrize("slots,extra,log_n,kernel,lanes", [
    (31, 0, 13, 1, 256), (32, 0, 13, 1, 128), (63, 0, 13, 1, 128), (64, 0, 13, 1, 64), (127, 0, 13, 1, 64),
    (128, 0, 13, 3, 32),     # few lanes: (8192 + 31) / 32 = 256 workgroups, the most that form takes
    (128, 0, 14, 4, 256),    # twice the rows: the global scratch
    (639, 0, 6, 3, 32),      # few lanes with 159.9 KB of LDS
    (640, 0, 6, 4, 256),     # one slot more: the global scratch
    (None, 450, 8, 2, 64),   # 150 live products and 450 shallow roots: >= 1024 needed nodes in ~150 levels, one wave per row
])
def test_slot_file_tiers(pkg, fe, ctx, oracle, monkeypatch, slots, extra, log_n, kernel, lanes):
    import sys

    monkeypatch.setenv("MSAMD_NO_JIT", "1")  # (the check runs no generated kernel; this spares the test their compilation)
    n = 1 << log_n
    k = slots or 150
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 4000))  # (the front-end compiles the right-nested sum recursively)
    try:
        for _ in range(3):  # the allocator needs a few slots besides the k products: find the k that gives `slots`
            inputs, pairs = chain_inputs(fe, k, extra)
            s = Sys(pkg, fe, ctx, oracle, inputs)
            info = s.dev.check_info(0)
            if slots is None or info["slots"] == slots:
                break
            k -= info["slots"] - slots
    finally:
        sys.setrecursionlimit(limit)
    assert slots is None or info["slots"] == slots
    assert info["lds_lanes"] == (lanes if kernel == 1 else 0) and (info["wave_steps"] > 0) == (kernel == 2) and info["roots"] == 1 + extra
    tr = chain_trace(pairs, n)
    tr[n - 3, 40] = (int(tr[n - 3, 40]) + 1) % P  # one bad row, in the last workgroup
    if extra:
        tr[n - 3, 41] = 1                         # ... where the shallow roots fail as well, and on the row behind it
        tr[n - 2, 41] = 1
    rep, _ = s.both([tr], [])
    c = rep.circuits[0]
    assert (c.kernel, c.lanes) == (kernel, lanes)
    assert rep.verdict == 1 and c.failing_rows == (2 if extra else 1) and c.first_failure == (n - 3, 0, P - 1)


# ---------------------------------------------------------------- other ways to make a witness, misuse
def test_witness_from_a_torch_tensor(fe, fib):
    tr = fib_trace(1 << 13)
    tr[4100, 1] = 9
    t = torch.from_numpy(np.ascontiguousarray(tr.T).view(np.int64)).cuda().T  # a column-major view of the n x 3 matrix
    assert t.shape == (1 << 13, 3) and t.stride() == (1, 1 << 13)
    w = fib.dev.witness_from_device([t], fe.pack_claims([]))
    rep, _ = fib.both([tr], [], witness=w)
    up = fib.dev.witness([tr], fe.pack_claims([])).check()
    assert [c.fields() for c in rep.circuits] == [c.fields() for c in up.circuits] and rep.verdict == up.verdict == 1


def test_misuse_is_an_error_and_the_context_stays_usable(pkg, fe, ctx, oracle, fib):
    tr = fib_trace(16)
    packed = fe.pack_claims([])
    with pytest.raises(pkg.MstarkError, match="device-resident"):
        fib.dev.host_witness([tr], packed).check()
    w = fib.dev.witness([tr], packed)
    for beta, gamma in (((P, 0), (1, 2)), ((1, 2), (3, P + 5))):
        with pytest.raises(pkg.MstarkError, match="non-canonical"):
            w.check(beta, gamma)
    eo = Sys(pkg, fe, ctx, oracle, fe.even_odd_inputs())
    remote = eo.dev.witness(fe.even_odd_traces(), fe.pack_claims([[0, 4, 1]]), remote_heights={1: 4})
    with pytest.raises(pkg.MstarkError, match="another rank"):
        remote.check()
    assert w.check().verdict == 0 and eo.dev.witness(fe.even_odd_traces(), fe.pack_claims([[0, 4, 1]])).check().verdict == 0
