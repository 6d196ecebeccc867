"""`-m gpu`: msbb_witness_check (csrc/bb_check.hip over csrc/check_dev.h) against the model of tests/witness_check_model_bb.py, which
tests/test_bb_witness_check_model.py anchors to the BabyBear oracle. Every figure of the report is deterministic and compared
exactly. References (model reports, traces) are computed once per case and left unchanged. The counterpart of
test_gpu_witness_check.py; shapes are the smallest that still reach the code named."""
import re
import sys

import numpy as np
import pytest
import torch  # (before the library opens the device: test_witness_from_a_torch_tensor)

import oracle_bb as ob
import witness_check_model_bb as wm
from test_bb_witness_check_model import BG, BG2, K, bb, bb_traces, compile_system, fe, pack, pkg, selector_inputs, selector_trace

pytestmark = pytest.mark.gpu
P = wm.P


@pytest.fixture(scope="module")
def ctx():
    c = pkg.Context(0)
    bb.set_poseidon2(c, K)
    ob.set_poseidon2(K)
    return c


class Sys:
    """one system on the device and in the oracle"""

    def __init__(self, ctx, inputs, params=None):
        self.blob, self.comp, self.params = compile_system(inputs, params)
        self.dev = bb.System(ctx, self.blob, len(self.comp))
        self.osys = ob.System(self.blob)

    def model(self, traces, claims, bg=BG):
        return wm.check(ob, self.osys, self.comp, traces, pack(claims), *bg)

    def both(self, traces, claims, bg=BG, witness=None):
        """device report (of `witness`, default: the uploaded traces) and model report, compared in every field"""
        w = witness or self.dev.witness(traces, pack(claims))
        rep = w.check(*bg)
        m = self.model(traces, claims, bg)
        assert rep.verdict == m.verdict, (rep.verdict, m.verdict, str(rep))
        assert rep.ok == m.ok and rep.final_accumulator == m.final_accumulator
        for i, (d, c) in enumerate(zip(rep.circuits, m.circuits)):
            assert d.fields() == c.fields(), ("circuit %d" % i, d.fields(), c.fields())
        return rep, w


def bb_inputs(name):
    with fe.field(fe.BABYBEAR):
        return getattr(fe, name)()


def fib_inputs():
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
def fib(ctx):
    return Sys(ctx, fib_inputs())


# ---------------------------------------------------------------- clean witnesses
@pytest.mark.parametrize("rows", [4, 1])  # 4: the reference's own rows; 1: the smallest height (w = 1, is_first and is_last on one row)
def test_clean_mul_air(ctx, rows):
    s = Sys(ctx, bb_inputs("mul_air_inputs"))
    rep, _ = s.both([bb_traces("mul_air")[0][:rows].copy()], [])
    assert rep.ok and rep.verdict == 0 and rep.circuits[0].height == rows and "satisfies" in str(rep)
    assert rep.circuits[0].kernel == 1 and rep.circuits[0].roots == 1 and len(rep.circuits[0].accumulator) == 4


def test_clean_even_odd_with_claim(ctx):
    s = Sys(ctx, bb_inputs("even_odd_inputs"))
    for bg in (BG, BG2):
        rep, _ = s.both(bb_traces("even_odd"), [[0, 4, 1]], bg)
        assert rep.verdict == 0 and [c.height for c in rep.circuits] == [4, 4]
        assert any(rep.circuits[0].accumulator) and rep.circuits[1].accumulator == (0, 0, 0, 0)


def test_clean_mul_air_many_workgroups(ctx):
    s = Sys(ctx, bb_inputs("mul_air_inputs"))
    rep, _ = s.both(bb_traces("mul_air", 1 << 13), [])
    assert rep.verdict == 0 and (rep.circuits[0].kernel, rep.circuits[0].lanes) == (1, 256)


# ---------------------------------------------------------------- one cell off
@pytest.mark.parametrize("row,col", [(0, 0), (0, 2), ((1 << 13) - 1, 1), ((1 << 13) - 1, 2), (4100, 1)],
                         ids=["row0", "row0_wrap_column", "last_row", "last_row_wrap_column", "middle"])
def test_one_cell_off(fib, row, col):
    n = 1 << 13  # 32 workgroups of 256 rows
    tr = fib_trace(n)
    tr[row, col] = (int(tr[row, col]) + 5) % P
    rep, w = fib.both([tr], [])
    c = rep.circuits[0]
    assert rep.verdict == 1 and 1 <= c.failing_rows <= 2 and c.first_failure is not None
    if col == 2:  # the column without a selector: the row in front reads the cell as its next row - for row 0 that is row n - 1
        assert sorted(int(x) for x in c.root_first if x != wm.NONE) == [min(row, (row - 1) % n)] and c.failing_rows == 2
    packed = pack([])
    assert fib.dev.verify_multiple_claims(packed, fib.dev.prove_multiple_claims(w).to_bytes()) != 0
    text = str(rep)
    assert re.search(r"circuit 0: constraint root \d+ non-zero on \d+ rows, first at row %d \(value 0x[0-9a-f]{16}\)" % c.first_failure[0], text), text


def test_check_between_two_proofs_does_not_change_the_proof(fib):
    tr = fib_trace(1 << 13)
    packed = pack([])
    w = fib.dev.witness([tr], packed)
    before = fib.dev.prove_multiple_claims(w).to_bytes()
    rep, _ = fib.both([tr], [], witness=w)
    assert rep.verdict == 0
    after = fib.dev.prove_multiple_claims(w).to_bytes()
    assert before == after and fib.dev.verify_multiple_claims(packed, after) == 0 and fib.osys.verify(packed, after) == 0


def test_named_report(fib):
    tr = fib_trace(16)
    tr[3, 1] += 1
    rep = fib.dev.witness([tr], pack([])).check(names=["Fib"], origins=[fib.comp[0].zero_origins])
    assert re.search(r"circuit 0 \(Fib\): constraint \d \(root \d\) non-zero on 2 rows, first at row 2 \(value 0x", str(rep)), str(rep)


def test_every_row_fails(fib):
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
def test_selector_polynomials(ctx, n):
    s = Sys(ctx, selector_inputs())
    rep, _ = s.both([selector_trace(n, True)], [])
    assert rep.verdict == 0
    rep, _ = s.both([selector_trace(n, False)], [])
    c = rep.circuits[0]
    assert rep.verdict == 1 and c.first_failure == (0, 0, (1 - n) % P) and int(c.root_first[1]) == n - 1


# ---------------------------------------------------------------- lookups
def test_lookup_balance(ctx):
    s = Sys(ctx, bb_inputs("even_odd_inputs"))
    for bg in (BG, BG2):
        rep, _ = s.both(bb_traces("even_odd"), [[0, 4, 1]], bg)
        assert rep.verdict == 0 and rep.final_accumulator == (0, 0, 0, 0)
        for claims in ([[0, 4, 0]], []):
            rep, _ = s.both(bb_traces("even_odd"), claims, bg)
            assert rep.verdict == pkg.CHECK_LOOKUPS and "lookups unbalanced" in str(rep) and rep.final_accumulator != (0, 0, 0, 0)
            assert re.search(r"ends at \((0x[0-9a-f]{16}, ){3}0x[0-9a-f]{16}\)$", str(rep)), str(rep)
            assert not any(c.failing_rows or any(int(x) for x in c.root_counts) for c in rep.circuits)


def ext_inputs():
    """the logUp step written again as a user's extension constraint, with the multiplicity read from ANOTHER column (m2):
    is_transition ((S' - S)(beta + m1) - m2), S = the four stage-2 coordinates (this and the next row), beta = publics 0..3"""
    with fe.field(fe.BABYBEAR):
        E, X = fe.Expr, fe.ExtExpr
        s_cur, s_next = X.coords([E.var(2, 0, k) for k in range(4)]), X.coords([E.var(2, 1, k) for k in range(4)])
        beta = X.coords([E.public(k) for k in range(4)])
        c = X.base(fe.IS_TRANSITION) * ((s_next - s_cur) * (beta + X.base(E.main(1))) - X.base(E.main(2)))
        return [fe.CircuitInputs(3, None, [], [c], [fe.Lookup.push(E.main(0), [E.main(1)])])]


def test_ext_constraint_reads_stage2_and_publics(ctx):
    s = Sys(ctx, ext_inputs())
    nodes = s.comp[0].nodes
    assert {nd[3] for nd in nodes if nd[0] == wm.K_VAR and nd[1] == wm.SRC_STAGE2} == {0, 1, 2, 3}  # all four coordinates
    assert {nd[3] for nd in nodes if nd[0] == wm.K_PUBLIC} >= {0, 1, 2, 3} and len(s.comp[0].zeros) == 4
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
def chain_inputs(k, extra=0, width=40):
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


def chain_trace(pairs, n, width):
    key = (len(pairs), n, width)
    if key not in _CHAIN:
        rng = np.random.default_rng(len(pairs) + n)
        tr = rng.integers(0, P, (n, width + 2), dtype=np.uint64)
        tot = np.zeros(n, dtype=np.uint64)
        for i, j in pairs:
            tot = (tot + tr[:, i] * tr[:, j] % np.uint64(P)) % np.uint64(P)
        tr[:, width] = tot
        tr[:, width + 1] = 0
        _CHAIN[key] = tr
    return _CHAIN[key].copy()


# check_dev.h over bb_check.hip's 4-byte words: a slot file of s 4-byte slots runs with slots in LDS at the largest of 256 / 128 / 64 lanes with
# s * lanes * 4 + 192 <= 64 KB: 256 lanes up to s = 63, 128 up to 127, 64 up to 255. Above that: a program with a wave schedule
# (>= 1024 needed nodes, at most 160 KB of 8-byte positions - a sum chain of depth 1278 has none) and <= 16384 rows takes the
# wave-per-row form; else <= 8192 rows (256 workgroups of 32 lanes) with s * 128 + 192 <= 160 KB, s <= 1278, take the few-lanes
# form; the rest the global scratch.
@pytest.mark.parametrize("slots,extra,log_n,width,kernel,lanes", [
    (63, 0, 13, 40, 1, 256), (64, 0, 13, 40, 1, 128), (127, 0, 13, 40, 1, 128), (128, 0, 13, 40, 1, 64), (255, 0, 13, 40, 1, 64),
    (256, 0, 13, 40, 3, 32),     # few lanes: (8192 + 31) / 32 = 256 workgroups, the most that form takes
    (256, 0, 14, 40, 4, 256),    # twice the rows: the global scratch
    (1278, 0, 6, 60, 3, 32),     # few lanes with 159.9 KB of LDS
    (1279, 0, 6, 60, 4, 256),    # one slot more: the global scratch
    (None, 450, 8, 40, 2, 64),   # 260 live products and 450 shallow roots: >= 1024 needed nodes in ~260 levels, one wave per row
])
def test_slot_file_tiers(ctx, monkeypatch, slots, extra, log_n, width, kernel, lanes):
    monkeypatch.setenv("MSAMD_NO_JIT", "1")  # (the check runs no generated kernel; this spares the test their compilation)
    n = 1 << log_n
    k = slots or 260
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 12000))  # (the front-end compiles the right-nested sum recursively)
    try:
        for _ in range(3):  # the allocator needs a few slots besides the k products: find the k that gives `slots`
            inputs, pairs = chain_inputs(k, extra, width)
            s = Sys(ctx, inputs)
            info = s.dev.check_info(0)
            if slots is None or info["slots"] == slots:
                break
            k -= info["slots"] - slots
    finally:
        sys.setrecursionlimit(limit)
    assert slots is None or info["slots"] == slots
    assert slots is not None or info["slots"] > 255  # (the wave form is reached only where the thread-per-row LDS form does not fit)
    assert info["lds_lanes"] == (lanes if kernel == 1 else 0) and (info["wave_steps"] > 0) == (kernel == 2) and info["roots"] == 1 + extra
    tr = chain_trace(pairs, n, width)
    tr[n - 3, width] = (int(tr[n - 3, width]) + 1) % P  # one bad row, in the last workgroup
    if extra:
        tr[n - 3, width + 1] = 1                        # ... where the shallow roots fail as well, and on the row behind it
        tr[n - 2, width + 1] = 1
    rep, _ = s.both([tr], [])
    c = rep.circuits[0]
    assert (c.kernel, c.lanes) == (kernel, lanes)
    assert rep.verdict == 1 and c.failing_rows == (2 if extra else 1) and c.first_failure == (n - 3, 0, P - 1)


# ---------------------------------------------------------------- other ways to make a witness, host waits, misuse
def test_witness_from_a_torch_tensor(fib):
    tr = fib_trace(1 << 13)
    tr[4100, 1] = 9
    t = torch.from_numpy(np.ascontiguousarray(tr.T).astype(np.uint32).view(np.int32)).cuda().T  # a column-major view of the n x 3 matrix
    assert t.shape == (1 << 13, 3) and t.stride() == (1, 1 << 13)
    w = fib.dev.witness_from_device([t], pack([]))
    rep, _ = fib.both([tr], [], witness=w)
    up = fib.dev.witness([tr], pack([])).check()
    assert [c.fields() for c in rep.circuits] == [c.fields() for c in up.circuits] and rep.verdict == up.verdict == 1


def test_one_host_wait_whatever_the_number_of_circuits(ctx):
    inputs, traces = bb_inputs("even_odd_inputs"), bb_traces("even_odd")
    waits = []
    for k in (1, 2):  # the Even circuit alone, then Even and Odd; one claim each time
        s = Sys(ctx, inputs[:k])
        w = s.dev.witness(traces[:k], pack([[0, 4, 1]]))
        w.check()  # (no check program is left to build)
        before = ctx.sync_count()
        rep = w.check()
        waits.append(ctx.sync_count() - before)
        assert rep.verdict == (0 if k == 2 else pkg.CHECK_LOOKUPS)
    assert waits == [1, 1]


def test_misuse_is_an_error_and_the_context_stays_usable(fib):
    tr = fib_trace(16)
    packed = pack([])
    with pytest.raises(pkg.MstarkError, match="device-resident"):
        fib.dev.host_witness([tr], packed).check()
    w = fib.dev.witness([tr], packed)
    for beta, gamma in (((P, 0, 0, 0), (1, 2, 3, 4)), ((1, 2, 3, 4), (3, 0, 0, P)), ((1, 2, P + 5, 4), (1, 2, 3, 4))):
        with pytest.raises(pkg.MstarkError, match="non-canonical"):
            w.check(beta, gamma)
    assert w.check().verdict == 0
