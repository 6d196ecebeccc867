"""Differential tests of the kernels quotient_jit.hip GENERATES per circuit and compiles with hiprtc at System creation -
the default path of every proof - on circuits authored to cross each branch of the five generators, the fallback thresholds
of the *_build functions and the disk cache of code objects.

Every case (1) asserts System.circuit_kernels first: a missing hiprtc, a failed compile or a moved threshold fails the test
instead of comparing the interpreter with itself (so that no test here can pass under an exported MSAMD_NO_JIT=1); (2) compares
with the oracle, exactly - everything is integer arithmetic; (3) builds the same blob again under MSAMD_NO_JIT=1 (flags 0)
and compares the interpreter kernels too, which only tells a generator fault from a shared one.

Which kernel a proof runs: a witness made from traces alone (System.witness or System.host_witness) runs the from-trace
stage-2 kernel whenever the circuit has one; the terms kernel fed by lookup values (plain or grouped) runs when the witness
carries explicit lookup values (System.witness(..., lookups=...); here the oracle's) or when there is no from-trace kernel."""
import hashlib
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

from __graft_entry__ import load_package
from conftest import P, rand_field

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_BB = (1 << 31) - (1 << 27) + 1
_pkg = load_package()
# the ctypes mirror's names of the MS_KERNEL_* bits; system_pair checks them against include/mstark.h
Q, Q_INL, S2, S2_GRP, S2_TR = (_pkg.KERNEL_QUOTIENT, _pkg.KERNEL_QUOTIENT_INLINE, _pkg.KERNEL_STAGE2, _pkg.KERNEL_STAGE2_GROUPED,
                               _pkg.KERNEL_STAGE2_TRACE)
HEADER = {k: int(v.rstrip("u"), 0) for k, v in re.findall(r"#define (MS_KERNEL_\w+) (\w+)", open(os.path.join(ROOT, "include", "mstark.h")).read())}

NEW_SECONDS = []  # (seconds, label) of every System creation with the generators on: `pytest -s` prints the slowest at the end


@pytest.fixture(scope="module", autouse=True)
def _cold_cache_and_compile_times(tmp_path_factory):
    """every kernel of this file is generated and compiled here: the code objects go to an empty MSAMD_JIT_CACHE, not to
    the package's persistent one, so the times below are cold ones (identical sources are still compiled once per process)"""
    mp = pytest.MonkeyPatch()
    mp.setenv("MSAMD_JIT_CACHE", str(tmp_path_factory.mktemp("jit_cache")))
    yield
    mp.undo()
    for s, label in sorted(NEW_SECONDS, reverse=True)[:12]:
        print("\n[generated kernels] System creation %-28s %6.2f s" % (label, s), end="")


def grouped(G):
    return S2 | S2_GRP | (G << HEADER["MS_KERNEL_STAGE2_GROUPS_SHIFT"])


def system_pair(pkg, ctx, monkeypatch, blob, n, want_flags, label, bb=False):
    """(system with generated kernels, the same blob under MSAMD_NO_JIT=1); the flags are asserted before anything runs"""
    assert [Q, Q_INL, S2, S2_GRP, S2_TR] == [HEADER["MS_KERNEL_" + k] for k in ("QUOTIENT", "QUOTIENT_INLINE", "STAGE2", "STAGE2_GROUPED", "STAGE2_TRACE")]
    assert pkg.kernel_groups(grouped(16)) == 16 and pkg.kernel_groups(S2) == 0 and HEADER["MS_KERNEL_STAGE2_GROUPS_MASK"] == 0x1F
    cls = pkg.babybear.System if bb else pkg.System
    t0 = time.time()
    g = cls(ctx, blob, n)
    NEW_SECONDS.append((time.time() - t0, label))
    got = [g.circuit_kernels(ci) for ci in range(n)]
    assert got == list(want_flags), "%s: circuit_kernels %s, expected %s" % (label, [hex(x) for x in got], [hex(x) for x in want_flags])
    monkeypatch.setenv("MSAMD_NO_JIT", "1")
    try:
        interp = cls(ctx, blob, n)
    finally:
        monkeypatch.delenv("MSAMD_NO_JIT")
    assert [interp.circuit_kernels(ci) for ci in range(n)] == [0] * n
    return g, interp


def live_and_dead(fe, c):
    """(used, unused) node counts of a compiled circuit, as the generators' needed[] sees them"""
    need = set(c.zeros)
    for m, args in c.lookups:
        need |= {m, *args}
    for i in range(len(c.nodes) - 1, -1, -1):
        kind, _, _, a, b = c.nodes[i]
        if i in need and kind in (fe.N_ADD, fe.N_SUB, fe.N_MUL, fe.N_NEG):
            need |= {a} if kind == fe.N_NEG else {a, b}
    return len(need), len(c.nodes) - len(need)


# ------------------------------------------------------------------ a) the quotient kernel, at the kernel level
def q_constraints(fe, n):
    """no lookups, n distinct user constraints of degree 2 (constraint count n + 2: the L == 0 pass-through is folded after them)"""
    E = fe.Expr

    def ev(b):
        m, mn = b.main()
        for k in range(n):
            b.assert_zero(m[k % 3] * mn[(k + 1) % 3] - E.const(k + 1))

    return fe.lookup_air(3, ev, [])


def q_lookups(fe, counts, zeros=0):
    """one lookup per entry of `counts` with that many arguments (distinct degree-1 expressions), `zeros` user constraints"""
    E = fe.Expr
    lookups = [fe.Lookup.push(E.main(j % 4), [E.main((j + k) % 4) + E.const(k) for k in range(na)]) for j, na in enumerate(counts)]

    def ev(b):
        m, mn = b.main()
        for k in range(zeros):
            b.assert_zero(m[k % 4] * mn[(k + 1) % 4] - E.const(k + 1))

    return fe.lookup_air(4, ev, lookups)


def q_mixed_operands(fe, pre_h=2):
    """ONE live constraint with: main and main-next of the same column, preprocessed current and next, the constants P-1 and
    2^63 (printed as ...ULL; over BabyBear P_bb - 1 and 2^63 mod P_bb), a negated selector, when_first_row + when_last_row + when_transition - and a constraint that
    folds to zero at compile time, whose nodes stay in the program unused (dead-node elimination, needed[])"""
    E = fe.Expr

    def ev(b):
        m, mn = b.main()
        p, pn = b.preprocessed()
        x = (m[0] * mn[0] - p[0] * pn[0]) * E.const(fe.P - 1) + E.const(1 << 63) * (-b.is_last_row()) * m[1] + p[1] - pn[1]
        b.when_first_row().when_last_row().when_transition().assert_zero(x)

        def dead():
            e = E.const(0)
            for k in range(24):
                e = e + (m[0] + E.const(100 + k)) * (mn[1] + E.const(200 + k))
            return e

        b.assert_zero(dead() - dead())  # sub(a, a) folds to the constant 0: no constraint, 140 nodes nobody reads

    return fe.lookup_air(2, ev, [], (np.arange(2 * pre_h, dtype=np.uint64).reshape(pre_h, 2) * np.uint64(0x9E3779B1) + np.uint64(5)) % np.uint64(fe.P))


def q_degree(fe, deg):
    E = fe.Expr

    def ev(b):
        m, mn = b.main()
        x = m[0]
        for k in range(1, deg):
            x = x * m[k]
        b.assert_zero(x - mn[0] + E.const(5))

    return fe.lookup_air(max(deg, 2), ev, [])


MIXED16 = [0, 1, 2, 3, 5, 8, 13, 21, 31, 32, 33, 33, 4, 6, 7, 9]
QUOTIENT_CASES = {
    # name: (builder, expected flags, expected quotient degree)
    "zeros1": (lambda fe, pre_h=2: q_constraints(fe, 1), Q | Q_INL, 1),  # circuit_source: L == 0 pass-through next to a user constraint
    # inline_tables_fit: constraint count = zeros + 2 <= QP_INLINE_ALPHA (64): 62 user constraints inline, 63 not (p.zh[qi])
    "zeros62": (lambda fe, pre_h=2: q_constraints(fe, 62), Q | Q_INL, 1),
    "zeros63": (lambda fe, pre_h=2: q_constraints(fe, 63), Q, 1),
    "zeros64": (lambda fe, pre_h=2: q_constraints(fe, 64), Q, 1),
    "zeros65": (lambda fe, pre_h=2: q_constraints(fe, 65), Q, 1),  # GlAccS, the split alpha-fold accumulator, at 67 terms
    "lookup_args0": (lambda fe, pre_h=2: q_lookups(fe, [0]), Q | Q_INL | S2 | S2_TR, 1),
    "lookup_args1": (lambda fe, pre_h=2: q_lookups(fe, [1]), Q | Q_INL | S2 | S2_TR, 1),
    "lookup_args32": (lambda fe, pre_h=2: q_lookups(fe, [32]), Q | Q_INL | S2 | S2_TR, 1),  # GlAcc dot product with QDyn::gpow[32], all of it
    "lookup_args33": (lambda fe, pre_h=2: q_lookups(fe, [33]), Q | Q_INL | S2 | S2_TR, 1),  # more than gpow holds: the Horner fingerprint
    "lookups16_mixed": (lambda fe, pre_h=2: q_lookups(fe, MIXED16, zeros=3), Q | Q_INL | S2 | S2_TR, 1),
    "mixed_operands": (q_mixed_operands, Q | Q_INL, 4),
    "degree1": (lambda fe, pre_h=2: q_degree(fe, 1), Q | Q_INL, 1),
    "degree9": (lambda fe, pre_h=2: q_degree(fe, 9), Q | Q_INL, 8),  # the highest the front end accepts at log_blowup 3 (quotient degree 8)
}


@pytest.mark.parametrize("name", list(QUOTIENT_CASES))
def test_quotient_kernel(pkg, ctx, oracle, fe, monkeypatch, name):
    build, flags, qdeg = QUOTIENT_CASES[name]
    compiled = fe.compile_circuit(build(fe))
    if name == "mixed_operands":
        live, dead = live_and_dead(fe, compiled)
        assert dead >= live and len(compiled.zeros) == 1, (live, dead)
    blob = fe.system_blob(fe.Params(3, 0, 0, 1, 1, 0, 0), [compiled])
    g, interp = system_pair(pkg, ctx, monkeypatch, blob, 1, [flags], name)
    o = oracle.System(blob)
    info = g.circuit_info(0)
    assert info == o.circuit_info(0) and info["quotient_degree"] == qdeg
    lq = qdeg.bit_length() - 1
    rng = np.random.default_rng(sum(name.encode()))
    for ln in (0, 1, 3, 6):
        N = 1 << (ln + lq)
        shapes = [(N, info["pre_width"]), (N, info["main_width"]), (N, info["stage2_width"]), 8, 2]
        sets = {
            "random": [rand_field(rng, s) for s in shapes],
            # every operand P-1: the Horner chain (33 arguments), GlAcc (32) and GlAccS (65+ constraints) at their largest terms
            "all P-1": [np.full(s, P - 1, dtype=np.uint64) for s in shapes],
            "all zero": [np.zeros(s, dtype=np.uint64) for s in shapes],
        }
        for what, (pre, s1, s2, publics, alpha) in sets.items():
            pre = pre if info["pre_width"] else None
            want = oracle.quotient_values(o, 0, publics, ln, lq, pre, s1, s2, alpha)
            got = g.quotient_values(0, publics, ln, lq, pre, s1, s2, alpha)
            ref = interp.quotient_values(0, publics, ln, lq, pre, s1, s2, alpha)
            assert np.array_equal(got, want), "%s, log_n %d, %s: generated kernel differs from the oracle (interpreter %s)" % (
                name, ln, what, "agrees with the oracle" if np.array_equal(ref, want) else "differs too")
            assert np.array_equal(ref, want), "%s, log_n %d, %s: interpreter differs from the oracle" % (name, ln, what)


# ------------------------------------------------------------------ b) the stage-2 kernels, through the prover
def s2_circuit(fe, w, counts, cols=None, pre=None, selectors=False, public_arg=False):
    """`len(counts)` lookups over the main columns `cols` (default: all `w`), lookup j with counts[j] arguments; every third
    argument reads the NEXT row (the wrap at the last row: rn = 0, at height 1 the row itself). pre: also read a preprocessed
    column, this row and the next. selectors: is_first / is_last / is_trans in multiplicities and in an argument."""
    E = fe.Expr
    cols = list(range(w)) if cols is None else cols
    sel = [fe.IS_FIRST_ROW, fe.IS_LAST_ROW, fe.IS_TRANSITION]
    lookups = []
    for j, na in enumerate(counts):
        mult = E.main(cols[j % len(cols)])
        if selectors:
            mult = mult * sel[j % 3]
        args = []
        for k in range(na):
            c = cols[(j + k) % len(cols)]
            a = E.main_next(c) if k % 3 == 2 else E.main(c) + E.const(k)
            if pre is not None and k % 2 == 0:
                a = a + E.var(fe.SRC_PRE, (k // 2) % 2, k % pre.shape[1])
            if selectors and k == 1:
                a = a + sel[(j + 1) % 3]
            if public_arg and k == 0:
                a = a + E.public(j % 4)
            args.append(a)
        lookups.append(fe.Lookup.push(mult, args) if j % 2 else fe.Lookup.pull(mult, args))

    def ev(b):
        m, mn = b.main()
        b.assert_zero(m[0] * mn[0] - m[w - 1])

    return fe.lookup_air(w, ev, lookups, pre)


def prove_all_ways(pkg, g, interp, o, traces, packed, what, explicit=True):
    """the oracle's proof against: a device-resident and a host-resident witness from the traces (from-trace kernel), a witness
    with the oracle's lookup values (terms kernel), and the interpreter system. A witness the oracle refuses (a zero message
    has no inverse) must be refused by every one of them."""
    ways = {"witness": lambda s: s.witness(traces, packed), "host_witness": lambda s: s.host_witness(traces, packed)}
    if explicit:
        ways["witness with lookup values"] = lambda s: s.witness(traces, packed, lookups=[
            o.compute_lookup_values(ci, t) if len(t) else (np.zeros((0, 1), dtype=np.uint64),) * 2 for ci, t in enumerate(traces)])
    try:
        want = o.prove(traces, packed)
    except RuntimeError:
        for s in (g, interp):
            for way, make in ways.items():
                with pytest.raises(pkg.MstarkError):
                    s.prove_multiple_claims(make(s))
        return None
    ref = interp.prove_multiple_claims(interp.witness(traces, packed)).to_bytes()
    for way, make in ways.items():
        got = g.prove_multiple_claims(make(g)).to_bytes()
        assert got == want, "%s, %s: proof differs from the oracle's (the interpreter's %s)" % (what, way, "agrees" if ref == want else "differs too")
    assert ref == want, "%s: the interpreter's proof differs from the oracle's" % what
    return want


STAGE2_CASES = {
    # name: (main width, argument counts, columns read, expected stage-2 bits)
    # stage2_source: plain mode up to 32 lookups (two batches of 16)
    "L1_no_args": (1, [0], None, S2),                    # a lookup of 0 arguments; odd main width; one (partial) batch
    "L15_odd_width": (3, [1] * 15, None, S2),            # odd total argument width (scalar loads), odd main width, batch of 15
    # even widths: ulonglong2 loads of the arguments in stage2_source; in stage2_trace_source the pair loads of the trace row, of
    # which only the odd column of each pair is used
    "L16_odd_columns": (4, [1] * 16, [1, 3], S2),
    "L17_args64": (2, [64] + [1] * 16, None, S2),        # a 64-argument lookup (MAX_GPOW); a last batch of one lookup
    "L32_odd_width": (5, [1] * 31 + [2], None, S2),      # the last plain size: G = 2 is not grouped
    # stage2_grouped_source: from 33 lookups a wave takes a group of 16
    "L33": (4, [1] * 33, None, grouped(3)),              # G = 3, a last group of one lookup
    "L48": (3, [1] * 48, None, grouped(3)),              # G = 3, three whole groups
    "L49": (2, [2] * 49, None, grouped(4)),              # G = 4, a last group of one lookup
}
# 1: the next row is the row itself (rn = 0); 1 and 2: fewer than 64 rows, the `live` mask of the grouped kernel; 64: one whole
# wave per group; 128: a second workgroup of the grouped kernel; 512: a second workgroup of the 256-thread kernels
HEIGHTS = (1, 2, 64, 128, 512)


@pytest.mark.parametrize("name", list(STAGE2_CASES))
def test_stage2_kernels(pkg, ctx, oracle, fe, monkeypatch, name):
    w, counts, cols, s2_bits = STAGE2_CASES[name]
    blob = fe.system_blob(fe.test_params(), [fe.compile_circuit(s2_circuit(fe, w, counts, cols))])
    g, interp = system_pair(pkg, ctx, monkeypatch, blob, 1, [Q | (Q_INL if 1 + 2 * len(counts) <= 64 else 0) | s2_bits | S2_TR], name)
    o = oracle.System(blob)
    assert g.circuit_info(0) == o.circuit_info(0) and g.circuit_info(0)["args_width"] == sum(counts)
    rng = np.random.default_rng(len(counts))
    packed = fe.pack_claims([[1, 2, 3]])
    proved = 0
    for h in HEIGHTS:
        # random multiplicities and arguments; then every main entry P-1
        for what, trace in (("random", rand_field(rng, (h, w))), ("all P-1", np.full((h, w), P - 1, dtype=np.uint64))):
            proved += prove_all_ways(pkg, g, interp, o, [trace], packed, "%s, height %d, %s" % (name, h, what)) is not None
    assert proved >= len(HEIGHTS)  # (refusals are legitimate, but not as the only thing this test ever sees)


def test_stage2_preprocessed_and_selectors(pkg, ctx, oracle, fe, monkeypatch):
    """two circuits: lookups over preprocessed columns (odd preprocessed width: scalar loads; this row and the next), and
    is_first / is_last / is_trans inside multiplicities and arguments (stage2_trace_source's selector locals); 20 lookups
    each, so that the second batch is a partial one in both kernels"""
    rng = np.random.default_rng(77)
    pre = rand_field(rng, (64, 3))
    circuits = [s2_circuit(fe, 2, [3] * 20, pre=pre), s2_circuit(fe, 3, [2] * 20, selectors=True)]
    blob = fe.system_blob(fe.test_params(), [fe.compile_circuit(c) for c in circuits])
    g, interp = system_pair(pkg, ctx, monkeypatch, blob, 2, [Q | Q_INL | S2 | S2_TR] * 2, "pre + selectors")
    o = oracle.System(blob)
    packed = fe.pack_claims([])
    for h in (1, 2, 128):
        traces = [rand_field(rng, (64, 2)), rand_field(rng, (h, 3))]
        assert prove_all_ways(pkg, g, interp, o, traces, packed, "pre + selectors, second height %d" % h) is not None
    traces = [np.full((64, 2), P - 1, dtype=np.uint64), np.zeros((0, 3), dtype=np.uint64)]  # the second circuit inactive
    prove_all_ways(pkg, g, interp, o, traces, packed, "pre + selectors, all P-1, second circuit inactive")


def test_stage2_top_group_count(pkg, ctx, oracle, fe, monkeypatch):
    """241 lookups: the top of the grouped kernel (G = 16: 1024-thread workgroups, a last group of one lookup), with empty
    argument lists. The issue's first choice, 256 lookups of one argument, takes 86 s of hiprtc cold (quotient 24 s, terms
    39 s, from-trace 23 s), over its own bound of 20 s, so 241 stands in as it prescribes (72 s: 26 + 23 + 23). The case
    of 257 lookups (no stage-2 kernels) is left out as prescribed: its quotient kernel alone compiles for 24 s. Times are
    those of the three *_jit_build calls with an empty cache, taken without a device."""
    L = 241
    blob = fe.system_blob(fe.test_params(), [fe.compile_circuit(s2_circuit(fe, 3, [0] * L))])
    g, interp = system_pair(pkg, ctx, monkeypatch, blob, 1, [Q | grouped(16) | S2_TR], "L = %d" % L)
    o = oracle.System(blob)
    rng = np.random.default_rng(L)
    for h in (2, 128):
        assert prove_all_ways(pkg, g, interp, o, [rand_field(rng, (h, 3))], fe.pack_claims([]), "L = %d, height %d" % (L, h)) is not None


# ------------------------------------------------------------------ c) the fallback thresholds of the *_build functions
@pytest.mark.parametrize("counts,s2_bits", [
    ([64], S2 | S2_TR), ([65], 0),                                    # MAX_GPOW arguments in one lookup: 64 inside, 65 outside
    ([64] * 16, S2 | S2_TR), ([64] * 16 + [1], 0),                    # total argument width 1024 inside, 1025 outside
], ids=["args64", "args65", "aw1024", "aw1025"])
def test_stage2_argument_limits(pkg, ctx, oracle, fe, monkeypatch, counts, s2_bits):
    blob = fe.system_blob(fe.test_params(), [fe.compile_circuit(s2_circuit(fe, 4, counts))])
    g, interp = system_pair(pkg, ctx, monkeypatch, blob, 1, [Q | Q_INL | s2_bits], "arguments %d" % sum(counts))
    o = oracle.System(blob)
    rng = np.random.default_rng(sum(counts))
    for h in (1, 64):
        assert prove_all_ways(pkg, g, interp, o, [rand_field(rng, (h, 4))], fe.pack_claims([[7]]), "%d arguments, height %d" % (sum(counts), h)) is not None


def test_public_input_in_a_lookup_argument(pkg, ctx, oracle, fe, monkeypatch):
    """a public input in the lookup prefix: no from-trace kernel (there are no publics at witness time), the terms kernel and the
    quotient kernel (p.dyn->publics[]) are generated. The reference cannot build such a witness from the traces, so neither the
    oracle nor the library may. With lookup values handed in the terms kernel runs: same proof as the interpreter system's (no
    such proof can verify - the arguments the quotient evaluates contain beta and gamma, which no witness can know - and the
    oracle has no prover for handed-in values; the terms kernel's source depends on the argument counts alone, and the oracle
    judges it in every case above). A stage-2 column in the lookup prefix is the other content limit of stage2_trace_jit_build:
    the front end refuses to author one, so that program is written by hand."""
    blob = fe.system_blob(fe.test_params(), [fe.compile_circuit(s2_circuit(fe, 2, [2] * 5, public_arg=True))])
    g, interp = system_pair(pkg, ctx, monkeypatch, blob, 1, [Q | Q_INL | S2], "public in a lookup")
    o = oracle.System(blob)
    rng = np.random.default_rng(5)
    info = g.circuit_info(0)
    for ln in (0, 3):
        N = 1 << ln
        s1, s2, publics, alpha = rand_field(rng, (N, 2)), rand_field(rng, (N, info["stage2_width"])), rand_field(rng, 8), rand_field(rng, 2)
        want = oracle.quotient_values(o, 0, publics, ln, 0, None, s1, s2, alpha)
        assert np.array_equal(g.quotient_values(0, publics, ln, 0, None, s1, s2, alpha), want)
        assert np.array_equal(interp.quotient_values(0, publics, ln, 0, None, s1, s2, alpha), want)
    trace, packed = rand_field(rng, (64, 2)), fe.pack_claims([])
    with pytest.raises(RuntimeError):
        o.prove([trace], packed)
    for s in (g, interp):
        with pytest.raises(pkg.MstarkError):
            s.prove_multiple_claims(s.witness([trace], packed))
        with pytest.raises(pkg.MstarkError):
            s.prove_multiple_claims(s.host_witness([trace], packed))
    values = [(rand_field(rng, (64, 5)), rand_field(rng, (64, 10)))]
    got = g.prove_multiple_claims(g.witness([trace], packed, lookups=values)).to_bytes()
    assert got == interp.prove_multiple_claims(interp.witness([trace], packed, lookups=values)).to_bytes()
    # lookup: multiplicity main[0], one argument = stage-2 column 0
    nodes = [(fe.N_VAR, fe.SRC_MAIN, 0, 0, 0), (fe.N_VAR, fe.SRC_STAGE2, 0, 0, 0)]
    blob = fe.system_blob(fe.test_params(), [fe.CompiledCircuit(nodes, [], [(0, [1])], 1, None)])
    g, interp = system_pair(pkg, ctx, monkeypatch, blob, 1, [Q | Q_INL | S2], "stage-2 column in a lookup")
    trace = rand_field(rng, (8, 1))
    with pytest.raises(RuntimeError):
        oracle.System(blob).prove([trace], packed)
    for s in (g, interp):
        with pytest.raises(pkg.MstarkError):
            s.prove_multiple_claims(s.witness([trace], packed))


def chain_circuit(fe, n_nodes, prefix=0):
    """a node program of exactly n_nodes: two columns, then a chain of additions (cheap to compile, every node live), its end
    the one constraint. prefix: one lookup whose multiplicity is node prefix - 1, so that the lookup prefix has that length"""
    nodes = [(fe.N_VAR, fe.SRC_MAIN, 0, 0, 0), (fe.N_VAR, fe.SRC_MAIN, 0, 1, 0)]
    while len(nodes) < n_nodes:
        nodes.append((fe.N_ADD, 0, 0, len(nodes) % 2, len(nodes) - 1))
    c = fe.CompiledCircuit(nodes, [n_nodes - 1], [(prefix - 1, [0, 1])] if prefix else [], 2, None)
    c.lookup_prefix_len = prefix
    return c


# Cold hiprtc times of the chain (empty cache, the *_jit_build calls alone, taken without a device): quotient kernel of 3000 nodes
# 15.7 s, from-trace kernel of a 3000-node prefix 15.2 s - each under the issue's bound of 20 s, together not, hence two tests and
# no circuit that gets both.
def test_quotient_node_limit(pkg, ctx, oracle, fe, monkeypatch):
    """quotient_jit_build: a program of 3000 nodes is compiled, one of 3001 is interpreted"""
    rng = np.random.default_rng(3000)
    for n_nodes, flags in ((3000, Q | Q_INL), (3001, 0)):
        blob = fe.system_blob(fe.test_params(), [chain_circuit(fe, n_nodes)])
        g, interp = system_pair(pkg, ctx, monkeypatch, blob, 1, [flags], "%d nodes" % n_nodes)
        o = oracle.System(blob)
        for ln in (0, 6):
            s1, s2, publics, alpha = rand_field(rng, (1 << ln, 2)), rand_field(rng, (1 << ln, 2)), rand_field(rng, 8), rand_field(rng, 2)
            want = oracle.quotient_values(o, 0, publics, ln, 0, None, s1, s2, alpha)
            assert np.array_equal(g.quotient_values(0, publics, ln, 0, None, s1, s2, alpha), want), n_nodes
            assert np.array_equal(interp.quotient_values(0, publics, ln, 0, None, s1, s2, alpha), want), n_nodes


def test_lookup_prefix_node_limit(pkg, ctx, oracle, fe, monkeypatch):
    """stage2_trace_jit_build: prefix_len > 3000 - a lookup prefix of 3000 nodes gets the from-trace kernel, one of 3001 does
    not. Both programs have 3001 nodes (no quotient kernel); the terms kernel does not depend on the program."""
    rng = np.random.default_rng(3001)
    for prefix, flags in ((3000, S2 | S2_TR), (3001, S2)):
        blob = fe.system_blob(fe.test_params(), [chain_circuit(fe, 3001, prefix)])
        g, interp = system_pair(pkg, ctx, monkeypatch, blob, 1, [flags], "lookup prefix of %d nodes" % prefix)
        o = oracle.System(blob)
        assert prove_all_ways(pkg, g, interp, o, [rand_field(rng, (64, 2))], fe.pack_claims([]), "prefix %d" % prefix) is not None


# ------------------------------------------------------------------ d) a random slice with the generators on
# Seeds chosen by running the front end and the oracles alone on the CPU (a case the oracle proves counts as proved):
# seed 2, 24 Goldilocks cases: 21 proved, 2 refused by the prover, 1 rejected by the front end; 42 circuits
# seed 4, 8 BabyBear cases: 6 proved, 2 rejected by the front end; 12 circuits
FUZZ_SEED, FUZZ_SEED_BB = 2, 4


def _fuzz():
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import fuzz_parity

    return fuzz_parity


def test_random_systems_generated_kernels(pkg, ctx, oracle, fe):
    """24 cases of tools/fuzz_parity.py with MSAMD_NO_JIT unset (the other random slices of the suite set it)"""
    fuzz = _fuzz()
    flags, tally = [], {}

    def seen(system):  # every circuit's quotient kernel was generated (these programs are far below the node limit)
        got = [system.circuit_kernels(ci) for ci in range(system.n_circuits)]
        assert all(f & Q for f in got), [hex(f) for f in got]
        flags.extend(got)

    rng = np.random.default_rng(FUZZ_SEED)
    for case in range(24):
        r = fuzz.one_case(pkg, fe, oracle, ctx, np.random.default_rng(rng.integers(0, 1 << 62)), case,
                          on_system=seen)
        tally[r] = tally.get(r, 0) + 1
    assert sum(1 for f in flags if f & Q) >= 16, [hex(f) for f in flags]
    assert tally.get("proved", 0) + tally.get("verified", 0) >= 16, tally


def test_random_systems_generated_kernels_babybear(pkg, ctx, fe):
    """8 cases over BabyBear / Poseidon2 (bb_circuit_source) against the oracle of that configuration"""
    import oracle_bb

    fuzz = _fuzz()
    flags, tally = [], {}

    def seen(system):
        got = [system.circuit_kernels(ci) for ci in range(system.n_circuits)]
        assert got == [Q] * len(got), [hex(f) for f in got]
        flags.extend(got)

    rng = np.random.default_rng(FUZZ_SEED_BB)
    with fe.field(fe.BABYBEAR):
        for case in range(8):
            r = fuzz.one_case(pkg, fe, oracle_bb, ctx, np.random.default_rng(rng.integers(0, 1 << 62)), case,
                              on_system=seen,
                              babybear=True, kperm=fe.poseidon2_constants())
            tally[r] = tally.get(r, 0) + 1
    assert flags and all(f == Q for f in flags), [hex(f) for f in flags]
    assert tally.get("proved", 0) + tally.get("verified", 0) >= 5, tally


# ------------------------------------------------------------------ e) BabyBear, directed
@pytest.mark.parametrize("name", list(QUOTIENT_CASES))
def test_babybear_quotient_kernel(pkg, ctx, fe, monkeypatch, name):
    """every circuit of a), authored over BabyBear (the builders take their constants from the front end's field: P_bb - 1 in
    place of P - 1), as whole proofs at log_blowup 3: bb_circuit_source's preprocessed operands (p.pre, st and st_next), the
    selector stack, dead nodes, L == 0, the E4 Horner chain of 0 .. 33 arguments (5 among the 16 mixed lookups), quotient
    degrees 1 .. 8 (log_q 3: i & (q - 1)). The preprocessed trace fixes the height, so there is one system per height; the
    generated source is the same, and is compiled once."""
    import oracle_bb

    build, _, qdeg = QUOTIENT_CASES[name]
    rng = np.random.default_rng(len(name))
    proved = 0
    for h in (1, 8, 64):
        with fe.field(fe.BABYBEAR):
            circuit = build(fe, pre_h=h)
            compiled = fe.compile_circuit(circuit)
            blob = fe.system_blob(fe.Params(3, 0, 0, 1, 8, 0, 0), [compiled], fe.poseidon2_constants())
            packed = fe.pack_claims([[1, 2]])
        if name == "mixed_operands":
            live, dead = live_and_dead(fe, compiled)
            assert dead >= live and len(compiled.zeros) == 1, (live, dead)
        g, interp = system_pair(pkg, ctx, monkeypatch, blob, 1, [Q], "babybear %s, height %d" % (name, h), bb=True)
        o = oracle_bb.System(blob)
        assert g.circuit_info(0) == o.circuit_info(0) and g.circuit_info(0)["quotient_degree"] == qdeg
        w = circuit.main_width
        for trace in (rng.integers(0, P_BB, (h, w), dtype=np.uint64), np.full((h, w), P_BB - 1, dtype=np.uint64)):
            try:
                want = o.prove([trace], packed)
            except RuntimeError:
                for s in (g, interp):
                    with pytest.raises(pkg.MstarkError):
                        s.prove_multiple_claims(s.witness([trace], packed))
                continue
            proved += 1
            ref = interp.prove_multiple_claims(interp.witness([trace], packed)).to_bytes()
            for way in ("witness", "host_witness"):
                got = g.prove_multiple_claims(getattr(g, way)([trace], packed)).to_bytes()
                assert got == want, "%s, height %d, %s: differs from the oracle (interpreter %s)" % (name, h, way, "agrees" if ref == want else "differs too")
            assert ref == want
    assert proved >= 3


# ------------------------------------------------------------------ f) the disk cache of code objects
CHILD = r"""
import hashlib, sys
import numpy as np
sys.path[:0] = [%(root)r, %(tests)r]
from __graft_entry__ import load_package
from test_gpu_generated_kernels import q_lookups
pkg = load_package()
fe = pkg.frontend
g = pkg.System.new(pkg.Context(0), fe.Params(3, 0, 0, 1, 1, 0, 0), [q_lookups(fe, [3, 1], zeros=1)])
info = g.circuit_info(0)
N = 8
col = lambda w, k: (np.arange(N * w, dtype=np.uint64).reshape(N, w) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(k)) %% np.uint64(0xFFFFFFFF00000001)
out = g.quotient_values(0, col(8, 1).reshape(-1)[:8], 3, 0, None, col(info["main_width"], 2), col(info["stage2_width"], 3), [5, 6])
print("RESULT", g.circuit_kernels(0), hashlib.sha256(out.tobytes()).hexdigest())
"""
MAGIC = b"MSJC0002"


def _run_child(cache):
    env = dict(os.environ, MSAMD_JIT_CACHE=str(cache))
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], env=env, capture_output=True,
                       text=True, timeout=180)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT")][-1].split()
    return int(line[1]), line[2]


def _valid(path):
    data = path.read_bytes()
    return len(data) > 40 and data[:8] == MAGIC and path.name == "q_" + data[8:24].hex() + ".co"


def test_disk_cache_rebuilds_stale_and_truncated_files(tmp_path, oracle, fe):
    """MSAMD_JIT_CACHE: files are MAGIC + the 32-byte key digest + the code object. A file whose digest is not the key's (stale or
    foreign) and one shorter than the header are ignored and rebuilt. (A valid header in front of a damaged body is NOT
    detected - the header carries no checksum of the body, see DESIGN.md - and is not tried here.)"""
    cache = tmp_path / "jit"
    cache.mkdir()
    flags, digest = _run_child(cache)  # child 1: empty directory
    assert flags == Q | Q_INL | S2 | S2_TR
    files = sorted(cache.glob("q_*.co"))
    assert len(files) == 3 and all(_valid(f) for f in files), files  # quotient, stage-2 terms, stage-2 from-trace
    assert not [f for f in cache.iterdir() if f not in files]     # no temporary files left behind
    data = bytearray(files[0].read_bytes())
    data[8 + 5] ^= 0xFF
    files[0].write_bytes(bytes(data))           # a digest that is not this program's
    files[1].write_bytes(MAGIC + b"\0" * 12)    # 20 bytes: shorter than the header
    assert not _valid(files[0]) and not _valid(files[1])
    assert _run_child(cache) == (flags, digest)  # child 2: same kernels, same values
    assert sorted(cache.glob("q_*.co")) == files and all(_valid(f) for f in files)
    # the values are the oracle's
    o = oracle.System(fe.system_blob(fe.Params(3, 0, 0, 1, 1, 0, 0), [fe.compile_circuit(q_lookups(fe, [3, 1], zeros=1))]))
    info, N, M = o.circuit_info(0), 8, np.uint64(0x9E3779B97F4A7C15)
    col = lambda w, k: (np.arange(N * w, dtype=np.uint64).reshape(N, w) * M + np.uint64(k)) % np.uint64(P)
    want = oracle.quotient_values(o, 0, col(8, 1).reshape(-1)[:8], 3, 0, None, col(info["main_width"], 2), col(info["stage2_width"], 3), [5, 6])
    assert hashlib.sha256(want.tobytes()).hexdigest() == digest
