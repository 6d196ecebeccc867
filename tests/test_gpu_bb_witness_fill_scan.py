"""`-m gpu`: the scan steps of msbb_witness_fill (csrc/bb_fill.hip) against the model of tests/fill_scan_model_bb.py, which
tests/test_bb_fill_scan_model.py pins to the definition. Every comparison is exact, device against model, read back through
w.trace(c). The counterpart of test_gpu_witness_fill_scan.py.

Heights come from T = babybear.fill_scan_info()[3], the rows of a scan tile: 1 (only init), 2, 64, T / 2 (a partial tile), T (the
last height of the one-launch form), 2 T (the first seam), 8 T, and 2 R T for the second round of the one-workgroup launch over
the tile aggregates (R from include/mstark_bb.h). Main widths 1, 2 and 14. Multipliers are random over the whole field with 0,
1, p - 1, p - 2, 2^27 and 2^31 - 2^28 placed among them and a zero at rows T - 1, T and T + 1: the chain restarts on both sides
of a tile seam. Inputs are 4-byte and 2-byte elements, of the full height and of half of it."""
import os
import re

import numpy as np
import pytest
import torch  # (before the library opens the device)

import fill_scan_model_bb as bsm
from test_bb_fill_scan_model import bb_refusal_blobs
from test_bb_witness_check_model import K, bb, fe, pack, pkg
from test_gpu_bb_lookup_balance import ctx  # noqa: F401  (the module-scoped context with the Poseidon2 permutation set)

pytestmark = pytest.mark.gpu
P = bsm.P
_CACHE = {}
EDGES = [0, 1, P - 1, P - 2, 1 << 27, (1 << 31) - (1 << 28)]
EDGES16 = [0, 1, 0xFFFF, 0x8000]
WIDTHS = (1, 2, 14)
INIT = P - 0x1234567  # a first value near the top of the field
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    """a numpy array of unsigned integers as a torch tensor on the GPU (same bits, same element size)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])).cuda()


def dev32(a):
    return dev(np.asarray(a).astype(np.uint32))


def same(got, want):
    return got.shape == want.shape and np.array_equal(got.astype(np.uint64), np.asarray(want, dtype=np.uint64))


def tile():
    if "T" not in _CACHE:
        _CACHE["T"] = bb.fill_scan_info(bb.compile_fill(1, 0, 1, [(0, fe.running_sum(fe.Expr.input(0)))]))[3]
    return _CACHE["T"]


def operands(rng, n, cols, T, wide=True):
    """n x cols canonical values (wide: over the field, as 4-byte elements; else below 2^16, as 2-byte elements): random, the
    edge values at random places and, each of them, at a row of column 0 - the multipliers' column - as far as there are rows;
    zeros in column 0 around the first tile seam"""
    edges = EDGES if wide else EDGES16
    a = rng.integers(0, P if wide else 1 << 16, size=(n, cols), dtype=np.uint64)
    flat = a.reshape(-1)
    for e in edges:
        flat[rng.integers(0, flat.size)] = e
    rows = rng.choice(n, size=min(n, len(edges)), replace=False)
    a[rows, 0] = np.array(edges[: len(rows)], dtype=np.uint64)
    for r in (T - 1, T, T + 1):
        if r < n:
            a[r, 0] = 0
    return a.astype(np.uint32 if wide else np.uint16)


def lab_system(ctx):
    """one circuit per main width, no preprocessed trace: the witness decides the height. Nothing is ever proved with it: the
    constraints are placeholders."""
    if "lab" not in _CACHE:
        E = fe.Expr
        with fe.field(fe.BABYBEAR):
            inputs = [fe.CircuitInputs(w, None, [E.main(0) * E.main(0) - E.main(0)], [], []) for w in WIDTHS]
            _CACHE["lab"] = bb.System.new(ctx, fe.test_params(), inputs, K)
    return _CACHE["lab"]


def lab_witness(ctx, rng, n):
    """every circuit active at height n, filled with random values -> (witness, traces)"""
    s = lab_system(ctx)
    traces = [rng.integers(0, P, size=(n, w), dtype=np.uint64) for w in WIDTHS]
    return s.witness_from_device([dev32(t) for t in traces], pack([])), traces


def fill_against_model(w, traces, ci, prog, inputs):
    """fill circuit ci on the device and in the model; `traces` follows. The report agrees with the host-only info calls, and
    the other circuits' traces stay byte-identical."""
    want = bsm.run(prog.blob, traces[ci], None, None if inputs is None else inputs.astype(np.uint64))
    rep = w.fill(ci, prog, None if inputs is None else dev(inputs))
    got = w.trace(ci)
    assert same(got, want), "circuit %d, rows %s" % (ci, np.nonzero((got != want).any(axis=1))[0][:8])
    info = bb.fill_program_info(prog)
    assert rep.fields() == (traces[ci].shape[0], len(prog.steps), info["instructions"], info["lds_lanes"]), str(rep)
    traces[ci] = got.astype(np.uint64)
    for other in range(len(traces)):
        if other != ci:
            assert same(w.trace(other), traces[other])
    return rep


def programs(width):
    """(name, program over inputs (multiplier, addend, third)) for one main width: both forms everywhere; from width 2 on
    coefficients that read the trace, and a later group that indexes a finished scan column; at width 14 ordinary -> scan ->
    ordinary reading the scan at offsets 0 and 1 -> a scan over that, with the additive form in the middle of it"""
    E = fe.Expr
    with fe.field(fe.BABYBEAR):
        m, x, y = E.input(0), E.input(1), E.input(2)
        if width == 1:
            return [("affine", bb.compile_fill(1, 0, 3, [(0, fe.scan(m, x, init=INIT))])),
                    ("additive", bb.compile_fill(1, 0, 3, [(0, fe.running_sum(x * y, init=INIT))])),
                    ("product", bb.compile_fill(1, 0, 3, [(0, fe.running_product(m + 1, init=P - 1))]))]
        if width == 2:
            return [("affine over a column", bb.compile_fill(2, 0, 3, [(0, m * y), (1, fe.scan(E.main(0), x - E.main_next(0), init=1))])),
                    ("additive over the old trace", bb.compile_fill(2, 0, 3, [(1, fe.running_sum(E.main(0) * y)), (0, E.main(1) * m)])),
                    # a later group reads the finished scan column at a computed row: 14 bits of the multiplier, so rows from the
                    # height on (which read 0) occur at every height of the test
                    ("at of a finished scan", bb.compile_fill(2, 0, 3, [(0, fe.scan(m, x, init=INIT)), (1, E.main_at(0, fe.bits(y, 0, 14)) + E.main_at(0, E.row()))]))]
        steps = [(0, m + fe.bits(x, 3, 20)), (1, x * y),                                    # ordinary
                 (2, fe.scan(E.main(0), E.main(1) - E.main(13), init=INIT)),                # a scan over them and an old column
                 (3, E.main_next(2) - E.main(2)), (4, E.main(2) * E.main(2)), (0, E.row()),  # ordinary: the scan at offsets 1 and 0
                 (5, fe.running_sum(E.main(3), init=7)),                                    # additive: telescopes back to column 2
                 (6, fe.scan(E.main(4) + E.main_next(5), fe.inv0(E.main(3)), init=0)),      # a scan over all of that
                 (7, E.main(6) - E.main_next(6))]
        return [("four stages", bb.compile_fill(14, 0, 3, steps))]


def heights(T):
    return [1, 2, 64, T // 2, T, 2 * T, 8 * T]


@pytest.mark.parametrize("k", range(7))
def test_scans_against_the_model(ctx, k):
    T = tile()
    n = heights(T)[k]
    rng = np.random.default_rng(900 + k)
    w, traces = lab_witness(ctx, rng, n)
    half = (n + 1) // 2
    for ci, width in enumerate(WIDTHS):
        for name, prog in programs(width):
            # inputs of the full height and of half of it (rows from their height on read 0), 4-byte and 2-byte elements
            for h_in, wide in sorted({(n, True), (half, True), (half, False), (n, False)}):
                fill_against_model(w, traces, ci, prog, operands(rng, n, 3, T, wide)[:h_in])
    # column 5 of the wide program telescopes: 7 + sum of (s_next - s) = 7 + s[r] - s[0] - a closed form next to the model
    wide = traces[2]
    assert np.array_equal(wide[:, 5].astype(object), (7 + wide[:, 2].astype(object) - INIT) % P)


def aggregates_per_round():
    """R of include/mstark_bb.h: the tile aggregates the one-workgroup launch handles per round"""
    text = open(os.path.join(ROOT, "include", "mstark_bb.h")).read()
    return int(re.search(r"R = (\d+) aggregates per round", text).group(1))


def test_aggregate_rounds_beyond_one(ctx):
    """the one-workgroup launch over the tile aggregates scans R of them per round: twice that many tiles, both forms, a restart
    around the seam between the two rounds, against the plain loop of the definition"""
    T, R = tile(), aggregates_per_round()
    n = 2 * R * T
    assert n <= 1 << 21 and n & (n - 1) == 0
    rng = np.random.default_rng(77)
    ops = operands(rng, n, 2, T)
    for r in (R * T - 1, R * T, R * T + 1):
        ops[r, 0] = 0
    E = fe.Expr
    s = lab_system(ctx)
    w = s.witness_from_device([dev32(np.zeros((n, 1), dtype=np.uint64)), None, None], pack([]))
    inputs = dev(ops)
    w.fill(0, bb.compile_fill(1, 0, 2, [(0, fe.scan(E.input(0), E.input(1), init=INIT))]), inputs)
    affine = w.trace(0)[:, 0].astype(np.uint64)
    w.fill(0, bb.compile_fill(1, 0, 2, [(0, fe.running_sum(E.input(1), init=INIT))]), inputs)
    additive = w.trace(0)[:, 0].astype(np.uint64)
    want_affine, want_additive = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    a, b, s1, s2 = ops[:, 0].tolist(), ops[:, 1].tolist(), INIT, INIT
    for r in range(n):  # the definition, one loop for both
        want_affine[r], want_additive[r] = s1, s2
        s1, s2 = (a[r] * s1 + b[r]) % P, (s2 + b[r]) % P
    assert np.array_equal(affine, want_affine), np.nonzero(affine != want_affine)[0][:8]
    assert np.array_equal(additive, want_additive), np.nonzero(additive != want_additive)[0][:8]


@pytest.mark.parametrize("form", ["lds", "scratch"])
def test_both_forms_of_the_coefficient_pass(ctx, form):
    T = tile()
    E = fe.Expr
    with fe.field(fe.BABYBEAR):
        m, x = E.input(0), E.input(1)
        leaves = [fe.bits(x + k, k % 25, 1 + k // 50) for k in range(300 if form == "scratch" else 8)]
        add = leaves[-1]
        for leaf in reversed(leaves[:-1]):  # every leaf is live before the first is consumed
            add = leaf - add
        prog = bb.compile_fill(2, 0, 3, [(0, m), (1, fe.scan(E.main(0), add, init=5))])
    info = bb.fill_program_info(prog)
    assert (info["lds_lanes"] == 0) == (form == "scratch") and bb.fill_scan_info(prog) == (1, 2, 0, T)
    assert form == "lds" or info["slots"] >= 300
    rng = np.random.default_rng(len(leaves))
    n = 2 * T
    w, traces = lab_witness(ctx, rng, n)
    rep = fill_against_model(w, traces, 1, prog, operands(rng, n, 3, T))
    assert rep.lds_lanes == info["lds_lanes"]


def test_heights_below_four_take_the_word_by_word_path(ctx):
    """The library's copy of a trace has leading dimension ld = n, a power of two (bmat, csrc/bb.h), and device allocations are
    256-byte aligned: from n = 4 on ld is a multiple of 4 and every dst column and every tile start lies on a 16-byte boundary,
    so no trace of this library reaches a 16-byte access at an unaligned address. ld = 1 and ld = 2 (heights 1 and 2) are the
    values that are no multiple of 4: there the dst column of an odd column number starts 4 or 8 bytes into a 16-byte line,
    and the four-row group ends beyond n, so the 4-byte accesses under the guard are taken - the same branch an unaligned
    address takes. Every column of the 14-wide circuit as dst, both forms, and the neighbours stay as they were."""
    E = fe.Expr
    rng = np.random.default_rng(5)
    for n in (1, 2):
        w, traces = lab_witness(ctx, rng, n)
        for dst in range(14):
            other = (dst + 1) % 14
            affine = bb.compile_fill(14, 0, 2, [(dst, fe.scan(E.input(0) + E.main(other), E.input(1), init=INIT))])
            additive = bb.compile_fill(14, 0, 2, [(dst, fe.running_sum(E.input(1) * E.main_next(other), init=dst))])
            for prog in (affine, additive):
                fill_against_model(w, traces, 2, prog, operands(rng, n, 2, tile()))


# ---------------------------------------------------------------- end to end: transition-constrained columns, filled and proved
ALPHA = (1 << 27) + 3


def airs():
    """[running sum: columns (x, s); Horner: columns (x, acc)], each with is_first * s, is_transition * (s_next - A s - B) and a
    lookup pair that reads the scanned column (the publics of a system are the four values of the lookup argument - challenges
    and boundary accumulators - and the pair is what makes them depend on the column). Call under field(BABYBEAR)."""
    def air(mul):
        def ev(b):
            local, nxt = b.main()
            b.when_first_row().assert_zero(local[1])
            b.when_transition().assert_zero(nxt[1] - mul * local[1] - local[0])
        E = fe.Expr
        return fe.lookup_air(2, ev, [fe.Lookup.push(1, [E.const(9), E.main(1)]), fe.Lookup.pull(1, [E.const(9), E.main(1)])])
    return [air(fe.Expr.const(1)), air(fe.Expr.const(ALPHA))]


def test_running_sum_and_horner_airs_end_to_end(ctx):
    T = tile()
    n = 2 * T
    E = fe.Expr
    with fe.field(fe.BABYBEAR):
        s = bb.System.new(ctx, fe.test_params(), airs(), K)
    x = operands(np.random.default_rng(31), n, 1, T)[:, 0].astype(np.uint64)
    traces = []
    for mul in (1, ALPHA):
        col, acc = np.zeros(n, dtype=np.uint64), 0
        for r in range(n):
            col[r] = acc
            acc = (mul * acc + int(x[r])) % P
        traces.append(np.stack([x, col], axis=1))
    packed = pack([])
    proof = s.prove_multiple_claims(s.witness(traces, packed)).to_bytes()  # from the host-built witness
    start = [np.stack([x, np.full(n, 5, dtype=np.uint64)], axis=1) for _ in range(2)]  # the scanned column holds something else
    w = s.witness_from_device([dev32(t) for t in start], packed)
    assert same(w.trace(0), start[0])  # (the read-back is a host wait: nothing of the setup is pending)
    before = ctx.sync_count()
    w.fill(0, bb.compile_fill(2, 0, 0, [(1, fe.running_sum(E.main(0)))]))
    w.fill(1, bb.compile_fill(2, 0, 0, [(1, fe.scan(ALPHA, E.main(0)))]))
    assert ctx.sync_count() == before  # no inputs: the calls only queue work
    assert same(w.trace(0), traces[0]) and same(w.trace(1), traces[1])
    assert w.check().verdict == 0 and w.lookup_balance().ok
    got = s.prove_multiple_claims(w).to_bytes()
    assert got == proof and s.verify_multiple_claims(packed, got) == 0


# ---------------------------------------------------------------- the pipeline: argsort -> gather -> scan on one circuit
def test_argsort_gather_scan(ctx):
    """a memory log in address order with, next to every row, how many rows in front of it hold the same address in one run:
    columns ADDR (the log), PERM (msbb_witness_argsort), S_ADDR = ADDR[PERM] (an indexed read) and RUN, the scan
    RUN[r + 1] = same(r) * (RUN[r] + 1) with same(r) = [S_ADDR[r + 1] == S_ADDR[r]], a restart wherever the address changes"""
    T = tile()
    n = 2 * T
    ADDR, PERM, S_ADDR, RUN = 0, 1, 2, 3
    E = fe.Expr
    with fe.field(fe.BABYBEAR):
        s = bb.System.new(ctx, fe.test_params(), [fe.CircuitInputs(4, None, [E.main(0) * E.main(0) - E.main(0)], [], [])], K)
        d = E.main_next(S_ADDR) - E.main(S_ADDR)
        eq = 1 - d * fe.inv0(d)
        prog = bb.compile_fill(4, 0, 0, [(S_ADDR, E.main_at(ADDR, E.main(PERM))), (RUN, fe.scan(eq, eq, init=0))])
    assert bb.fill_scan_info(prog)[:3] == (1, 2, 0)
    rng = np.random.default_rng(404)
    addr = rng.integers(0, n // 8, size=n, dtype=np.uint64)  # eight rows per address on average
    addr[rng.choice(n, size=T + 40, replace=False)] = 17     # and one run longer than a tile
    log = np.stack([addr, np.full(n, 3, dtype=np.uint64), np.full(n, 4, dtype=np.uint64), np.full(n, 5, dtype=np.uint64)], axis=1)
    w = s.witness_from_device([dev32(log)], pack([]))
    w.argsort(0, [ADDR], PERM)
    w.fill(0, prog)
    got = w.trace(0).astype(np.uint64)
    perm = np.argsort(addr, kind="stable")
    srt = addr[perm]
    run = np.zeros(n, dtype=np.uint64)
    for r in range(1, n):
        run[r] = run[r - 1] + 1 if srt[r] == srt[r - 1] else 0
    assert run.max() >= T
    assert np.array_equal(got[:, ADDR], addr) and np.array_equal(got[:, PERM], perm.astype(np.uint64))
    assert np.array_equal(got[:, S_ADDR], srt) and np.array_equal(got[:, RUN], run)


# ---------------------------------------------------------------- refusals and host waits
def test_refusals_write_nothing_and_leave_the_context_usable(ctx):
    T = tile()
    n = 2 * T
    rng = np.random.default_rng(12)
    w, traces = lab_witness(ctx, rng, n)
    E, N = fe.Expr, fe
    nodes = [(N.N_VAR, N.SRC_INPUT, 0, 0, 0), (N.N_CONST, 0, 0, 3, 0), (N.N_VAR, N.SRC_MAIN, 0, 1, 0), (N.N_VAR, N.SRC_MAIN, 1, 1, 0),
             (N.N_ROW, 0, 0, 0, 0), (N.N_AT, N.SRC_MAIN, 0, 1, 4)]
    good_inputs = operands(rng, n, 1, T)
    bad_inputs = good_inputs.copy()
    bad_inputs[T + 1, 0] = P
    good = bb.compile_fill(2, 0, 1, [(0, E.input(0)), (1, fe.scan(E.main(0), E.input(0), init=3))])
    other_field = fe.compile_fill(2, 0, 1, [(0, E.input(0)), (1, fe.scan(E.main(0), E.input(0), init=3))])
    assert other_field.blob[:8] == b"\0MFILL02" and good.blob[:8] == b"\0MFILB02"
    with fe.field(fe.BABYBEAR):
        blob = lambda steps, scans: fe.fill_blob(2, 0, 1, nodes, steps, scans)
        cases = [(blob([(1, 2)], [(0, 1, 0)]), good_inputs, ("own dst",)),
                 (blob([(1, 3)], [(0, 1, 0)]), good_inputs, ("own dst",)),
                 (blob([(1, 5)], [(0, 1, 0)]), good_inputs, ("indexed read of main column 1",)),
                 (blob([(0, 0)], [(0, 1, P)]), good_inputs, ("init",)),
                 (blob([(0, 0), (1, 0)], [(1, 1, 0), (0, 1, 0)]), good_inputs, ("ascending",)),
                 (blob([(0, 0)], [(1, 1, 0)]), good_inputs, ("step index",)),
                 (blob([(0, 0)], [(0, 6, 0)]), good_inputs, ("mul root",)),
                 (blob([(0, 3), (1, 0)], [(1, 1, 0)]), good_inputs, ("offset-1",)),
                 (blob([(0, 0)], [(0, 1, 0)])[:-8], good_inputs, ("truncated",)),
                 (other_field.blob, good_inputs, ("magic",)),  # the other configuration's second format
                 (good.blob, bad_inputs, ("row %d" % (T + 1), "column 0")),  # found behind the compiler, before the first launch
                 (good.blob, None, ("input",))]
    for program, inputs, words in cases:
        with pytest.raises(pkg.MstarkError) as e:
            w.fill(1, program, None if inputs is None else dev(inputs))
        assert str(e.value).startswith("msbb_witness_fill: ") and all(x in str(e.value) for x in words), str(e.value)
        assert all(same(w.trace(ci), traces[ci]) for ci in range(len(WIDTHS)))
    for what, program, _ in bb_refusal_blobs(fe)[1]:  # the host-only cases, widths (2, 1) and (3, 1): refused as a program before the widths are compared
        with pytest.raises(pkg.MstarkError):
            w.fill(1, program, dev(good_inputs))
    assert all(same(w.trace(ci), traces[ci]) for ci in range(len(WIDTHS)))
    fill_against_model(w, traces, 1, good, good_inputs)  # the context and the witness are as good as new


def test_host_waits(ctx):
    T = tile()
    n = 2 * T
    rng = np.random.default_rng(13)
    w, traces = lab_witness(ctx, rng, n)
    E = fe.Expr
    no_inputs = bb.compile_fill(14, 0, 0, [(0, E.row() + 1), (1, fe.scan(E.main(0), E.main(13))), (2, E.main_next(1)), (3, fe.running_sum(E.main(2)))])
    assert same(w.trace(2), traces[2])  # (the read-back is a host wait: nothing of the setup is pending)
    before = ctx.sync_count()
    w.fill(2, no_inputs)
    assert ctx.sync_count() == before  # two scans, four groups: the call only queues work (include/mstark_bb.h, "Host waits")
    assert same(w.trace(2), bsm.run(no_inputs.blob, traces[2]))
    with_inputs = bb.compile_fill(1, 0, 1, [(0, fe.running_sum(E.input(0)))])
    inputs = dev(operands(rng, n, 1, T))
    torch.cuda.synchronize()
    before = ctx.sync_count()
    w.fill(0, with_inputs, inputs)
    assert ctx.sync_count() == before + 1  # the offender word of the inputs, as without scans
