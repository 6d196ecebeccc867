"""`-m gpu`: the scan steps of ms_witness_fill (csrc/fill.hip) against the model of tests/fill_scan_model.py, which
tests/test_fill_scan_model.py pins to the definition. Every comparison is exact, device against model.

Heights come from T = fill_scan_info()[3], the rows of a scan tile: 1 (only init), 2, 64, T / 2 (a partial tile), T (the last
height of the one-launch form), 2 T (the first seam), 8 T, and 256 T * 2 = 2^19 at T = 1024 - trace heights are powers of two,
so that is the smallest height above 256 T, from which the one-workgroup launch over the tile aggregates takes a second round
of 256 aggregates. Main widths 1, 2 and 14. Multipliers are random over the whole field with 0, 1, p - 1, 2^32 - 1 and 2^32
placed among them and a zero at rows T - 1, T and T + 1: the chain restarts on both sides of a tile seam."""
import numpy as np
import pytest
import torch  # (before the library opens the device)

import fill_scan_model as fsm
from test_fill_scan_model import scan_refusal_blobs

pytestmark = pytest.mark.gpu
P = fsm.P
_CACHE = {}
EDGES = [0, 1, P - 1, (1 << 32) - 1, 1 << 32, P - 2, 1 << 63, 0xFFFFFFFF00000000]
WIDTHS = (1, 2, 14)
INIT = 0xFFFFFFFE00000003  # a first value with both limbs busy


def dev(a):
    """a numpy array of unsigned integers as a torch tensor on the GPU (same bits, same element size)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])).cuda()


def tile(pkg, fe):
    if "T" not in _CACHE:
        _CACHE["T"] = pkg.fill_scan_info(fe.compile_fill(1, 0, 1, [(0, fe.running_sum(fe.Expr.input(0)))]))[3]
    return _CACHE["T"]


def operands(rng, n, cols, T):
    """n x cols canonical values: random, the edge values at random places and, each of them, at a row of column 0 - the
    multipliers' column - as far as there are rows; zeros in column 0 around the first tile seam"""
    a = rng.integers(0, P, size=(n, cols), dtype=np.uint64)
    flat = a.reshape(-1)
    for e in EDGES:
        flat[rng.integers(0, flat.size)] = e
    rows = rng.choice(n, size=min(n, len(EDGES)), replace=False)
    a[rows, 0] = np.array(EDGES[: len(rows)], dtype=np.uint64)
    for r in (T - 1, T, T + 1):
        if r < n:
            a[r, 0] = 0
    return a


def lab_system(pkg, fe, ctx):
    """one circuit per main width, no preprocessed trace: the witness decides the height. Nothing is ever proved with it: the
    constraints are placeholders."""
    if "lab" not in _CACHE:
        E = fe.Expr
        _CACHE["lab"] = pkg.System.new(ctx, fe.test_params(), [fe.CircuitInputs(w, None, [E.main(0) * E.main(0) - E.main(0)], [], []) for w in WIDTHS])
    return _CACHE["lab"]


def lab_witness(pkg, fe, ctx, rng, n):
    """every circuit active at height n, filled with random values -> (witness, traces)"""
    s = lab_system(pkg, fe, ctx)
    traces = [rng.integers(0, P, size=(n, w), dtype=np.uint64) for w in WIDTHS]
    return s.witness_from_device([dev(t) for t in traces], fe.pack_claims([])), traces


def fill_against_model(pkg, w, traces, ci, prog, inputs):
    """fill circuit ci on the device and in the model; `traces` follows. The report agrees with the host-only info calls."""
    want = fsm.run(prog.blob, traces[ci], None, inputs)
    rep = w.fill(ci, prog, None if inputs is None else dev(inputs))
    got = w.trace(ci)
    assert np.array_equal(got, want), "circuit %d, rows %s" % (ci, np.nonzero((got != want).any(axis=1))[0][:8])
    info = pkg.fill_program_info(prog)
    assert rep.fields() == (traces[ci].shape[0], len(prog.steps), info["instructions"], info["lds_lanes"]), str(rep)
    traces[ci] = got
    for other in range(len(traces)):
        if other != ci:
            assert np.array_equal(w.trace(other), traces[other])
    return rep


def programs(fe, width):
    """(name, program over inputs (multiplier, addend, third)) for one main width: both forms everywhere; from width 2 on
    coefficients that read the trace; at width 14 ordinary -> scan -> ordinary reading the scan at offsets 0 and 1 -> a scan over
    that, with the additive form in the middle of it"""
    E = fe.Expr
    m, x, y = E.input(0), E.input(1), E.input(2)
    if width == 1:
        return [("affine", fe.compile_fill(1, 0, 3, [(0, fe.scan(m, x, init=INIT))])),
                ("additive", fe.compile_fill(1, 0, 3, [(0, fe.running_sum(x * y, init=INIT))])),
                ("product", fe.compile_fill(1, 0, 3, [(0, fe.running_product(m + 1, init=P - 1))]))]
    if width == 2:
        return [("affine over a column", fe.compile_fill(2, 0, 3, [(0, m * y), (1, fe.scan(E.main(0), x - E.main_next(0), init=1))])),
                ("additive over the old trace", fe.compile_fill(2, 0, 3, [(1, fe.running_sum(E.main(0) * y)), (0, E.main(1) * m)]))]
    steps = [(0, m + fe.bits(x, 3, 20)), (1, x * y),                                    # ordinary
             (2, fe.scan(E.main(0), E.main(1) - E.main(13), init=INIT)),                # a scan over them and an old column
             (3, E.main_next(2) - E.main(2)), (4, E.main(2) * E.main(2)), (0, E.row()),  # ordinary: the scan at offsets 1 and 0
             (5, fe.running_sum(E.main(3), init=7)),                                    # additive: telescopes back to column 2
             (6, fe.scan(E.main(4) + E.main_next(5), fe.inv0(E.main(3)), init=0)),      # a scan over all of that
             (7, E.main(6) - E.main_next(6))]
    return [("four stages", fe.compile_fill(14, 0, 3, steps))]


def heights(T):
    return [1, 2, 64, T // 2, T, 2 * T, 8 * T]


@pytest.mark.parametrize("k", range(7))
def test_scans_against_the_model(pkg, fe, ctx, k):
    T = tile(pkg, fe)
    n = heights(T)[k]
    rng = np.random.default_rng(900 + k)
    w, traces = lab_witness(pkg, fe, ctx, rng, n)
    for ci, width in enumerate(WIDTHS):
        for name, prog in programs(fe, width):
            # inputs of the full height, and shorter than the circuit where there is room (rows from their height on read 0)
            for h_in in sorted({n, (n + 1) // 2}):
                fill_against_model(pkg, w, traces, ci, prog, operands(rng, n, 3, T)[:h_in])
    # column 5 of the wide program telescopes: 7 + sum of (s_next - s) = 7 + s[r] - s[0] - a closed form next to the model
    wide = traces[2]
    assert np.array_equal(wide[:, 5].astype(object), (7 + wide[:, 2].astype(object) - INIT) % P)


def test_aggregate_rounds_beyond_one(pkg, fe, ctx):
    """the one-workgroup launch over the tile aggregates scans 256 of them per round: twice that many tiles, both forms"""
    T = tile(pkg, fe)
    n = 2 * 256 * T
    assert n <= 1 << 20
    rng = np.random.default_rng(77)
    ops = operands(rng, n, 2, T)
    for r in (256 * T - 1, 256 * T, 256 * T + 1):  # and a restart around the seam between the two rounds
        ops[r, 0] = 0
    E = fe.Expr
    s = lab_system(pkg, fe, ctx)
    w = s.witness_from_device([dev(np.zeros((n, 1), dtype=np.uint64)), None, None], fe.pack_claims([]))
    inputs = dev(ops)
    w.fill(0, fe.compile_fill(1, 0, 2, [(0, fe.scan(E.input(0), E.input(1), init=INIT))]), inputs)
    affine = w.trace(0)[:, 0]
    w.fill(0, fe.compile_fill(1, 0, 2, [(0, fe.running_sum(E.input(1), init=INIT))]), inputs)
    additive = w.trace(0)[:, 0]
    want_affine, want_additive = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    a, b, s1, s2 = ops[:, 0].tolist(), ops[:, 1].tolist(), INIT, INIT
    for r in range(n):  # the definition, one loop for both
        want_affine[r], want_additive[r] = s1, s2
        s1, s2 = (a[r] * s1 + b[r]) % P, (s2 + b[r]) % P
    assert np.array_equal(affine, want_affine), np.nonzero(affine != want_affine)[0][:8]
    assert np.array_equal(additive, want_additive), np.nonzero(additive != want_additive)[0][:8]


@pytest.mark.parametrize("form", ["lds", "scratch"])
def test_both_forms_of_the_coefficient_pass(pkg, fe, ctx, form):
    T = tile(pkg, fe)
    E = fe.Expr
    m, x = E.input(0), E.input(1)
    leaves = [fe.bits(x + k, k % 57, 1 + k // 57) for k in range(300 if form == "scratch" else 8)]
    add = leaves[-1]
    for leaf in reversed(leaves[:-1]):  # every leaf is live before the first is consumed
        add = leaf - add
    prog = fe.compile_fill(2, 0, 3, [(0, m), (1, fe.scan(E.main(0), add, init=5))])
    info = pkg.fill_program_info(prog)
    assert (info["lds_lanes"] == 0) == (form == "scratch") and pkg.fill_scan_info(prog) == (1, 2, 0, T)
    rng = np.random.default_rng(len(leaves))
    n = 2 * T
    w, traces = lab_witness(pkg, fe, ctx, rng, n)
    rep = fill_against_model(pkg, w, traces, 1, prog, operands(rng, n, 3, T))
    assert rep.lds_lanes == info["lds_lanes"]


# ---------------------------------------------------------------- end to end: transition-constrained columns, filled and proved
ALPHA = (1 << 32) + 3


def airs(fe):
    """[running sum: columns (x, s); Horner: columns (x, acc)], each with is_first * s, is_transition * (s_next - A s - B) and a
    lookup pair that reads the scanned column"""
    def air(mul):
        def ev(b):
            local, nxt = b.main()
            b.when_first_row().assert_zero(local[1])
            b.when_transition().assert_zero(nxt[1] - mul * local[1] - local[0])
        E = fe.Expr
        return fe.lookup_air(2, ev, [fe.Lookup.push(1, [E.const(9), E.main(1)]), fe.Lookup.pull(1, [E.const(9), E.main(1)])])
    return [air(fe.Expr.const(1)), air(fe.Expr.const(ALPHA))]


@pytest.mark.parametrize("route", ["device", "held"])
def test_running_sum_and_horner_airs_end_to_end(pkg, fe, ctx, oracle, route):
    T = tile(pkg, fe)
    n = 2 * T
    E = fe.Expr
    if "e2e" not in _CACHE:
        s = pkg.System.new(ctx, fe.test_params(), airs(fe))
        x = operands(np.random.default_rng(31), n, 1, T)[:, 0]
        traces = []
        for mul in (1, ALPHA):
            col, acc = np.zeros(n, dtype=np.uint64), 0
            for r in range(n):
                col[r] = acc
                acc = (mul * acc + int(x[r])) % P
            traces.append(np.stack([x, col], axis=1))
        packed = fe.pack_claims([])
        _CACHE["e2e"] = (s, x, traces, packed, s.prove_multiple_claims(s.witness(traces, packed)).to_bytes())
    s, x, traces, packed, proof = _CACHE["e2e"]
    start = [np.stack([x, np.full(n, 5, dtype=np.uint64)], axis=1) for _ in range(2)]  # the scanned column holds something else
    if route == "device":
        w = s.witness_from_device([dev(t) for t in start], packed)
    else:
        osys = oracle.System(s.blob)
        w = s.witness(start, packed, lookups=[osys.compute_lookup_values(ci, t) for ci, t in enumerate(start)])
    assert np.array_equal(w.trace(0), start[0])  # (the read-back is a host wait: nothing of the setup is pending)
    before = ctx.sync_count()
    w.fill(0, fe.compile_fill(2, 0, 0, [(1, fe.running_sum(E.main(0)))]))
    w.fill(1, fe.compile_fill(2, 0, 0, [(1, fe.scan(ALPHA, E.main(0)))]))
    assert ctx.sync_count() == before  # no inputs: the calls only queue work, held lookup values included
    assert np.array_equal(w.trace(0), traces[0]) and np.array_equal(w.trace(1), traces[1])
    assert w.check().verdict == 0 and w.lookup_balance().ok
    got = s.prove_multiple_claims(w).to_bytes()
    assert got == proof and s.verify_multiple_claims(packed, got) == 0


# ---------------------------------------------------------------- refusals and host waits
def test_refusals_write_nothing_and_leave_the_context_usable(pkg, fe, ctx):
    T = tile(pkg, fe)
    n = 2 * T
    rng = np.random.default_rng(12)
    w, traces = lab_witness(pkg, fe, ctx, rng, n)
    E, N = fe.Expr, fe
    nodes = [(N.N_VAR, N.SRC_INPUT, 0, 0, 0), (N.N_CONST, 0, 0, 3, 0), (N.N_VAR, N.SRC_MAIN, 0, 1, 0), (N.N_VAR, N.SRC_MAIN, 1, 1, 0)]
    blob = lambda steps, scans: fe.fill_blob(2, 0, 1, nodes, steps, scans)
    good_inputs = operands(rng, n, 1, T)
    bad_inputs = good_inputs.copy()
    bad_inputs[T + 1, 0] = P
    good = fe.compile_fill(2, 0, 1, [(0, E.input(0)), (1, fe.scan(E.main(0), E.input(0), init=3))])
    cases = [(blob([(1, 2)], [(0, 1, 0)]), good_inputs, ("own dst",)),
             (blob([(1, 3)], [(0, 1, 0)]), good_inputs, ("own dst",)),
             (blob([(0, 0)], [(0, 1, P)]), good_inputs, ("init",)),
             (blob([(0, 0), (1, 0)], [(1, 1, 0), (0, 1, 0)]), good_inputs, ("ascending",)),
             (blob([(0, 0)], [(1, 1, 0)]), good_inputs, ("step index",)),
             (blob([(0, 0)], [(0, 4, 0)]), good_inputs, ("mul root",)),
             (blob([(0, 3), (1, 0)], [(1, 1, 0)]), good_inputs, ("offset-1",)),
             (blob([(0, 0)], [(0, 1, 0)])[:-8], good_inputs, ("truncated",)),
             (good.blob, bad_inputs, ("row %d" % (T + 1), "column 0")),  # found behind the compiler, before the first launch
             (good.blob, None, ("input",))]
    for program, inputs, words in cases:
        with pytest.raises(pkg.MstarkError) as e:
            w.fill(1, program, None if inputs is None else dev(inputs))
        assert str(e.value).startswith("ms_witness_fill: ") and all(x in str(e.value) for x in words), str(e.value)
        assert all(np.array_equal(w.trace(ci), traces[ci]) for ci in range(len(WIDTHS)))
    for what, program, _ in scan_refusal_blobs(fe)[1]:  # the host-only cases, widths (2, 1): refused as a program before the widths are compared
        with pytest.raises(pkg.MstarkError):
            w.fill(1, program, dev(good_inputs))
    assert all(np.array_equal(w.trace(ci), traces[ci]) for ci in range(len(WIDTHS)))
    fill_against_model(pkg, w, traces, 1, good, good_inputs)  # the context and the witness are as good as new


def test_host_waits(pkg, fe, ctx):
    T = tile(pkg, fe)
    n = 2 * T
    rng = np.random.default_rng(13)
    w, traces = lab_witness(pkg, fe, ctx, rng, n)
    E = fe.Expr
    no_inputs = fe.compile_fill(14, 0, 0, [(0, E.row() + 1), (1, fe.scan(E.main(0), E.main(13))), (2, E.main_next(1)), (3, fe.running_sum(E.main(2)))])
    assert np.array_equal(w.trace(2), traces[2])  # (the read-back is a host wait: nothing of the setup is pending)
    before = ctx.sync_count()
    w.fill(2, no_inputs)
    assert ctx.sync_count() == before  # two scans, four groups: the call only queues work (include/mstark.h, "Host waits")
    assert np.array_equal(w.trace(2), fsm.run(no_inputs.blob, traces[2]))
    with_inputs = fe.compile_fill(1, 0, 1, [(0, fe.running_sum(E.input(0)))])
    inputs = dev(operands(rng, n, 1, T))
    torch.cuda.synchronize()
    before = ctx.sync_count()
    w.fill(0, with_inputs, inputs)
    assert ctx.sync_count() == before + 1  # the offender word of the inputs, as without scans
