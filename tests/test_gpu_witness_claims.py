"""`-m gpu`: ms_witness_claims_fill (csrc/fill.hip, csrc/claims_dev.h) against the model of tests/claims_model.py, which
tests/test_claims_model.py pins to the definition. Every comparison is exact, device against model, through
SystemWitness.claims(), which reads the device copy of the claims.

The lab system: a circuit of 14 columns without a preprocessed trace and one of 6 columns with a 2-column preprocessed trace of
2048 rows. Heights 1, 2, 64, 256, 1024 (one compaction tile exactly) and 2048 (two). No index asks the device to read out of
bounds: an index from the source's height on reads 0 by definition, and that value is what is checked. After every call every
trace is compared with what it held, and the report with claims_program_info."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the library opens the device)

import claims_model as cm

pytestmark = pytest.mark.gpu
P = cm.P
_CACHE = {}
MAIN, PRE, PRE_H = 0, 1, 2048
WIDTHS = (14, 6)
HEIGHTS = (1, 2, 64, 256, 1024, 2048)
TILE = 1024


def dev(a):
    """a numpy array of unsigned integers as a torch tensor on the GPU (same bits, same element size)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])).cuda()


def lab_system(pkg, fe, ctx):
    """Nothing is ever proved with it: the constraints are placeholders. -> (system, its preprocessed traces per circuit)"""
    if "lab" not in _CACHE:
        E = fe.Expr
        c = [E.main(0) * E.main(0) - E.main(0)]
        pre = np.random.default_rng(77).integers(0, P, size=(PRE_H, 2), dtype=np.uint64)
        pre[5, 1], pre[PRE_H - 1, 0] = P - 1, 0
        s = pkg.System.new(ctx, fe.test_params(), [fe.CircuitInputs(WIDTHS[MAIN], None, c, [], []), fe.CircuitInputs(WIDTHS[PRE], pre, c, [], [])])
        _CACHE["lab"] = (s, [None, pre])
    return _CACHE["lab"]


def lab_traces(rng, heights):
    """random traces, None for the inactive; column 1 holds row indices in [0, 2 h) with the edges h - 1, h, p - 1, 2^32 + 1"""
    out = []
    for ci, h in enumerate(heights):
        if not h:
            out.append(None)
            continue
        t = rng.integers(0, P, size=(h, WIDTHS[ci]), dtype=np.uint64)
        t[:, 1] = rng.integers(0, 2 * h, size=h, dtype=np.uint64)
        for k, e in enumerate((h - 1, h, P - 1, (1 << 32) + 1, 0)):
            t[(7 * k) % h, 1] = e
        t[h - 1, 0] = P - 1
        out.append(t)
    return out


def lab_witness(pkg, fe, ctx, traces, claims=()):
    s, _ = lab_system(pkg, fe, ctx)
    return s.witness_from_device([None if t is None else dev(t) for t in traces], fe.pack_claims([list(c) for c in claims]))


def same_traces(w, traces):
    for ci, t in enumerate(traces):
        if t is not None:
            assert np.array_equal(w.trace(ci), t), "the trace of circuit %d changed" % ci


def fill_against_model(pkg, fe, ctx, w, traces, ci, prog, rows=None, inputs=None, append=False):
    """the call on the device and in the model: the witness's claims afterwards, the report, the traces"""
    _, pres = lab_system(pkg, fe, ctx)
    before = w.claims()
    n = traces[ci].shape[0]
    want = cm.claims(prog.blob, traces[ci], pres[ci], inputs, n if rows is None else rows, before if append else None)
    rep = w.fill_claims(ci, prog, rows, None if inputs is None else dev(inputs), append=append)
    got = w.claims()
    assert np.array_equal(got[0], want[0]), "offsets: %s" % (np.nonzero(got[0][: len(want[0])] != want[0][: len(got[0])])[0][:8],)
    assert np.array_equal(got[1], want[1]), "elements differ first at %s" % (np.nonzero(got[1] != want[1])[0][:8],)
    if append:  # the old claims stay, the offsets continue
        assert np.array_equal(got[0][: len(before[0])], before[0]) and np.array_equal(got[1][: len(before[1])], before[1])
    info = pkg.claims_program_info(prog)
    emitted = len(want[0]) - (len(before[0]) if append else 1)
    assert rep.fields() == (n if rows is None else rows, emitted, info["instructions"], info["lds_lanes"]), str(rep)
    same_traces(w, traces)
    return rep


def lab_program(fe, keep=None, n_inputs=2):
    """W = 4 over the 14-column circuit: every kind of read a claim program has, the ones a fill program refuses of assigned
    columns included (nothing is assigned here)"""
    E = fe.Expr
    return fe.compile_claims(14, 0, n_inputs, [E.main(0) + E.main_next(2) * 3, E.main_at(3, E.main(1)) + E.row(), E.input(0) - E.input_next(0),
                                               fe.bits(E.main(4), 5, 20) + E.input_at(0, E.main(1)) * fe.lt(E.main(5), E.main(6))], keep=keep)


def rows_for(n):
    return sorted({0, 1, n - 1, n} | ({TILE - 1, TILE, TILE + 1} if n == 2 * TILE else set()))


@pytest.mark.parametrize("n", HEIGHTS)
def test_lab_circuit_heights_and_rows(pkg, fe, ctx, n):
    E = fe.Expr
    rng = np.random.default_rng(8100 + n)
    traces = lab_traces(rng, [n, 0])
    h_in = (n + 1) // 2  # rows from here on read 0
    inputs = np.stack([rng.integers(0, P, size=h_in, dtype=np.uint64), rng.integers(0, 3, size=h_in, dtype=np.uint64)], axis=1)
    plain, masked = lab_program(fe), lab_program(fe, keep=E.main(7) + E.input(1))
    traces[MAIN][:, 7] = np.where(rng.integers(0, 2, size=n), 0, traces[MAIN][:, 7])  # about half the rows behind the inputs are dropped
    w = lab_witness(pkg, fe, ctx, traces)
    for rows in rows_for(n):
        assert fill_against_model(pkg, fe, ctx, w, traces, MAIN, plain, rows, inputs).claims == rows
        fill_against_model(pkg, fe, ctx, w, traces, MAIN, masked, rows, inputs)
    fill_against_model(pkg, fe, ctx, w, traces, MAIN, plain, None, inputs)  # rows=None: the whole height


def test_preprocessed_circuit(pkg, fe, ctx):
    E = fe.Expr
    rng = np.random.default_rng(8200)
    traces = lab_traces(rng, [64, PRE_H])
    w = lab_witness(pkg, fe, ctx, traces)
    prog = fe.compile_claims(6, 2, 0, [E.preprocessed(0) + E.main(0), E.var(fe.SRC_PRE, 1, 1) * E.main_next(5), E.pre_at(1, E.main(1))], keep=fe.bits(E.preprocessed(1), 0, 1))
    for rows in (PRE_H, TILE + 1, 1):
        fill_against_model(pkg, fe, ctx, w, traces, PRE, prog, rows)
    # pre_at at an index from the height on is 0, and the last row's next row is row 0
    offs, data = w.claims()
    assert len(offs) - 1 == int(lab_system(pkg, fe, ctx)[1][PRE][0, 1]) & 1
    fill_against_model(pkg, fe, ctx, w, traces, MAIN, fe.compile_claims(14, 0, 0, [E.main(13)]), append=True)  # another circuit's claims behind them


def keep_patterns(rng, n):
    r = np.arange(n)
    pats = {"all rows": np.ones(n), "no row": np.zeros(n), "first row only": r == 0, "last row only": r == n - 1, "alternating": r % 2,
            "either side of the tile boundary": (r == TILE - 1) | (r == TILE), "density 1/64": rng.integers(0, 64, size=n) == 0,
            "density 63/64": rng.integers(0, 64, size=n) != 0}
    return {k: np.asarray(v).astype(np.uint64) for k, v in pats.items()}


@pytest.mark.parametrize("n", [TILE, 2 * TILE])
def test_keep_patterns(pkg, fe, ctx, n):
    """the mask is an input column, so one witness serves every pattern; a kept flag may be any non-zero value"""
    E = fe.Expr
    rng = np.random.default_rng(8300 + n)
    traces = lab_traces(rng, [n, 0])
    w = lab_witness(pkg, fe, ctx, traces)
    prog = lab_program(fe, keep=E.input(1))
    absent = lab_program(fe)
    values = rng.integers(0, P, size=n, dtype=np.uint64)
    assert fill_against_model(pkg, fe, ctx, w, traces, MAIN, absent, n, np.stack([values, np.zeros(n, dtype=np.uint64)], axis=1)).claims == n
    for name, mask in keep_patterns(rng, n).items():
        flag = mask * rng.integers(1, P, size=n, dtype=np.uint64)
        rep = fill_against_model(pkg, fe, ctx, w, traces, MAIN, prog, n, np.stack([values, flag], axis=1))
        assert rep.claims == int(mask.sum()), name


WIDTH_CASES = [(1, 256), (4, 256), (49, 128), (100, 64), (200, 0)]


@pytest.mark.parametrize("width,lanes", WIDTH_CASES)
def test_widths_and_kernel_forms(pkg, fe, ctx, width, lanes):
    """W = 1, 4 and 49 (the BLAKE3 system's claims), and the slot file at 256 / 128 / 64 lanes and in the global scratch: every
    element stays live to the end of the row, so W distinct elements need at least W slots"""
    E = fe.Expr
    rng = np.random.default_rng(8400 + width)
    n = 2 * TILE
    traces = lab_traces(rng, [n, 0])
    traces[MAIN][:, 9] = rng.integers(0, 3, size=n, dtype=np.uint64)
    w = lab_witness(pkg, fe, ctx, traces)
    elements = [E.main(k % 3) * (k + 2) + E.main_next(3 + k % 2) for k in range(width)]  # (few columns: a loaded column stays live too)
    plain, masked = fe.compile_claims(14, 0, 0, elements), fe.compile_claims(14, 0, 0, elements, keep=E.main(9))
    for prog in (plain, masked):
        info = pkg.claims_program_info(prog)
        assert info["lds_lanes"] == lanes and info["width"] == width, info
    small = width > 49  # (the model walks every node of every row: the wide programs get fewer rows, the same paths)
    fill_against_model(pkg, fe, ctx, w, traces, MAIN, plain, 300 if small else TILE + 300)
    for rows in (TILE + 1, 700) if small else (n, TILE + 1, 700):  # two tiles, a second tile of one row, one tile
        fill_against_model(pkg, fe, ctx, w, traces, MAIN, masked, rows)
    fill_against_model(pkg, fe, ctx, w, traces, MAIN, masked, 300 if small else n, append=True)


def test_append(pkg, fe, ctx):
    E = fe.Expr
    rng = np.random.default_rng(8500)
    n = 2 * TILE
    traces = lab_traces(rng, [n, PRE_H])
    s, _ = lab_system(pkg, fe, ctx)
    ragged = [[1, 2, 3], [], [P - 1], [4, 5, 6, 7, 8]]  # a host-given list, through ms_witness_create
    w = s.witness(traces, fe.pack_claims(ragged))
    offs, data = w.claims()
    assert offs.tolist() == [0, 3, 3, 4, 9] and data.tolist() == [1, 2, 3, P - 1, 4, 5, 6, 7, 8]
    three = fe.compile_claims(14, 0, 0, [E.main(0), E.row(), E.main_next(13)], keep=fe.bits(E.main(2), 0, 2))
    two = fe.compile_claims(6, 2, 0, [E.preprocessed(0), E.main(5)])
    fill_against_model(pkg, fe, ctx, w, traces, MAIN, three, append=True)        # behind the ragged list, two tiles with a mask
    fill_against_model(pkg, fe, ctx, w, traces, PRE, two, 5, append=True)        # another circuit, another width
    fill_against_model(pkg, fe, ctx, w, traces, MAIN, three, 0, append=True)     # nothing emitted: the list stays
    offs, data = w.claims()
    assert offs[:5].tolist() == [0, 3, 3, 4, 9] and data[:9].tolist() == [1, 2, 3, P - 1, 4, 5, 6, 7, 8] and offs[-1] == len(data)
    assert np.array_equal(np.diff(offs[-6:]), np.full(5, 2, dtype=np.uint64))
    fill_against_model(pkg, fe, ctx, w, traces, PRE, two, 3)                     # replace ...
    assert w.claims()[0].tolist() == [0, 2, 4, 6]
    fill_against_model(pkg, fe, ctx, w, traces, MAIN, three, TILE, append=True)  # ... and append after replace
    fill_against_model(pkg, fe, ctx, w, traces, MAIN, three, 0)                  # replace by nothing
    assert w.claims()[0].tolist() == [0] and w.claims()[1].size == 0
    # the Level-2 view of the claims follows: the accumulator of the device list is that of the same list given by the host
    fill_against_model(pkg, fe, ctx, w, traces, PRE, two, 4)
    offs, data = w.claims()
    given = s.witness(traces, (offs, data))
    beta, gamma = (3, 5), (7, 11)
    assert w.claims_accumulator(beta, gamma) == given.claims_accumulator(beta, gamma)


def test_refusals_leave_the_witness_as_it_was(pkg, fe, ctx):
    E = fe.Expr
    rng = np.random.default_rng(8600)
    n = 2 * TILE
    traces = lab_traces(rng, [n, 0])
    s, _ = lab_system(pkg, fe, ctx)
    start = [[9, 8], [7]]
    w = lab_witness(pkg, fe, ctx, traces, start)
    claims0 = w.claims()
    prog, keep = lab_program(fe), lab_program(fe, keep=E.input(1))
    inputs = np.stack([rng.integers(0, P, size=n, dtype=np.uint64), rng.integers(0, 2, size=n, dtype=np.uint64)], axis=1)
    d_inputs = dev(inputs)

    def refused(text, call):
        with pytest.raises(pkg.MstarkError, match=text) as e:
            call()
        assert str(e.value).startswith("ms_witness_claims_fill: ") or "fill_claims inputs" in str(e.value), str(e.value)
        got = w.claims()
        assert np.array_equal(got[0], claims0[0]) and np.array_equal(got[1], claims0[1]), text
        same_traces(w, traces)

    def raw(mode, system=s):
        a = np.frombuffer(prog.blob, dtype=np.uint8)
        summary = np.zeros(4, dtype=np.uint64)
        mat = pkg.DevMatrix(d_inputs.data_ptr(), n, 8, 2, 1)
        rows = n
        rc = pkg.lib().ms_witness_claims_fill(system.h, w.h, C.c_size_t(MAIN), a.ctypes.data_as(pkg.u8p), C.c_size_t(a.size), C.c_size_t(rows), C.byref(mat),
                                              None, C.c_uint32(mode), summary.ctypes.data_as(pkg.u64p))
        if rc:
            raise pkg.MstarkError(pkg.lib().ms_last_error().decode())

    for append in (False, True):
        refused(r"rows 2049 is above the circuit's height 2048", lambda: w.fill_claims(MAIN, prog, n + 1, d_inputs, append=append))
        refused(r"circuit 1 is inactive \(height 0\)", lambda: w.fill_claims(PRE, fe.compile_claims(6, 2, 0, [E.main(0)]), 0, append=append))
        refused(r"circuit 2 is out of range", lambda: w.fill_claims(2, prog, 1, d_inputs, append=append))
        refused(r"the program is for main_width 13 and preprocessed width 0, circuit 0 has 14 and 0", lambda: w.fill_claims(MAIN, fe.compile_claims(13, 0, 0, [E.main(0)]), append=append))
        refused(r"the program is for main_width 14 and preprocessed width 1, circuit 0 has 14 and 0", lambda: w.fill_claims(MAIN, fe.compile_claims(14, 1, 0, [E.main(0)]), append=append))
        refused(r"the program reads 2 input columns and no input matrix was given", lambda: w.fill_claims(MAIN, keep, append=append))
        refused(r"input height 4096 is above the circuit's height 2048", lambda: w.fill_claims(MAIN, keep, n, dev(np.zeros((2 * n, 2), dtype=np.uint64)), append=append))
        refused(r"fill_claims inputs: width 3, the program reads 2 input columns", lambda: w.fill_claims(MAIN, keep, n, dev(np.zeros((n, 3), dtype=np.uint64)), append=append))
        refused(r"a fill program, not a claim program", lambda: w.fill_claims(MAIN, fe.compile_fill(14, 0, 0, [(0, E.main(1))]), append=append))
    refused(r"mode 2 \(MS_CLAIMS_REPLACE = 0, MS_CLAIMS_APPEND = 1\)", lambda: raw(2))
    refused(r"mode 4294967295", lambda: raw(0xFFFFFFFF))
    # a non-canonical input value, with its row and column: the evaluation has run by then, into buffers of the call alone
    for program in (prog, keep):
        for (r, c, v) in ((0, 0, P), (TILE + 7, 1, (1 << 64) - 1), (n - 1, 0, P + 5)):
            bad = inputs.copy()
            bad[r, c] = v
            if r < n - 1:
                bad[n - 1, 1] = P  # a later offender is not the one named
            for append in (False, True):
                refused(r"non-canonical input value: row %d, column %d$" % (r, c), lambda: w.fill_claims(MAIN, program, n, dev(bad), append=append))
    # witnesses this call does not take; each is refused before anything else is looked at
    other = pkg.System.new(ctx, fe.test_params(), [fe.CircuitInputs(14, None, [E.main(0) * E.main(0) - E.main(0)], [], [])])
    refused(r"the witness does not belong to this system", lambda: raw(0, other))
    packed = fe.pack_claims(start)
    host = s.host_witness(traces, packed)
    with pytest.raises(pkg.MstarkError, match=r"ms_witness_claims_fill: takes a device-resident witness"):
        host.fill_claims(MAIN, prog, n, d_inputs)
    with pytest.raises(pkg.MstarkError, match=r"ms_witness_claims: a host-resident witness"):
        host.claims()
    remote = s.witness([traces[MAIN], None], packed, remote_heights={PRE: PRE_H})
    with pytest.raises(pkg.MstarkError, match=r"ms_witness_claims_fill: this witness lacks traces that another rank computes"):
        remote.fill_claims(MAIN, prog, n, d_inputs)
    assert np.array_equal(remote.claims()[0], packed[0]) and np.array_equal(remote.claims()[1], packed[1]) and np.array_equal(remote.trace(MAIN), traces[MAIN])
    sliced = s.host_witness_sliced(traces, packed[0], 1, packed[1][1:2], packed[1])
    with pytest.raises(pkg.MstarkError, match=r"ms_witness_claims_fill: this witness holds only a slice of its claims"):
        sliced.fill_claims(MAIN, prog, n, d_inputs)
    with pytest.raises(pkg.MstarkError, match=r"ms_witness_claims: this witness holds only a slice of its claims"):
        sliced.claims()
    # ms_witness_claims with buffers that are too small: MS_ERR_BUFFER and the needed sizes, nothing written
    nc, ne = C.c_size_t(), C.c_size_t()
    offs, data = np.full(3, 99, dtype=np.uint64), np.full(3, 99, dtype=np.uint64)
    for cap_o, cap_d in ((2, 3), (3, 2), (0, 0)):
        rc = pkg.lib().ms_witness_claims(w.h, offs.ctypes.data_as(pkg.u64p), C.c_size_t(cap_o), data.ctypes.data_as(pkg.u64p), C.c_size_t(cap_d), C.byref(nc), C.byref(ne))
        assert (rc, nc.value, ne.value) == (-3, 2, 3) and offs.tolist() == [99] * 3 and data.tolist() == [99] * 3
    # the context is usable and the witness takes the next call
    same_traces(w, traces)
    fill_against_model(pkg, fe, ctx, w, traces, MAIN, keep, n, inputs, append=True)


def test_end_to_end_u32_add(pkg, fe, ctx, oracle):
    """pairs -> fill -> fill_claims -> derive_multiplicities -> check -> prove, from zero traces and no claims"""
    n = 1 << 10
    s = pkg.System.new(ctx, fe.bench_params(), fe.u32_add_system_inputs())
    xs, ys = fe.xorshift_pairs(n)
    traces, claims = fe._u32_add_traces(xs, ys, n)
    packed = fe.pack_claims(claims)
    w = s.witness_from_device([dev(np.zeros_like(t)) for t in traces], fe.pack_claims([]))
    w.fill(1, fe.u32_add_fill_program(n), dev(np.stack([xs, ys], axis=1).astype(np.uint32)))
    # before fill_claims nothing balances: every byte that occurs is pushed and the table's multiplicities are still zero, and every
    # addition is pulled by the circuit and claimed by nobody
    used_bytes = len(np.unique(traces[1][:, :12]))
    additions = len(np.unique(claims, axis=0))
    before = w.lookup_balance()
    assert not before.ok and before.unbalanced == used_bytes + additions and before.claims_count == 0
    assert before.slot_counts[1][0] == n and sum(before.slot_counts[1][1:]) == 12 * n
    rep = w.fill_claims(1, fe.u32_add_claims_program(), rows=n)
    info = pkg.claims_program_info(fe.u32_add_claims_program())
    assert rep.fields() == (n, n, info["instructions"], info["lds_lanes"]) and info["lds_lanes"] == 256
    offs, data = w.claims()
    assert np.array_equal(offs, packed[0]) and np.array_equal(data, packed[1]) and np.array_equal(data.reshape(n, 4), claims)
    between = w.lookup_balance()
    assert not between.ok and between.unbalanced == used_bytes and between.slot_counts[1][0] == 0 and between.claims_count == 0
    assert w.derive_multiplicities([(0, 0)]).ok
    assert np.array_equal(w.trace(0), traces[0]) and np.array_equal(w.trace(1), traces[1])
    assert w.lookup_balance().ok and w.check().verdict == 0
    proof = s.prove_multiple_claims(w).to_bytes()
    assert proof == s.prove_multiple_claims(s.witness(traces, packed)).to_bytes()
    osys = oracle.System(s.blob)
    assert proof == osys.prove(traces, packed) and osys.verify(packed, proof) == 0
    # the generator of the bench workload holds the same claims
    g_offs, g_data = s.bench_witness_on_device(n).claims()
    assert np.array_equal(g_offs, offs) and np.array_equal(g_data, data)
