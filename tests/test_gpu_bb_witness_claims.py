"""`-m gpu`: msbb_witness_claims_fill (csrc/bb_fill.hip, csrc/claims_fill.h, csrc/claims_dev.h) against the model of
tests/claims_model_bb.py, which tests/test_bb_claims_model.py pins to the definition. Every comparison is exact, device against
model, through Witness.claims(), which reads the device copy of the claims and shows canonical values.

The lab system, under field(BABYBEAR): a circuit of 14 columns without a preprocessed trace and one of 6 columns with a 2-column
preprocessed trace of 2048 rows. Heights 1, 2, 64, 256, 1024 (one compaction tile exactly) and 2048 (two). No index asks the
device to read out of bounds: an index from the source's height on reads 0 by definition, and that value is what is checked.
After every call every trace is compared with what it held, and the report with claims_program_info.

Two refusals of the list in include/mstark_bb.h cannot be reached through the interface and are not provoked here: the system
comes from the witness, so no call pairs a witness with another system, and msbb_witness_create_device refuses a circuit whose
height differs from its preprocessed trace's, so no witness holds one. The driver keeps both checks."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the library opens the device)

import claims_model_bb as cb
from test_bb_fill_model import halves
from test_bb_witness_check_model import K, bb, fe, pack, pkg
from test_gpu_bb_lookup_balance import ctx  # noqa: F401  (the module-scoped context with the Poseidon2 permutation set)

pytestmark = pytest.mark.gpu
P = cb.P
_CACHE = {}
MAIN, PRE, PRE_H = 0, 1, 2048
WIDTHS = (14, 6)
HEIGHTS = (1, 2, 64, 256, 1024, 2048)
TILE = 1024
EDGES = (0, 1, P - 1, P - 2, 1 << 30, (1 << 27) - 1)
U = {1: np.uint8, 2: np.uint16, 4: np.uint32}


def dev(a):
    """a numpy array of unsigned integers as a torch tensor on the GPU (same bits, same element size)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])).cuda()


def dev32(a):
    return dev(np.asarray(a).astype(np.uint32))


def rand_field(rng, shape, below=P):
    """values in [0, below), the edges of the field mixed in where they fit"""
    a = rng.integers(0, below, size=shape, dtype=np.uint64)
    flat = a.reshape(-1)
    for e in EDGES:
        if flat.size and e < below:
            flat[rng.integers(0, flat.size)] = e
    return a


def lab_system(ctx):
    """Nothing is ever proved with it: the constraints are placeholders. -> (system, its preprocessed traces per circuit)"""
    if "lab" not in _CACHE:
        E = fe.Expr
        pre = rand_field(np.random.default_rng(77), (PRE_H, 2))
        pre[5, 1], pre[PRE_H - 1, 0] = P - 1, 0
        with fe.field(fe.BABYBEAR):
            c = [E.main(0) * E.main(0) - E.main(0)]
            inputs = [fe.CircuitInputs(WIDTHS[MAIN], None, c, [], []), fe.CircuitInputs(WIDTHS[PRE], pre, c, [], [])]
            _CACHE["lab"] = (bb.System.new(ctx, fe.test_params(), inputs, K), [None, pre])
    return _CACHE["lab"]


def lab_traces(rng, heights):
    """random traces with the field's edges, None for the inactive; column 1 holds row indices in [0, 2 h) with the edges h - 1,
    h, p - 1 and 0"""
    out = []
    for ci, h in enumerate(heights):
        if not h:
            out.append(None)
            continue
        t = rand_field(rng, (h, WIDTHS[ci]))
        t[:, 1] = rng.integers(0, 2 * h, size=h, dtype=np.uint64)
        for k, e in enumerate((h - 1, h, P - 1, 0)):
            t[(7 * k) % h, 1] = e
        t[h - 1, 0] = P - 1
        out.append(t)
    return out


def lab_witness(ctx, traces, claims=()):
    s, _ = lab_system(ctx)
    return s.witness_from_device([None if t is None else dev32(t) for t in traces], pack([list(c) for c in claims]))


def same_traces(w, traces):
    for ci, t in enumerate(traces):
        if t is not None:
            assert np.array_equal(w.trace(ci).astype(np.uint64), t), "the trace of circuit %d changed" % ci


def same_claims(got, want, what=""):
    assert got[1].dtype == np.uint32
    assert np.array_equal(got[0], want[0]), "offsets %s" % what
    assert np.array_equal(got[1], np.asarray(want[1], dtype=np.uint32)), "elements differ first at %s %s" % (np.nonzero(got[1] != want[1])[0][:8], what)


def on_device(inputs, eb=4, strided=False):
    if inputs is None:
        return None
    if strided:  # h x w with strides (1, h): column-major
        t = dev(np.ascontiguousarray(inputs.T).astype(U[eb])).t()
        assert tuple(t.shape) == inputs.shape and (inputs.shape[0] == 1 or t.stride() == (1, inputs.shape[0]))
        return t
    return dev(inputs.astype(U[eb]))


def fill_against_model(ctx, w, traces, ci, prog, rows=None, inputs=None, eb=4, append=False, strided=False):
    """the call on the device and in the model: the witness's claims afterwards, the report, the traces"""
    _, pres = lab_system(ctx)
    before = w.claims()
    n = traces[ci].shape[0]
    want = cb.claims(prog.blob, traces[ci], pres[ci], inputs, n if rows is None else rows, before if append else None)
    rep = w.fill_claims(ci, prog, rows, on_device(inputs, eb, strided), append=append)
    got = w.claims()
    same_claims(got, want)
    if append:  # the old claims stay, the offsets continue
        assert np.array_equal(got[0][: len(before[0])], before[0]) and np.array_equal(got[1][: len(before[1])], before[1])
    info = bb.claims_program_info(prog)
    emitted = len(want[0]) - (len(before[0]) if append else 1)
    assert rep.fields() == (n if rows is None else rows, emitted, info["instructions"], info["lds_lanes"]), str(rep)
    same_traces(w, traces)
    return rep


def lab_program(keep=None, n_inputs=2):
    """W = 4 over the 14-column circuit: every kind of read a claim program has, the ones a fill program refuses of assigned
    columns included (nothing is assigned here)"""
    E = fe.Expr
    with fe.field(fe.BABYBEAR):
        return fe.compile_claims(14, 0, n_inputs, [E.main(0) + E.main_next(2) * 3, E.main_at(3, E.main(1)) + E.row(), E.input(0) - E.input_next(0),
                                                   fe.bits(E.main(4), 5, 20) + E.input_at(0, E.main(1)) * fe.lt(E.main(5), E.main(6))], keep=keep)


def rows_for(n):
    return sorted({0, 1, n - 1, n} | ({TILE - 1, TILE, TILE + 1} if n == 2 * TILE else set()))


@pytest.mark.parametrize("n", HEIGHTS)
def test_lab_circuit_heights_and_rows(ctx, n):
    E = fe.Expr
    rng = np.random.default_rng(9100 + n)
    traces = lab_traces(rng, [n, 0])
    h_in = (n + 1) // 2  # rows from here on read 0
    inputs = {eb: np.stack([rand_field(rng, h_in, below=min(P, 1 << (8 * eb))), rng.integers(0, 3, size=h_in, dtype=np.uint64)], axis=1) for eb in U}
    plain, masked = lab_program(), lab_program(keep=E.main(7) + E.input(1))
    traces[MAIN][:, 7] = np.where(rng.integers(0, 2, size=n), 0, traces[MAIN][:, 7])  # about half the rows behind the inputs are dropped
    w = lab_witness(ctx, traces)
    k = 0
    for rows in rows_for(n):
        for prog in (plain, masked):  # the element sizes take turns
            eb = (1, 2, 4)[k % 3]
            k += 1
            rep = fill_against_model(ctx, w, traces, MAIN, prog, rows, inputs[eb], eb)
            assert prog is masked or rep.claims == rows
    for eb in U:  # rows=None: the whole height, at every element size
        fill_against_model(ctx, w, traces, MAIN, masked, None, inputs[eb], eb)
    fill_against_model(ctx, w, traces, MAIN, plain, None, inputs[2], 2, strided=True)
    fill_against_model(ctx, w, traces, MAIN, masked, None, inputs[4], 4, strided=True)


def test_preprocessed_circuit(ctx):
    E = fe.Expr
    rng = np.random.default_rng(9200)
    traces = lab_traces(rng, [64, PRE_H])
    w = lab_witness(ctx, traces)
    with fe.field(fe.BABYBEAR):
        prog = fe.compile_claims(6, 2, 0, [E.preprocessed(0) + E.main(0), E.var(fe.SRC_PRE, 1, 1) * E.main_next(5), E.pre_at(1, E.main(1))],
                                 keep=fe.bits(E.preprocessed(1), 0, 1))
    for rows in (PRE_H, TILE + 1, 1):
        fill_against_model(ctx, w, traces, PRE, prog, rows)
    # with rows = 1 the one claim is there exactly when the flag of row 0 is set
    assert len(w.claims()[0]) - 1 == int(lab_system(ctx)[1][PRE][0, 1]) & 1
    with fe.field(fe.BABYBEAR):
        fill_against_model(ctx, w, traces, MAIN, fe.compile_claims(14, 0, 0, [E.main(13)]), append=True)  # another circuit's claims behind them


def keep_patterns(rng, n):
    r = np.arange(n)
    pats = {"all rows": np.ones(n), "no row": np.zeros(n), "first row only": r == 0, "last row only": r == n - 1, "alternating": r % 2,
            "either side of the tile boundary": (r == TILE - 1) | (r == TILE), "density 1/64": rng.integers(0, 64, size=n) == 0,
            "density 63/64": rng.integers(0, 64, size=n) != 0}
    return {k: np.asarray(v).astype(np.uint64) for k, v in pats.items()}


@pytest.mark.parametrize("n", [TILE, 2 * TILE])
def test_keep_patterns(ctx, n):
    """the mask is an input column, so one witness serves every pattern; a kept flag may be any non-zero value, 1 and p - 1 among
    them: the device compares the Montgomery word, which is 0 exactly when the value is"""
    E = fe.Expr
    rng = np.random.default_rng(9300 + n)
    traces = lab_traces(rng, [n, 0])
    w = lab_witness(ctx, traces)
    prog, absent = lab_program(keep=E.input(1)), lab_program()
    values = rand_field(rng, n)
    assert fill_against_model(ctx, w, traces, MAIN, absent, n, np.stack([values, np.zeros(n, dtype=np.uint64)], axis=1)).claims == n
    for name, mask in keep_patterns(rng, n).items():
        flag = mask * rng.integers(1, P, size=n, dtype=np.uint64)
        kept = np.nonzero(mask)[0]
        for at, v in zip(kept[:2], (1, P - 1)):
            flag[at] = v
        rep = fill_against_model(ctx, w, traces, MAIN, prog, n, np.stack([values, flag], axis=1))
        assert rep.claims == int(mask.sum()), name


def wide_elements(width):
    """W distinct elements over few columns: every element stays live to the end of the row, so W elements need at least W slots"""
    E = fe.Expr
    return [E.main(k % 3) * (k + 2) + E.main_next(3 + k % 2) for k in range(width)]


# 4-byte slots: 256 lanes up to 64 live slots, 128 up to 128, 64 up to 256, else the global scratch
WIDTH_CASES = [(1, 256), (4, 256), (49, 256), (100, 128), (200, 64), (300, 0)]


@pytest.mark.parametrize("width,lanes", WIDTH_CASES)
def test_widths_and_kernel_forms(ctx, width, lanes):
    E = fe.Expr
    rng = np.random.default_rng(9400 + width)
    n = 2 * TILE
    traces = lab_traces(rng, [n, 0])
    traces[MAIN][:, 9] = rng.integers(0, 3, size=n, dtype=np.uint64)
    w = lab_witness(ctx, traces)
    plain, masked = bb.compile_claims(14, 0, 0, wide_elements(width)), bb.compile_claims(14, 0, 0, wide_elements(width), keep=E.main(9))
    for prog in (plain, masked):
        info = bb.claims_program_info(prog)
        assert info["lds_lanes"] == lanes and info["width"] == width, info
    small = width > 49  # (the model walks every node of every row: the wide programs get fewer rows, the same paths)
    fill_against_model(ctx, w, traces, MAIN, plain, 300 if small else TILE + 300)
    for rows in (700, TILE + 1, TILE + 40) if small else (700, TILE + 1, n):  # one tile, a second tile of one row, two tiles
        fill_against_model(ctx, w, traces, MAIN, masked, rows)
    fill_against_model(ctx, w, traces, MAIN, masked, 300 if small else n, append=True)
    assert {f for _, f in WIDTH_CASES} == {256, 128, 64, 0}


def test_append(ctx):
    E = fe.Expr
    rng = np.random.default_rng(9500)
    n = 2 * TILE
    traces = lab_traces(rng, [n, PRE_H])
    s, _ = lab_system(ctx)
    ragged = [[1, 2, 3], [], [P - 1], [4, 5, 6, 7, 8]]  # a host-given list of nine elements: what follows starts at an odd word
    w = lab_witness(ctx, traces, ragged)
    offs, data = w.claims()
    assert offs.tolist() == [0, 3, 3, 4, 9] and data.tolist() == [1, 2, 3, P - 1, 4, 5, 6, 7, 8]
    with fe.field(fe.BABYBEAR):
        three = fe.compile_claims(14, 0, 0, [E.main(0), E.row(), E.main_next(13)], keep=fe.bits(E.main(2), 0, 2))
        bare = fe.compile_claims(14, 0, 0, [E.main(0), E.row(), E.main_next(13)])
        two = fe.compile_claims(6, 2, 0, [E.preprocessed(0), E.main(5)])
    fill_against_model(ctx, w, traces, MAIN, three, append=True)        # behind the ragged list, two tiles with a mask
    fill_against_model(ctx, w, traces, PRE, two, 5, append=True)        # another circuit, another width
    fill_against_model(ctx, w, traces, MAIN, three, 0, append=True)     # nothing emitted: the list stays
    offs, data = w.claims()
    assert offs[:5].tolist() == [0, 3, 3, 4, 9] and data[:9].tolist() == [1, 2, 3, P - 1, 4, 5, 6, 7, 8] and offs[-1] == len(data)
    assert np.array_equal(np.diff(offs[-6:]), np.full(5, 2, dtype=np.uint64))
    odd = lab_witness(ctx, traces, ragged)
    fill_against_model(ctx, odd, traces, MAIN, bare, TILE + 3, append=True)  # without a mask: the pass itself writes from the odd word on
    fill_against_model(ctx, odd, traces, MAIN, three, 700, append=True)      # one tile with a mask: the copy of the packed rows
    fill_against_model(ctx, w, traces, PRE, two, 3)                     # replace ...
    assert w.claims()[0].tolist() == [0, 2, 4, 6]
    fill_against_model(ctx, w, traces, MAIN, three, TILE, append=True)  # ... and append after replace
    fill_against_model(ctx, w, traces, MAIN, three, 0)                  # replace by nothing
    assert w.claims()[0].tolist() == [0] and w.claims()[1].size == 0
    fill_against_model(ctx, w, traces, MAIN, three, 0, append=True)     # and nothing behind nothing
    # the Level-2 view of the claims follows: the accumulator of the device list is that of the same list given by the host
    fill_against_model(ctx, w, traces, PRE, two, 4)
    fill_against_model(ctx, w, traces, MAIN, three, 40, append=True)
    offs, data = w.claims()
    given = s.witness([t.astype(np.uint32) for t in traces], (offs, data))
    beta, gamma = (3, 5, 7, 11), (13, 17, 19, 23)
    assert bb.claims_accumulator(w, beta, gamma) == bb.claims_accumulator(given, beta, gamma)
    ch_w, ch_g = bb.Challenger(s), bb.Challenger(s)
    ch_w.observe_claims(w)
    ch_g.observe_claims(given)
    assert ch_w.sample_ext() == ch_g.sample_ext()  # the host copy, which the transcript absorbs


def test_refusals_leave_the_witness_as_it_was(ctx):
    E = fe.Expr
    rng = np.random.default_rng(9600)
    n = 2 * TILE
    traces = lab_traces(rng, [n, PRE_H])
    s, _ = lab_system(ctx)
    start = [[9, 8], [P - 1]]
    w = lab_witness(ctx, traces, start)
    claims0 = w.claims()
    assert claims0[0].tolist() == [0, 2, 3] and claims0[1].tolist() == [9, 8, P - 1]
    prog, keep = lab_program(), lab_program(keep=E.input(1))
    inputs = np.stack([rand_field(rng, n), rng.integers(0, 2, size=n, dtype=np.uint64)], axis=1)
    d_inputs = dev32(inputs)

    def refused(text, call, witness=None, claims=None):
        witness, claims = witness or w, claims or claims0
        with pytest.raises(pkg.MstarkError, match=text) as e:
            call()
        assert str(e.value).startswith("msbb_witness_claims_fill: ") or "fill_claims inputs" in str(e.value), str(e.value)
        same_claims(witness.claims(), claims, text)
        same_traces(witness, traces if witness is w else [traces[MAIN], None])

    def raw(mode, program=True, summary=True, wh=None):
        a = np.frombuffer(prog.blob, dtype=np.uint8)
        out = np.zeros(4, dtype=np.uint64)
        mat = pkg.DevMatrix(d_inputs.data_ptr(), n, 4, 2, 1)
        rc = pkg.lib().msbb_witness_claims_fill(w.h if wh is None else wh, C.c_size_t(MAIN), a.ctypes.data_as(bb.u8p) if program else None, C.c_size_t(a.size),
                                                C.c_size_t(n), C.byref(mat), None, C.c_uint32(mode), out.ctypes.data_as(bb.u64p) if summary else None)
        if rc:
            raise pkg.MstarkError(pkg.lib().ms_last_error().decode())

    with fe.field(fe.BABYBEAR):
        narrow, pre1, six = fe.compile_claims(13, 0, 0, [E.main(0)]), fe.compile_claims(14, 1, 0, [E.main(0)]), fe.compile_claims(6, 2, 0, [E.main(0)])
        a_fill = fe.compile_fill(14, 0, 0, [(0, E.main(1))])
    goldilocks = fe.compile_claims(14, 0, 2, [E.input(0)])
    half = lab_witness(ctx, [traces[MAIN], None], start)
    for append in (False, True):
        refused(r"rows 2049 is above the circuit's height 2048", lambda: w.fill_claims(MAIN, prog, n + 1, d_inputs, append=append))
        refused(r"circuit 1 is inactive \(height 0\)", lambda: half.fill_claims(PRE, six, 0, append=append), half)
        refused(r"circuit 2 is out of range", lambda: w.fill_claims(2, prog, 1, d_inputs, append=append))
        refused(r"the program is for main_width 13 and preprocessed width 0, circuit 0 has 14 and 0", lambda: w.fill_claims(MAIN, narrow, append=append))
        refused(r"the program is for main_width 14 and preprocessed width 1, circuit 0 has 14 and 0", lambda: w.fill_claims(MAIN, pre1, append=append))
        refused(r"the program is for main_width 6 and preprocessed width 2, circuit 0 has 14 and 0", lambda: w.fill_claims(MAIN, six, append=append))
        refused(r"the program reads 2 input columns and no input matrix was given", lambda: w.fill_claims(MAIN, keep, append=append))
        refused(r"input height 4096 is above the circuit's height 2048", lambda: w.fill_claims(MAIN, keep, n, dev32(np.zeros((2 * n, 2))), append=append))
        refused(r"fill_claims inputs: width 3, the program reads 2 input columns", lambda: w.fill_claims(MAIN, keep, n, dev32(np.zeros((n, 3))), append=append))
        refused(r"input matrix: .*elem_bytes", lambda: w.fill_claims(MAIN, keep, n, dev(inputs.astype(np.uint64)), append=append))  # 8-byte elements
        refused(r"a fill program, not a claim program", lambda: w.fill_claims(MAIN, a_fill, append=append))
        refused(r"not a claim program \(wrong magic\)", lambda: w.fill_claims(MAIN, goldilocks, n, d_inputs, append=append))
        refused(r"truncated program blob", lambda: w.fill_claims(MAIN, prog.blob[:-8], n, d_inputs, append=append))
    refused(r"mode 2 \(MS_CLAIMS_REPLACE = 0, MS_CLAIMS_APPEND = 1\)", lambda: raw(2))
    refused(r"mode 4294967295", lambda: raw(0xFFFFFFFF))
    refused(r"null argument", lambda: raw(0, summary=False))
    refused(r"null argument", lambda: raw(0, program=False))
    with pytest.raises(pkg.MstarkError, match=r"msbb_witness_claims_fill: null argument"):
        raw(0, wh=C.c_void_p())
    # a non-canonical 4-byte input, with its row and column: the evaluation has run by then, into buffers of the call alone
    for program in (prog, keep):
        for (r, c, v) in ((0, 0, P), (TILE + 7, 1, (1 << 32) - 1), (n - 1, 0, P + 5)):
            bad = inputs.copy()
            bad[r, c] = v
            if r < n - 1:
                bad[n - 1, 1] = P  # a later offender is not the one named
            for append in (False, True):
                refused(r"non-canonical input value: row %d, column %d$" % (r, c), lambda: w.fill_claims(MAIN, program, n, dev32(bad), append=append))
    # a host-resident witness keeps its claims on the host: neither call takes it, and its arrays stay what they were
    host_traces = [t.astype(np.uint32) for t in traces]
    host = s.host_witness(host_traces, pack(start))
    with pytest.raises(pkg.MstarkError, match=r"msbb_witness_claims_fill: takes a device-resident witness"):
        host.fill_claims(MAIN, prog, n, d_inputs)
    with pytest.raises(pkg.MstarkError, match=r"msbb_witness_claims: a host-resident witness"):
        host.claims()
    assert all(np.array_equal(a, b) for a, b in zip(host_traces, traces))
    # msbb_witness_claims with buffers that are too small: MS_ERR_BUFFER and the needed sizes, nothing written
    nc, ne = C.c_size_t(), C.c_size_t()
    offs, data = np.full(3, 99, dtype=np.uint64), np.full(3, 99, dtype=np.uint32)
    for cap_o, cap_d in ((2, 3), (3, 2), (0, 0)):
        rc = pkg.lib().msbb_witness_claims(w.h, offs.ctypes.data_as(bb.u64p), C.c_size_t(cap_o), data.ctypes.data_as(bb.u32p), C.c_size_t(cap_d), C.byref(nc), C.byref(ne))
        assert (rc, nc.value, ne.value) == (-3, 2, 3) and offs.tolist() == [99] * 3 and data.tolist() == [99] * 3
    # the context is usable and the witness takes the next call
    same_traces(w, traces)
    fill_against_model(ctx, w, traces, MAIN, keep, n, inputs, append=True)
    fill_against_model(ctx, half, [traces[MAIN], None], MAIN, keep, n, inputs)


def test_host_waits(ctx):
    """at most two: [the offender word and the kept total, one read-back], the host copy (include/mstark_bb.h, "Host waits")"""
    E = fe.Expr
    rng = np.random.default_rng(9650)
    n = 2 * TILE
    traces = lab_traces(rng, [n, 0])
    w = lab_witness(ctx, traces)
    inputs = dev32(np.stack([rand_field(rng, n), rng.integers(0, 2, size=n, dtype=np.uint64)], axis=1))
    bare = bb.compile_claims(14, 0, 0, [E.main(0)])
    w.trace(MAIN)
    torch.cuda.synchronize()
    for prog, ins, waits in ((bare, None, 1), (lab_program(), inputs, 2), (lab_program(keep=E.input(1)), inputs, 2), (bb.compile_claims(14, 0, 0, [E.main(0)], keep=E.main(2)), None, 2)):
        before = ctx.sync_count()
        w.fill_claims(MAIN, prog, n, ins)
        assert ctx.sync_count() == before + waits, (prog.has_keep, ins is not None)


def test_end_to_end_u32_add(ctx):
    """pairs -> fill -> fill_claims -> derive_multiplicities -> check -> lookup_balance -> prove, from zero traces and no claims"""
    n = 1 << 10
    with fe.field(fe.BABYBEAR):
        s = bb.System.new(ctx, fe.test_params(), fe.u32_add_system_inputs(), K)
        traces, claims = fe.u32_add_bench_witness(n)
        fill_prog, claims_prog = fe.u32_add_halves_fill_program(n), fe.u32_add_claims_program()
    want = np.array([[int(v) % P for v in c] for c in claims], dtype=np.uint32)
    packed = pack(want.tolist())
    w = s.witness_from_device([dev32(np.zeros_like(t)) for t in traces], pack([]))
    assert w.claims()[0].tolist() == [0] and w.claims()[1].size == 0
    w.fill(1, fill_prog, dev(halves(*fe.xorshift_pairs(n)).astype(np.uint16)))
    before = w.lookup_balance()
    assert not before.ok  # every addition is pulled by the circuit and claimed by nobody, and the table's multiplicities are zero
    rep = w.fill_claims(1, claims_prog, rows=n)
    info = bb.claims_program_info(claims_prog)
    assert rep.fields() == (n, n, info["instructions"], info["lds_lanes"]) and info["lds_lanes"] == 256
    offs, data = w.claims()
    assert np.array_equal(offs, packed[0]) and np.array_equal(data, packed[1]) and np.array_equal(data.reshape(n, 4), want)
    between = w.lookup_balance()
    assert not between.ok and between.unbalanced < before.unbalanced  # the additions cancel now; the table's multiplicities are still zero
    assert w.derive_multiplicities([(0, 0)]).ok
    assert np.array_equal(w.trace(0).astype(np.uint64), traces[0]) and np.array_equal(w.trace(1).astype(np.uint64), traces[1])
    assert w.check().verdict == 0
    assert w.lookup_balance().ok
    proof = s.prove_multiple_claims(w).to_bytes()
    assert proof == s.prove_multiple_claims(s.witness(traces, packed)).to_bytes()
    assert s.verify_multiple_claims(packed, proof) == 0
