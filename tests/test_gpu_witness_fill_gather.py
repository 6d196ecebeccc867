"""`-m gpu`: the indexed reads of ms_witness_fill (csrc/fill.hip, OP_AT) against the model of tests/fill_gather_model.py, which
tests/test_fill_gather_model.py pins to the definition. Every comparison is exact, device against model.

Heights 1, 2, 64 (a partial workgroup), 256 (one workgroup exactly) and 512 (two). Main widths 1, 2, 14 and 3, and one circuit of
6 columns with a 2-column preprocessed trace at 512 rows. Index columns: random in [0, 2 n) (half of them beyond the height),
the edge values 0, n - 1, n, h_in - 1, h_in, p - 1, 2^32 and 2^32 + 1 at rows 0, 1, ... (in as many columns as it takes at a
small height), a full permutation, and every row pointing at one row. No index asks the device to read out of bounds: a row
from the height on reads 0 by definition, and that value is checked."""
import numpy as np
import pytest
import torch  # (before the library opens the device)

import fill_gather_model as gm
from test_fill_gather_model import gather_refusal_blobs

pytestmark = pytest.mark.gpu
P = gm.GOLDILOCKS_P
_CACHE = {}
WIDTHS = (1, 2, 14, 3)
PRE, PRE_H = len(WIDTHS), 512
HEIGHTS = (1, 2, 64, 256, 512)


def dev(a):
    """a numpy array of unsigned integers as a torch tensor on the GPU (same bits, same element size)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])).cuda()


def lab_system(pkg, fe, ctx):
    """one circuit per main width without preprocessed trace (the witness decides the height) and one with. Nothing is ever
    proved with it: the constraints are placeholders."""
    if "lab" not in _CACHE:
        E = fe.Expr
        c = [E.main(0) * E.main(0) - E.main(0)]
        pre = np.random.default_rng(2025).integers(0, P, size=(PRE_H, 2), dtype=np.uint64)
        _CACHE["lab"] = (pkg.System.new(ctx, fe.test_params(), [fe.CircuitInputs(w, None, c, [], []) for w in WIDTHS] + [fe.CircuitInputs(6, pre, c, [], [])]), pre)
    return _CACHE["lab"]


def lab_witness(pkg, fe, ctx, rng, n):
    """the circuits without preprocessed trace at height n, the one with at its own, all random -> (witness, traces)"""
    s, _ = lab_system(pkg, fe, ctx)
    traces = [rng.integers(0, P, size=(n, w), dtype=np.uint64) for w in WIDTHS] + [rng.integers(0, P, size=(PRE_H, 6), dtype=np.uint64)]
    return s.witness_from_device([dev(t) for t in traces], fe.pack_claims([])), traces


def index_columns(rng, n, h_in, wide):
    """[(name, n indices)]; wide: the element holds 64 bits (else indices stay below 2^32)"""
    edges = [0, n - 1, n, h_in - 1, h_in] + ([P - 1, 1 << 32, (1 << 32) + 1] if wide else [(1 << 32) - 1])
    out = [("random", rng.integers(0, 2 * n, size=n, dtype=np.uint64)), ("permutation", rng.permutation(n).astype(np.uint64)),
           ("one row", np.full(n, rng.integers(0, n), dtype=np.uint64))]
    for k in range(0, len(edges), n):
        col = rng.integers(0, 2 * n, size=n, dtype=np.uint64)
        chunk = edges[k:k + n]
        col[: len(chunk)] = np.array(chunk, dtype=np.uint64)
        out.append(("edges from %d" % k, col))
    return out


def fill_against_model(pkg, fe, ctx, w, traces, ci, prog, inputs):
    """fill circuit ci on the device and in the model; `traces` follows. The report agrees with the host-only info call, and
    what the program does not assign - other columns, other circuits - stays as it was."""
    _, pre = lab_system(pkg, fe, ctx)
    want = gm.run(prog.blob, traces[ci], pre if ci == PRE else None, None if inputs is None else inputs.astype(np.uint64))
    rep = w.fill(ci, prog, None if inputs is None else dev(inputs))
    got = w.trace(ci)
    assert np.array_equal(got, want), "circuit %d, rows %s" % (ci, np.nonzero((got != want).any(axis=1))[0][:8])
    info = pkg.fill_program_info(prog)
    assert rep.fields() == (traces[ci].shape[0], len(prog.steps), info["instructions"], info["lds_lanes"]), str(rep)
    others = [c for c in range(traces[ci].shape[1]) if c not in {d for d, _ in prog.steps}]
    assert np.array_equal(got[:, others], traces[ci][:, others])
    traces[ci] = got
    for other in range(len(traces)):
        if other != ci:
            assert np.array_equal(w.trace(other), traces[other])
    return rep


def programs(fe, width):
    """(name, program) over inputs (values, index, second index) for one main width"""
    E = fe.Expr
    v, i, j, row = E.input(0), E.input(1), E.input(2), E.row()
    if width == 1:
        return [("input_at", fe.compile_fill(1, 0, 3, [(0, E.input_at(0, i))]))]
    if width == 2:
        return [("main_at of an untouched column", fe.compile_fill(2, 0, 3, [(0, E.main_at(1, i) + v)])),
                ("an at under an at", fe.compile_fill(2, 0, 3, [(0, E.main_at(1, E.input_at(2, i)))]))]
    if width == 3:
        return []
    k8 = fe.bits(row, 3, 29) * 8  # the row rounded down to a multiple of 8
    steps = [(0, E.input_at(0, k8) + E.main_at(13, k8 + 7)), (1, E.main(0) * E.input_at(0, E.input_at(2, E.input_at(1, row)))),
             (2, fe.running_sum(E.input_at(0, i) * E.main_at(0, j), init=3)),     # a scan whose coefficients index inputs and a finished column
             (3, fe.scan(E.main_at(12, i), E.input_at(1, row), init=1)),          # and the multiplier too
             (4, E.main_at(2, j) - E.main_at(3, fe.bits(E.main(1), 0, 10))), (5, E.main_at(2, fe.bits(E.main_at(13, 0), 0, 9)))]  # finished scan columns
    return [("ordinary, two scans, ordinary", fe.compile_fill(14, 0, 3, steps))]


@pytest.mark.parametrize("n", HEIGHTS)
def test_indexed_reads_against_the_model(pkg, fe, ctx, n):
    rng = np.random.default_rng(4000 + n)
    w, traces = lab_witness(pkg, fe, ctx, rng, n)
    for ci, width in enumerate(WIDTHS):
        for name, prog in programs(fe, width):
            for h_in in sorted({n, (n + 1) // 2}):
                for wide in (True, False):
                    for what, col in index_columns(rng, n, h_in, wide):
                        inputs = rng.integers(0, P if wide else 1 << 32, size=(n, 3), dtype=np.uint64)
                        inputs[:, 1] = col
                        inputs[:, 2] = rng.integers(0, n + n // 4 + 1, size=n, dtype=np.uint64)
                        inputs = inputs[:h_in].astype(np.uint64 if wide else np.uint32)
                        fill_against_model(pkg, fe, ctx, w, traces, ci, prog, inputs)
                        if width == 1:  # the definition, next to the model: a row from the height on reads 0, anything below it the cell
                            idx = np.zeros(n, dtype=np.uint64)
                            idx[:h_in] = col[:h_in]
                            beyond = idx >= np.uint64(h_in)
                            got = traces[ci][:, 0]
                            assert not got[beyond].any(), (name, what)
                            assert np.array_equal(got[~beyond], inputs[:, 0].astype(np.uint64)[idx[~beyond].astype(np.int64)])


def test_preprocessed_trace_at_computed_rows(pkg, fe, ctx):
    E = fe.Expr
    rng = np.random.default_rng(41)
    w, traces = lab_witness(pkg, fe, ctx, rng, 64)
    _, pre = lab_system(pkg, fe, ctx)
    i = E.input(0)
    prog = fe.compile_fill(6, 2, 1, [(0, E.pre_at(0, i)), (1, E.pre_at(1, E.main_at(5, 0) + i)), (2, E.pre_at(1, E.row()) - E.var(fe.SRC_PRE, 0, 1))])
    for what, col in index_columns(rng, PRE_H, PRE_H // 2, True):
        for h_in in (PRE_H, PRE_H // 2):
            fill_against_model(pkg, fe, ctx, w, traces, PRE, prog, col[:h_in].reshape(-1, 1))
    assert not traces[PRE][:, 2].any() and pre[:, 1].all()  # column 2: preprocessed column 1 through an identity index minus itself


@pytest.mark.parametrize("form", ["lds", "scratch"])
def test_both_kernel_forms(pkg, fe, ctx, form):
    E = fe.Expr
    n = 512
    src = E.main_at(13, E.input(1))
    leaves = [fe.bits(src + k, k % 57, 1 + k // 57) for k in range(300 if form == "scratch" else 8)]
    t = leaves[-1]
    for leaf in reversed(leaves[:-1]):  # every leaf is live before the first is consumed
        t = leaf - t
    # ... and an indexed read behind the deepest point, whose row comes from the result
    prog = fe.compile_fill(14, 0, 3, [(0, t), (3, E.main_at(13, fe.bits(E.main(0), 0, 10)) + E.input_at(0, fe.bits(E.main(0), 1, 9)))])
    info = pkg.fill_program_info(prog)
    assert (info["lds_lanes"] == 0) == (form == "scratch") and (form == "lds" or info["slots"] >= 300), info
    rng = np.random.default_rng(len(leaves))
    w, traces = lab_witness(pkg, fe, ctx, rng, n)
    inputs = rng.integers(0, P, size=(n, 3), dtype=np.uint64)
    inputs[:, 1] = rng.integers(0, 2 * n, size=n, dtype=np.uint64)
    rep = fill_against_model(pkg, fe, ctx, w, traces, 2, prog, inputs)
    assert rep.lds_lanes == info["lds_lanes"]


def test_scan_coefficient_pass_in_the_global_scratch(pkg, fe, ctx):
    E = fe.Expr
    n = 512
    leaves = [fe.bits(E.input_at(0, E.input(1)) + k, k % 57, 1 + k // 57) for k in range(300)]
    t = leaves[-1]
    for leaf in reversed(leaves[:-1]):
        t = leaf - t
    prog = fe.compile_fill(2, 0, 3, [(0, fe.scan(E.main_at(1, E.input(2)), t, init=5))])
    assert pkg.fill_program_info(prog)["lds_lanes"] == 0
    rng = np.random.default_rng(300)
    w, traces = lab_witness(pkg, fe, ctx, rng, n)
    inputs = rng.integers(0, P, size=(n, 3), dtype=np.uint64)
    inputs[:, 1:] = rng.integers(0, 2 * n, size=(n, 2), dtype=np.uint64)
    fill_against_model(pkg, fe, ctx, w, traces, 1, prog, inputs)


def test_rows_per_item(pkg, fe, ctx):
    k, items, n = 8, 64, 512
    prog = fe.rows_per_item_fill_program(k)
    assert prog.main_width == 3 and prog.n_inputs == 4 and any(kind == fe.N_AT for kind, _, _, _, _ in prog.nodes)
    rng = np.random.default_rng(8)
    w, traces = lab_witness(pkg, fe, ctx, rng, n)
    for h_in in (items, items - 5):  # all rows used, and rows behind the last item
        words = rng.integers(0, 1 << 16, size=(h_in, 4), dtype=np.uint64)
        fill_against_model(pkg, fe, ctx, w, traces, 3, prog, words.astype(np.uint32))
        r = np.arange(n)
        item, j = r >> 3, r & 7
        padded = np.zeros((n, 4), dtype=np.uint64)
        padded[:h_in] = words
        limb = (padded[item, j >> 1] >> (8 * (j & 1)).astype(np.uint64)) & np.uint64(0xFF)
        assert np.array_equal(traces[3], np.stack([item.astype(np.uint64), j.astype(np.uint64), limb], axis=1))


# ---------------------------------------------------------------- end to end: a permuted copy of a column, checked and proved
def test_permuted_copy_end_to_end(pkg, fe, ctx):
    n = 512
    E = fe.Expr
    s = pkg.System.new(ctx, fe.test_params(), [fe.CircuitInputs(2, None, [], [], [fe.Lookup.push(1, [E.main(0)]), fe.Lookup.pull(1, [E.main(1)])])])
    rng = np.random.default_rng(52)
    a = rng.permutation(4 * n)[:n].astype(np.uint64) + np.uint64(1)  # distinct, non-zero
    perm = rng.permutation(n).astype(np.uint64)
    packed = fe.pack_claims([])
    prog = fe.compile_fill(2, 0, 1, [(1, E.main_at(0, E.input(0)))])
    host = np.stack([a, a[perm.astype(np.int64)]], axis=1)
    proof = s.prove_multiple_claims(s.witness([host], packed)).to_bytes()
    w = s.witness_from_device([dev(np.stack([a, np.zeros_like(a)], axis=1))], packed)
    w.fill(0, prog, dev(perm.astype(np.uint32)).reshape(n, 1))
    assert np.array_equal(w.trace(0), host)
    assert w.check().verdict == 0 and w.lookup_balance().ok
    got = s.prove_multiple_claims(w).to_bytes()
    assert got == proof and s.verify_multiple_claims(packed, got) == 0
    # one index duplicated: a[perm[7]] is pulled twice, a[perm[8]] never
    dup = perm.copy()
    dup[8] = dup[7]
    w.fill(0, prog, dev(dup.astype(np.uint32)).reshape(n, 1))
    rep = w.lookup_balance()
    assert not rep.ok and rep.unbalanced == 2
    assert sorted(tuple(e.args) for e in rep.entries) == sorted([(int(a[perm[7]]),), (int(a[perm[8]]),)])
    assert {e.net for e in rep.entries} == {1, P - 1}


# ---------------------------------------------------------------- refusals and host waits
def test_refusals_write_nothing_and_leave_the_context_usable(pkg, fe, ctx):
    n = 64
    rng = np.random.default_rng(12)
    w, traces = lab_witness(pkg, fe, ctx, rng, n)
    N = fe
    A, M, row, x, one = N.N_AT, N.SRC_MAIN, (N.N_ROW, 0, 0, 0, 0), (N.N_VAR, N.SRC_INPUT, 0, 0, 0), (N.N_CONST, 0, 0, 1, 0)
    blob = lambda nodes, steps, scans=None: fe.fill_blob(2, 0, 1, nodes, steps, scans)
    inputs = rng.integers(0, n, size=(n, 1), dtype=np.uint64)
    cases = [(blob([row, (A, M, 0, 0, 0)], [(0, 1)]), ("indexed read of main column 0", "step group 0")),                 # the same group
             (blob([row, (A, M, 0, 0, 0), x, one], [(1, 1), (0, 2)], [(1, 3, 0)]), ("indexed read", "step group 1 assigns")),  # a later group
             (blob([row, (A, M, 0, 0, 0), one], [(0, 1)], [(0, 2, 0)]), ("indexed read of main column 0",)),              # a scan's own dst
             (blob([row, (A, M, 0, 2, 0)], [(0, 1)]), ("out of range",)),
             (blob([row, (A, N.SRC_INPUT, 0, 1, 0)], [(0, 1)]), ("out of range",)),
             (blob([row, (A, N.SRC_PRE, 0, 0, 0)], [(0, 1)]), ("out of range",)),                                         # no preprocessed trace
             (blob([row, (A, M, 1, 1, 0)], [(0, 1)]), ("offset field",)),
             (blob([row, (A, 7, 0, 0, 0)], [(0, 1)]), ("unknown source",)),
             (blob([row, (A, N.SRC_STAGE2, 0, 0, 0)], [(0, 1)]), ("stage-2",)),
             (blob([(A, M, 0, 1, 1), row], [(0, 0)]), ("forward",))]
    for program, words in cases:
        with pytest.raises(pkg.MstarkError) as e:
            w.fill(1, program, dev(inputs))
        assert str(e.value).startswith("ms_witness_fill: ") and all(t in str(e.value) for t in words), str(e.value)
        assert all(np.array_equal(w.trace(ci), traces[ci]) for ci in range(len(traces)))
    good, host_cases, scan_cases, _ = gather_refusal_blobs(fe)  # widths (3, 1): refused as a program before the widths are compared
    for what, program, _ in host_cases + scan_cases:
        with pytest.raises(pkg.MstarkError):
            w.fill(1, program, dev(inputs))
    assert all(np.array_equal(w.trace(ci), traces[ci]) for ci in range(len(traces)))
    E = fe.Expr
    fill_against_model(pkg, fe, ctx, w, traces, 1, fe.compile_fill(2, 0, 1, [(0, E.main_at(1, E.input(0)))]), inputs)  # as good as new


def test_host_waits(pkg, fe, ctx):
    n = 256
    rng = np.random.default_rng(13)
    w, traces = lab_witness(pkg, fe, ctx, rng, n)
    E = fe.Expr
    no_inputs = fe.compile_fill(14, 0, 0, [(0, E.main_at(13, fe.bits(E.main(12), 0, 9))), (1, fe.running_sum(E.main_at(0, E.row() + 1))), (2, E.main_at(1, E.main(0)))])
    assert np.array_equal(w.trace(2), traces[2])  # (the read-back is a host wait: nothing of the setup is pending)
    before = ctx.sync_count()
    w.fill(2, no_inputs)
    assert ctx.sync_count() == before  # no inputs: the call only queues work (include/mstark.h, "Host waits")
    assert np.array_equal(w.trace(2), gm.run(no_inputs.blob, traces[2]))
    with_inputs = fe.compile_fill(1, 0, 2, [(0, E.input_at(0, E.input(1)))])
    inputs = dev(rng.integers(0, n, size=(n, 2), dtype=np.uint64))
    torch.cuda.synchronize()
    before = ctx.sync_count()
    w.fill(0, with_inputs, inputs)
    assert ctx.sync_count() == before + 1  # the offender word of the inputs, as without indexed reads
