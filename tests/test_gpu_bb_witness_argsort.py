"""`-m gpu`: msbb_witness_argsort (csrc/bb_argsort.hip) against the model of tests/argsort_model_bb.py, which
tests/test_bb_argsort_model.py pins to the definition. Every comparison is exact, device against model, read back through
w.trace(c) as canonical values. The counterpart of test_gpu_witness_argsort.py.

Heights come from bb.sort_info(): T rows per tile and R per-tile counts per round of the offsets step. 1, 2, 64, T / 2 (a partial
tile), T, 2 T (the first tile seam), 8 T, and the smallest power of two whose 256 x tiles digit-major array exceeds R (capped at
2^20), from which the one-workgroup offsets step takes more than one round. A lab system of placeholder circuits of main widths
2, 3 and 14; witnesses come from witness_from_device and nothing of it is proved.

Teeth, on a scratch copy: with bb_from_monty taken out of the two key reads of bb_argsort.hip - the Montgomery words sorted as
they lie - 20 of the 22 cases here fail (all but the two one-row cases).

Not covered, because msbb_witness* cannot express them: the witness of another system handle (the call takes the witness alone
and finds the system through it, so there is no second handle to pass); a circuit without a trace on this device (every
device-resident witness of this configuration has a trace for each active circuit); a height above 2^27 (the witness-making
calls refuse it, so no witness reaches the call)."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the library opens the device)

import argsort_model_bb as bm
from test_bb_witness_check_model import K, bb, fe, pack, pkg
from test_gpu_bb_lookup_balance import ctx  # noqa: F401  (the module-scoped context with the Poseidon2 permutation set)

pytestmark = pytest.mark.gpu
P = bm.P
_CACHE = {}
EDGES = [0, 1, P - 1, P - 2, 1 << 27, (1 << 27) + 1, (1 << 24) - 1, 1 << 24, 0xFF, 0x100]
WIDTHS = (2, 3, 14)
CALL = "msbb_witness_argsort: "
u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


def dev32(a):
    """a numpy array of canonical values as a torch tensor of 4-byte elements on the GPU"""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.uint32)).view(np.int32)).cuda()


def same(got, want):
    return got.shape == want.shape and np.array_equal(got.astype(np.uint64), np.asarray(want, dtype=np.uint64))


def heights():
    T, bits, R, max_keys = bb.sort_info()
    assert R > 0
    big = 1
    while 256 * ((big + T - 1) // T) <= R:
        big *= 2
    return [1, 2, 64, T // 2, T, 2 * T, 8 * T, min(big, 1 << 20)]


def lab_inputs():
    E = fe.Expr
    return [fe.CircuitInputs(w, None, [E.main(0) * E.main(0) - E.main(0)], [], []) for w in WIDTHS]


def lab_system(ctx):
    """one circuit per main width, no preprocessed trace: the witness decides the height. Nothing is ever proved with it: the
    constraints are placeholders."""
    if "lab" not in _CACHE:
        with fe.field(fe.BABYBEAR):
            _CACHE["lab"] = bb.System.new(ctx, fe.test_params(), lab_inputs(), K)
    return _CACHE["lab"]


def lab_witness(ctx, rng, n, columns=None):
    """every circuit active at height n, filled with random values; columns {(circuit, column): values} -> (witness, traces)"""
    s = lab_system(ctx)
    traces = [rng.integers(0, P, size=(n, w), dtype=np.uint64) for w in WIDTHS]
    for (ci, col), values in (columns or {}).items():
        traces[ci][:, col] = values
    return s.witness_from_device([dev32(t) for t in traces], pack([])), traces


def sort_against_model(w, traces, ci, keys, dst, rank):
    """one call on the device and in the model; `traces` follows. Every other column and every other circuit is unchanged (the
    model's output is the whole trace), and the report agrees with the height, the key count and the digits that differ."""
    want = bm.run(traces[ci], keys, dst, rank)
    rep = w.argsort(ci, keys, dst, rank=rank)
    got = w.trace(ci)
    assert same(got, want), "circuit %d keys %s rank %s, rows %s" % (ci, keys, rank, np.nonzero((got != want).any(axis=1))[0][:8])
    assert rep.fields() == (traces[ci].shape[0], len(keys)) + bm.passes(traces[ci], keys), str(rep)
    traces[ci] = want
    for other in range(len(traces)):
        if other != ci:
            assert same(w.trace(other), traces[other])
    return rep


def contents(rng, n):
    """(name, key column) - the key contents every height is run with"""
    rnd = rng.integers(0, P, size=n, dtype=np.uint64)
    places = rng.choice(n, size=min(n, len(EDGES)), replace=False)
    rnd[places] = np.array(EDGES[: len(places)], dtype=np.uint64)
    r = np.arange(n, dtype=np.uint64)
    pool = rng.integers(0, P, size=max(1, n // 2), dtype=np.uint64)
    return [("random", rnd),
            ("constant", np.full(n, 0x01234567, dtype=np.uint64)),
            ("bits", rng.integers(0, 2, size=n, dtype=np.uint64)),
            ("bytes", rng.integers(0, 256, size=n, dtype=np.uint64)),
            ("sorted", np.sort(pool[rng.integers(0, len(pool), size=n)])),                   # (n values out of n / 2: ties)
            ("descending", np.uint64(P - 1) - r * np.uint64(1901)),                            # (2^20 x 1901 < p; every digit moves)
            ("second digit", np.uint64(0x11220044) | (rng.integers(0, 256, size=n, dtype=np.uint64) << np.uint64(8))),
            ("top digit", np.uint64(0x345678) | (rng.integers(0, 0x78, size=n, dtype=np.uint64) << np.uint64(24)))]


@pytest.mark.parametrize("k", range(8))
def test_key_contents_at_every_height(ctx, k):
    """one key column: width 2 (key 0, dst 1) and width 3 (key 2, dst 0), PERM and RANK"""
    n = heights()[k]
    rng = np.random.default_rng(2200 + k)
    for name, col in contents(rng, n):
        assert int(col.max()) < P
        if name == "random" and n >= 64:
            # what fails if the Montgomery words were sorted where they lie: their order is another one (at 1 row there is one
            # order, and at 2 rows the two agree as often as not, so this is asked from 64 rows on)
            assert bm.permutation(bm.monty(col).reshape(-1, 1), [0]).tolist() != bm.permutation(col.reshape(-1, 1), [0]).tolist()
        w, traces = lab_witness(ctx, rng, n, {(0, 0): col, (1, 2): col})
        identity = np.arange(n, dtype=np.uint64)
        for ci, key, dst in ((0, 0, 1), (1, 2, 0)):
            for rank in (False, True):
                rep = sort_against_model(w, traces, ci, [key], dst, rank)
                assert rep.passes + rep.skipped == 4
                if name == "constant":
                    assert rep.passes == 0 and np.array_equal(traces[ci][:, dst], identity)
                if name == "bytes":
                    assert rep.passes <= 1
                if name in ("second digit", "top digit"):
                    assert rep.passes <= 1
                if name == "descending" and not rank:
                    assert np.array_equal(traces[ci][:, dst], identity[::-1])
                if name == "sorted":  # ties or not, a sorted column keeps its rows where they are
                    assert np.array_equal(traces[ci][:, dst], identity)


@pytest.mark.parametrize("k", range(8))
def test_width_14_two_keys_at_every_height(ctx, k):
    """keys at columns 13 and 0, dst at 7: the primary key has four distinct values, the secondary is random over the field"""
    n = heights()[k]
    rng = np.random.default_rng(2300 + k)
    primary = np.array([3, P - 1, 1 << 27, 1 << 24], dtype=np.uint64)[rng.integers(0, 4, size=n)]
    w, traces = lab_witness(ctx, rng, n, {(2, 13): primary})
    for rank in (False, True):
        sort_against_model(w, traces, 2, [13, 0], 7, rank)


def test_several_keys(ctx):
    T = bb.sort_info()[0]
    for n in (64, T // 2, 2 * T):
        rng = np.random.default_rng(2400 + n)
        cols = {(2, 1): rng.integers(0, 3, size=n, dtype=np.uint64),                              # three keys: few, bytes, field
                (2, 2): rng.integers(0, 256, size=n, dtype=np.uint64) << np.uint64(16),
                (1, 0): rng.integers(0, 2, size=n, dtype=np.uint64), (1, 1): rng.integers(0, 2, size=n, dtype=np.uint64)}
        w, traces = lab_witness(ctx, rng, n, cols)
        for rank in (False, True):
            sort_against_model(w, traces, 2, [1, 2, 3], 0, rank)
            sort_against_model(w, traces, 1, [0, 1], 2, rank)                                    # ties in both keys: the row index decides
            twice = sort_against_model(w, traces, 2, [5, 4, 5], 9, rank).fields()                  # the same column twice ...
            column = traces[2][:, 9].copy()
            once = sort_against_model(w, traces, 2, [5, 4], 9, rank).fields()                      # ... changes nothing
            assert np.array_equal(traces[2][:, 9], column) and twice[0] == once[0] and twice[1] == once[1] + 1


@pytest.mark.parametrize("n_of", ["64", "2T"])
def test_eight_keys(ctx, n_of):
    n = 64 if n_of == "64" else 2 * bb.sort_info()[0]
    rng = np.random.default_rng(2500 + n)
    # few values per key, so that every key decides somewhere; one byte-valued, one over the field, one constant
    cols = {(2, c): rng.integers(0, 2, size=n, dtype=np.uint64) << np.uint64(8 * ((c - 1) % 4)) for c in range(1, 6)}
    cols[(2, 6)] = rng.integers(0, 256, size=n, dtype=np.uint64)
    cols[(2, 8)] = np.full(n, 9, dtype=np.uint64)
    w, traces = lab_witness(ctx, rng, n, cols)
    for rank in (False, True):
        rep = sort_against_model(w, traces, 2, [8, 1, 2, 3, 4, 5, 6, 7], 0, rank)
        assert rep.keys == 8 and rep.passes + rep.skipped == 32


def test_one_host_wait(ctx):
    n = 2 * bb.sort_info()[0]
    rng = np.random.default_rng(26)
    w, traces = lab_witness(ctx, rng, n)
    assert same(w.trace(2), traces[2])  # (the read-back is a host wait: nothing of the setup is pending)
    for keys, dst, rank in (([13], 7, False), ([0, 13, 5], 1, True)):
        before = ctx.sync_count()
        w.argsort(2, keys, dst, rank=rank)
        assert ctx.sync_count() == before + 1  # the histograms of all key columns in one copy (include/mstark_bb.h, "Host waits")
        traces[2] = bm.run(traces[2], keys, dst, rank)
        assert same(w.trace(2), traces[2])


def test_refusals_write_nothing_and_leave_the_context_usable(ctx):
    n = 64
    rng = np.random.default_rng(27)
    s = lab_system(ctx)
    w, traces = lab_witness(ctx, rng, n)
    unchanged = lambda: all(same(w.trace(ci), traces[ci]) for ci in range(len(WIDTHS)))

    def refused(call, *words):
        with pytest.raises(pkg.MstarkError) as e:
            call()
        assert str(e.value).startswith(CALL) and all(x in str(e.value) for x in words), str(e.value)
        assert unchanged()

    refused(lambda: w.argsort(3, [0], 1), "out of range")
    refused(lambda: w.argsort(0, [], 1), "key columns")
    refused(lambda: w.argsort(2, [0] * 9, 1), "key columns")
    refused(lambda: w.argsort(0, [2], 1), "key column 2", "main_width 2")
    refused(lambda: w.argsort(1, [0, 3], 1), "key column 3", "main_width 3")
    refused(lambda: w.argsort(1, [0], 3), "dst column 3", "main_width 3")
    refused(lambda: w.argsort(2, [4, 7, 1], 7), "among the keys")
    refused(lambda: w.argsort(2, [4], 7, rank=2), "what = 2")
    # a host-resident witness, an inactive circuit
    host = [t.astype(np.uint32) for t in traces]
    hw = s.host_witness(host, pack([]))
    refused(lambda: hw.argsort(0, [0], 1), "device-resident")
    assert all(same(a, b) for a, b in zip(host, traces))
    half = s.witness_from_device([dev32(traces[0]), None, dev32(traces[2])], pack([]))
    refused(lambda: half.argsort(1, [0], 1), "inactive")
    assert same(half.trace(0), traces[0]) and same(half.trace(2), traces[2])
    # null arguments are an error code, and the witness is as good as new
    L = pkg.lib()
    keys, summary = np.array([0], dtype=np.uint32), np.zeros(4, dtype=np.uint64)
    args = lambda wh, kp, sp: (wh, C.c_size_t(0), kp, C.c_size_t(1), C.c_uint32(1), C.c_uint32(0), sp)
    for bad in (args(w.h, None, summary.ctypes.data_as(u64p)), args(None, keys.ctypes.data_as(u32p), summary.ctypes.data_as(u64p)),
                args(w.h, keys.ctypes.data_as(u32p), None)):
        assert L.msbb_witness_argsort(*bad) == -1
        assert L.ms_last_error().decode().startswith(CALL) and "null" in L.ms_last_error().decode() and unchanged()
    assert L.msbb_witness_argsort(*args(w.h, keys.ctypes.data_as(u32p), summary.ctypes.data_as(u64p))) == 0
    before = traces[0]
    traces[0] = bm.run(before, [0], 1)
    assert unchanged() and tuple(int(x) for x in summary) == (n, 1) + bm.passes(before, [0])
    for rank in (False, True):
        sort_against_model(w, traces, 2, [13, 0], 7, rank)


# ---------------------------------------------------------------- end to end: an offline memory check - sort, gather, prove
ADDR, VAL, S_ADDR, S_VAL = 0, 1, 2, 3


def memory_air():
    """the memory circuit of test_gpu_witness_argsort restated for this field (call under field(BABYBEAR)): columns (addr, val,
    s_addr, s_val), the log and the log in address order. is_transition * d * (d - 1) with d = s_addr_next - s_addr; the log is
    pushed and the sorted log pulled, so the two are permutations of each other"""
    E = fe.Expr

    def ev(b):
        local, nxt = b.main()
        d = nxt[S_ADDR] - local[S_ADDR]
        b.when_transition().assert_zero(d * (d - 1))

    return fe.lookup_air(4, ev, [fe.Lookup.push(1, [E.const(7), E.main(ADDR), E.main(VAL)]), fe.Lookup.pull(1, [E.const(7), E.main(S_ADDR), E.main(S_VAL)])])


def test_memory_argument_end_to_end(ctx):
    n = 2 * bb.sort_info()[0]
    E = fe.Expr
    rng = np.random.default_rng(51)
    addr = np.concatenate([np.arange(n // 4, dtype=np.uint64), rng.integers(0, n // 4, size=n - n // 4, dtype=np.uint64)])
    rng.shuffle(addr)
    assert set(addr.tolist()) == set(range(n // 4))  # every address at least once: the sorted column steps by 0 or 1
    val = rng.integers(0, P, size=n, dtype=np.uint64)
    perm = np.lexsort([addr]).astype(np.int64)  # the numpy route
    full = np.stack([addr, val, addr[perm], val[perm]], axis=1)
    with fe.field(fe.BABYBEAR):
        s = bb.System.new(ctx, fe.test_params(), [memory_air()], K)
        prog = fe.compile_fill(4, 0, 0, [(S_VAL, E.main_at(VAL, E.main(S_ADDR))), (S_ADDR, E.main_at(ADDR, E.main(S_ADDR)))])
    packed = pack([])
    proof = s.prove_multiple_claims(s.witness([full], packed)).to_bytes()  # a witness built on the host from the numpy route
    start = full.copy()
    start[:, S_ADDR], start[:, S_VAL] = 5, (np.arange(n, dtype=np.uint64) * np.uint64(0x10001) + np.uint64(3)) % np.uint64(P)  # junk
    w = s.witness_from_device([dev32(start)], packed)
    assert same(w.trace(0), start)  # (the read-back is a host wait: nothing of the setup is pending)
    before = ctx.sync_count()
    rep = w.argsort(0, [ADDR], dst=S_ADDR)
    assert ctx.sync_count() == before + 1
    assert rep.fields() == (n, 1) + bm.passes(start, [ADDR])
    assert same(w.trace(0), bm.run(start, [ADDR], S_ADDR))
    w.fill(0, prog)
    assert same(w.trace(0), full)
    assert w.check().verdict == 0 and w.lookup_balance().ok
    got = s.prove_multiple_claims(w).to_bytes()
    assert got == proof and s.verify_multiple_claims(packed, got) == 0
