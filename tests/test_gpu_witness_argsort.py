"""`-m gpu`: ms_witness_argsort (csrc/argsort.hip) against the model of tests/argsort_model.py, which tests/test_argsort_model.py
pins to the definition. Every comparison is exact, device against model.

Heights come from sort_info(): T rows per tile and R per-tile counts per round of the offsets step. 1, 2, 64, T / 2 (a partial
tile), T, 2 T (the first tile seam), 8 T, and the smallest power of two whose 256 x tiles digit-major array exceeds R (capped at
2^20), from which the one-workgroup offsets step takes more than one round. A lab system of placeholder circuits of main widths
2, 3 and 14; witnesses come from witness_from_device and nothing of it is proved.

Not covered: the refusal of a height above 2^31. Heights are powers of two, so the smallest refused witness has 2^32 rows - 64 GiB
at two columns - and no test of a few seconds builds one. A circuit without a trace on this device exists only in a witness with
has_remote set, which is refused first; that refusal is covered."""
import numpy as np
import pytest
import torch  # (before the library opens the device)

import argsort_model as am

pytestmark = pytest.mark.gpu
P = (1 << 64) - (1 << 32) + 1
_CACHE = {}
EDGES = [0, 1, P - 1, P - 2, (1 << 32) - 1, 1 << 32, 1 << 63, 0xFFFFFFFF00000000]
WIDTHS = (2, 3, 14)
CALL = "ms_witness_argsort: "


def dev(a):
    """a numpy array of unsigned integers as a torch tensor on the GPU (same bits, same element size)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])).cuda()


def heights(pkg):
    T, bits, R, max_keys = pkg.sort_info()
    assert R > 0  # (the offsets step has rounds; were it 0, 2^18 would be the one larger height)
    big = 1
    while 256 * ((big + T - 1) // T) <= R:
        big *= 2
    return [1, 2, 64, T // 2, T, 2 * T, 8 * T, min(big, 1 << 20)]


def lab_system(pkg, fe, ctx):
    """one circuit per main width, no preprocessed trace: the witness decides the height. Nothing is ever proved with it: the
    constraints are placeholders."""
    if "lab" not in _CACHE:
        E = fe.Expr
        _CACHE["lab"] = pkg.System.new(ctx, fe.test_params(), [fe.CircuitInputs(w, None, [E.main(0) * E.main(0) - E.main(0)], [], []) for w in WIDTHS])
    return _CACHE["lab"]


def lab_witness(pkg, fe, ctx, rng, n, columns=None):
    """every circuit active at height n, filled with random values; columns {(circuit, column): values} -> (witness, traces)"""
    s = lab_system(pkg, fe, ctx)
    traces = [rng.integers(0, P, size=(n, w), dtype=np.uint64) for w in WIDTHS]
    for (ci, col), values in (columns or {}).items():
        traces[ci][:, col] = values
    return s.witness_from_device([dev(t) for t in traces], fe.pack_claims([])), traces


def sort_against_model(w, traces, ci, keys, dst, rank):
    """one call on the device and in the model; `traces` follows. Every other column and every other circuit is unchanged (the
    model's output is the whole trace), and the report agrees with the height, the key count and the digits that differ."""
    want = am.run(traces[ci], keys, dst, rank)
    rep = w.argsort(ci, keys, dst, rank=rank)
    got = w.trace(ci)
    assert np.array_equal(got, want), "circuit %d keys %s rank %s, rows %s" % (ci, keys, rank, np.nonzero((got != want).any(axis=1))[0][:8])
    assert rep.fields() == (traces[ci].shape[0], len(keys)) + am.passes(traces[ci], keys), str(rep)
    traces[ci] = got
    for other in range(len(traces)):
        if other != ci:
            assert np.array_equal(w.trace(other), traces[other])
    return rep


def contents(rng, n):
    """(name, key column) - the key contents every height is run with"""
    rnd = rng.integers(0, P, size=n, dtype=np.uint64)
    places = rng.choice(n, size=min(n, len(EDGES)), replace=False)
    rnd[places] = np.array(EDGES[: len(places)], dtype=np.uint64)
    r = np.arange(n, dtype=np.uint64)
    return [("random", rnd),
            ("constant", np.full(n, 0x0123456789ABCDEF, dtype=np.uint64)),
            ("bits", rng.integers(0, 2, size=n, dtype=np.uint64)),
            ("bytes", rng.integers(0, 256, size=n, dtype=np.uint64)),
            ("sorted", np.sort(rng.integers(0, P, size=n, dtype=np.uint64))),
            ("descending", np.uint64(P - 1) - r * np.uint64(0xF00000001)),
            ("middle digit", np.uint64(0x1122334400667788) | (rng.integers(0, 256, size=n, dtype=np.uint64) << np.uint64(24))),
            ("top byte", np.uint64(0x12345678) | (rng.integers(0, 256, size=n, dtype=np.uint64) << np.uint64(56)))]


@pytest.mark.parametrize("k", range(8))
def test_key_contents_at_every_height(pkg, fe, ctx, k):
    """one key column: width 2 (key 0, dst 1) and width 3 (key 2, dst 0), PERM and RANK"""
    n = heights(pkg)[k]
    rng = np.random.default_rng(1200 + k)
    for name, col in contents(rng, n):
        assert int(col.max()) < P
        w, traces = lab_witness(pkg, fe, ctx, rng, n, {(0, 0): col, (1, 2): col})
        for ci, key, dst in ((0, 0, 1), (1, 2, 0)):
            for rank in (False, True):
                rep = sort_against_model(w, traces, ci, [key], dst, rank)
                if name == "constant":
                    assert rep.passes == 0 and np.array_equal(traces[ci][:, dst], np.arange(n, dtype=np.uint64))
                if name == "bytes":
                    assert rep.passes <= 1 and rep.passes + rep.skipped == 8
                if name == "descending" and not rank:
                    assert np.array_equal(traces[ci][:, dst], np.arange(n, dtype=np.uint64)[::-1])
                if name == "sorted":  # ties or not, a sorted column keeps its rows where they are
                    assert np.array_equal(traces[ci][:, dst], np.arange(n, dtype=np.uint64))


@pytest.mark.parametrize("k", range(8))
def test_width_14_two_keys_at_every_height(pkg, fe, ctx, k):
    """keys at columns 13 and 0, dst at 7: the primary key has four distinct values, the secondary is random over the field"""
    n = heights(pkg)[k]
    rng = np.random.default_rng(1300 + k)
    primary = np.array([3, P - 1, 1 << 63, 1 << 32], dtype=np.uint64)[rng.integers(0, 4, size=n)]
    w, traces = lab_witness(pkg, fe, ctx, rng, n, {(2, 13): primary})
    for rank in (False, True):
        sort_against_model(w, traces, 2, [13, 0], 7, rank)


def test_several_keys(pkg, fe, ctx):
    T = pkg.sort_info()[0]
    for n in (64, T // 2, 2 * T):
        rng = np.random.default_rng(1400 + n)
        cols = {(2, 1): rng.integers(0, 3, size=n, dtype=np.uint64),                              # three keys: few, bytes, field
                (2, 2): rng.integers(0, 256, size=n, dtype=np.uint64) << np.uint64(40),
                (1, 0): rng.integers(0, 2, size=n, dtype=np.uint64), (1, 1): rng.integers(0, 2, size=n, dtype=np.uint64)}
        w, traces = lab_witness(pkg, fe, ctx, rng, n, cols)
        for rank in (False, True):
            sort_against_model(w, traces, 2, [1, 2, 3], 0, rank)
            sort_against_model(w, traces, 1, [0, 1], 2, rank)                                    # ties in both keys: the row index decides
            twice = sort_against_model(w, traces, 2, [5, 4, 5], 9, rank).fields()                  # the same column twice ...
            column = traces[2][:, 9].copy()
            once = sort_against_model(w, traces, 2, [5, 4], 9, rank).fields()                      # ... changes nothing
            assert np.array_equal(traces[2][:, 9], column) and twice[0] == once[0] and twice[1] == once[1] + 1


@pytest.mark.parametrize("n_of", ["64", "2T"])
def test_eight_keys(pkg, fe, ctx, n_of):
    n = 64 if n_of == "64" else 2 * pkg.sort_info()[0]
    rng = np.random.default_rng(1500 + n)
    # few values per key, so that every key decides somewhere; one byte-valued, one over the field, one constant
    cols = {(2, c): rng.integers(0, 2, size=n, dtype=np.uint64) << np.uint64(8 * c) for c in range(1, 6)}
    cols[(2, 6)] = rng.integers(0, 256, size=n, dtype=np.uint64)
    cols[(2, 8)] = np.full(n, 9, dtype=np.uint64)
    w, traces = lab_witness(pkg, fe, ctx, rng, n, cols)
    for rank in (False, True):
        rep = sort_against_model(w, traces, 2, [8, 1, 2, 3, 4, 5, 6, 7], 0, rank)
        assert rep.keys == 8 and rep.passes + rep.skipped == 64


def test_one_host_wait(pkg, fe, ctx):
    n = 2 * pkg.sort_info()[0]
    rng = np.random.default_rng(16)
    w, traces = lab_witness(pkg, fe, ctx, rng, n)
    assert np.array_equal(w.trace(2), traces[2])  # (the read-back is a host wait: nothing of the setup is pending)
    for keys, dst, rank in (([13], 7, False), ([0, 13, 5], 1, True)):
        before = ctx.sync_count()
        w.argsort(2, keys, dst, rank=rank)
        assert ctx.sync_count() == before + 1  # the histograms of all key columns in one copy (include/mstark.h, "Host waits")
        traces[2] = am.run(traces[2], keys, dst, rank)
        assert np.array_equal(w.trace(2), traces[2])


def test_refusals_write_nothing_and_leave_the_context_usable(pkg, fe, ctx):
    import ctypes as C

    n = 64
    rng = np.random.default_rng(17)
    s = lab_system(pkg, fe, ctx)
    w, traces = lab_witness(pkg, fe, ctx, rng, n)
    unchanged = lambda: all(np.array_equal(w.trace(ci), traces[ci]) for ci in range(len(WIDTHS)))

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
    # the witness of another system (same circuits, another handle)
    E = fe.Expr
    other = pkg.System.new(ctx, fe.test_params(), [fe.CircuitInputs(x, None, [E.main(0) * E.main(0) - E.main(0)], [], []) for x in WIDTHS])
    keys, summary = np.array([0], dtype=np.uint32), np.zeros(4, dtype=np.uint64)

    def raw(system):
        pkg._check(pkg.lib().ms_witness_argsort(system.h, w.h, C.c_size_t(0), keys.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_size_t(1), C.c_uint32(1),
                                               C.c_uint32(0), summary.ctypes.data_as(C.POINTER(C.c_uint64))))

    refused(lambda: raw(other), "does not belong")
    # a host-resident witness, a witness with a circuit another rank computes, an inactive circuit
    host = [t.copy() for t in traces]
    hw = s.host_witness(host, fe.pack_claims([]))
    refused(lambda: hw.argsort(0, [0], 1), "device-resident")
    assert all(np.array_equal(a, b) for a, b in zip(host, traces))
    remote = s.witness(traces, fe.pack_claims([]), remote_heights={1: n})
    refused(lambda: remote.argsort(0, [0], 1), "another rank")
    half = s.witness_from_device([dev(traces[0]), None, dev(traces[2])], fe.pack_claims([]))
    refused(lambda: half.argsort(1, [0], 1), "inactive")
    assert np.array_equal(half.trace(0), traces[0]) and np.array_equal(half.trace(2), traces[2])
    # null arguments are an error code, and the witness is as good as new
    L = pkg.lib()
    assert L.ms_witness_argsort(s.h, w.h, C.c_size_t(0), None, C.c_size_t(1), C.c_uint32(1), C.c_uint32(0), summary.ctypes.data_as(C.POINTER(C.c_uint64))) == -1
    assert L.ms_witness_argsort(s.h, None, C.c_size_t(0), keys.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_size_t(1), C.c_uint32(1), C.c_uint32(0),
                                summary.ctypes.data_as(C.POINTER(C.c_uint64))) == -1
    assert "null" in L.ms_last_error().decode() and unchanged()
    raw(s)
    traces[0] = am.run(traces[0], [0], 1)
    assert unchanged() and tuple(int(x) for x in summary) == (n, 1) + am.passes(traces[0], [0])
    for rank in (False, True):
        sort_against_model(w, traces, 2, [13, 0], 7, rank)


# ---------------------------------------------------------------- end to end: an offline memory check - sort, gather, prove
ADDR, VAL, S_ADDR, S_VAL = 0, 1, 2, 3


def memory_air(fe):
    """columns (addr, val, s_addr, s_val): the log, and the log in address order. is_transition * d * (d - 1) with
    d = s_addr_next - s_addr; the log is pushed and the sorted log pulled, so the two are permutations of each other"""
    E = fe.Expr

    def ev(b):
        local, nxt = b.main()
        d = nxt[S_ADDR] - local[S_ADDR]
        b.when_transition().assert_zero(d * (d - 1))

    return fe.lookup_air(4, ev, [fe.Lookup.push(1, [E.const(7), E.main(ADDR), E.main(VAL)]), fe.Lookup.pull(1, [E.const(7), E.main(S_ADDR), E.main(S_VAL)])])


@pytest.mark.parametrize("route", ["device", "held"])
def test_memory_argument_end_to_end(pkg, fe, ctx, oracle, route):
    n = 2 * pkg.sort_info()[0]
    E = fe.Expr
    if "e2e" not in _CACHE:
        rng = np.random.default_rng(41)
        addr = np.concatenate([np.arange(n // 4, dtype=np.uint64), rng.integers(0, n // 4, size=n - n // 4, dtype=np.uint64)])
        rng.shuffle(addr)
        assert set(addr.tolist()) == set(range(n // 4))  # every address at least once: the sorted column steps by 0 or 1
        val = rng.integers(0, P, size=n, dtype=np.uint64)
        perm = np.lexsort([addr]).astype(np.int64)  # the numpy route
        full = np.stack([addr, val, addr[perm], val[perm]], axis=1)
        s = pkg.System.new(ctx, fe.test_params(), [memory_air(fe)])
        packed = fe.pack_claims([])
        _CACHE["e2e"] = (s, full, packed, s.prove_multiple_claims(s.witness([full], packed)).to_bytes())
    s, full, packed, proof = _CACHE["e2e"]
    start = full.copy()
    start[:, S_ADDR], start[:, S_VAL] = 5, np.arange(n, dtype=np.uint64) * np.uint64(0x100000001) + np.uint64(3)  # junk
    if route == "device":
        w = s.witness_from_device([dev(start)], packed)
    else:
        w = s.witness([start], packed, lookups=[oracle.System(s.blob).compute_lookup_values(0, start)])
    assert np.array_equal(w.trace(0), start)  # (the read-back is a host wait: nothing of the setup is pending)
    before = ctx.sync_count()
    rep = w.argsort(0, [ADDR], dst=S_ADDR)
    assert ctx.sync_count() == before + 1  # held lookup values included
    assert rep.fields() == (n, 1) + am.passes(start, [ADDR])
    assert np.array_equal(w.trace(0), am.run(start, [ADDR], S_ADDR))
    w.fill(0, fe.compile_fill(4, 0, 0, [(S_VAL, E.main_at(VAL, E.main(S_ADDR))), (S_ADDR, E.main_at(ADDR, E.main(S_ADDR)))]))
    assert np.array_equal(w.trace(0), full)
    assert w.check().verdict == 0 and w.lookup_balance().ok
    got = s.prove_multiple_claims(w).to_bytes()
    assert got == proof and s.verify_multiple_claims(packed, got) == 0
