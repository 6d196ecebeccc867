"""GPU tests of witnesses created from DEVICE memory (ms_witness_create_device / msbb_witness_create_device,
System.witness_from_device): the ingest kernels copy exactly what the strided view holds, for every layout and element
size; proofs are byte-identical to those of an uploaded witness and of the oracle; non-canonical values are named by
circuit, row and column; malformed descriptions are refused on the host; the inputs may be destroyed after the call;
the producer's stream is honoured; Level 2 and the BabyBear configuration take such witnesses too.

Inputs are made with numpy from fixed seeds and moved with torch. Elements of 2, 4 and 8 bytes travel as signed tensors of
the same bits (the library reads them as unsigned whatever the dtype)."""
import os

import numpy as np
import pytest
import torch

from conftest import P, rand_field

pytestmark = pytest.mark.gpu

WIDTHS = [1, 14, 65, 130]  # one element, the bench width, one column past a 64-tile, two tiles plus two
LAYOUTS = ["row", "col", "colslice", "rowstep"]
UNSIGNED = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
SIGNED_BITS = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}


def T(a):
    """numpy array of unsigned elements -> CUDA tensor holding the same bits"""
    return torch.from_numpy(np.ascontiguousarray(a).view(SIGNED_BITS[a.dtype.itemsize])).cuda()


def ff(shape, dtype):
    """a CUDA tensor whose every byte is 0xFF (as 8-byte elements: 2^64 - 1, not canonical)"""
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(255)
    return t


def layout(t, kind):
    h, w = t.shape
    if kind == "row":
        return t
    if kind == "col":
        return t.t().contiguous().t()
    if kind == "colslice":  # a column slice of a tensor 7 columns wider
        big = ff((h, w + 7), t.dtype)
        big[:, 3:3 + w] = t
        return big[:, 3:3 + w]
    assert kind == "rowstep"  # every second row of a tensor of twice the height
    big = ff((2 * h, w), t.dtype)
    big[::2] = t
    return big[::2]


def values(rng, h, w, eb):
    """edge values of the field for 8-byte elements, the full range of the type for narrow ones"""
    if eb == 8:
        return rand_field(rng, (h, w))
    a = rng.integers(0, 1 << (8 * eb), size=(h, w), dtype=np.uint64).astype(UNSIGNED[eb])
    flat = a.reshape(-1)
    flat[0] = (1 << (8 * eb)) - 1
    flat[-1] = 0 if flat.size > 1 else flat[-1]
    return a


def narrowest(a):
    for eb in (1, 2, 4):
        if int(a.max()) < 1 << (8 * eb):
            return a.astype(UNSIGNED[eb])
    return a


@pytest.fixture(scope="module")
def wide_system(pkg, ctx, fe):
    """four circuits of main widths WIDTHS with one trivial constraint each (never proved: only the witness is looked at)"""
    def circuit(w):
        def ev(b):
            m, mn = b.main()
            b.assert_zero(m[0] - mn[0])

        return fe.lookup_air(w, ev, [])

    old = os.environ.get("MSAMD_NO_JIT")
    os.environ["MSAMD_NO_JIT"] = "1"  # nothing of these circuits is ever run: no kernels to generate
    try:
        return pkg.System.new(ctx, fe.test_params(), [circuit(w) for w in WIDTHS])
    finally:
        if old is None:
            del os.environ["MSAMD_NO_JIT"]
        else:
            os.environ["MSAMD_NO_JIT"] = old


def balanced_u32_witness(fe, n):
    """the bench workload's witness for n additions with the padding rows' lookups answered: a padding row still pushes its twelve
    zero bytes (fe.u32_add_bench_witness leaves them unmatched, so only full traces verify), which the byte table's
    multiplicity of 0 must count for the verifier to accept"""
    traces, claims = fe.u32_add_bench_witness(n)
    traces[0][0, 0] += np.uint64(12 * (traces[1].shape[0] - n))
    return traces, claims


@pytest.fixture(scope="module")
def u32(pkg, ctx, fe, oracle):
    """the [ByteTable, U32Add] system with 5 and 300 additions (heights 8 and 512): traces, claims, the oracle's proof - computed
    once - and the proof of the uploaded witness, which must be the same bytes"""
    system = pkg.System.new(ctx, fe.bench_params(), fe.u32_add_system_inputs())
    osys = oracle.System(system.blob)
    cases = {}
    for n in (5, 300):
        traces, claims = balanced_u32_witness(fe, n)
        packed = fe.pack_claims(claims)
        expect = osys.prove(traces, packed)
        assert system.prove_multiple_claims(system.witness(traces, packed)).to_bytes() == expect
        assert system.verify_multiple_claims(packed, expect) == 0
        cases[n] = (traces, packed, expect)
    return system, cases


def good_call(u32):
    """a device witness of the small U32 system on the same context, proved: the bytes of the oracle's proof"""
    system, cases = u32
    traces, packed, expect = cases[5]
    w = system.witness_from_device([T(t) for t in traces], packed)
    assert system.prove_multiple_claims(w).to_bytes() == expect


# ------------------------------------------------------------------ 1. exact ingest
@pytest.mark.parametrize("eb", [1, 2, 4, 8])
@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("h", [1, 2, 64, 512])
def test_exact_ingest(wide_system, fe, h, kind, eb):
    """what the witness holds is the view, element for element; padding columns and skipped rows (all 0xFF bytes) are neither
    copied nor flagged"""
    rng = np.random.default_rng(100000 + 100 * h + 10 * LAYOUTS.index(kind) + eb)
    arrs = [values(rng, h, w, eb) for w in WIDTHS]
    views = [layout(T(a), kind) for a in arrs]
    w = wide_system.witness_from_device(views, fe.pack_claims([]))
    for ci, a in enumerate(arrs):
        got = w.trace(ci)
        assert got.shape == a.shape and np.array_equal(got, a.astype(np.uint64)), "circuit %d (width %d)" % (ci, WIDTHS[ci])


@pytest.mark.parametrize("kind,eb", [("row", 8), ("col", 8), ("colslice", 1), ("rowstep", 4)])
def test_exact_ingest_more_work_than_one_grid(wide_system, fe, kind, eb):
    """2^19 rows of the bench width: more 16-byte vectors, tiles and elements than one grid of the largest size covers, so every
    kernel form goes round its grid-stride loop"""
    h = 1 << 19
    a = values(np.random.default_rng(7 + eb), h, 14, eb)
    w = wide_system.witness_from_device([None, layout(T(a), kind), None, None], fe.pack_claims([]))
    assert np.array_equal(w.trace(1), a.astype(np.uint64))
    assert w.trace(0).size == 0


@pytest.fixture(scope="module")
def w16_system(pkg, ctx, fe):
    """one circuit of main width 16: a row of 1-, 2- and 4-byte elements is a whole number of 16-byte vectors"""
    def ev(b):
        m, mn = b.main()
        b.assert_zero(m[0] - mn[0])

    old = os.environ.get("MSAMD_NO_JIT")
    os.environ["MSAMD_NO_JIT"] = "1"
    try:
        return pkg.System.new(ctx, fe.test_params(), [fe.lookup_air(16, ev, [])])
    finally:
        if old is None:
            del os.environ["MSAMD_NO_JIT"]
        else:
            os.environ["MSAMD_NO_JIT"] = old


@pytest.mark.parametrize("eb", [1, 2, 4, 8])
@pytest.mark.parametrize("kind", ["rowstep", "aligned_colslice"])
@pytest.mark.parametrize("h", [2, 64, 512])
def test_exact_ingest_vector_loads_over_strided_rows(w16_system, fe, h, kind, eb):
    """rows that are NOT contiguous with each other but each a whole number of aligned 16-byte vectors, for every element size: the
    16-byte-load form walking more than one row (the widths of test_exact_ingest reach it for 8-byte elements only)"""
    a = values(np.random.default_rng(500 + 10 * h + eb), h, 16, eb)
    t = T(a)
    if kind == "rowstep":
        view = layout(t, "rowstep")
    else:  # columns 16 .. 31 of a tensor of 32: base and pitch stay multiples of 16 bytes
        big = ff((h, 32), t.dtype)
        big[:, 16:] = t
        view = big[:, 16:]
    assert view.data_ptr() % 16 == 0 and (view.stride(0) * eb) % 16 == 0 and view.stride(1) == 1
    w = w16_system.witness_from_device([view], fe.pack_claims([]))
    assert np.array_equal(w.trace(0), a.astype(np.uint64))


# ------------------------------------------------------------------ 2. proof parity
def _device_inputs(traces, packed, mode, claims):
    trs = [T(t if mode == "u64" else narrowest(t)) for t in traces]
    if mode == "narrow":
        assert trs[1].element_size() == 1  # the additions' trace holds bytes and a carry: uint8
    cl = (T(packed[0]), T(packed[1])) if claims == "device" else packed
    return trs, cl


@pytest.mark.parametrize("jit", ["jit", "no_jit"])
@pytest.mark.parametrize("claims", ["host", "device"])
@pytest.mark.parametrize("mode", ["u64", "narrow"])
@pytest.mark.parametrize("n", [5, 300])
def test_proof_parity(pkg, ctx, fe, u32, monkeypatch, n, mode, claims, jit):
    system, cases = u32
    traces, packed, expect = cases[n]
    if jit == "no_jit":
        monkeypatch.setenv("MSAMD_NO_JIT", "1")
        system = pkg.System.new(ctx, fe.bench_params(), fe.u32_add_system_inputs())
        assert system.circuit_kernels(1) == 0
    trs, cl = _device_inputs(traces, packed, mode, claims)
    w = system.witness_from_device(trs, cl)
    proof = system.prove_multiple_claims(w).to_bytes()
    assert proof == expect, "device-created witness: the proof differs from the oracle's and the uploaded witness's"
    assert system.verify_multiple_claims(packed, proof) == 0
    for ci, t in enumerate(traces):
        assert np.array_equal(w.trace(ci), t)


def test_proof_parity_inactive_and_preprocessed_circuit(pkg, ctx, fe, oracle):
    """[ByteTable (preprocessed), U32Add, U32Add] with the third circuit inactive (None)"""
    system = pkg.System.new(ctx, fe.test_params(), fe.multi_u32_add_system_inputs(2))
    traces, claims = balanced_u32_witness(fe, 20)
    packed = fe.pack_claims(claims)
    host_traces = traces + [np.zeros((0, 14), dtype=np.uint64)]
    expect = oracle.System(system.blob).prove(host_traces, packed)
    assert system.prove_multiple_claims(system.witness(host_traces, packed)).to_bytes() == expect
    w = system.witness_from_device([T(traces[0]), layout(T(narrowest(traces[1])), "col"), None], packed)
    proof = system.prove_multiple_claims(w).to_bytes()
    assert proof == expect and system.verify_multiple_claims(packed, proof) == 0
    with pytest.raises(pkg.MstarkError, match="preprocessed trace height"):  # the byte table has 256 preprocessed rows
        system.witness_from_device([T(traces[0][:128]), T(traces[1]), None], packed)


# ------------------------------------------------------------------ 3. validation
@pytest.mark.parametrize("value", [P, (1 << 64) - 1])
@pytest.mark.parametrize("where", ["first", "last", "middle_colmajor"])
def test_noncanonical_value_is_named(pkg, wide_system, fe, u32, value, where):
    h, ci = 64, 2
    w = WIDTHS[ci]
    a = rand_field(np.random.default_rng(31), (h, w))
    r, c, kind = {"first": (0, 0, "row"), "last": (h - 1, w - 1, "rowstep"), "middle_colmajor": (37, 21, "col")}[where]
    a[r, c] = np.uint64(value)
    views = [None, None, layout(T(a), kind), None]
    with pytest.raises(pkg.MstarkError, match=r"non-canonical trace value: circuit 2, row %d, column %d$" % (r, c)):
        wide_system.witness_from_device(views, fe.pack_claims([]))
    good_call(u32)


@pytest.mark.parametrize("kind", ["row", "col"])
def test_lower_flat_index_of_two_offenders_is_named(pkg, wide_system, fe, u32, kind):
    """(3, 7) comes before (10, 2) in r * w + c, although column 2 comes first in a column-major source"""
    a = rand_field(np.random.default_rng(32), (64, 14))
    a[3, 7] = np.uint64(P)
    a[10, 2] = np.uint64((1 << 64) - 1)
    with pytest.raises(pkg.MstarkError, match=r"circuit 1, row 3, column 7$"):
        wide_system.witness_from_device([None, layout(T(a), kind), None, None], fe.pack_claims([]))
    good_call(u32)


@pytest.mark.parametrize("kind", LAYOUTS)
def test_all_p_minus_one_is_accepted(wide_system, fe, kind):
    a = np.full((64, 65), P - 1, dtype=np.uint64)
    w = wide_system.witness_from_device([None, None, layout(T(a), kind), None], fe.pack_claims([]))
    assert np.array_equal(w.trace(2), a)


# ------------------------------------------------------------------ 4. refusals
class Described:
    """a device matrix described by hand (__cuda_array_interface__): what no tensor library would hand over"""

    def __init__(self, ptr, shape, typestr="<u8", strides=None, keep=None):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "strides": strides, "version": 3}
        self.keep = keep


def test_refusals_on_the_host(pkg, wide_system, fe, u32):
    """each raises, decided on the host: nothing is launched, nothing faults or hangs"""
    none = fe.pack_claims([])
    t = T(rand_field(np.random.default_rng(41), (8, 14)))
    p = t.data_ptr()

    def refuse(obj, pattern):
        with pytest.raises(pkg.MstarkError, match=pattern):
            wide_system.witness_from_device([None, obj, None, None], none)

    refuse(Described(p, (4, 14), "|V3"), r"elem_bytes must be one of 1, 2, 4, 8 \(got 3\)")
    refuse(Described(p, (4, 14), strides=(0, 8)), "strides must be positive")
    refuse(Described(p, (4, 14), strides=(14 * 8, 0)), "strides must be positive")
    refuse(t[:3], "power of two")
    refuse(Described(p + 1, (4, 14)), "not aligned to 8 bytes")
    refuse(Described(0, (4, 14)), "null pointer with height 4")
    host = np.zeros((4, 14), dtype=np.uint64)
    refuse(Described(host.ctypes.data, (4, 14), keep=host), "not a pointer to device memory")  # the pointer query decides
    refuse(Described(p, (4, 14), strides=(1 << 62, 8)), "overflow")
    refuse(Described(p, (1 << 27, 14)), "supported maximum")
    refuse(Described(p, (4, 14), strides=(1 << 30, 8)), "into an allocation of")  # a view that leaves its allocation
    good_call(u32)


@pytest.mark.parametrize("claims", ["host", "device"])
def test_bad_claims_are_refused(pkg, u32, claims):
    system, cases = u32
    traces, (offs, data), expect = cases[5]
    trs = [T(t) for t in traces]
    dev = (lambda o, d: (T(o), T(d))) if claims == "device" else (lambda o, d: (o, d))
    bad_offs = offs.copy()
    bad_offs[2] = bad_offs[1] - 1
    with pytest.raises(pkg.MstarkError, match="non-decreasing"):
        system.witness_from_device(trs, dev(bad_offs, data))
    bad_offs = offs.copy()
    bad_offs[0] = 1
    with pytest.raises(pkg.MstarkError, match="start at 0"):
        system.witness_from_device(trs, dev(bad_offs, data))
    bad_data = data.copy()
    bad_data[len(data) // 2] = np.uint64(P)
    with pytest.raises(pkg.MstarkError, match="non-canonical claim value"):
        system.witness_from_device(trs, dev(offs, bad_data))
    w = system.witness_from_device(trs, dev(offs, data))
    assert system.prove_multiple_claims(w).to_bytes() == expect


# ------------------------------------------------------------------ 5. lifetime
def test_sources_may_be_destroyed_after_the_call(u32):
    system, cases = u32
    traces, packed, expect = cases[300]
    trs, cl = [T(t) for t in traces], (T(packed[0]), T(packed[1]))
    w = system.witness_from_device(trs, cl)
    for x in trs + list(cl):
        x.zero_()
    del trs, cl, x
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    assert system.prove_multiple_claims(w).to_bytes() == expect


# ------------------------------------------------------------------ 6. stream ordering
@pytest.mark.parametrize("how", ["explicit_handle", "current_stream"])
def test_producer_stream_is_waited_for(wide_system, fe, how):
    """the trace is the end of a chain of 48 elementwise launches on a non-default stream, handed over without any synchronisation.
    (A pass does not prove the ordering - it guards against the argument being ignored, next to a reading of
    ingest_wait_for_producer.)"""
    h, steps = 1 << 16, 48
    base = np.random.default_rng(61).integers(0, 1 << 40, size=(h, 14), dtype=np.uint64)
    x0 = T(base)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        x = x0
        for k in range(steps):
            x = x + (k + 1)
        views = [None, x, None, None]
        if how == "explicit_handle":
            w = wide_system.witness_from_device(views, fe.pack_claims([]), stream=side.cuda_stream)
        else:
            w = wide_system.witness_from_device(views, fe.pack_claims([]))  # torch's current stream: `side`
    assert np.array_equal(w.trace(1), base + np.uint64(steps * (steps + 1) // 2))
    torch.cuda.current_stream().wait_stream(side)


# ------------------------------------------------------------------ 7. Level 2
def test_commit_stage1_of_a_device_created_witness(u32):
    system, cases = u32
    traces, packed, _ = cases[300]
    hs, ws = [t.shape[0] for t in traces], [t.shape[1] for t in traces]
    up = system.witness(traces, packed).commit_stage1(hs, ws)
    dev = system.witness_from_device([T(narrowest(t)) for t in traces], packed).commit_stage1(hs, ws)
    assert dev.cap == up.cap and len(dev.cap) >= 32


# ------------------------------------------------------------------ 8. BabyBear
@pytest.fixture(scope="module")
def bsys(pkg, ctx, fe):
    with fe.field(fe.BABYBEAR):
        system = pkg.babybear.System.new(ctx, fe.test_params(), fe.mul_air_inputs(), fe.poseidon2_constants())
        smoke, rows64, none = fe.mul_air_smoke_trace(), fe.mul_air_trace(64), fe.pack_claims([])
    return system, {"smoke": smoke, "rows64": rows64}, none


@pytest.mark.parametrize("kind", ["row", "col", "colslice", "rowstep"])
@pytest.mark.parametrize("name", ["smoke", "rows64"])
def test_babybear_proof_parity(bsys, name, kind):
    system, traces, none = bsys
    trace = traces[name]
    expect = system.prove_multiple_claims(system.witness([trace], none)).to_bytes()
    w = system.witness_from_device([layout(T(trace.astype(np.uint32)), kind)], none)
    assert system.prove_multiple_claims(w).to_bytes() == expect
    assert system.verify_multiple_claims(none, expect) == 0


@pytest.mark.parametrize("kind", ["row", "col"])
def test_babybear_modulus_is_flagged_and_p_minus_one_accepted(pkg, fe, bsys, kind):
    system, traces, none = bsys
    BB_P = fe.BABYBEAR["P"]
    a = traces["rows64"].astype(np.uint32)
    a[41, 1] = BB_P
    a[50, 0] = 0xFFFFFFFF  # a later offender in row-major order, an earlier one in a column-major source
    with pytest.raises(pkg.MstarkError, match=r"non-canonical trace value: circuit 0, row 41, column 1$"):
        system.witness_from_device([layout(T(a), kind)], none)
    ok = np.array([[BB_P - 1, BB_P - 1, 1]] * 4, dtype=np.uint32)  # (-1) (-1) = 1
    expect = system.prove_multiple_claims(system.witness([ok], none)).to_bytes()
    assert system.prove_multiple_claims(system.witness_from_device([layout(T(ok), kind)], none)).to_bytes() == expect


@pytest.mark.parametrize("eb", [1, 2])
@pytest.mark.parametrize("kind", ["row", "col"])
def test_babybear_narrow_trace(bsys, kind, eb):
    system, _, none = bsys
    r = np.arange(64, dtype=np.uint64)
    a, b = r % 16, (7 * r + 3) % 16
    trace = np.stack([a, b, a * b], axis=1)  # products below 226: a uint8 trace
    expect = system.prove_multiple_claims(system.witness([trace], none)).to_bytes()
    w = system.witness_from_device([layout(T(trace.astype(UNSIGNED[eb])), kind)], none)
    assert system.prove_multiple_claims(w).to_bytes() == expect


def test_babybear_refusals(pkg, bsys):
    system, traces, none = bsys
    with pytest.raises(pkg.MstarkError, match=r"elem_bytes must be one of 1, 2, 4 \(got 8\)"):
        system.witness_from_device([T(traces["rows64"])], none)
    with pytest.raises(pkg.MstarkError, match="power of two"):
        system.witness_from_device([T(traces["rows64"].astype(np.uint32))[:48]], none)
    host = np.zeros((4, 3), dtype=np.uint32)
    with pytest.raises(pkg.MstarkError, match="not a pointer to device memory"):
        system.witness_from_device([Described(host.ctypes.data, (4, 3), "<u4", keep=host)], none)
    w = system.witness_from_device([T(traces["smoke"].astype(np.uint32))], none)
    assert system.prove_multiple_claims(w).to_bytes() == system.prove_multiple_claims(system.witness([traces["smoke"]], none)).to_bytes()
