"""`-m gpu`: ms_witness_fill (csrc/fill.hip) against the model of tests/fill_model.py, which tests/test_fill_model.py pins to
the witness builders. Every comparison is exact, device against model. Shapes: the U32Add circuit at 16 rows (a partial
workgroup), 128 and 4 096 (16 workgroups of 256 lanes); the random programs at heights 1 (row n - 1's next row is itself), 4 (the
wrap of offset 1) and 512 (more than one workgroup at every lane count)."""
import numpy as np
import pytest
import torch  # (before the library opens the device)

import fill_model as fm
from test_fill_model import SEQ_OLD, SEQ_WANT, sequential_program

pytestmark = pytest.mark.gpu
P = fm.P
_CACHE = {}
EDGES = [0, 1, 2, P - 1, P - 2, (1 << 32) - 1, 1 << 32, 1 << 63, 0xFFFFFFFF00000000, 0x00000000FFFFFFFF]


def dev(a):
    """a numpy array of unsigned integers as a torch tensor on the GPU (same bits, same element size)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])).cuda()


def rand_field(rng, shape):
    a = rng.integers(0, P, size=shape, dtype=np.uint64)
    flat = a.reshape(-1)
    for e in EDGES:
        if flat.size:
            flat[rng.integers(0, flat.size)] = e
    return a


# ---------------------------------------------------------------- the bench system: U32Add filled from (x, y)
def u32_system(pkg, fe, ctx):
    if "u32" not in _CACHE:
        _CACHE["u32"] = pkg.System.new(ctx, fe.test_params(), fe.u32_add_system_inputs())
    return _CACHE["u32"]


def u32_case(pkg, fe, ctx, n):
    """(system, builder's traces, packed claims, the proof of the host-built witness), computed once per n"""
    key = ("u32", n)
    if key not in _CACHE:
        s = u32_system(pkg, fe, ctx)
        traces, claims = fe.u32_add_bench_witness(n)
        packed = fe.pack_claims(claims)
        _CACHE[key] = (s, traces, packed, s.prove_multiple_claims(s.witness(traces, packed)).to_bytes())
    return _CACHE[key]


def empty_witness(s, oracle, traces, packed, route):
    """a witness of the right heights whose traces are all zeros. device: torch tensors through ms_witness_create_device;
    held: ms_witness_create with explicit lookup values (the zero traces' own), which the witness then holds"""
    zeros = [np.zeros_like(t) for t in traces]
    if route == "device":
        return s.witness_from_device([dev(z) for z in zeros], packed)
    osys = oracle.System(s.blob)
    return s.witness(zeros, packed, lookups=[osys.compute_lookup_values(ci, z) for ci, z in enumerate(zeros)])


@pytest.mark.parametrize("route", ["device", "held"])
@pytest.mark.parametrize("n,layout", [(16, "u32"), (128, "u32"), (128, "u64_column_major"), (4096, "u32")])
def test_u32_add_witness_from_pairs(pkg, fe, ctx, oracle, n, layout, route):
    s, traces, packed, proof = u32_case(pkg, fe, ctx, n)
    xs, ys = fe.xorshift_pairs(n)
    if layout == "u32":
        inputs = dev(np.stack([xs, ys], axis=1).astype(np.uint32))
    else:
        inputs = dev(np.stack([xs, ys], axis=0)).t()  # n x 2 with strides (1, n)
        assert tuple(inputs.shape) == (n, 2) and inputs.stride() == (1, n)
    w = empty_witness(s, oracle, traces, packed, route)
    rep = w.fill(1, fe.u32_add_fill_program(n), inputs)
    assert rep.fields() == (traces[1].shape[0], 14, 19, 256), str(rep)
    assert w.derive_multiplicities([(0, 0)]).ok
    assert np.array_equal(w.trace(0), traces[0]) and np.array_equal(w.trace(1), traces[1])
    assert w.check().verdict == 0 and w.lookup_balance().ok
    got = s.prove_multiple_claims(w).to_bytes()
    assert got == proof and s.verify_multiple_claims(packed, got) == 0


# ---------------------------------------------------------------- random programs on a circuit of its own
HEIGHTS = (1, 4, 512)


def lab_system(pkg, fe, ctx):
    """one system for everything below: per height a circuit [6 main columns, 2 preprocessed], a bystander of 3 columns and a
    circuit of 4 columns without preprocessed trace. Nothing is ever proved with it: the constraints are placeholders."""
    if "lab" not in _CACHE:
        E = fe.Expr
        rng = np.random.default_rng(2024)
        pres = [rand_field(rng, (h, 2)) for h in HEIGHTS]
        inputs = [fe.CircuitInputs(6, pre, [E.main(0) * E.main(1) - E.main(2)], [], []) for pre in pres]
        inputs += [fe.CircuitInputs(3, None, [E.main(0) * E.main(1) - E.main(2)], [], []),
                   fe.CircuitInputs(4, None, [E.main(0) * E.main(1) - E.main(2)], [], [])]
        _CACHE["lab"] = (pkg.System.new(ctx, fe.test_params(), inputs), pres)
    return _CACHE["lab"]


BYSTANDER, SEQ = len(HEIGHTS), len(HEIGHTS) + 1
CLAIMS = [[1, 2, 3], [P - 1], [], [7, 0]]


def lab_witness(pkg, fe, ctx, rng, hi, seq_trace=None):
    """a witness with circuit `hi` (height HEIGHTS[hi]) and the bystander active -> (witness, the traces it was made from)"""
    s, _ = lab_system(pkg, fe, ctx)
    traces = [None] * (len(HEIGHTS) + 2)
    if hi is not None:
        traces[hi] = rand_field(rng, (HEIGHTS[hi], 6))
    traces[BYSTANDER] = rand_field(rng, (8, 3))
    if seq_trace is not None:
        traces[SEQ] = np.array(seq_trace, dtype=np.uint64)
    w = s.witness_from_device([None if t is None else dev(t) for t in traces], fe.pack_claims(CLAIMS))
    return w, traces


def random_expr(fe, rng, depth):
    """every operator and both offsets; main columns 4 and 5 are never assigned, so their next row may be read"""
    E = fe.Expr
    if depth == 0 or rng.random() < 0.15:
        k = rng.integers(0, 9)
        if k == 0:
            return E.main(int(rng.integers(0, 6)))
        if k == 1:
            return E.main_next(int(rng.integers(4, 6)))
        if k == 2:
            return E.var(fe.SRC_PRE, int(rng.integers(0, 2)), int(rng.integers(0, 2)))
        if k in (3, 4):
            return E.input(int(rng.integers(0, 3)))
        if k == 5:
            return E.input_next(int(rng.integers(0, 3)))
        if k == 6:
            return E.row()
        return E.const(EDGES[int(rng.integers(0, len(EDGES)))] if k == 7 else int(rng.integers(0, P, dtype=np.uint64)))
    a, b = random_expr(fe, rng, depth - 1), random_expr(fe, rng, depth - 1)
    k = rng.integers(0, 9)
    if k == 8:
        lo = int(rng.integers(0, 64))
        return fe.bits(a, lo, int(rng.integers(1, 65 - lo)))
    return [lambda: a + b, lambda: a - b, lambda: a * b, lambda: -a, lambda: fe.inv0(a), lambda: fe.lt(a, b), lambda: fe.bit_xor(a, b),
            lambda: fe.bit_and(a, b)][k]()


def against_model(pkg, fe, ctx, rng, hi, prog, inputs):
    """fill circuit `hi` of a fresh witness on the device and in the model; everything else must stay as it was"""
    _, pres = lab_system(pkg, fe, ctx)
    w, traces = lab_witness(pkg, fe, ctx, rng, hi)
    acc = w.claims_accumulator(pkg.CHECK_BETA, pkg.CHECK_GAMMA)
    want = fm.run(prog.blob, traces[hi], pres[hi], inputs)
    rep = w.fill(hi, prog, None if inputs is None else dev(inputs))
    got = w.trace(hi)
    assert np.array_equal(got, want), "rows %s" % np.nonzero((got != want).any(axis=1))[0][:8]
    assigned = sorted({d for d, _ in prog.steps})
    others = [c for c in range(6) if c not in assigned]
    assert np.array_equal(got[:, others], traces[hi][:, others])  # (the model says so too; this is the statement itself)
    assert np.array_equal(w.trace(BYSTANDER), traces[BYSTANDER])
    assert w.claims_accumulator(pkg.CHECK_BETA, pkg.CHECK_GAMMA) == acc
    assert (rep.rows, rep.steps) == (HEIGHTS[hi], len(prog.steps))
    return rep


@pytest.mark.parametrize("hi", range(len(HEIGHTS)))
def test_random_programs(pkg, fe, ctx, hi):
    n = HEIGHTS[hi]
    rng = np.random.default_rng(700 + n)
    seen = set()
    for k in range(10):
        steps = [(int(rng.integers(0, 4)), random_expr(fe, rng, 4)) for _ in range(int(rng.integers(1, 7)))]
        prog = fe.compile_fill(6, 2, 3, steps)
        seen |= {node[0] for node in prog.nodes}
        h_in = n if k % 2 == 0 else max(1, int(rng.integers(1, n + 1)) - 1)  # the full height, and 0 < h_in < n where there is room
        against_model(pkg, fe, ctx, rng, hi, prog, rand_field(rng, (h_in, 3)))
    assert seen >= {fe.N_CONST, fe.N_VAR, fe.N_ADD, fe.N_SUB, fe.N_MUL, fe.N_NEG, fe.N_ROW, fe.N_BITS, fe.N_INV0, fe.N_LT, fe.N_XOR, fe.N_AND}


def chain_program(fe, leaves):
    """`leaves` distinct bits leaves, all computed before the first is consumed and then consumed last one first: t_k = b_k -
    t_(k+1), and the walk of an operator takes its first operand first. The slot file holds them all at the deepest point."""
    E = fe.Expr
    b = [fe.bits(E.input(k % 3), k % 57, 1 + k // 57) for k in range(leaves)]
    t = b[-1]
    for k in range(leaves - 2, -1, -1):
        t = b[k] - t
    return fe.compile_fill(6, 2, 3, [(0, t), (3, E.main(0) * E.var(fe.SRC_PRE, 1, 1) + E.main_next(5))])


@pytest.mark.parametrize("leaves,form", [(8, (256,)), (40, (64, 128)), (300, (0,)), (70, (64,))])  # (40 slots take 128 lanes, 70 take 64; last: the ids above stay)
def test_every_kernel_form(pkg, fe, ctx, leaves, form):
    prog = chain_program(fe, leaves)
    info = pkg.fill_program_info(prog)
    assert info["lds_lanes"] in form and info["slots"] >= leaves and info["assigned_columns"] == 2, info
    rng = np.random.default_rng(leaves)
    rep = against_model(pkg, fe, ctx, rng, HEIGHTS.index(512), prog, rand_field(rng, (512, 3)))
    assert rep.lds_lanes == info["lds_lanes"] and rep.instructions == info["instructions"]


def test_sequential_semantics_and_host_waits_without_inputs(pkg, fe, ctx):
    w, _ = lab_witness(pkg, fe, ctx, np.random.default_rng(5), None, seq_trace=SEQ_OLD)
    assert w.trace(SEQ).tolist() == SEQ_OLD  # (the read-back is a host wait: nothing of the setup is pending)
    before = ctx.sync_count()
    rep = w.fill(SEQ, sequential_program(fe))
    assert ctx.sync_count() == before  # no inputs: the call only queues work (include/mstark.h, "Host waits")
    assert w.trace(SEQ).tolist() == SEQ_WANT and rep.fields()[:2] == (2, 4)


def test_host_waits_with_inputs(pkg, fe, ctx):
    s, traces, packed, _ = u32_case(pkg, fe, ctx, 16)
    w = s.witness_from_device([dev(np.zeros_like(t)) for t in traces], packed)
    inputs = dev(np.stack(fe.xorshift_pairs(16), axis=1).astype(np.uint32))
    prog = fe.u32_add_fill_program(16)
    torch.cuda.synchronize()
    before = ctx.sync_count()
    w.fill(1, prog, inputs)
    assert ctx.sync_count() == before + 1  # the offender word of the inputs (include/mstark.h, "Host waits")
    assert np.array_equal(w.trace(1), traces[1])


def test_inputs_ordered_behind_the_producer_stream(pkg, fe, ctx):
    n = 4096
    s, traces, packed, _ = u32_case(pkg, fe, ctx, n)
    w = s.witness_from_device([dev(np.zeros_like(t)) for t in traces], packed)
    prog = fe.u32_add_fill_program(n)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        v = torch.arange(2 * n, dtype=torch.int64, device="cuda").reshape(n, 2)
        for _ in range(20):  # a queue of small launches the fill must wait for
            v = (v * 2654435761 + 12345) & 0xFFFFFFFF
        w.fill(1, prog, v, stream=side)  # no synchronisation in between
    torch.cuda.synchronize()
    want = fm.run(prog.blob, np.zeros((n, 14), dtype=np.uint64), None, v.cpu().numpy().astype(np.uint64))
    assert np.array_equal(w.trace(1), want)


def test_refusals_write_nothing(pkg, fe, ctx):
    n = 16
    s, traces, packed, proof = u32_case(pkg, fe, ctx, n)
    rng = np.random.default_rng(11)
    start = [rand_field(rng, t.shape) for t in traces]
    w = s.witness_from_device([dev(t) for t in start], packed)
    prog = fe.u32_add_fill_program(n)
    good = np.stack(fe.xorshift_pairs(n), axis=1)
    bad = good.copy()
    bad[5, 1] = P
    bad[9, 0] = P + 3  # a later offender: the first one in row-major order is named
    narrow = fe.compile_fill(13, 0, 2, [(0, fe.Expr.input(0))])
    cases = [(dev(bad), prog, 1, ("row 5", "column 1")),
             (dev(np.zeros((2 * n, 2), dtype=np.uint32)), prog, 1, ("height",)),
             (None, prog, 1, ("input",)),                       # n_inputs > 0 and no matrix
             (dev(good.astype(np.uint32)), narrow, 1, ("main_width 13",)),
             (dev(good.astype(np.uint32)), prog, 0, ("main_width 14",)),
             (dev(good.astype(np.uint32)), prog, 2, ("out of range",))]
    for inputs, program, circuit, words in cases:
        with pytest.raises(pkg.MstarkError) as e:
            w.fill(circuit, program, inputs)
        assert str(e.value).startswith("ms_witness_fill: ") and all(x in str(e.value) for x in words), str(e.value)
        assert np.array_equal(w.trace(0), start[0]) and np.array_equal(w.trace(1), start[1])
    # a host-resident witness, and an inactive circuit
    host = [t.copy() for t in start]
    hw = s.host_witness(host, packed)
    with pytest.raises(pkg.MstarkError, match="device-resident"):
        hw.fill(1, prog, dev(good.astype(np.uint32)))
    assert all(np.array_equal(a, b) for a, b in zip(host, start))
    half = s.witness_from_device([dev(start[0]), None], fe.pack_claims([]))
    with pytest.raises(pkg.MstarkError, match="inactive"):
        half.fill(1, prog, dev(good.astype(np.uint32)))
    assert np.array_equal(half.trace(0), start[0])
    # the context is as good as new: a fresh witness is filled and proved
    fresh = s.witness_from_device([dev(np.zeros_like(t)) for t in traces], packed)
    fresh.fill(1, prog, dev(good.astype(np.uint32)))
    assert fresh.derive_multiplicities([(0, 0)]).ok
    got = s.prove_multiple_claims(fresh).to_bytes()
    assert got == proof and s.verify_multiple_claims(packed, got) == 0
