"""`-m gpu`: msbb_witness_fill (csrc/bb_fill.hip) against the model of tests/fill_model_bb.py, which tests/test_bb_fill_model.py
pins to the witness builder. Every comparison is exact, device against model, read back through w.trace(c). Shapes: the U32Add
circuit at 16 rows (a partial workgroup), 128 (half of one) and 4 096 (16 workgroups of 256 lanes); the random programs at heights
1 (the next row is the row itself), 4 (the wrap of offset 1) and 512 (more than one workgroup at every lane count). The
counterpart of test_gpu_witness_fill.py."""
import numpy as np
import pytest
import torch  # (before the library opens the device)

import fill_model_bb as fm
from test_bb_fill_model import halves
from test_bb_witness_check_model import K, bb, fe, pack, pkg
from test_fill_model import SEQ_OLD, SEQ_WANT, sequential_program
from test_gpu_bb_lookup_balance import ctx  # noqa: F401  (the module-scoped context with the Poseidon2 permutation set)

pytestmark = pytest.mark.gpu
P = fm.P
_CACHE = {}
EDGES = [0, 1, 2, P - 1, P - 2, 0x40000000, 0x3FFFFFFF, 0x08000000, 0x07FFFFFF, 0xFFFF, 0x10000]
BG = (bb.CHECK_BETA, bb.CHECK_GAMMA)


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


def same(got, want):
    return got.shape == want.shape and np.array_equal(got.astype(np.uint64), np.asarray(want, dtype=np.uint64))


# ---------------------------------------------------------------- the bench system: U32Add filled from the 16-bit halves
def u32_system(ctx):
    if "u32" not in _CACHE:
        with fe.field(fe.BABYBEAR):
            _CACHE["u32"] = bb.System.new(ctx, fe.test_params(), fe.u32_add_system_inputs(), K)
    return _CACHE["u32"]


def u32_case(ctx, n):
    """(system, builder's traces, packed claims, the proof of the host-built witness, the halves program), computed once per n"""
    key = ("u32", n)
    if key not in _CACHE:
        s = u32_system(ctx)
        with fe.field(fe.BABYBEAR):
            traces, claims = fe.u32_add_bench_witness(n)
            prog = fe.u32_add_halves_fill_program(n)
        packed = pack([[int(v) % P for v in c] for c in claims])
        _CACHE[key] = (s, traces, packed, s.prove_multiple_claims(s.witness(traces, packed)).to_bytes(), prog)
    return _CACHE[key]


def zero_witness(s, traces, packed):
    return s.witness_from_device([dev32(np.zeros_like(t)) for t in traces], packed)


@pytest.mark.parametrize("n,layout", [(16, "u16"), (128, "u16"), (128, "i32"), (128, "u16_column_major"), (4096, "u16")])
def test_u32_add_witness_from_halves(ctx, n, layout):
    s, traces, packed, proof, prog = u32_case(ctx, n)
    h4 = halves(*fe.xorshift_pairs(n))
    if layout == "u16":
        inputs = dev(h4.astype(np.uint16))
        assert inputs.element_size() == 2 and inputs.is_contiguous()
    elif layout == "i32":
        inputs = dev(h4.astype(np.uint32))
        assert inputs.dtype == torch.int32
    else:
        inputs = dev(np.ascontiguousarray(h4.T).astype(np.uint16)).t()  # n x 4 with strides (1, n)
        assert tuple(inputs.shape) == (n, 4) and inputs.stride() == (1, n)
    w = zero_witness(s, traces, packed)
    rep = w.fill(1, prog, inputs)
    assert rep.fields() == (traces[1].shape[0], 14, 24, 256), str(rep)
    assert w.derive_multiplicities([(0, 0)]).ok
    assert same(w.trace(0), traces[0]) and same(w.trace(1), traces[1])
    assert w.check().verdict == 0 and w.lookup_balance().ok
    got = s.prove_multiple_claims(w).to_bytes()
    assert got == proof and s.verify_multiple_claims(packed, got) == 0


# ---------------------------------------------------------------- random programs on a circuit of its own
HEIGHTS = (1, 4, 512)
BYSTANDER, SEQ = len(HEIGHTS), len(HEIGHTS) + 1
CLAIMS = [[1, 2, 3], [P - 1], [], [7, 0]]


def lab_system(ctx):
    """one system for everything below: per height a circuit [6 main columns, 2 preprocessed], a bystander of 3 columns and a
    circuit of 4 columns without preprocessed trace. Nothing is ever proved with it: the constraints are placeholders."""
    if "lab" not in _CACHE:
        E = fe.Expr
        rng = np.random.default_rng(2024)
        pres = [rand_field(rng, (h, 2)) for h in HEIGHTS]
        with fe.field(fe.BABYBEAR):
            inputs = [fe.CircuitInputs(6, pre, [E.main(0) * E.main(1) - E.main(2)], [], []) for pre in pres]
            inputs += [fe.CircuitInputs(3, None, [E.main(0) * E.main(1) - E.main(2)], [], []),
                       fe.CircuitInputs(4, None, [E.main(0) * E.main(1) - E.main(2)], [], [])]
            _CACHE["lab"] = (bb.System.new(ctx, fe.test_params(), inputs, K), pres)
    return _CACHE["lab"]


def lab_witness(ctx, rng, hi, seq_trace=None):
    """a witness with circuit `hi` (height HEIGHTS[hi]) and the bystander active -> (witness, the traces it was made from)"""
    s, _ = lab_system(ctx)
    traces = [None] * (len(HEIGHTS) + 2)
    if hi is not None:
        traces[hi] = rand_field(rng, (HEIGHTS[hi], 6))
    traces[BYSTANDER] = rand_field(rng, (8, 3))
    if seq_trace is not None:
        traces[SEQ] = np.array(seq_trace, dtype=np.uint64)
    w = s.witness_from_device([None if t is None else dev32(t) for t in traces], pack(CLAIMS))
    return w, traces


def random_expr(rng, depth):
    """every operator, both offsets and the three sources; main columns 4 and 5 are never assigned, so their next row may be read.
    Call under field(BABYBEAR)."""
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
        return E.const(EDGES[int(rng.integers(0, len(EDGES)))] if k == 7 else int(rng.integers(0, P)))
    a, b = random_expr(rng, depth - 1), random_expr(rng, depth - 1)
    k = rng.integers(0, 9)
    if k == 8:
        lo = int(rng.integers(0, 32))
        return fe.bits(a, lo, int(rng.integers(1, 33 - lo)))
    return [lambda: a + b, lambda: a - b, lambda: a * b, lambda: -a, lambda: fe.inv0(a), lambda: fe.lt(a, b), lambda: fe.bit_xor(a, b),
            lambda: fe.bit_and(a, b)][k]()


def against_model(ctx, rng, hi, prog, inputs, elem_bytes=4):
    """fill circuit `hi` of a fresh witness on the device and in the model; everything else must stay as it was"""
    _, pres = lab_system(ctx)
    w, traces = lab_witness(ctx, rng, hi)
    acc = bb.claims_accumulator(w, *BG)
    want = fm.run(prog.blob, traces[hi], pres[hi], inputs)
    on_dev = None if inputs is None else dev(inputs.astype({1: np.uint8, 2: np.uint16, 4: np.uint32}[elem_bytes]))
    rep = w.fill(hi, prog, on_dev)
    got = w.trace(hi)
    assert same(got, want), "rows %s" % np.nonzero((got != want).any(axis=1))[0][:8]
    assigned = sorted({d for d, _ in prog.steps})
    others = [c for c in range(6) if c not in assigned]
    assert same(got[:, others], traces[hi][:, others])  # (the model says so too; this is the statement itself)
    assert same(w.trace(BYSTANDER), traces[BYSTANDER])
    assert bb.claims_accumulator(w, *BG) == acc
    assert (rep.rows, rep.steps) == (HEIGHTS[hi], len(prog.steps))
    return rep


@pytest.mark.parametrize("hi", range(len(HEIGHTS)))
def test_random_programs(ctx, hi):
    n = HEIGHTS[hi]
    rng = np.random.default_rng(700 + n)
    seen = set()
    for k in range(10):
        with fe.field(fe.BABYBEAR):
            steps = [(int(rng.integers(0, 4)), random_expr(rng, 4)) for _ in range(int(rng.integers(1, 7)))]
            prog = fe.compile_fill(6, 2, 3, steps)
        seen |= {node[0] for node in prog.nodes}
        h_in = n if k % 2 == 0 else max(1, int(rng.integers(1, n + 1)) - 1)  # the full height, and 0 < h_in < n where there is room
        eb = (1, 2, 4)[k % 3]  # the model is given the same small values the narrow elements hold
        against_model(ctx, rng, hi, prog, rand_field(rng, (h_in, 3), below=min(P, 1 << (8 * eb))), elem_bytes=eb)
    assert seen >= {fe.N_CONST, fe.N_VAR, fe.N_ADD, fe.N_SUB, fe.N_MUL, fe.N_NEG, fe.N_ROW, fe.N_BITS, fe.N_INV0, fe.N_LT, fe.N_XOR, fe.N_AND}


FIELDS = [(lo, length) for length in range(1, 32) for lo in range(0, 32 - length)]  # lo + length <= 31, all distinct


def chain_program(leaves):
    """`leaves` distinct bits leaves, all computed before the first is consumed and then consumed last one first: t_k = b_k -
    t_(k+1), and the walk of an operator takes its first operand first. The slot file holds them all at the deepest point."""
    E = fe.Expr
    with fe.field(fe.BABYBEAR):
        b = [fe.bits(E.input(k % 3), *FIELDS[k // 3]) for k in range(leaves)]
        t = b[-1]
        for k in range(leaves - 2, -1, -1):
            t = b[k] - t
        return fe.compile_fill(6, 2, 3, [(0, t), (3, E.main(0) * E.var(fe.SRC_PRE, 1, 1) + E.main_next(5))])


def lanes_of(slots):
    """the 64 KB rule of include/mstark_bb.h for four-byte slots"""
    return next((th for th in (256, 128, 64) if slots * th * 4 <= 64 * 1024), 0)


FORMS = [(8, 256), (100, 128), (200, 64), (300, 0)]


@pytest.mark.parametrize("leaves,form", FORMS)
def test_every_kernel_form(ctx, leaves, form):
    prog = chain_program(leaves)
    info = bb.fill_program_info(prog)
    assert info["slots"] >= leaves and info["assigned_columns"] == 2, info
    assert info["lds_lanes"] == lanes_of(info["slots"]) == form, info
    rng = np.random.default_rng(leaves)
    rep = against_model(ctx, rng, HEIGHTS.index(512), prog, rand_field(rng, (512, 3)))
    assert rep.lds_lanes == info["lds_lanes"] and rep.instructions == info["instructions"]
    assert {f for _, f in FORMS} == {256, 128, 64, 0}  # the four cases between them: every form


def test_sequential_semantics_and_host_waits_without_inputs(ctx):
    w, _ = lab_witness(ctx, np.random.default_rng(5), None, seq_trace=SEQ_OLD)
    assert w.trace(SEQ).tolist() == SEQ_OLD  # (the read-back is a host wait: nothing of the setup is pending)
    with fe.field(fe.BABYBEAR):
        prog = sequential_program(fe)
    before = ctx.sync_count()
    rep = w.fill(SEQ, prog)
    assert ctx.sync_count() == before  # no inputs: the call only queues work (include/mstark_bb.h, "Host waits")
    assert w.trace(SEQ).tolist() == SEQ_WANT and rep.fields()[:2] == (2, 4)


def test_host_waits_with_inputs(ctx):
    s, traces, packed, _, prog = u32_case(ctx, 16)
    w = zero_witness(s, traces, packed)
    inputs = dev(halves(*fe.xorshift_pairs(16)).astype(np.uint16))
    torch.cuda.synchronize()
    before = ctx.sync_count()
    w.fill(1, prog, inputs)
    assert ctx.sync_count() == before + 1  # the offender word of the inputs (include/mstark_bb.h, "Host waits")
    assert same(w.trace(1), traces[1])


def test_inputs_ordered_behind_the_producer_stream(ctx):
    n = 4096
    s, traces, packed, _, prog = u32_case(ctx, n)
    w = zero_witness(s, traces, packed)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        v = torch.arange(4 * n, dtype=torch.int64, device="cuda").reshape(n, 4)
        for _ in range(20):  # a queue of small launches the fill must wait for
            v = (v * 2654435761 + 12345) & 0xFFFF  # 16 bits: below p, and what the halves program expects
        v = v.to(torch.int32)
        w.fill(1, prog, v, stream=side)  # no synchronisation in between
    torch.cuda.synchronize()
    want = fm.run(prog.blob, np.zeros((n, 14), dtype=np.uint64), None, v.cpu().numpy().astype(np.uint64))
    assert same(w.trace(1), want)


def test_refusals_write_nothing(ctx):
    n = 16
    s, traces, packed, proof, prog = u32_case(ctx, n)
    rng = np.random.default_rng(11)
    start = [rand_field(rng, t.shape) for t in traces]
    w = s.witness_from_device([dev32(t) for t in start], packed)
    good = halves(*fe.xorshift_pairs(n))
    bad = good.copy()
    bad[5, 1] = P
    bad[9, 0] = P + 3  # a later offender: the first one in row-major order is named
    with fe.field(fe.BABYBEAR):
        narrow = fe.compile_fill(13, 0, 4, [(0, fe.Expr.input(0))])
    goldilocks = fe.u32_add_halves_fill_program(n)  # the same nodes under the other field's magic
    assert goldilocks.blob[8:] == prog.blob[8:] and goldilocks.blob[:8] != prog.blob[:8]
    cases = [(dev32(bad), prog, 1, ("row 5", "column 1")),
             (dev(np.zeros((2 * n, 4), dtype=np.uint16)), prog, 1, ("height",)),
             (None, prog, 1, ("input",)),                       # n_inputs > 0 and no matrix
             (dev32(good), narrow, 1, ("main_width 13",)),
             (dev32(good), prog, 0, ("main_width 14",)),
             (dev32(good), prog, 2, ("out of range",)),
             (dev(good.astype(np.uint64)), prog, 1, ("input", "elem_bytes")),  # 8-byte elements are no BabyBear input
             (dev32(good), goldilocks, 1, ("magic",))]
    for inputs, program, circuit, words in cases:
        with pytest.raises(pkg.MstarkError) as e:
            w.fill(circuit, program, inputs)
        assert str(e.value).startswith("msbb_witness_fill: ") and all(x in str(e.value) for x in words), str(e.value)
        assert same(w.trace(0), start[0]) and same(w.trace(1), start[1])
    # a host-resident witness, and an inactive circuit
    host = [t.astype(np.uint32) for t in start]
    hw = s.host_witness(host, packed)
    with pytest.raises(pkg.MstarkError, match="device-resident"):
        hw.fill(1, prog, dev32(good))
    assert all(same(a, b) for a, b in zip(host, start))
    half = s.witness_from_device([dev32(start[0]), None], pack([]))
    with pytest.raises(pkg.MstarkError, match="inactive"):
        half.fill(1, prog, dev32(good))
    assert same(half.trace(0), start[0])
    # the context is as good as new: a fresh witness is filled, derived and proved
    fresh = zero_witness(s, traces, packed)
    fresh.fill(1, prog, dev32(good))
    assert fresh.derive_multiplicities([(0, 0)]).ok
    got = s.prove_multiple_claims(fresh).to_bytes()
    assert got == proof and s.verify_multiple_claims(packed, got) == 0
