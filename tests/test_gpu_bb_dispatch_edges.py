"""GPU parity of the BabyBear / Poseidon2 path at the sizes where csrc/bb_kernels.hip switches kernels, which the other
BabyBear modules do not reach - every comparison bit-exact against the oracle compiled for the same configuration:
A. Merkle trees above COOP_MAX = 2^15 nodes: the single-lane leaf_hash_k (several absorbed blocks, a ragged last block,
   columns of several matrices, an injected group) and compress_k (with and without injection), and both sides of the
   threshold; the oracle's path verifier accepts the device's openings and rejects them with one sibling word changed.
B. scan_totals_k past one pass of 1024 block totals (the carry between passes): the claims accumulator beyond 2^20 claims,
   and stage 2 of a whole proof of the U32Add system at 2^17 rows x 13 lookups = 1664 blocks, also driven step by step.
C. subtree_k across workgroups (MSBB_SUBTREE_MAX_LOG above its default of 7): roots published, ticket counter, the last
   workgroup finishing the tree; and fused FRI rounds in which a workgroup owns more than 64 leaves.
References are computed once per input and shared between the cases that need them."""
import zlib

import numpy as np
import pytest

import oracle_bb as ob
from __graft_entry__ import load_package
from test_gpu_bb_level2 import level2_prove

pytestmark = pytest.mark.gpu
pkg = load_package()
fe = pkg.frontend
bb = pkg.babybear
P = fe.BABYBEAR["P"]
K = fe.poseidon2_constants()


@pytest.fixture(scope="module")
def ctx():
    c = pkg.Context(0)
    bb.set_poseidon2(c, K)
    ob.set_poseidon2(K)
    return c


def rand_field(rng, shape):
    v = rng.integers(0, P, shape, dtype=np.uint64)
    edge = np.array([0, 1, 2, P - 1, P - 2, 1 << 27, (1 << 27) + 1], dtype=np.uint64)
    mask = rng.random(shape) < 0.1
    return np.where(mask, edge[rng.integers(0, len(edge), shape)], v)


def _assert_same_bytes(got, want, what):
    """(asserting on two proofs themselves makes a failing pytest diff them, which takes minutes: compare first)"""
    same = got == want
    where = "" if same else "lengths %d / %d" % (len(got), len(want)) if len(got) != len(want) else "first at byte %d" % next(
        i for i in range(len(got)) if got[i] != want[i])
    assert same, "%s: bytes differ, %s" % (what, where)


# ---------------------------------------------------------------- Merkle trees (A and C share the checks)
_MATS, _TREES = {}, {}


def _reference_tree(shapes, cap_h):
    """(matrices, the oracle's tree over them): the matrices depend on the shapes alone, the tree is built once per cap height"""
    key = tuple(shapes)
    if key not in _MATS:
        rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
        _MATS[key] = [rand_field(rng, s) for s in shapes]
    if (key, cap_h) not in _TREES:
        _TREES[key, cap_h] = ob.Mmcs(_MATS[key], cap_h)
    return _MATS[key], _TREES[key, cap_h]


def _check_mmcs(ctx, shapes, cap_h):
    mats, o = _reference_tree(shapes, cap_h)
    g = bb.Mmcs(ctx, mats, cap_h)
    assert np.array_equal(g.cap, np.frombuffer(o.cap, dtype=np.uint32)), "cap differs"
    heights = [s[0] for s in shapes]
    maxh = max(heights)
    rng = np.random.default_rng(maxh + cap_h)
    odd = 0  # bit k set for every shorter matrix of height maxh >> k: its row (index >> k) is then odd
    for h in heights:
        if h < maxh:
            odd |= maxh // h
    indices = {0, 1, maxh // 2, maxh - 1, int(rng.integers(0, maxh)), int(rng.integers(0, maxh)), int(rng.integers(0, maxh)) | odd}
    bound = min(heights) >= (1 << cap_h)  # shorter matrices are not bound by a cap this tall
    for index in sorted(indices):
        gv, gp = g.open(index)
        ov, op = o.open(index)
        assert np.array_equal(gv, ov), ("opened values", index)
        assert np.array_equal(gp, np.frombuffer(op, dtype=np.uint32)), ("siblings", index)
        if bound:
            assert o.verify(index, gv, gp.tobytes(), g.cap.tobytes()) == 1, ("the oracle's verifier rejects the device's opening", index)
            bad = gp.copy()
            pos = int(rng.integers(0, bad.size))
            bad[pos] = (int(bad[pos]) + 1) % P
            assert o.verify(index, gv, bad.tobytes(), g.cap.tobytes()) == 0, ("a changed sibling word is accepted", index, pos)


@pytest.mark.parametrize("cap_h", [0, 3])
@pytest.mark.parametrize("shapes", [
    [(1 << 16, 9), (1 << 16, 8)],                  # leaf_hash_k: two matrices, 17 columns = blocks of 8, 8 and 1; compress_k, no injection
    [(1 << 16, 1)],                                # one partial block
    [(1 << 16, 8)],                                # exactly one full block
    [(1 << 17, 3), (1 << 16, 17), (1 << 15, 1)],   # compress_k + leaf_hash_k injecting at 2^16, then the cooperative pair at exactly 2^15
    [(1 << 16, 2), (1 << 15, 9)],                  # single-lane leaves, cooperative first compression and injected group
    [(1 << 17, 1), (1 << 16, 1), (1 << 16, 7)],    # two matrices in the injected group
], ids=lambda s: "+".join("%dx%d" % (h.bit_length() - 1, w) for h, w in s))
def test_mmcs_above_coop_max(ctx, shapes, cap_h):
    _check_mmcs(ctx, shapes, cap_h)


# ---------------------------------------------------------------- B: scans past one pass of block totals
@pytest.fixture(scope="module")
def claims_system(ctx):
    """the claims do not depend on the traces: the 4-row MulAir carries them"""
    with fe.field(fe.BABYBEAR):
        return bb.System.new(ctx, fe.test_params(), fe.mul_air_inputs(), K), fe.mul_air_smoke_trace()


@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, 1 << 20, (1 << 20) + 1, (1 << 20) + 1025])
def test_claims_accumulator_block_total_passes(ctx, claims_system, n):
    """1024 claims per block, 1024 block totals per pass of scan_totals_k: above 2^20 claims the carry crosses passes"""
    system, trace = claims_system
    rng = np.random.default_rng(n)
    lens = rng.integers(0, 6, n)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    data = rand_field(rng, int(offs[-1]))
    beta, gamma = ([int(x) for x in rng.integers(0, P, 4)] for _ in range(2))
    w = system.witness([trace], (offs, data))
    assert bb.claims_accumulator(w, beta, gamma) == ob.claims_accumulator((offs, data), beta, gamma)


def test_stage2_block_total_passes_in_a_proof(ctx):
    """[ByteTable, U32Add] at 2^17 additions: stage 2 scans 2^17 rows x 13 lookups = 1664 blocks of 1024, two passes of
    scan_totals_k (2^16 rows would fit one); 2^17 claims. Eight queries and no proof of work keep the rest short. The whole
    proof equals the oracle's, the oracle's verifier accepts it, and the Level-2 loop yields the same bytes."""
    with fe.field(fe.BABYBEAR):
        params = fe.Params(1, 0, 0, 1, 8, 0, 0)
        system = bb.System.new(ctx, params, fe.u32_add_system_inputs(), K)
        traces, claims = fe.u32_add_bench_witness(1 << 17)
        packed = fe.pack_claims(claims)
    info = system.circuit_info(1)
    assert traces[1].shape[0] * info["num_lookups"] > 1 << 20 and len(packed[0]) - 1 == 1 << 17
    o = ob.System(system.blob)
    want = o.prove(traces, packed)
    got = system.prove_multiple_claims(system.witness(traces, packed)).to_bytes()
    _assert_same_bytes(got, want, "msbb_prove against the oracle")
    assert o.verify(packed, got) == 0
    stepwise, _, _ = level2_prove(system, params, traces, packed)
    _assert_same_bytes(stepwise, want, "the Level-2 loop against the oracle")


# ---------------------------------------------------------------- C: the one-launch tree across workgroups
SUBTREE_LOGS = [10, 11, 13, 16]


@pytest.mark.parametrize("shapes", [
    # (what the largest value, 16, makes of each; a smaller one runs layer by layer down to 2^max_log children first)
    [(1 << 10, 3)],                   # one workgroup of 1024 children
    [(1 << 11, 3)],                   # 256 workgroups of 8
    [(1 << 13, 2), (1 << 11, 3)],     # the one-launch form starts right below the last injection
    [(1 << 16, 2)],                   # 256 workgroups of 256
    [(1 << 17, 1)],                   # one layer-by-layer step first
], ids=lambda s: "+".join("%dx%d" % (h.bit_length() - 1, w) for h, w in s))
@pytest.mark.parametrize("max_log", SUBTREE_LOGS, ids=lambda v: "log%d" % v)
def test_mmcs_subtree_across_workgroups(ctx, monkeypatch, max_log, shapes):
    monkeypatch.setenv("MSBB_SUBTREE_MAX_LOG", str(max_log))
    for cap_h in (0, 2):
        _check_mmcs(ctx, shapes, cap_h)


_PROOFS = {}


def _proof_case(ctx, case):
    """(system, traces, packed claims, the oracle's proof, the oracle's verdict on it), made once per case"""
    if case not in _PROOFS:
        with fe.field(fe.BABYBEAR):
            if case == "even_odd":
                inputs, traces, claims = fe.even_odd_inputs(), fe.even_odd_traces(), [[0, 4, 1]]
            else:
                inputs, traces, claims = fe.mul_air_inputs(), [fe.mul_air_trace(1 << int(case[4:]))], []
            g = bb.System.new(ctx, fe.test_params(), inputs, K)
            packed = fe.pack_claims(claims)
        o = ob.System(g.blob)
        want = o.prove(traces, packed)
        _PROOFS[case] = (g, traces, packed, want, o.verify(packed, want))
    return _PROOFS[case]


@pytest.mark.parametrize("case", ["mul_13", "mul_17", "even_odd"])
@pytest.mark.parametrize("max_log", SUBTREE_LOGS, ids=lambda v: "log%d" % v)
def test_proofs_with_subtree_across_workgroups(ctx, monkeypatch, max_log, case):
    """fused FRI rounds whose leaves span several workgroups, the challenger step in the last one to arrive: the bytes are the
    oracle's (what the library writes with the variable unset), from a device- and from a host-resident witness"""
    g, traces, packed, want, verdict = _proof_case(ctx, case)
    assert verdict == 0
    monkeypatch.setenv("MSBB_SUBTREE_MAX_LOG", str(max_log))
    got = g.prove_multiple_claims(g.witness(traces, packed)).to_bytes()
    _assert_same_bytes(got, want, "device-resident witness against the oracle")
    hw = g.host_witness(traces, packed)
    for _ in range(2):
        _assert_same_bytes(g.prove_multiple_claims(hw).to_bytes(), want, "host-resident witness against the oracle")
    assert g.verify(packed, got) == verdict, "product verifier (msbb_verify) disagrees with the oracle's"
