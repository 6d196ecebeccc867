"""GPU parity of the Goldilocks / BLAKE3 path at the sizes where the host code switches kernels and which the other
modules do not reach (hash.hip, open.hip, lookup.hip, prover.hip) - every comparison bit-exact against the oracle:
A. Merkle trees (build_levels / subtree_k): the register-level first level of a workgroup that owns 2048 children, plain
   and with an injected group there (chunked and multi-chunk rows), 512 and 1024 workgroups, the layer-by-layer kernels
   (compress3_k, compress3_lds_k and its three-position guard, compress_layer_k<INJ, MULTI>) in front of a late subtree_k
   or tree_tail_k, under MSAMD_SUBTREE_MAX_LOG and MSAMD_NO_SUBTREE. The oracle's path verifier accepts the device's
   openings and rejects them with one sibling word changed.
B. BLAKE3 streams above 2048 chunks: cv_level_k with an odd last chaining value at one level and at two successive ones.
C. Whole proofs of six circuits whose LDEs have 2^15 .. 2^11 and 2^9 rows (2^14 .. 2^10 and 2^8 at blow-up 2), so that a
   shorter reduced opening rolls in at every FRI round above the single-workgroup tail, in front of it and inside it,
   through fused and unfused rounds and the hand-over between them (MSAMD_FRI_FUSED_MAX_LOG); and the bench system under
   the same knobs.
D. The claims accumulator at one block of 4096 claims more or less and past one pass of scan_totals_k; stage 2 with more
   than 16 lookups per row (second chunk of for_each_inverse, ragged tile of stage2_write_k) and lookups of more than 64
   arguments (the Horner branch of message()).
References are computed once per input and shared between the knob values."""
import zlib

import numpy as np
import pytest

from conftest import P, rand_field

pytestmark = pytest.mark.gpu

_MATS, _TREES, _PROOFS = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release_references():
    """(the widest matrix here is 270 MB and the oracle's tree holds a copy: nothing of it outlives the module)"""
    yield
    for cache in (_MATS, _TREES, _PROOFS):
        cache.clear()


def _assert_same_bytes(got, want, what):
    """(asserting on two proofs themselves makes a failing pytest diff them, which takes minutes: compare first)"""
    same = got == want
    where = "" if same else "lengths %d / %d" % (len(got), len(want)) if len(got) != len(want) else "first at byte %d" % next(
        i for i in range(len(got)) if got[i] != want[i])
    assert same, "%s: bytes differ, %s" % (what, where)


def _shape_id(shapes):
    return "+".join("%dx%d" % (h.bit_length() - 1, w) for h, w in shapes)


# ---------------------------------------------------------------- A: Merkle trees
def _reference_tree(oracle, shapes, cap_h):
    """(matrices, the oracle's tree over them): the matrices depend on the shapes alone, the tree is built once per cap height"""
    key = tuple(shapes)
    if key not in _MATS:
        rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
        _MATS[key] = [rand_field(rng, s) for s in shapes]
    if (key, cap_h) not in _TREES:
        _TREES[key, cap_h] = oracle.Mmcs(_MATS[key], cap_h)
    return _MATS[key], _TREES[key, cap_h]


def _leaves_per_workgroup(maxh, max_log):
    """Leaves below one workgroup of subtree_k when the one-launch form starts at the tallest layer it may take (2^max_log
    digests; hash.hip subtree_children_per_group: one workgroup up to 1024 children, else len / 256 clamped to 8 .. 2048
    children each). Where the launch starts lower its workgroups own a power-of-two multiple of this, so a boundary
    between two of these spans is a boundary there as well. -> (leaves per workgroup, workgroups)"""
    child_len = min(maxh, 1 << max_log)
    sub = child_len if child_len <= 1024 else min(max(child_len // 256, 8), 2048)
    nb = child_len // sub
    return maxh // nb, nb


def _check_mmcs(pkg, ctx, oracle, shapes, cap_h, max_log=20):
    mats, o = _reference_tree(oracle, shapes, cap_h)
    g = pkg.Mmcs(ctx, mats, cap_h)
    _assert_same_bytes(g.cap, o.cap, "cap")
    heights = [s[0] for s in shapes]
    maxh = max(heights)
    span, nb = _leaves_per_workgroup(maxh, max_log)
    odd = 0  # bit k set for every shorter matrix of height maxh >> k: its row (index >> k) is then odd
    for h in heights:
        if h < maxh:
            odd |= maxh // h
    mid = nb // 2
    indices = {0, 1, maxh // 2, maxh - 1,
               span // 3, mid * span + span // 3, maxh - 1 - span // 3,   # inside the first, a middle and the last workgroup's sub-tree
               (mid * span + span // 5) | odd}
    if nb > 1:
        indices |= {(mid + 1) * span - 1, (mid + 1) * span}                 # both sides of one boundary between workgroups
    rng = np.random.default_rng(maxh + cap_h)
    assert min(heights) >= 1 << cap_h  # (shorter matrices would not be bound by a cap this tall)
    for index in sorted(indices):
        gv, gp = g.open(index)
        ov, op = o.open(index)
        assert np.array_equal(gv, ov), ("opened values", index)
        assert gp == op, ("siblings", index)
        assert o.verify(index, gv, gp, g.cap) == 1, ("the oracle's verifier rejects the device's opening", index)
        bad = np.frombuffer(gp, dtype=np.uint32).copy()
        pos = int(rng.integers(0, bad.size))
        bad[pos] ^= np.uint32(1 << int(rng.integers(0, 32)))
        assert o.verify(index, gv, bad.tobytes(), g.cap) == 0, ("a changed sibling word is accepted", index, pos)


# default dispatch (MSAMD_SUBTREE_MAX_LOG unset = 20): a layer of 2^19 digests or more gives workgroups of 2048 children,
# whose first level runs in registers
@pytest.mark.parametrize("shapes,cap_h", [
    ([(1 << 19, 1)], 0),                      # sub == 2048, plain: 256 workgroups
    ([(1 << 19, 1)], 3),
    ([(1 << 19, 1), (1 << 18, 2)], 0),        # the injected group at the register level (p.inj_len == glen there)
    ([(1 << 19, 1), (1 << 18, 2)], 3),
    ([(1 << 19, 1), (1 << 18, 129)], 0),      # the same with rows longer than one BLAKE3 chunk (hash_row<true>)
    ([(1 << 19, 2), (1 << 10, 3)], 0),        # injection inside a workgroup's sub-tree in LDS (tree_level<true>, n = 2)
    ([(1 << 20, 1), (1 << 8, 3)], 0),         # nb = 512, injection in the first level over the 512 roots
    ([(1 << 21, 1), (1 << 18, 1)], 0),        # compress3_k's guard with the injection at li + 2: compress_layer_k, then subtree_k (nb = 512)
    ([(1 << 21, 1)], 0),                      # compress3_k (n3 = 2^18), then subtree_k over 2^18 digests
], ids=lambda v: _shape_id(v) if isinstance(v, list) else "cap%d" % v)
def test_mmcs_tall_trees(pkg, ctx, oracle, shapes, cap_h):
    _check_mmcs(pkg, ctx, oracle, shapes, cap_h)


# MSAMD_SUBTREE_MAX_LOG=21, the largest the kernel claims: one launch over 2^21 digests = 1024 workgroups of 2048 children;
# the last workgroup to arrive reads the 1024 roots = 8192 words, which is all of subtree_k's `sh`
@pytest.mark.parametrize("shapes", [
    [(1 << 21, 1)],
    [(1 << 21, 1), (1 << 9, 2)],              # injection in the first level over the 1024 roots
], ids=_shape_id)
def test_mmcs_subtree_upper_limit(pkg, ctx, oracle, monkeypatch, shapes):
    monkeypatch.setenv("MSAMD_SUBTREE_MAX_LOG", "21")
    _check_mmcs(pkg, ctx, oracle, shapes, 0, max_log=21)


# The threshold pulled down under a 2^14-leaf tree: the layers above it run compress3_lds_k (three levels, only if none of
# them takes an injected group) or compress_layer_k, then subtree_k from 2^max_log digests (tree_tail_k from 2^10 with
# MSAMD_NO_SUBTREE=1). What value 11 makes of each shape:
@pytest.mark.parametrize("shapes", [
    [(1 << 14, 1), (1 << 13, 2)],                 # guard position li: compress_layer_k<true>, compress_layer_k, subtree_k
    [(1 << 14, 1), (1 << 12, 2)],                 # li + 1: compress_layer_k, compress_layer_k<true>, subtree_k
    [(1 << 14, 1), (1 << 11, 2)],                 # li + 2: two plain layers, compress_layer_k<true>, subtree_k
    [(1 << 14, 1), (1 << 10, 2)],                 # compress3_lds_k, then the injection in subtree_k's first level
    [(1 << 14, 1), (1 << 3, 2)],                  # compress3_lds_k, then the injection over the 256 roots' upper levels
    [(1 << 14, 1), (1 << 12, 2), (1 << 6, 3)],    # one injection on each side of the threshold
    [(1 << 14, 2), (1 << 12, 200)],               # a wide injected layer on the layer path: compress_layer_k<true, true>
], ids=_shape_id)
@pytest.mark.parametrize("knob", ["MSAMD_SUBTREE_MAX_LOG=10", "MSAMD_SUBTREE_MAX_LOG=11", "MSAMD_SUBTREE_MAX_LOG=13", "MSAMD_NO_SUBTREE=1"])
def test_mmcs_threshold_pulled_down(pkg, ctx, oracle, monkeypatch, knob, shapes):
    name, value = knob.split("=")
    monkeypatch.setenv(name, value)
    for cap_h in (0, 2):
        _check_mmcs(pkg, ctx, oracle, shapes, cap_h, max_log=int(value) if name == "MSAMD_SUBTREE_MAX_LOG" else 10)


# ---------------------------------------------------------------- B: BLAKE3 streams above the tail's 2048 chunks
@pytest.mark.parametrize("n", [
    2048 * 1024,              # exactly 2048 chunks: the last size cv_tail_k takes alone
    2048 * 1024 + 1,          # 2049 chunks: cv_level_k carries an odd last value, 1025 values to the tail
    4098 * 1024 + 517,        # 4099 -> 2050 -> 1025 -> tail: odd, even, then an odd count inside the tail
    8197 * 1024,              # 8197 -> 4099 -> 2050 -> tail: odd at two successive levels, last chunk full
])
def test_blake3_stream_above_the_tail(ctx, oracle, n):
    data = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes()
    assert ctx.blake3(data) == oracle.hash_bytes(data)


# ---------------------------------------------------------------- C: whole proofs
def _reference_proof(pkg, ctx, oracle, fe, case):
    """(inputs, params, traces, packed claims, the oracle's system, the oracle's proof, the oracle's verdict on it) once per case"""
    if case not in _PROOFS:
        if case[0] == "heights":
            heights = [1 << k for k in (13, 12, 11, 10, 9, 7)]
            inputs = fe.pythagorean_inputs() * len(heights)
            traces, claims = [fe.pythagorean_trace(h) for h in heights], []
            params = fe.Params(log_blowup=case[1], cap_height=0, log_final_poly_len=0, num_queries=12, commit_proof_of_work_bits=2,
                               query_proof_of_work_bits=3)
        else:
            inputs, params = fe.u32_add_system_inputs(), fe.bench_params()
            traces, claims = fe.u32_add_bench_witness(1 << 13)
        packed = fe.pack_claims(claims)
        o = oracle.System(pkg.System.new(ctx, params, inputs).blob)
        want = o.prove(traces, packed)
        _PROOFS[case] = (inputs, params, traces, packed, o, want, o.verify(packed, want))
    return _PROOFS[case]


def _prove_under_knob(pkg, ctx, oracle, fe, monkeypatch, case, knob):
    """_prove_both of test_gpu_prove.py with the knob set and the oracle's side shared: -> the device's proof"""
    inputs, params, traces, packed, o, want, verdict = _reference_proof(pkg, ctx, oracle, fe, case)
    assert verdict == 0
    if knob:
        name, value = knob.split("=")
        monkeypatch.setenv(name, value)
    g = pkg.System.new(ctx, params, inputs)
    assert g.preprocessed_commit() == o.preprocessed_commit()
    proof = g.prove_multiple_claims(g.witness(traces, packed)).to_bytes()
    _assert_same_bytes(proof, want, "ms_prove against the oracle")
    assert o.verify(packed, proof) == 0
    assert g.verify_multiple_claims(packed, proof) == 0
    return proof


# Six pythagorean circuits of 2^13, 2^12, 2^11, 2^10, 2^9 and 2^7 rows. At blow-up 4 the FRI inputs have 2^15 .. 2^11 and
# 2^9 values, the commit phase folds 2^15 -> 2^14 -> 2^13 -> 2^12 -> 2^11 (roll-ins of 2^14, 2^13, 2^12, 2^11), and from 2^11
# values on the single-workgroup tail takes over (fri_tail_k; 2^9 rolls in inside it). A round that commits a vector of
# 2r values (r leaves) is fused with the fold in front of it when fri_round_fusable(2r): r <= 2^MSAMD_FRI_FUSED_MAX_LOG
# (default 21). Writing F(n) for "fold to n values fused with the round that commits them", U(n) for fri_fold_dev to n
# values (+L: it also hashes the next round's leaves), each with the roll-in of n values, the loop of fri_prove gives
#   no knob                     leaves of round 0 from deep_reduce, tree; F(2^14) F(2^13) F(2^12) U(2^11) tail
#   MSAMD_FRI_FUSED_MAX_LOG=11  U(2^14)+L tree, U(2^13)+L tree, F(2^12), U(2^11), tail
#   MSAMD_FRI_FUSED_MAX_LOG=12  U(2^14)+L tree, F(2^13) F(2^12) U(2^11) tail: an unfused round hands over to a fused one
#   MSAMD_NO_FRI_FUSED=1        U(2^14)+L U(2^13)+L U(2^12)+L, each followed by its tree; U(2^11); tail
#   MSAMD_NO_FRI_TAIL=1         as without a knob down to F(2^12), then F(2^11) F(2^10) .. F(2^3) U(2^2): 2^9 rolls into a fused round
#   MSAMD_NO_DEEP_LEAVES=1      round 0 hashes its own leaves (fri_tree_build from the vector), then as without a knob
#   MSAMD_HOST_FRI=1            the host-driven loop: fri_tree_build, cap_and_grind and fri_fold with the roll-in, every round
#   MSAMD_NO_SUBTREE=1          nothing is fusable: as MSAMD_NO_FRI_FUSED, the trees layer by layer with tree_tail_k<CH>
#   MSAMD_SUBTREE_MAX_LOG=11    fused rounds as without a knob; round 0's tree (2^14 leaves) and every input commitment run
#                               compress3_lds_k down to 2^11 digests, then subtree_k
# At blow-up 2 every size is halved: 2^14 -> .. -> 2^11, roll-ins of 2^13, 2^12, 2^11 above the tail, 2^10 and 2^8 inside it;
# value 11 gives U(2^13)+L tree, F(2^12), U(2^11), tail; value 12 is the default plan F(2^13) F(2^12) U(2^11) tail.
KNOBS = [None, "MSAMD_FRI_FUSED_MAX_LOG=11", "MSAMD_FRI_FUSED_MAX_LOG=12", "MSAMD_NO_FRI_FUSED=1", "MSAMD_NO_FRI_TAIL=1",
         "MSAMD_NO_DEEP_LEAVES=1", "MSAMD_HOST_FRI=1", "MSAMD_NO_SUBTREE=1", "MSAMD_SUBTREE_MAX_LOG=11"]


@pytest.mark.parametrize("knob", KNOBS, ids=lambda k: k or "default")
@pytest.mark.parametrize("log_blowup", [2, 1], ids=lambda v: "blowup%d" % (1 << v))
def test_roll_ins_at_every_round_above_the_tail(pkg, ctx, oracle, fe, monkeypatch, log_blowup, knob):
    _prove_under_knob(pkg, ctx, oracle, fe, monkeypatch, ("heights", log_blowup), knob)


# [ByteTable, U32Add] at 2^13 additions, the system of test_alternative_paths_give_the_same_proof: 2^15-row LDEs, the second
# height is the 256-row byte table, which rolls in inside the tail. FRI_FUSED_MAX_LOG as above without roll-ins above the tail;
# SUBTREE_MAX_LOG=4 leaves subtree_k the top of every tree only (16 digests, one workgroup), 11 starts it at 2^11
@pytest.mark.parametrize("knob", ["MSAMD_FRI_FUSED_MAX_LOG=11", "MSAMD_FRI_FUSED_MAX_LOG=12", "MSAMD_SUBTREE_MAX_LOG=4", "MSAMD_SUBTREE_MAX_LOG=11"])
def test_bench_system_under_the_size_knobs(pkg, ctx, oracle, fe, monkeypatch, knob):
    if "default" not in _PROOFS:
        _PROOFS["default"] = _prove_under_knob(pkg, ctx, oracle, fe, monkeypatch, ("bench",), None)
    got = _prove_under_knob(pkg, ctx, oracle, fe, monkeypatch, ("bench",), knob)
    _assert_same_bytes(got, _PROOFS["default"], "against the proof with no knob set")


# ---------------------------------------------------------------- D: lookups
# claims_acc_k takes 4096 claims per block; scan_totals_k sums 256 block totals per pass, so its carry between passes
# starts at 2^20 + 1 claims
@pytest.mark.parametrize("n", [4095, 4096, 4097, 1 << 20, (1 << 20) + 1, (1 << 20) + 4097])
def test_claims_accumulator_block_edges(ctx, oracle, n):
    rng = np.random.default_rng(n)
    lens = rng.integers(0, 4, n)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    data = rand_field(rng, int(offs[-1]))
    beta, gamma = ([int(x) for x in rng.integers(2, P, 2, dtype=np.uint64)] for _ in range(2))
    assert ctx.claims_accumulator((offs, data), beta, gamma) == oracle.claims_accumulator((offs, data), beta, gamma)


# 33 lookups per row: three chunks of for_each_inverse (16, 16, 1), five tiles of stage2_write_k (the last with one term);
# widths 0 and 1, MAX_GPOW = 64 (the last width on precomputed powers of gamma), 65 and 130 (Horner). With every argument
# P - 1 the unreduced accumulation over 64 products and every Horner step see the largest operand.
# 17 lookups at 2048 rows: the second chunk together with two blocks of the row scan
@pytest.mark.parametrize("h,widths,args", [(64, [0, 1, 64, 65, 130] + [2] * 28, "random"), (64, [0, 1, 64, 65, 130] + [2] * 28, "max"),
                                           (2048, [1] * 17, "random")], ids=["h64-33-random", "h64-33-max", "h2048-17-random"])
def test_stage2_many_and_wide_lookups(ctx, oracle, h, widths, args):
    rng = np.random.default_rng(h + len(widths))
    offs = np.concatenate([[0], np.cumsum(widths)]).astype(np.uint64)
    mult = rand_field(rng, (h, len(widths)))
    a = rand_field(rng, (h, int(offs[-1]))) if args == "random" else np.full((h, int(offs[-1])), P - 1, dtype=np.uint64)
    # challenges are uniformly random in the protocol: no edge values here (a zero message has no inverse)
    beta, gamma = ([int(x) for x in rng.integers(2, P, 2, dtype=np.uint64)] for _ in range(2))
    gt, ga = ctx.stage2_trace(mult, offs, a, beta, gamma, [3, 9])
    ot, oa = oracle.stage2_trace(mult, offs, a, beta, gamma, [3, 9])
    assert ga == oa
    assert np.array_equal(gt, ot)
