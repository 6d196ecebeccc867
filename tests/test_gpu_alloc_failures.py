"""`-m gpu`: what the witness-building calls leave behind when a device allocation fails, at every allocation point of each call
and in both fields. Context.debug_fail_alloc(nth) makes the nth allocation from then on throw on the host, before hipMalloc;
alloc_failure_sweep.sweep makes one call under nth = 1, 2, ... until it returns. After every failure the case's contract is
checked - the witness, its claims and its held lookup values as before the call (the proof of the oracle sees stale held
values), or no witness at all - and after the success the call's result. A lower bound on the failing points, counted in the
source and cited next to each number, shows that the path the case names was taken.

Expected values come from the models of tests/ and from the oracle provers, never from a run of the library. The module has a
context of its own: the countdown is per context, so a countdown left armed reaches no other module. The systems of the other
GPU modules are bound to their contexts, so the systems here are made for this one, from the same circuit inputs, programs
and operand generators."""
import numpy as np
import pytest
import torch  # (before the library opens the device)

import argsort_model as am
import fill_gather_model as gm
import multiplicity_model as mm
import multiplicity_model_bb as mmb
from alloc_failure_sweep import own_cache, sweep

pytestmark = pytest.mark.gpu
P = gm.GOLDILOCKS_P
_CACHE = {}


@pytest.fixture(scope="module")
def actx(pkg):
    """the context of the sweeps, with the BabyBear permutation set"""
    import oracle_bb as ob
    from test_bb_witness_check_model import K, bb

    c = pkg.Context(0)
    bb.set_poseidon2(c, K)
    ob.set_poseidon2(K)
    yield c
    c.debug_fail_alloc(0)
    _CACHE.clear()  # the systems of this context go with it, not at interpreter exit


def dev(a):
    """a numpy array of unsigned integers as a torch tensor on the GPU (same bits, same element size)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])).cuda()


def once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def dense(s, traces):
    """the traces as the oracle takes them: an inactive circuit is a trace of no rows"""
    return [np.zeros((0, s.circuit_info(ci)["main_width"]), dtype=np.uint64) if t is None else np.asarray(t, dtype=np.uint64) for ci, t in enumerate(traces)]


def gl_witness(s, osys, traces, packed, route):
    """device: torch tensors through ms_witness_create_device, no held lookup values. held: ms_witness_create with explicit
    lookup values (the traces' own, from the oracle), which the witness then holds whatever kernels the system has"""
    if route == "device":
        return s.witness_from_device([None if t is None else dev(t) for t in traces], packed)
    if not any(s.circuit_info(ci)["num_lookups"] for ci in range(s.n_circuits)):
        return s.witness(traces, packed)
    full = dense(s, traces)
    return s.witness(full, packed, lookups=[osys.compute_lookup_values(ci, t) for ci, t in enumerate(full)])


class Unchanged:
    """the all-or-nothing checks of a Goldilocks witness: every trace byte-identical to `traces`, the claims' accumulator the
    oracle's, and the proof the oracle's proof of `traces` - which is what sees held lookup values that are stale"""

    def __init__(self, pkg, oracle, s, osys, w, packed):
        self.pkg, self.oracle, self.s, self.osys, self.w, self.packed = pkg, oracle, s, osys, w, packed
        self.acc = oracle.claims_accumulator(packed, pkg.CHECK_BETA, pkg.CHECK_GAMMA)
        self.proofs = {}

    def __call__(self, traces, when, key):
        for ci, t in enumerate(dense(self.s, traces)):
            got = self.w.trace(ci)
            assert got.shape[0] == t.shape[0] and np.array_equal(got, t.reshape(got.shape)), "trace differs %s: circuit %d" % (when, ci)
        assert self.w.claims_accumulator(self.pkg.CHECK_BETA, self.pkg.CHECK_GAMMA) == self.acc, "claims differ %s" % when
        if key not in self.proofs:  # (once per case and state)
            self.proofs[key] = self.osys.prove(dense(self.s, traces), self.packed)
        assert self.s.prove_multiple_claims(self.w).to_bytes() == self.proofs[key], "proof differs %s" % when


def mutate_case(pkg, oracle, ctx, label, s, traces, packed, route, call, want, at_least, after=None):
    """the sweep of a call that mutates a Goldilocks witness made from `traces`; `want`: the model's traces after a success"""
    osys = oracle.System(s.blob)
    w = gl_witness(s, osys, traces, packed, route)
    same = Unchanged(pkg, oracle, s, osys, w, packed)
    same(traces, "before the first call", "before")

    def success(result):
        same(want, "after the successful call", "after")
        if after:
            after(result)

    return sweep(pkg, ctx, label, lambda: call(w), lambda nth: same(traces, "after a failed call (allocation %d)" % nth, "before"), success, at_least)


# ---------------------------------------------------------------- a. ms_witness_fill
# The device allocations of the call, fl_witness_fill in csrc/fill_dev.h (one driver for both fields): d_code, d_outs and d_consts
# always; scratch when a group's slot file goes to the global scratch; tmp when there is a scan, and aggs and starts when the
# height is above one scan tile; inp and bad when the program reads inputs. All of them precede the first launch that writes
# the trace (the group loop), and the held lookup values are recomputed by one launch without an allocation (GlFill::after).
FILL_ALWAYS, FILL_SCRATCH, FILL_SCAN, FILL_TILES, FILL_INPUTS = 3, 1, 1, 2, 2


def scan_lab(pkg, fe, ctx):
    """the two scan circuits of test_gpu_witness_fill_scan (columns (x, s), a lookup pair on s), on this module's context"""
    from test_gpu_witness_fill_scan import airs

    return once("scan", lambda: pkg.System.new(ctx, fe.test_params(), airs(fe)))


def memory_lab(pkg, fe, ctx):
    """the memory circuit of test_gpu_witness_argsort (columns addr, val, s_addr, s_val; the log pushed, the sorted log pulled)"""
    from test_gpu_witness_argsort import memory_air

    return once("memory", lambda: pkg.System.new(ctx, fe.test_params(), [memory_air(fe)]))


def fill_programs(pkg, fe, ctx):
    """name -> (system, traces before, packed claims, circuit, program, inputs, preprocessed, lower bound)"""
    import test_gpu_witness_fill as tf
    import test_gpu_witness_fill_scan as ts
    from test_gpu_witness_argsort import ADDR, S_ADDR, S_VAL, VAL

    def make():
        E = fe.Expr
        out = {}
        # (i) the U32Add program over inputs at n = 128: slots in LDS, no scan
        n = 128
        s = pkg.System.new(ctx, fe.test_params(), fe.u32_add_system_inputs())
        traces, claims = fe.u32_add_bench_witness(n)
        rng = np.random.default_rng(3101)
        start = [tf.rand_field(rng, t.shape) for t in traces]
        pairs = np.stack(fe.xorshift_pairs(n), axis=1).astype(np.uint64)
        out["u32_add"] = (s, start, fe.pack_claims(claims), 1, fe.u32_add_fill_program(n), pairs, None, FILL_ALWAYS + FILL_INPUTS)
        # (ii) an ordinary group, an affine scan and an additive scan at two scan tiles
        T = ts.tile(pkg, fe)
        n = 2 * T
        s = scan_lab(pkg, fe, ctx)
        m, x, y = E.input(0), E.input(1), E.input(2)
        prog = fe.compile_fill(2, 0, 3, [(0, m * y), (1, fe.scan(E.main(0), x, init=ts.INIT)), (0, fe.running_sum(E.main(1) * y, init=7))])
        assert pkg.fill_program_info(prog)["lds_lanes"] != 0 and pkg.fill_scan_info(prog)[3] == T
        rng = np.random.default_rng(3102)
        start = [rng.integers(0, P, size=(n, 2), dtype=np.uint64) for _ in range(2)]
        out["groups_and_scans"] = (s, start, fe.pack_claims([]), 0, prog, ts.operands(rng, n, 3, T), None,
                                   FILL_ALWAYS + FILL_SCAN + FILL_TILES + FILL_INPUTS)
        # (iii) 300 live leaves: the slot file lies in the global scratch
        with own_cache(tf):
            s, pres = tf.lab_system(pkg, fe, ctx)
        hi = tf.HEIGHTS.index(512)
        prog = tf.chain_program(fe, 300)
        assert pkg.fill_program_info(prog)["lds_lanes"] == 0
        rng = np.random.default_rng(3103)
        start = [None] * (len(tf.HEIGHTS) + 2)
        start[hi], start[tf.BYSTANDER] = tf.rand_field(rng, (512, 6)), tf.rand_field(rng, (8, 3))
        out["global_scratch"] = (s, start, fe.pack_claims(tf.CLAIMS), hi, prog, tf.rand_field(rng, (512, 3)), pres[hi],
                                 FILL_ALWAYS + FILL_SCRATCH + FILL_INPUTS)
        # (iv) the argsort-then-fill example of include/mstark.h: S_ADDR holds the sorting permutation and is overwritten by the
        # addresses read through it - run twice it gives another witness
        n = 64
        s = memory_lab(pkg, fe, ctx)
        rng = np.random.default_rng(3104)
        log = np.stack([rng.integers(0, n // 4, size=n, dtype=np.uint64), rng.integers(0, P, size=n, dtype=np.uint64),
                        np.zeros(n, dtype=np.uint64), rng.integers(0, P, size=n, dtype=np.uint64)], axis=1)
        log = am.run(log, [ADDR], S_ADDR)
        prog = fe.compile_fill(4, 0, 0, [(S_VAL, E.main_at(VAL, E.main(S_ADDR))), (S_ADDR, E.main_at(ADDR, E.main(S_ADDR)))])
        once_run = gm.run(prog.blob, log)
        assert not np.array_equal(gm.run(prog.blob, once_run), once_run)  # not idempotent
        out["indexed_overwrite"] = (s, [log], fe.pack_claims([]), 0, prog, None, None, FILL_ALWAYS)
        # all nine allocations: inputs, a non-additive scan over two tiles whose coefficient pass has 300 live leaves
        n = 2 * T
        s = scan_lab(pkg, fe, ctx)
        leaves = [fe.bits(x + k, k % 57, 1 + k // 57) for k in range(300)]
        add = leaves[-1]
        for leaf in reversed(leaves[:-1]):  # every leaf is live before the first is consumed
            add = leaf - add
        prog = fe.compile_fill(2, 0, 3, [(0, m), (1, fe.scan(E.main(0), add, init=5))])
        assert pkg.fill_program_info(prog)["lds_lanes"] == 0 and pkg.fill_scan_info(prog)[:3] == (1, 2, 0)
        rng = np.random.default_rng(3105)
        start = [rng.integers(0, P, size=(n, 2), dtype=np.uint64) for _ in range(2)]
        out["all_nine"] = (s, start, fe.pack_claims([]), 1, prog, ts.operands(rng, n, 3, T), None,
                           FILL_ALWAYS + FILL_SCRATCH + FILL_SCAN + FILL_TILES + FILL_INPUTS)
        assert out["all_nine"][-1] == 9
        return out

    return once("fill programs", make)


@pytest.mark.parametrize("route", ["device", "held"])
@pytest.mark.parametrize("name", ["u32_add", "groups_and_scans", "global_scratch", "indexed_overwrite", "all_nine"])
def test_fill(pkg, fe, actx, oracle, name, route):
    s, start, packed, ci, prog, inputs, pre, at_least = fill_programs(pkg, fe, actx)[name]
    want = once(("fill model", name), lambda: [gm.run(prog.blob, t, pre, inputs) if c == ci else t for c, t in enumerate(start)])
    d_inputs = None if inputs is None else dev(inputs)

    def report(rep):
        assert rep.fields()[:2] == (start[ci].shape[0], len(prog.steps)), str(rep)

    mutate_case(pkg, oracle, actx, "fill %s %s" % (name, route), s, start, packed, route, lambda w: w.fill(ci, prog, d_inputs), want, at_least, after=report)


# msbb_witness_fill, the same driver (fl_witness_fill in csrc/fill_dev.h with BbFill of csrc/bb_fill.hip): d_code, d_outs and d_consts,
# scratch in the global-scratch form, inp and bad with inputs - all before the first launch; a witness of this configuration holds
# no lookup values
@pytest.mark.parametrize("name", ["u32_halves", "global_scratch"])
def test_bb_fill(pkg, actx, name):
    import oracle_bb as ob
    import test_gpu_bb_witness_fill as tb
    from test_bb_fill_model import halves
    from test_bb_multiplicity_model import bb, cases, compiled_of, fe as bfe, pack

    if name == "u32_halves":  # the U32Add program over the 16-bit halves at 16 rows, slots in LDS, on junk traces
        inputs, traces, claims, _ = cases()["u32_16"]
        blob, comp, osys = compiled_of(inputs)
        s = once("bb dm system", lambda: bb.System(actx, blob, len(comp)))
        with bfe.field(bfe.BABYBEAR):
            prog = bfe.u32_add_halves_fill_program(16)
        rng = np.random.default_rng(3111)
        start = [tb.rand_field(rng, np.asarray(t).shape) for t in traces]
        ci, pre, packed = 1, None, pack(claims)
        operands = halves(*bfe.xorshift_pairs(16)).astype(np.uint16)
        assert bb.fill_program_info(prog)["lds_lanes"] != 0
        at_least = FILL_ALWAYS + FILL_INPUTS
    else:  # 300 live leaves on the lab system of test_gpu_bb_witness_fill
        with own_cache(tb):
            s, pres = once("bb fill lab", lambda: tb.lab_system(actx))
        osys = ob.System(s.blob)
        ci = tb.HEIGHTS.index(512)
        prog = tb.chain_program(300)
        assert bb.fill_program_info(prog)["lds_lanes"] == 0
        rng = np.random.default_rng(3112)
        start = [np.zeros((0, w), dtype=np.uint64) for w in (6, 6, 6, 3, 4)]
        start[ci], start[tb.BYSTANDER] = tb.rand_field(rng, (512, 6)), tb.rand_field(rng, (8, 3))
        pre, packed = pres[ci], pack(tb.CLAIMS)
        operands = tb.rand_field(rng, (512, 3)).astype(np.uint32)
        at_least = FILL_ALWAYS + FILL_SCRATCH + FILL_INPUTS
    want = [gm.run(prog.blob, t, pre, operands.astype(np.uint64)) if c == ci else t for c, t in enumerate(start)]
    proofs = [osys.prove(t, packed) for t in (start, want)]
    w = s.witness_from_device([tb.dev32(t) if len(t) else None for t in start], packed)
    d_operands = dev(operands)

    def unchanged(state, when):
        for c, t in enumerate((start, want)[state]):
            assert tb.same(w.trace(c), np.asarray(t)), "trace differs %s: circuit %d" % (when, c)
        assert s.prove_multiple_claims(w).to_bytes() == proofs[state], "proof differs %s" % when

    unchanged(0, "before the first call")
    sweep(pkg, actx, "bb fill %s" % name, lambda: w.fill(ci, prog, d_operands), lambda nth: unchanged(0, "after a failed call (allocation %d)" % nth),
          lambda rep: unchanged(1, "after the successful call"), at_least)


# ---------------------------------------------------------------- b. ms_witness_argsort
# The device allocations of witness_argsort, csrc/argsort.hip: keys_a (l. 254), slots and d_hist (l. 255) before the call's host
# wait (l. 262); keys_b (l. 278), idx_a and idx_b (l. 279) and counts (l. 280) after it, and only when some digit pass runs. The
# first write to the trace is the last launch but one (as_final_k, l. 299).
SORT_BEFORE_WAIT, SORT_AFTER_WAIT = 3, 4


@pytest.mark.parametrize("route", ["device", "held"])
@pytest.mark.parametrize("keys", ["random", "two_rank", "constant"])
@pytest.mark.parametrize("tiles", [1, 2])
def test_argsort(pkg, fe, actx, oracle, tiles, keys, route):
    from test_gpu_witness_argsort import ADDR, S_ADDR, S_VAL, VAL

    n = tiles * pkg.sort_info()[0]
    s = memory_lab(pkg, fe, actx)

    def make():
        rng = np.random.default_rng(3200 + n)
        t = rng.integers(0, P, size=(n, 4), dtype=np.uint64)
        if keys == "two_rank":
            t[:, ADDR] = np.array([3, P - 1, 1 << 63, 1 << 32], dtype=np.uint64)[rng.integers(0, 4, size=n)]
        if keys == "constant":
            t[:, ADDR] = 0x0123456789ABCDEF
        args = {"random": ([VAL], S_ADDR, False), "two_rank": ([ADDR, VAL], S_VAL, True), "constant": ([ADDR], S_ADDR, False)}[keys]
        return t, args, am.run(t, *args), am.passes(t, args[0])

    t, (cols, dst, rank), want, (passes, skipped) = once(("argsort", n, keys), make)
    assert {"random": passes == 8, "two_rank": passes > 8, "constant": passes == 0}[keys]
    at_least = SORT_BEFORE_WAIT + (SORT_AFTER_WAIT if passes else 0)

    def report(rep):
        assert rep.fields() == (n, len(cols), passes, skipped), str(rep)

    mutate_case(pkg, oracle, actx, "argsort %d rows %s %s" % (n, keys, route), s, [t], fe.pack_claims([]), route,
                lambda w: w.argsort(0, cols, dst, rank=rank), [want], at_least, after=report)


# ---------------------------------------------------------------- c. derive_multiplicities, both fields
# The device allocations of witness_derive_multiplicities, one driver for both fields (dm_derive, csrc/multiplicity_dev.h):
# table (l. 226, in LbRun::alloc_table, csrc/lb_dev.h, l. 367), slot_of (l. 227), rep, marks, wg_prefix, wg_counts and d_srcs
# (l. 228, in LbRun::alloc_rest, csrc/lb_dev.h, l. 372-376), d_tg (l. 229) and, with room for entries, d_entries and d_args
# (l. 237-238) - all before dm_zero_k, the first write to the witness. In front of them GlLookup::sources (csrc/gl_lb.h,
# l. 108-109) takes two temporaries per circuit with lookups whose values the witness does not hold, and BbLookup::sources
# (csrc/bb_lb.h, l. 104-108) takes three per circuit with lookups.
DM_OWN, DM_ENTRIES, DM_PER_CIRCUIT_GL, DM_PER_CIRCUIT_BB = 8, 2, 2, 3


def dm_cases(fe, oracle):
    """name -> (circuit inputs, traces before, claims, targets): the garbage-columns witness of the 16-addition case and the
    case with one byte message that no table row serves"""
    from test_gpu_derive_multiplicities import unserved_case
    from test_multiplicity_model import cases, garbage, system_of

    def make():
        inputs, traces, claims, targets = cases(fe)["u32_16"]
        _, comp = system_of(oracle, fe, inputs)
        return {"balanced": (inputs, garbage(traces, comp, targets), claims, targets), "unserved": unserved_case(fe)}

    return once("dm cases", make)


@pytest.mark.parametrize("route", ["device", "held"])
@pytest.mark.parametrize("name", ["balanced", "unserved"])
def test_derive_multiplicities(pkg, fe, actx, oracle, name, route):
    from test_multiplicity_model import system_of

    inputs, traces, claims, targets = dm_cases(fe, oracle)[name]
    s = once("dm system", lambda: pkg.System.new(actx, fe.test_params(), inputs))
    osys, comp = system_of(oracle, fe, inputs)
    packed = fe.pack_claims(claims)
    want, m = once(("dm model", name), lambda: mm.derive(osys, comp, traces, packed, targets, 64))
    assert (m.unserved > 0) == (name == "unserved") and (name == "balanced" or len(m.entries) == 1)

    def success(rep):
        assert rep.fields() == m.fields() and rep.ok == m.ok, str(rep)

    at_least = DM_OWN + DM_ENTRIES + (2 * DM_PER_CIRCUIT_GL if route == "device" else 0)
    mutate_case(pkg, oracle, actx, "derive_multiplicities %s %s" % (name, route), s, traces, packed, route,
                lambda w: w.derive_multiplicities(targets, entries=64), want, at_least, after=success)


@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("name", ["balanced", "unserved"])
def test_bb_derive_multiplicities(pkg, actx, name, route):
    from test_bb_multiplicity_model import bb, cases, compiled_of, garbage, pack
    from test_gpu_bb_derive_multiplicities import same, unserved_case, upload

    if name == "balanced":
        inputs, traces, claims, targets = cases()["u32_16"]
        traces = once("bb dm garbage", lambda: garbage(traces, compiled_of(inputs)[1], targets))
    else:
        inputs, traces, claims, targets = once("bb dm unserved", unserved_case)
    blob, comp, osys = compiled_of(inputs)
    s = once("bb dm system", lambda: bb.System(actx, blob, len(comp)))
    packed = pack(claims)
    want, m = once(("bb dm model", name), lambda: mmb.derive(osys, comp, traces, packed, targets, 64))
    assert (m.unserved > 0) == (name == "unserved")
    proofs = once(("bb dm proofs", name), lambda: [osys.prove(t, packed) for t in (traces, want)])
    w = upload(s, traces, packed, route)

    def unchanged(state, when):
        for c, t in enumerate((traces, want)[state]):
            assert same(w.trace(c), t), "trace %d differs %s" % (c, when)
        assert s.prove_multiple_claims(w).to_bytes() == proofs[state], "proof differs %s" % when

    def success(rep):
        assert rep.fields() == m.fields() and rep.ok == m.ok, str(rep)
        unchanged(1, "after the successful call")

    unchanged(0, "before the first call")
    sweep(pkg, actx, "bb derive_multiplicities %s %s" % (name, route), lambda: w.derive_multiplicities(targets, entries=64),
          lambda nth: unchanged(0, "after a failed call (allocation %d)" % nth), success, DM_OWN + DM_ENTRIES + 2 * DM_PER_CIRCUIT_BB)


# ---------------------------------------------------------------- d. witness_check, both fields, on systems made for the test
# The device allocations of witness_check. csrc/check.hip: publics (l. 81), acc (l. 82), the counters of CkCounters
# (csrc/check_dev.h, l. 263) and one stage-2 trace per active circuit (l. 91). csrc/bb_check.hip: the same three (l. 110-112),
# and on a circuit's first check check_program builds and keeps its program, whose Montgomery constants are one allocation
# (l. 82) behind those of build_program; it publishes the program last (l. 85-86).
CHECK_OWN, CHECK_PER_CIRCUIT, CHECK_BB_FIRST_BUILD = 3, 1, 1


def same_check(rep, m, ext4=False):
    assert rep.verdict == m.verdict and rep.ok == m.ok, (rep.verdict, m.verdict, str(rep))
    assert not ext4 or rep.final_accumulator == m.final_accumulator
    for i, (d, c) in enumerate(zip(rep.circuits, m.circuits)):
        assert d.fields() == c.fields(), ("circuit %d" % i, d.fields(), c.fields())


@pytest.mark.parametrize("witness", ["clean", "failing_row"])
def test_witness_check(pkg, fe, actx, oracle, witness):
    from test_gpu_witness_check import BG, Sys

    traces, claims = fe.u32_add_bench_witness(16)
    traces, claims = [t.copy() for t in traces], [list(c) for c in claims]
    if witness == "failing_row":
        traces[1][5, 8] = (int(traces[1][5, 8]) + 1) % 256  # a byte of the sum: the row's constraint and a byte message
    s = Sys(pkg, fe, actx, oracle, fe.u32_add_system_inputs())  # a system of its own: nothing has been checked with it
    m = s.model(traces, claims)
    assert (m.verdict == 0) == (witness == "clean")
    w = s.dev.witness(traces, fe.pack_claims(claims))

    def unchanged():
        assert all(np.array_equal(w.trace(ci), t) for ci, t in enumerate(traces))

    def failed(nth):
        same_check(w.check(*BG), m)
        unchanged()

    sweep(pkg, actx, "witness_check %s" % witness, lambda: w.check(*BG), failed, lambda rep: (same_check(rep, m), unchanged()),
          CHECK_OWN + 2 * CHECK_PER_CIRCUIT)


@pytest.mark.parametrize("witness", ["clean", "failing_row"])
def test_bb_witness_check(pkg, actx, witness):
    from test_bb_witness_check_model import bb_traces
    from test_gpu_bb_derive_multiplicities import same
    from test_gpu_bb_witness_check import BG, Sys, bb_inputs

    traces, claims = [np.array(t, dtype=np.uint64) for t in bb_traces("even_odd")], [[0, 4, 1]]
    if witness == "failing_row":
        traces[0][1, 1] = (int(traces[0][1, 1]) + 1) % mmb.P  # a failing row of circuit 0, and its message off balance
    assert mmb.P == 2013265921
    inputs = bb_inputs("even_odd_inputs")
    model = Sys(actx, inputs)
    m = model.model(traces, claims)
    assert (m.verdict == 0) == (witness == "clean")
    from test_bb_witness_check_model import pack

    def fresh():
        """a system nothing has been checked with: its first check builds the programs of both circuits"""
        s = Sys(actx, inputs)
        return s, s.dev.witness(traces, pack(claims))

    # every allocation point of the first check, each on a system of its own: a failure during the build leaves no program
    # behind that the unarmed check would then run
    state = {}

    def renew():
        state["s"], state["w"] = fresh()

    def unchanged():
        assert all(same(state["w"].trace(ci), t) for ci, t in enumerate(traces))

    def failed(nth):
        same_check(state["w"].check(*BG), m, ext4=True)
        unchanged()

    sweep(pkg, actx, "bb witness_check %s, first check" % witness, lambda: state["w"].check(*BG), failed,
          lambda rep: (same_check(rep, m, ext4=True), unchanged()), CHECK_OWN + 2 * CHECK_PER_CIRCUIT + 2 * CHECK_BB_FIRST_BUILD, before=renew)
    # and every point of a later check, the programs being there
    sweep(pkg, actx, "bb witness_check %s, later check" % witness, lambda: state["w"].check(*BG), failed,
          lambda rep: (same_check(rep, m, ext4=True), unchanged()), CHECK_OWN + 2 * CHECK_PER_CIRCUIT)


# ---------------------------------------------------------------- e. lookup_balance, both fields
# The device allocations of witness_lookup_balance, one driver for both fields (lb_balance, csrc/balance_dev.h): table (l. 93, in
# LbRun::alloc_table, csrc/lb_dev.h, l. 367), rep, marks, wg_prefix, wg_counts and d_srcs (l. 94, in LbRun::alloc_rest,
# csrc/lb_dev.h, l. 372-376) and, behind the first host wait and only when some group is unbalanced and there is room for
# entries, d_entries and d_args (l. 113-114); the field's sources in front, as for (c).
LB_OWN, LB_ENTRIES = 6, 2


@pytest.mark.parametrize("route", ["device", "held"])
@pytest.mark.parametrize("name", ["even_odd_wrong_claim", "u32_one_cell"])
def test_lookup_balance(pkg, fe, actx, oracle, name, route):
    import importlib

    from test_lookup_balance_model import cases, model_of

    b3 = importlib.import_module("multi_stark_amd.blake3_circuit")
    inputs, traces, claims, balanced = cases(fe, b3)[name]
    m, osys, comp = model_of(oracle, fe, b3, name, 64)
    assert not balanced and m.unbalanced > 0
    s = once(("lb system", id(inputs)), lambda: pkg.System(actx, fe.system_blob(fe.test_params(), comp), len(comp)))
    w = gl_witness(s, osys, traces, fe.pack_claims(claims), route)

    def same_report(rep):
        assert rep.fields() == m.fields() and not rep.ok, str(rep)
        assert all(np.array_equal(w.trace(ci), np.asarray(t, dtype=np.uint64)) for ci, t in enumerate(traces))

    sweep(pkg, actx, "lookup_balance %s %s" % (name, route), lambda: w.lookup_balance(entries=64), lambda nth: same_report(w.lookup_balance(entries=64)),
          same_report, LB_OWN + LB_ENTRIES + (len(inputs) * DM_PER_CIRCUIT_GL if route == "device" else 0))


@pytest.mark.parametrize("name", ["even_odd_wrong_claim", "u32_one_cell"])
def test_bb_lookup_balance(pkg, actx, name):
    from test_bb_lookup_balance_model import bb, cases, compiled_of, model_of, pack
    from test_gpu_bb_derive_multiplicities import same

    inputs, traces, claims, balanced = cases()[name]
    blob, comp, _ = compiled_of(name)
    m = model_of(name, 64)
    assert not balanced and m.unbalanced > 0
    s = once(("bb lb system", id(inputs)), lambda: bb.System(actx, blob, len(comp)))
    w = s.witness(traces, pack(claims))

    def same_report(rep):
        assert rep.fields() == m.fields() and not rep.ok, str(rep)
        assert all(same(w.trace(ci), np.asarray(t)) for ci, t in enumerate(traces))

    sweep(pkg, actx, "bb lookup_balance %s" % name, lambda: w.lookup_balance(entries=64), lambda nth: same_report(w.lookup_balance(entries=64)),
          same_report, LB_OWN + LB_ENTRIES + len(inputs) * DM_PER_CIRCUIT_BB)


# ---------------------------------------------------------------- f. the calls that make a witness
def create_case(pkg, ctx, label, make, check, at_least):
    """a failed call yields no witness (it raises); the unarmed repeat yields one that `check` accepts"""
    sweep(pkg, ctx, label, make, lambda nth: check(make(), nth == 1), lambda w: check(w, True), at_least)


def u32_16(pkg, fe, ctx, oracle):
    """(system, traces, packed claims, the oracle's proof) of the 16-addition witness, once"""
    def make():
        from test_multiplicity_model import cases

        inputs, traces, claims, _ = cases(fe)["u32_16"]
        s = pkg.System.new(ctx, fe.test_params(), inputs)
        packed = fe.pack_claims(claims)
        return s, [np.asarray(t, dtype=np.uint64) for t in traces], packed, oracle.System(s.blob).prove(traces, packed)

    return once("u32_16", make)


def gl_created(s, traces, proof):
    def check(w, prove):
        assert all(np.array_equal(w.trace(ci), t) for ci, t in enumerate(traces))
        assert not prove or s.prove_multiple_claims(w).to_bytes() == proof  # (after the first failure and after the success)

    return check


# ms_witness_create on the two-circuit system, csrc/prover.hip: per circuit its trace (l. 584) and arg_offsets (l. 593) - and
# mult and args (l. 598-599) where the values are materialised -, then the claims' offsets and data (l. 626-627)
CREATE_PER_CIRCUIT, CREATE_CLAIMS = 2, 2


def test_system_witness(pkg, fe, actx, oracle):
    s, traces, packed, proof = u32_16(pkg, fe, actx, oracle)
    create_case(pkg, actx, "system.witness", lambda: s.witness(traces, packed), gl_created(s, traces, proof), 2 * CREATE_PER_CIRCUIT + CREATE_CLAIMS)


# ms_witness_create_device, csrc/prover.hip: bad (l. 514), one trace per circuit (l. 519), d_offs (l. 522) and d_data (l. 528),
# then witness_from_device: arg_offsets per circuit with lookups (l. 440) - and mult and args (l. 451-452) where materialised
CREATE_DEVICE_OWN = 3


@pytest.mark.parametrize("kind,form", [("row", "vec"), ("col", "tiled"), ("colslice", "plain")])
def test_witness_from_device(pkg, fe, actx, oracle, kind, form):
    from test_gpu_bb_device_witness import bb_layout, form_of_view

    s, traces, packed, proof = u32_16(pkg, fe, actx, oracle)
    views = [bb_layout(dev(t), kind) for t in traces]
    # (the Goldilocks witness is row-major: launch() of csrc/ingest.hip takes the rows as S and the columns as F, which is the
    # restated dispatch on the transposed view)
    assert form_of_view(views[1].t())[0] == form
    clones = [v.clone() for v in views]
    check = gl_created(s, traces, proof)

    def checked(w, prove):
        check(w, prove)
        assert all(bool((v == c).all()) for v, c in zip(views, clones)), "the caller's tensor was changed"

    def make():
        try:
            return s.witness_from_device(views, packed)
        except pkg.MstarkError:
            assert all(bool((v == c).all()) for v, c in zip(views, clones)), "the caller's tensor was changed by a failed call"
            raise

    create_case(pkg, actx, "witness_from_device %s" % form, make, checked, CREATE_DEVICE_OWN + 2 + 2)


# msbb_witness_create_device, csrc/bb_prover.hip: bad (l. 258), one trace per circuit, the claims' offsets and data (l. 195-196)
@pytest.mark.parametrize("kind,form", [("col", "vec"), ("row", "tiled"), ("col_pitch3", "plain")])
def test_bb_witness_from_device(pkg, actx, kind, form):
    from test_bb_multiplicity_model import bb, cases, compiled_of, pack
    from test_gpu_bb_derive_multiplicities import same
    from test_gpu_bb_device_witness import bb_layout, form_of_view

    inputs, traces, claims, _ = cases()["u32_16"]
    blob, comp, osys = compiled_of(inputs)
    s = once("bb dm system", lambda: bb.System(actx, blob, len(comp)))
    packed = pack(claims)
    proof = once("bb u32_16 proof", lambda: osys.prove(traces, packed))
    views = [bb_layout(dev(np.asarray(t).astype(np.uint32)), kind) for t in traces]
    assert form_of_view(views[1])[0] == form
    clones = [v.clone() for v in views]

    def checked(w, prove):
        assert all(same(w.trace(ci), t) for ci, t in enumerate(traces))
        assert not prove or s.prove_multiple_claims(w).to_bytes() == proof
        assert all(bool((v == c).all()) for v, c in zip(views, clones)), "the caller's tensor was changed"

    def make():
        try:
            return s.witness_from_device(views, packed)
        except pkg.MstarkError:
            assert all(bool((v == c).all()) for v, c in zip(views, clones)), "the caller's tensor was changed by a failed call"
            raise

    create_case(pkg, actx, "bb witness_from_device %s" % form, make, checked, 1 + 2 + 2)


# ms_witness_u32_add_bench, csrc/witness_gen.hip: d_jump (l. 109), the two traces (l. 112-113), d_offs and d_data (l. 114), then
# witness_from_device: arg_offsets per circuit (csrc/prover.hip, l. 440)
def test_bench_witness_on_device(pkg, fe, actx, oracle):
    n = 1000
    s = once("bench system", lambda: pkg.System.new(actx, fe.test_params(), fe.u32_add_system_inputs()))
    traces, claims = fe.u32_add_bench_witness(n)
    packed = fe.pack_claims(claims)
    proof = oracle.System(s.blob).prove(traces, packed)
    create_case(pkg, actx, "bench_witness_on_device", lambda: s.bench_witness_on_device(n), gl_created(s, traces, proof), 5 + 2)


# ms_witness_blake3_compressions, csrc/witness_gen.hip: nine traces (l. 482), the compression circuit's lookup values (l. 484-485),
# d_in, d_out and d_scratch (l. 486), d_offs and d_data (l. 487), then arg_offsets per circuit with lookups
def test_blake3_witness_on_device(pkg, fe, actx, oracle):
    import importlib

    from test_gpu_blake3_witness import _case, _check_traces

    b3 = importlib.import_module("multi_stark_amd.blake3_circuit")
    states, claims, traces, packed = _case(b3, fe, "n3_129_bytes")
    comp = [fe.compile_circuit(ci) for ci in b3.blake3_system_inputs()]
    s = pkg.System(actx, fe.system_blob(fe.test_params(), comp), 9)
    s.params = fe.test_params()
    proof = oracle.System(s.blob).prove(traces, packed)
    with_lookups = sum(1 for ci in range(9) if s.circuit_info(ci)["num_lookups"])

    def check(w, prove):
        _check_traces(w, traces)
        assert np.array_equal(w.states_out, np.array([c[33:] for c in claims], dtype=np.uint32))
        assert not prove or s.prove_multiple_claims(w).to_bytes() == proof

    create_case(pkg, actx, "blake3_witness_on_device", lambda: s.blake3_witness_on_device(states), check, 16 + with_lookups)


# ---------------------------------------------------------------- g. verify_batch, both fields
# One device allocation: the batch's staged bytes (csrc/verify_batch.h, l. 219), shared by both fields' collectors.
def test_verify_batch(pkg, fe, actx, oracle):
    from test_gpu_verify_batch import _field_tampers

    s, traces, packed, proof = u32_16(pkg, fe, actx, oracle)
    o = oracle.System(s.blob)
    tampers = _field_tampers(proof, 0)
    items = [(packed, proof), (packed, tampers["lowest input sibling[q0]"]), (packed, tampers["input value, round 0[q0]"])]
    want = [o.verify(c, p) for c, p in items]
    assert want[0] == 0 and want[1] != 0 and want[2] != 0

    def same_verdicts(got):
        assert got == want and got == [s.verify(c, p) for c, p in items]

    sweep(pkg, actx, "verify_batch", lambda: s.verify_batch(items), lambda nth: same_verdicts(s.verify_batch(items)), same_verdicts, 1)


def test_bb_verify_batch(pkg, actx):
    from test_bb_multiplicity_model import bb, cases, compiled_of, pack
    from test_gpu_bb_verify_batch import _query_tampers

    inputs, traces, claims, _ = cases()["u32_16"]
    blob, comp, o = compiled_of(inputs)
    s = once("bb dm system", lambda: bb.System(actx, blob, len(comp)))
    packed = pack(claims)
    proof = once("bb u32_16 proof", lambda: o.prove(traces, packed))
    tampers = _query_tampers(proof, 0)
    items = [(packed, proof), (packed, tampers["lowest input path digest [query 0]"]), (packed, tampers["opened input row value, round 0 [query 0]"])]
    accept = [o.verify(c, p) == 0 for c, p in items]
    assert accept == [True, False, False]

    def same_verdicts(got):
        assert [v == 0 for v in got] == accept and got == [s.verify(c, p) for c, p in items]

    sweep(pkg, actx, "bb verify_batch", lambda: s.verify_batch(items), lambda nth: same_verdicts(s.verify_batch(items)), same_verdicts, 1)
