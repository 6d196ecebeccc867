"""`-m gpu`: two host threads, each with its own Context(0), systems and witnesses, on ONE device at the same time - the mode of
INTEGRATION.md "Two proofs in flight", for both configurations and for the entry points no other test runs concurrently.
Contexts of one device share process-wide state: the BabyBear twiddle tables, the hiprtc code objects and their disk cache,
the pack pool of the narrow upload, the page-lock counts of caller memory, the thread-local error text. Every expected value
comes from where the single-context tests take theirs (the oracles, the models, the Python witness builder), computed once
before the threads start; a serial run of the library is never the reference. ctypes releases the GIL inside a call, so the
two threads are inside the library together. A worker that fails aborts the barrier: the other stops at its next step."""
import importlib
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest
import torch  # noqa: F401  (before the library opens the device, as the modules imported below do)

import lookup_balance_model as lm
import oracle_bb as ob
import witness_check_model as wm
import witness_check_model_bb as wmb
from __graft_entry__ import load_package
from conftest import rand_field
from test_bb_lookup_balance_model import cases as bb_cases, compiled_of as bb_compiled_of, model_of as bb_model_of
from test_bb_witness_check_model import BG as BB_BG, K, compile_system as bb_compile_system, pack as bb_pack
from test_gpu_bb_verify_batch import _query_tampers
from test_gpu_blake3_witness import _case as b3_case, _check_traces
from test_gpu_derive_multiplicities import unserved_case
from test_gpu_verify_batch import _field_tampers
from test_multiplicity_model import cases as mult_cases, garbage, model_of as mult_model_of, system_of
from test_witness_check_model import BG

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = load_package()
fe = pkg.frontend
bb = pkg.babybear
JOIN_S = 120  # no step below takes a second; a worker still alive after this long is reported as hung


def run_threads(bodies):
    """one thread per body(barrier); every exception of a worker is collected, the first real one is raised here"""
    barrier = threading.Barrier(len(bodies))
    errors = []

    def worker(i):
        try:
            bodies[i](barrier)
        except BaseException as e:  # noqa: BLE001
            errors.append((i, e))
            barrier.abort()  # the other worker stops at its next barrier: nothing goes on using the GPU after a failure

    threads = [threading.Thread(target=worker, args=(i,), daemon=True) for i in range(len(bodies))]
    for t in threads:
        t.start()
    deadline = time.monotonic() + JOIN_S
    for t in threads:
        t.join(timeout=max(0.0, deadline - time.monotonic()))
    real = [(i, e) for i, e in errors if not isinstance(e, threading.BrokenBarrierError)]
    for i, e in (real or errors)[1:]:
        print("thread %d also raised %r" % (i, e))
    if real or errors:
        raise (real or errors)[0][1]
    assert not any(t.is_alive() for t in threads), "a worker thread did not finish within %d s" % JOIN_S


def wait(barrier):
    barrier.wait(timeout=JOIN_S)


def same_check(rep, m, final=False):
    """a device CheckReport against the model's, field by field (Sys.both of test_gpu_witness_check.py / test_gpu_bb_witness_check.py)"""
    assert rep.verdict == m.verdict, (rep.verdict, m.verdict, str(rep))
    assert rep.ok == m.ok and len(rep.circuits) == len(m.circuits)
    if final:
        assert rep.final_accumulator == m.final_accumulator
    for i, (d, c) in enumerate(zip(rep.circuits, m.circuits)):
        assert d.fields() == c.fields(), ("circuit %d" % i, d.fields(), c.fields())


# ---------------------------------------------------------------- a) cold BabyBear twiddle tables, in a fresh process
# The child computes the oracle's values itself (tests/oracle_bb.py), before its threads start, and reads nothing outside the
# repository. One trial per height, the largest first: the trial at height h is the first use of the 2^h table in the process
# (the one before it made 2^(h+1) and 2^(h+2)), and that is the table thread A's first LDE creates right behind its trace copies.
COLD_SCRIPT = r"""
import ctypes as C, os, sys, threading, time
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import oracle_bb as ob
from __graft_entry__ import load_package
pkg = load_package(); fe = pkg.frontend; bb = pkg.babybear
P = fe.BABYBEAR["P"]
K = fe.poseidon2_constants()
ob.set_poseidon2(K)
sys.setswitchinterval(2e-5)  # thread B's busy-wait must not keep the interpreter lock from thread A for the default 5 ms
TRIAL_S = 6  # (a trial takes some tens of milliseconds; the parent's limit on the whole child is shorter than two of these)
STAGGER_US = {14: 0, 15: 50, 16: 100, 17: 200, 18: 400, 19: 800}
ctx_a, ctx_b = pkg.Context(0), pkg.Context(0)
with fe.field(fe.BABYBEAR):
    system = bb.System.new(ctx_a, fe.test_params(), fe.mul_air_inputs(), K)
    packed = fe.pack_claims([])
oracle_system = ob.System(system.blob)
wrong = []


def dft(ctx, m):
    # bb.dft_batch without its range check of the input: the stagger below is the only delay behind the barrier
    out = np.empty_like(m)
    if pkg.lib().msbb_dft_batch(ctx.h, m.ctypes.data_as(bb.u32p), C.c_size_t(m.shape[0]), C.c_size_t(1), C.c_int32(0), out.ctypes.data_as(bb.u32p)) != 0:
        raise RuntimeError(pkg.lib().ms_last_error().decode())
    return out


for log_h in (19, 18, 17, 16, 15, 14):
    with fe.field(fe.BABYBEAR):
        trace = fe.mul_air_trace(1 << log_h)
    rng = np.random.default_rng(log_h)
    mats = [rng.integers(0, P, (1 << (log_h + k), 1), dtype=np.uint64) for k in (0, 1)]
    want_proof = oracle_system.prove([trace], packed)
    want_dft = [ob.dft_batch(m) for m in mats]
    mats = [m.astype(np.uint32) for m in mats]  # as msbb_dft_batch takes them: nothing is converted behind the barrier
    hw = system.host_witness([trace], packed)
    if not hw.pinned:
        raise SystemExit("the host buffers could not be page-locked: the asynchronous trace copies this test is about do not happen")
    for phase in ("cold", "warm"):
        barrier, errors, got = threading.Barrier(2), [], {}

        def guarded(body):
            def run():
                try:
                    body()
                except BaseException as e:
                    errors.append(e)
                    barrier.abort()
            return run

        def prover():
            barrier.wait(timeout=TRIAL_S)
            got["proof"] = system.prove_multiple_claims(hw).to_bytes()

        def transforms():
            barrier.wait(timeout=TRIAL_S)
            until = time.perf_counter() + STAGGER_US[log_h] * 1e-6
            while time.perf_counter() < until:
                pass
            got["dft"] = [dft(ctx_b, m) for m in mats]

        threads = [threading.Thread(target=guarded(f), daemon=True) for f in (prover, transforms)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=TRIAL_S)
        if errors:
            raise errors[0]
        if any(t.is_alive() for t in threads):
            raise SystemExit("height 2^%d, %s: a thread did not finish" % (log_h, phase))
        sides = []
        if got["proof"] != want_proof:
            sides.append("proof (thread A)")
        for k in (0, 1):
            if not np.array_equal(got["dft"][k], want_dft[k]):
                sides.append("transform of 2^%d rows (thread B)" % (log_h + k))
        print("TRIAL log_h=%d %s stagger=%dus: %s" % (log_h, phase, STAGGER_US[log_h], "; ".join(sides) or "both equal the oracle's"), flush=True)
        if sides:
            wrong.append((log_h, phase, sides))
    del hw
if wrong:
    raise SystemExit("differs from the oracle: %r" % (wrong,))
print("COLD-OK", flush=True)
"""


def test_cold_twiddle_tables_created_while_another_context_transforms():
    """Regression test of the twiddle cache (csrc/bb_kernels.hip twiddles()): a table used to be published with its fill still
    queued on the creating context's stream, behind that context's asynchronous trace copies, and a transform of another
    context could read it unwritten. Six heights, each the first use of its table size in the child process; per height thread
    A proves the MulAir from a pinned host-resident witness while thread B, staggered by 0 .. 800 us, transforms 2^h and
    2^(h+1) rows on its own context; then the same again with the tables warm. Everything must equal the oracle's.
    A guard of the ordering, not a reproduction: one run on the code before the fix passed at all six heights as well."""
    # the whole child on the MI355X box, the quotient kernel's hiprtc compilation included: 4.2 s (the slowest run seen); times three
    r = subprocess.run([sys.executable, "-c", COLD_SCRIPT, ROOT], capture_output=True, text=True, timeout=13)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "COLD-OK" in r.stdout and r.stdout.count("TRIAL") == 12, (r.returncode, r.stdout[-3000:], r.stderr[-4000:])


# ---------------------------------------------------------------- b) mixed work, both fields, warm process
class Expected:
    """inputs and expected results of every step of the mixed run: oracles and models on the CPU, once"""

    def __init__(self, oracle):
        b3 = importlib.import_module("multi_stark_amd.blake3_circuit")
        ob.set_poseidon2(K)
        # --- Goldilocks: [ByteTable, U32Add] at 2^10 additions under the bench parameters
        self.u32_inputs = fe.u32_add_system_inputs()
        comp = [fe.compile_circuit(ci) for ci in self.u32_inputs]
        self.gl_blob = fe.system_blob(fe.bench_params(), comp)
        osys = oracle.System(self.gl_blob)
        self.gl_traces, claims = fe.u32_add_bench_witness(1 << 10)
        self.gl_packed = fe.pack_claims(claims)
        self.gl_proof = osys.prove(self.gl_traces, self.gl_packed)
        assert osys.verify(self.gl_packed, self.gl_proof) == 0
        bad = _field_tampers(self.gl_proof, 1)["lowest input sibling[q1]"]
        self.gl_items = [(self.gl_packed, p) for p in (self.gl_proof, bad, self.gl_proof, self.gl_proof)]
        self.gl_verdicts = [osys.verify(c, p) for c, p in self.gl_items]
        assert self.gl_verdicts == [0, 2, 0, 0]
        self.gl_check = wm.check(oracle, osys, comp, self.gl_traces, self.gl_packed, *BG)
        assert self.gl_check.verdict == 0
        # --- the unbalanced 16-addition witness, and u32_128 with garbage in the multiplicity column (test parameters)
        inputs, traces, claims, self.targets = unserved_case(fe)
        osys_t, comp_t = system_of(oracle, fe, inputs)
        self.test_blob = fe.system_blob(fe.test_params(), comp_t)
        self.unserved_traces, self.unserved_packed = traces, fe.pack_claims(claims)
        self.unserved_balance = lm.balance(osys_t, comp_t, traces, self.unserved_packed, 64)
        assert self.unserved_balance.unbalanced > 0
        inputs128, self.traces128, claims128, targets128 = mult_cases(fe)["u32_128"]
        assert inputs128 is inputs and targets128 == self.targets
        self.garbage128 = garbage(self.traces128, comp_t, self.targets)
        self.packed128 = fe.pack_claims(claims128)
        self.derived128, self.derive_report = mult_model_of(oracle, fe, "u32_128")
        assert self.derive_report.ok and not np.array_equal(self.garbage128[0], self.traces128[0])
        # --- the nine-circuit BLAKE3 system, three compressions
        self.b3_states, b3_claims, self.b3_traces, self.b3_packed = b3_case(b3, fe, "n3_129_bytes")
        self.b3_states_out = np.array([c[33:] for c in b3_claims], dtype=np.uint32)
        self.b3_blob = fe.system_blob(fe.test_params(), [fe.compile_circuit(ci) for ci in b3.blake3_system_inputs()])
        self.b3_proof = oracle.System(self.b3_blob).prove(self.b3_traces, self.b3_packed)
        # --- BabyBear: the MulAir at 2^11 rows and the even/odd system with its claim
        with fe.field(fe.BABYBEAR):
            self.mul_inputs, self.eo_inputs = fe.mul_air_inputs(), fe.even_odd_inputs()
            self.mul_trace, self.eo_traces = fe.mul_air_trace(1 << 11), fe.even_odd_traces()
        self.none, self.eo_claim, self.eo_wrong_claim = bb_pack([]), bb_pack([[0, 4, 1]]), bb_pack([[0, 4, 0]])
        self.mul_blob, mul_comp, _ = bb_compile_system(self.mul_inputs)
        self.eo_blob, eo_comp, _ = bb_compile_system(self.eo_inputs)
        omul, oeo = ob.System(self.mul_blob), ob.System(self.eo_blob)
        self.mul_proof = omul.prove([self.mul_trace], self.none)
        self.eo_proof = oeo.prove(self.eo_traces, self.eo_claim)
        assert omul.verify(self.none, self.mul_proof) == 0 and oeo.verify(self.eo_claim, self.eo_proof) == 0
        nq = fe.test_params().num_queries
        bad = _query_tampers(self.mul_proof, nq // 2)["FRI sibling coordinate 2 [query %d]" % (nq // 2)]
        self.bb_items = [(self.none, p) for p in (self.mul_proof, bad, self.mul_proof)]
        # nothing the transcript absorbs changes: an opening error (2) that only the kernels can find; the oracle rejects it too
        self.bb_verdicts = [0, 2, 0]
        assert [omul.verify(c, p) == 0 for c, p in self.bb_items] == [v == 0 for v in self.bb_verdicts]
        self.bb_checks = [(0, [self.mul_trace], self.none, wmb.check(ob, omul, mul_comp, [self.mul_trace], self.none, *BB_BG)),
                          (1, self.eo_traces, self.eo_claim, wmb.check(ob, oeo, eo_comp, self.eo_traces, self.eo_claim, *BB_BG)),
                          (1, self.eo_traces, self.eo_wrong_claim, wmb.check(ob, oeo, eo_comp, self.eo_traces, self.eo_wrong_claim, *BB_BG))]
        assert [m.verdict for _, _, _, m in self.bb_checks] == [0, 0, pkg.CHECK_LOOKUPS]
        _, self.lb_traces, lb_claims, balanced = bb_cases()["u32_one_cell"]
        self.lb_blob, lb_comp, _ = bb_compiled_of("u32_one_cell")
        self.lb_n = len(lb_comp)
        self.lb_packed, self.lb_report = bb_pack(lb_claims), bb_model_of("u32_one_cell")
        assert not balanced and self.lb_report.unbalanced == 4


@pytest.fixture(scope="module")
def expected(oracle):
    return Expected(oracle)


class Rig:
    """what one thread owns: a context and its systems (created on the main thread, one rig after the other)"""

    def __init__(self, e):
        self.ctx = pkg.Context(0)
        self.gl = pkg.System(self.ctx, e.gl_blob, 2)
        self.gl_test = pkg.System(self.ctx, e.test_blob, 2)
        self.b3 = pkg.System(self.ctx, e.b3_blob, 9)
        self.mul = bb.System(self.ctx, e.mul_blob, 1)
        self.eo = bb.System(self.ctx, e.eo_blob, 2)
        self.lb = bb.System(self.ctx, e.lb_blob, e.lb_n)
        # caller memory of the host-resident witnesses: every rig has its own
        self.gl_host = [t.copy() for t in e.gl_traces]
        self.mul_host, self.eo_host = [e.mul_trace.astype(np.uint32)], [t.astype(np.uint32) for t in e.eo_traces]

    def close(self):
        for name in ("gl", "gl_test", "b3", "mul", "eo", "lb"):
            delattr(self, name)
        self.ctx.close()


def gl_prove_device(r, e):
    w = r.gl.witness(e.gl_traces, e.gl_packed)
    assert r.gl.prove_multiple_claims(w).to_bytes() == e.gl_proof


def gl_prove_host(r, e):
    hw = r.gl.host_witness(r.gl_host, e.gl_packed)
    assert hw.pinned
    for _ in range(2):
        assert r.gl.prove_multiple_claims(hw).to_bytes() == e.gl_proof


def gl_verify_batch(r, e):
    assert r.gl.verify_batch(e.gl_items) == e.gl_verdicts


def gl_check(r, e):
    same_check(r.gl.witness(e.gl_traces, e.gl_packed).check(*BG), e.gl_check)


def gl_lookup_balance(r, e):
    rep = r.gl_test.witness(e.unserved_traces, e.unserved_packed).lookup_balance()
    assert rep.fields() == e.unserved_balance.fields() and not rep.ok, str(rep)


def gl_derive(r, e):
    w = r.gl_test.witness(e.garbage128, e.packed128)
    rep = w.derive_multiplicities(e.targets)
    assert rep.fields() == e.derive_report.fields() and rep.ok, str(rep)
    for c, want in enumerate(e.derived128):
        assert np.array_equal(w.trace(c), want) and np.array_equal(want, e.traces128[c]), "trace of circuit %d" % c


def gl_blake3(r, e):
    w = r.b3.blake3_witness_on_device(e.b3_states)
    assert np.array_equal(w.states_out, e.b3_states_out)
    _check_traces(w, e.b3_traces)
    assert r.b3.prove_multiple_claims(w).to_bytes() == e.b3_proof


def bb_prove_device(r, e):
    assert r.mul.prove_multiple_claims(r.mul.witness([e.mul_trace], e.none)).to_bytes() == e.mul_proof
    assert r.eo.prove_multiple_claims(r.eo.witness(e.eo_traces, e.eo_claim)).to_bytes() == e.eo_proof


def bb_prove_host(r, e):
    hm, he = r.mul.host_witness(r.mul_host, e.none), r.eo.host_witness(r.eo_host, e.eo_claim)
    assert hm.pinned and he.pinned and np.shares_memory(hm.keep[0], r.mul_host[0])
    for _ in range(2):
        assert r.mul.prove_multiple_claims(hm).to_bytes() == e.mul_proof
        assert r.eo.prove_multiple_claims(he).to_bytes() == e.eo_proof


def bb_verify_batch(r, e):
    assert r.mul.verify_batch(e.bb_items) == e.bb_verdicts


def bb_check(r, e):
    for which, traces, packed, model in e.bb_checks:
        same_check((r.mul, r.eo)[which].witness(traces, packed).check(*BB_BG), model, final=True)


def bb_lookup_balance(r, e):
    rep = r.lb.witness(e.lb_traces, e.lb_packed).lookup_balance()
    assert rep.fields() == e.lb_report.fields() and not rep.ok, str(rep)


GL_STEPS = [gl_prove_device, gl_prove_host, gl_verify_batch, gl_check, gl_lookup_balance, gl_derive, gl_blake3]
BB_STEPS = [bb_prove_device, bb_prove_host, bb_verify_batch, bb_check, bb_lookup_balance]


def test_mixed_work_on_two_contexts(expected, monkeypatch):
    """Two work lists of the same twelve calls, Goldilocks first in one and BabyBear first in the other. Thread 0 walks its list
    forwards, thread 1 walks its list rotated by one, with a barrier before every step: two DIFFERENT calls overlap at each of
    the twelve steps, of one field or of both. A second pass swaps the lists. Every step compares all it produces."""
    monkeypatch.setenv("MSAMD_PACK_MIN_BYTES", "0")  # the narrow upload (and the device's one pack pool) also at this size
    lists = [GL_STEPS + BB_STEPS, BB_STEPS + GL_STEPS]
    n = len(lists[0])
    t0 = time.perf_counter()
    rigs = [Rig(expected), Rig(expected)]
    spent = {"two rigs": time.perf_counter() - t0}
    try:
        for swap in (0, 1):
            plan = [lists[swap], lists[1 - swap][1:] + lists[1 - swap][:1]]
            assert all(plan[0][i] is not plan[1][i] for i in range(n))

            def body(t):
                def run(barrier):
                    for step in plan[t]:
                        wait(barrier)
                        t0 = time.perf_counter()
                        try:
                            step(rigs[t], expected)
                            spent[(swap, t, step.__name__)] = time.perf_counter() - t0
                        except AssertionError as err:
                            raise AssertionError("pass %d, thread %d, %s next to %s: %s" % (
                                swap, t, step.__name__, plan[1 - t][plan[t].index(step)].__name__, err)) from err
                return run

            run_threads([body(0), body(1)])
    finally:
        print("\n".join("%-40s %6.3f s" % (k, v) for k, v in sorted(spent.items(), key=lambda kv: -kv[1])[:12]))
        for r in rigs:
            r.close()


# ---------------------------------------------------------------- c) one hiprtc program first seen by both threads at once
def fresh_circuit():
    """q_lookups of test_gpu_generated_kernels.py with constants no other test uses: the three generated sources (quotient,
    stage-2 terms, stage-2 from the trace) are new to the process and to the cache directory"""
    E = fe.Expr
    lookups = [fe.Lookup.push(E.main(j % 4), [E.main((j + k) % 4) + E.const(770001 + 131 * j + k) for k in range(na)]) for j, na in enumerate([2, 5, 1])]

    def ev(b):
        m, mn = b.main()
        for k in range(2):
            b.assert_zero(m[k % 4] * mn[(k + 1) % 4] - E.const(990001 + k))

    return fe.lookup_air(4, ev, lookups)


def test_same_generated_program_first_built_by_both_threads(oracle, tmp_path, monkeypatch):
    cache = tmp_path / "jit"
    cache.mkdir()
    monkeypatch.setenv("MSAMD_JIT_CACHE", str(cache))
    monkeypatch.delenv("MSAMD_NO_JIT", raising=False)
    blob = fe.system_blob(fe.test_params(), [fe.compile_circuit(fresh_circuit())])
    trace, packed = rand_field(np.random.default_rng(4242), (64, 4)), fe.pack_claims([[1, 2, 3]])
    want = oracle.System(blob).prove([trace], packed)
    flags = pkg.KERNEL_QUOTIENT | pkg.KERNEL_QUOTIENT_INLINE | pkg.KERNEL_STAGE2 | pkg.KERNEL_STAGE2_TRACE
    ctxs = [pkg.Context(0), pkg.Context(0)]
    host = [trace.copy(), trace.copy()]
    made = {}

    def prove_both_ways(t, s):
        assert s.prove_multiple_claims(s.witness([trace], packed)).to_bytes() == want
        assert s.prove_multiple_claims(s.host_witness([host[t]], packed)).to_bytes() == want

    def first(t):
        def run(barrier):
            wait(barrier)
            s = made[t] = pkg.System(ctxs[t], blob, 1)  # both threads generate and ask for the same three programs
            assert s.circuit_kernels(0) == flags, hex(s.circuit_kernels(0))
            wait(barrier)
            prove_both_ways(t, s)
        return run

    try:
        run_threads([first(0), first(1)])
        files = sorted(p.name for p in cache.iterdir())
        assert len(files) == 3 and all(f.startswith("q_") and f.endswith(".co") for f in files), files  # one per program, no *.<pid> left
        # again, thread 1 on the interpreter kernels (MSAMD_NO_JIT acts where the system is created)
        monkeypatch.setenv("MSAMD_NO_JIT", "1")
        interp = pkg.System(ctxs[1], blob, 1)
        monkeypatch.delenv("MSAMD_NO_JIT")
        assert interp.circuit_kernels(0) == 0

        def again_generated(barrier):
            wait(barrier)
            s = pkg.System(ctxs[0], blob, 1)
            assert s.circuit_kernels(0) == flags
            prove_both_ways(0, s)

        def again_interpreter(barrier):
            wait(barrier)
            prove_both_ways(1, interp)

        run_threads([again_generated, again_interpreter])
        assert sorted(p.name for p in cache.iterdir()) == files
        del interp
    finally:
        made.clear()
        for c in ctxs:
            c.close()


# ---------------------------------------------------------------- d) one set of host buffers, two contexts
def _shared_buffers(make_system, arrays, packed, want):
    """both contexts page-lock the SAME arrays (host_range_pin counts per range); three proofs each at once; then the first
    owner goes and the second must still hold its lock"""
    ctxs = [pkg.Context(0), pkg.Context(0)]
    systems = [make_system(c) for c in ctxs]
    witnesses = [s.host_witness(arrays, packed) for s in systems]
    try:
        for w in witnesses:
            assert w.pinned and all(np.shares_memory(k, a) for k, a in zip(w.keep, arrays))  # the caller's memory itself, not a copy

        def body(t):
            def run(barrier):
                wait(barrier)
                for _ in range(3):
                    assert systems[t].prove_multiple_claims(witnesses[t]).to_bytes() == want
            return run

        run_threads([body(0), body(1)])
        witnesses[0] = systems[0] = None  # the first witness, its system and its context are destroyed
        ctxs[0].close()
        for _ in range(2):
            assert systems[1].prove_multiple_claims(witnesses[1]).to_bytes() == want
    finally:
        witnesses[:] = systems[:] = [None, None]
        for c in ctxs:
            c.close()


def test_goldilocks_host_buffers_shared_by_two_contexts(expected, monkeypatch):
    monkeypatch.setenv("MSAMD_PACK_MIN_BYTES", "0")  # both threads narrow in the device's one pack pool
    arrays = [np.ascontiguousarray(t, dtype=np.uint64).copy() for t in expected.gl_traces]
    _shared_buffers(lambda c: pkg.System(c, expected.gl_blob, 2), arrays, expected.gl_packed, expected.gl_proof)


def test_babybear_host_buffers_shared_by_two_contexts(expected):
    arrays = [np.ascontiguousarray(expected.mul_trace, dtype=np.uint32)]
    _shared_buffers(lambda c: bb.System(c, expected.mul_blob, 1), arrays, expected.none, expected.mul_proof)


# ---------------------------------------------------------------- e) errors stay with their thread
def test_errors_stay_with_their_thread(expected):
    """thread 1 is refused three times on the host (nothing reaches a kernel) while thread 0 proves; the refusals carry their own
    texts, thread 0 sees none of them - neither as an exception nor in ms_last_error(), which is per thread"""
    e = expected
    ctxs = [pkg.Context(0), pkg.Context(0)]
    s0, s1 = pkg.System(ctxs[0], e.gl_blob, 2), pkg.System(ctxs[1], e.test_blob, 2)
    w0 = s0.witness(e.gl_traces, e.gl_packed)
    w1 = s1.witness(e.traces128, e.packed128)
    odd_height = [np.zeros((256 if c == 0 else 3, s1.circuit_info(c)["main_width"]), dtype=np.uint64) for c in range(2)]
    seen = {}

    def prover(barrier):
        wait(barrier)
        for _ in range(5):
            assert s0.prove_multiple_claims(w0).to_bytes() == e.gl_proof
        wait(barrier)  # thread 1's refusals are over
        seen["thread 0"] = pkg.lib().ms_last_error().decode()

    def refused(barrier):
        wait(barrier)
        texts = []
        for _ in range(3):
            for call, text in ((lambda: w1.derive_multiplicities([(1, 1)]), "not eligible"),
                               (lambda: s1.witness(odd_height, e.packed128), "power of two"),
                               (lambda: s1.blake3_witness_on_device(np.zeros((2, 32), dtype=np.uint32)), "not the nine-circuit BLAKE3")):
                with pytest.raises(pkg.MstarkError, match=text) as info:
                    call()
                texts.append(str(info.value))
                assert pkg.lib().ms_last_error().decode() == texts[-1]
        seen["thread 1"] = texts
        wait(barrier)

    try:
        run_threads([prover, refused])
        assert len(seen["thread 1"]) == 9 and len(set(seen["thread 1"])) == 3
        assert seen["thread 0"] not in seen["thread 1"] and "BLAKE3" not in seen["thread 0"]
        assert np.array_equal(w1.trace(0), e.traces128[0])  # refused before anything was written
    finally:
        w0 = w1 = s0 = s1 = None
        for c in ctxs:
            c.close()
