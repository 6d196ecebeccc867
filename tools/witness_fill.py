"""ms_witness_fill from the command line: the bench workload ([ByteTable, U32Add]) made three ways at a chosen size, timed
alternately in one run.
  python tools/witness_fill.py [--log-size 20] [--reps 9]
Part 1: a witness of zero traces in HBM is filled from an n x 2 uint32 tensor of (x, y) pairs by the U32Add fill program
(frontend.u32_add_fill_program), ByteTable's column is derived (ms_witness_derive_multiplicities), and the result is compared with
the host builder's traces and, proof bytes against proof bytes, with the witness of the hand-written generator.
Part 2, three routes to the same witness, alternating inside every repetition:
  fill      ms_witness_fill of U32Add from the tensor, then ms_witness_derive_multiplicities; the witness (zero traces, the
            claims) exists beforehand, as it does for a caller who fills one witness again and again
  generator ms_witness_u32_add_bench: the hand-written kernel, which also makes the pairs, the claims and the witness itself
  host      frontend._u32_add_traces (numpy) and ms_witness_create (upload, from_stage_1); the pairs exist beforehand
ms_witness_fill alone (followed by a synchronisation) is a line of its own.
  python tools/witness_fill.py --config babybear [--log-size 20] [--reps 9]
--config babybear: msbb_witness_fill on the same workload authored over BabyBear (Poseidon2, test parameters; the claims' u32
words reduced mod p). U32Add is filled from an n x 4 uint16 tensor of the pairs' 16-bit halves by
frontend.u32_add_halves_fill_program (a field below 2^31 cannot hold x + y), ByteTable's column is derived
(msbb_witness_derive_multiplicities), and the result is compared with the host builder's traces and, proof bytes against proof
bytes, with the host-built witness. There is no BabyBear generator in HBM, so two routes alternate: fill + derive (and
msbb_witness_fill alone) against the host route, frontend._u32_add_traces (numpy) and msbb_witness_create.
Timing: wall time of each route (all return synchronised), alternating after two warm-up rounds; median, minimum and maximum are
printed. No figure here is a share of peak."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="goldilocks", choices=["goldilocks", "babybear"])
ap.add_argument("--log-size", type=int, default=20)
ap.add_argument("--reps", type=int, default=9)
args = ap.parse_args()

pkg = load_package()
fe = pkg.frontend
ctx = pkg.Context(0)
n = 1 << args.log_size
TARGETS = [(0, 0)]


def timed(fns, reps):
    out = [[] for _ in fns]
    for i in range(reps + 2):
        for fn, o in zip(fns, out):
            ctx.sync()
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            dt = 1e3 * (time.perf_counter() - t)
            if i >= 2:
                o.append(dt)
    return out


def line(what, v):
    print("%-52s median %9.3f ms  (min %.3f, max %.3f, %d calls)" % (what, statistics.median(v), min(v), max(v), len(v)), flush=True)


def babybear():
    bb = pkg.babybear
    k = fe.poseidon2_constants()
    bb.set_poseidon2(ctx, k)
    xs, ys = fe.xorshift_pairs(n)
    with fe.field(fe.BABYBEAR):
        system = bb.System.new(ctx, fe.test_params(), fe.u32_add_system_inputs(), k)
        traces, claims = fe._u32_add_traces(xs, ys, n)
        packed = fe.pack_claims(claims)  # (a 2-D array: reduced mod p)
        prog = fe.u32_add_halves_fill_program(n)
    print("fill program: %d nodes, %d steps; %s" % (len(prog.nodes), len(prog.steps), bb.fill_program_info(prog)))
    m16, s16 = np.uint64(0xFFFF), np.uint64(16)
    halves = torch.from_numpy(np.stack([xs & m16, xs >> s16, ys & m16, ys >> s16], axis=1).astype(np.uint16).view(np.int16)).cuda()
    w = system.witness_from_device([torch.zeros(t.shape, dtype=torch.int32, device="cuda") for t in traces], packed)

    rep = w.fill(1, prog, halves)
    dm = w.derive_multiplicities(TARGETS)
    print("u32add over BabyBear at 2^%d additions, U32Add filled from the halves: %s" % (args.log_size, rep))
    print(dm)
    same = bool(np.array_equal(w.trace(0), traces[0])) and bool(np.array_equal(w.trace(1), traces[1]))
    host = system.witness(traces, packed)
    proof = system.prove_multiple_claims(w).to_bytes()
    same_proof = proof == system.prove_multiple_claims(host).to_bytes()
    print("traces equal the host builder's: %s; proof equals the host-built witness's: %s; check().verdict: %d" % (same, same_proof, w.check().verdict),
          flush=True)
    assert same and same_proof and dm.ok
    del host

    print("\n# two routes to the same witness, alternating")
    state = {}

    def fill_route():
        w.fill(1, prog, halves)
        w.derive_multiplicities(TARGETS)

    def fill_alone():
        w.fill(1, prog, halves)
        ctx.sync()

    def host_traces():
        state["traces"] = fe._u32_add_traces(xs, ys, n)[0]

    def host_create():
        state["host"] = None  # (the previous upload's memory goes back first)
        state["host"] = system.witness(state["traces"], packed)

    t_fill, t_alone, t_tr, t_cr = timed([fill_route, fill_alone, host_traces, host_create], args.reps)
    line("fill: msbb_witness_fill + derive_multiplicities", t_fill)
    line("      msbb_witness_fill alone", t_alone)
    line("host: frontend._u32_add_traces", t_tr)
    line("host: msbb_witness_create (both traces)", t_cr)
    total = [a + b for a, b in zip(t_tr, t_cr)]
    line("host route, the two steps together", total)
    print("host route / fill route = %.1f" % (statistics.median(total) / statistics.median(t_fill)))
    assert np.array_equal(w.trace(1), traces[1]) and np.array_equal(w.trace(0), traces[0])
    state.clear()  # witnesses go before their system


if args.config == "babybear":
    babybear()
    sys.exit(0)

system = pkg.System.new(ctx, fe.bench_params(), fe.u32_add_system_inputs())
xs, ys = fe.xorshift_pairs(n)
traces, claims = fe._u32_add_traces(xs, ys, n)
packed = fe.pack_claims(claims)
prog = fe.u32_add_fill_program(n)
print("fill program: %d nodes, %d steps; %s" % (len(prog.nodes), len(prog.steps), pkg.fill_program_info(prog)))
pairs = torch.from_numpy(np.stack([xs, ys], axis=1).astype(np.uint32).view(np.int32)).cuda()
w = system.witness_from_device([torch.zeros(t.shape, dtype=torch.int64, device="cuda") for t in traces], packed)

rep = w.fill(1, prog, pairs)
dm = w.derive_multiplicities(TARGETS)
print("u32add at 2^%d additions, U32Add filled from the pairs: %s" % (args.log_size, rep))
print(dm)
same = bool(np.array_equal(w.trace(0), traces[0])) and bool(np.array_equal(w.trace(1), traces[1]))
gen = system.bench_witness_on_device(n)
proof = system.prove_multiple_claims(w).to_bytes()
same_proof = proof == system.prove_multiple_claims(gen).to_bytes()
print("traces equal the host builder's: %s; proof equals the generator's witness's: %s; check().verdict: %d" % (same, same_proof, w.check().verdict),
      flush=True)
assert same and same_proof and dm.ok
del gen

print("\n# three routes to the same witness, alternating")
state = {}


def fill_route():
    w.fill(1, prog, pairs)
    w.derive_multiplicities(TARGETS)


def fill_alone():
    w.fill(1, prog, pairs)
    ctx.sync()


def generator():
    state["gen"] = None  # (the previous witness's memory goes back first)
    state["gen"] = system.bench_witness_on_device(n)
    ctx.sync()


def host_traces():
    state["traces"] = fe._u32_add_traces(xs, ys, n)[0]


def host_create():
    state["host"] = None
    state["host"] = system.witness(state["traces"], packed)


t_fill, t_alone, t_gen, t_tr, t_cr = timed([fill_route, fill_alone, generator, host_traces, host_create], args.reps)
line("fill: ms_witness_fill + derive_multiplicities", t_fill)
line("      ms_witness_fill alone", t_alone)
line("generator: ms_witness_u32_add_bench", t_gen)
line("host: frontend._u32_add_traces", t_tr)
line("host: ms_witness_create (both traces, from_stage_1)", t_cr)
total = [a + b for a, b in zip(t_tr, t_cr)]
line("host route, the two steps together", total)
m = statistics.median
print("fill route / generator = %.2f, host route / fill route = %.1f" % (m(t_fill) / m(t_gen), m(total) / m(t_fill)))
assert np.array_equal(w.trace(1), traces[1]) and np.array_equal(w.trace(0), traces[0])
state.clear()  # witnesses go before their system, and both before the interpreter takes the module apart
del w
del system
