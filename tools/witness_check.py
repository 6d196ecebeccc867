"""ms_witness_check from the command line: build one of the front-end's systems at a chosen size, optionally corrupt one cell,
print the report, and time the check next to ms_prove on the SAME device-resident witness:
  python tools/witness_check.py [--system u32add|pythagorean|even_odd|blake3] [--log-size 20] [--corrupt CIRCUIT,ROW,COL] [--reps 9]
  python tools/witness_check.py --config babybear [--log-size 20] [--corrupt 0,ROW,COL] [--reps 9]
--log-size: log2 of the additions (u32add), of the rows (pythagorean), of the hashed bytes (blake3); ignored for even_odd.
--config babybear: msbb_witness_check next to msbb_prove on the MulAir of the reference's second configuration (BabyBear, degree-4
extension, Poseidon2; test parameters) at 2^log-size rows; --system is ignored.
Timing: wall time of each call (both return synchronised, with their result on the host), the two alternating inside every
repetition after two warm-up rounds; median, minimum and maximum are printed, and the check's kernel class (`witness_check`,
HIP events around its launches, in a pass of its own) beside them. No figure here is a share of peak."""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="goldilocks", choices=["goldilocks", "babybear"])
ap.add_argument("--system", default="u32add", choices=["u32add", "pythagorean", "even_odd", "blake3"])
ap.add_argument("--log-size", type=int, default=20)
ap.add_argument("--corrupt", default=None, help="CIRCUIT,ROW,COL: that cell gets 1 added")
ap.add_argument("--reps", type=int, default=9)
args = ap.parse_args()

pkg = load_package()
fe = pkg.frontend
ctx = pkg.Context(0)
names = None
check_name, prove_name = "ms_witness_check", "ms_prove"
if args.config == "babybear":
    args.system = "mul_air"
    check_name, prove_name = "msbb_witness_check", "msbb_prove"
    pkg.babybear.set_poseidon2(ctx, fe.poseidon2_constants())
    with fe.field(fe.BABYBEAR):
        inputs, params, names = fe.mul_air_inputs(), fe.test_params(), ["MulAir"]
        traces, claims = [fe.mul_air_trace(1 << args.log_size)], []
elif args.system == "u32add":
    inputs, params, names = fe.u32_add_system_inputs(), fe.bench_params(), ["ByteTable", "U32Add"]
    traces, claims = fe.u32_add_bench_witness(1 << args.log_size)
    claims = [list(c) for c in claims]
elif args.system == "pythagorean":
    inputs, params, names = fe.pythagorean_inputs(), fe.test_params(), ["Pythagorean"]
    traces, claims = [fe.pythagorean_trace(1 << args.log_size)], []
elif args.system == "even_odd":
    inputs, params, names = fe.even_odd_inputs(), fe.test_params(), ["Even", "Odd"]
    traces, claims = fe.even_odd_traces(), [[0, 4, 1]]
else:
    b3 = importlib.import_module("multi_stark_amd.blake3_circuit")
    inputs, params = b3.blake3_system_inputs(), fe.test_params()
    names = ["byte pairs", "u32_xor", "u32_add", "rot8", "rot16", "rot12", "rot7", "g", "compression"]
    claims = [b3.compression_claim(i) for i in b3.blake3_compressions(bytes(i & 255 for i in range(1 << args.log_size)))[0]]
    traces = b3.blake3_witness(claims)
if args.config == "babybear":
    with fe.field(fe.BABYBEAR):
        compiled = [fe.compile_circuit(ci) for ci in inputs]
        system = pkg.babybear.System(ctx, fe.system_blob(params, compiled, fe.poseidon2_constants()), len(compiled))
        packed = fe.pack_claims(claims)
    modulus = fe.BABYBEAR["P"]
else:
    compiled = [fe.compile_circuit(ci) for ci in inputs]
    system = pkg.System(ctx, fe.system_blob(params, compiled), len(compiled))
    packed = fe.pack_claims(claims)
    modulus = fe.P
system.params = params
if args.corrupt:
    ci, row, col = (int(x) for x in args.corrupt.split(","))
    traces = [np.array(t, dtype=np.uint64) for t in traces]
    traces[ci][row, col] = (int(traces[ci][row, col]) + 1) % modulus
w = system.witness(traces, packed)
print("%s: traces %s, %d claims" % (args.system, [tuple(t.shape) for t in traces], len(claims)), flush=True)

rep = w.check(names=names, origins=[c.zero_origins for c in compiled])
print("verdict %d" % rep.verdict)
print(rep)
for c in rep.circuits:
    print("  circuit %d: height %d, %d roots, kernel form %d at %d lanes, %d failing rows" % (c.index, c.height, c.roots, c.kernel, c.lanes, c.failing_rows))

t_check, t_prove = [], []
for i in range(args.reps + 2):
    for fn, out in ((lambda: w.check(), t_check), (lambda: system.prove_multiple_claims(w), t_prove)):
        ctx.sync()
        t = time.perf_counter()
        fn()
        dt = 1e3 * (time.perf_counter() - t)
        if i >= 2:
            out.append(dt)
ctx.set_profile(["witness_check", "stage2"])
ctx.reset_stats()
w.check()
st = ctx.kernel_stats()
for what, v in ((check_name, t_check), (prove_name, t_prove)):
    print("%-*s median %9.3f ms  (min %.3f, max %.3f, %d calls)" % (len(check_name) + 1, what, statistics.median(v), min(v), max(v), len(v)))
if args.config == "babybear":  # (this configuration's stage-2 launches carry no profiling events)
    print("check / prove = %.3f; inside one check: class witness_check %.3f ms (%d launches)" % (
        statistics.median(t_check) / statistics.median(t_prove), st["witness_check"]["ms"], st["witness_check"]["launches"]))
else:
    print("check / prove = %.3f; inside one check: class witness_check %.3f ms (%d launches), class stage2 %.3f ms (%d launches)" % (
        statistics.median(t_check) / statistics.median(t_prove), st["witness_check"]["ms"], st["witness_check"]["launches"],
        st["stage2"]["ms"], st["stage2"]["launches"]))
