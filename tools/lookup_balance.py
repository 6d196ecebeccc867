"""ms_witness_lookup_balance from the command line: the bench workload ([ByteTable, U32Add]) generated in HBM at a chosen size,
optionally with one cell changed; print the report and time the call.
  python tools/lookup_balance.py [--log-size 20] [--corrupt CIRCUIT,ROW,COL] [--reps 9] [--entries 16]
Part 1: the report of the witness (with --corrupt: of the witness with that cell's lowest bit flipped).
Part 2: ms_witness_lookup_balance, ms_witness_check and ms_prove alternating on the SAME device-resident (clean) witness.
Part 3: the balance call alone, at equal message count (14 x 2^log-size), on three witnesses: the bench witness (12 x 2^log-size
byte messages on 256 tuples), a witness whose 14 x 2^log-size tuples are all distinct (14 slots pushing (slot, row); every group
unbalanced), and the bench witness with one cell changed (the unbalanced path with its second host wait).
  python tools/lookup_balance.py --config babybear [--log-size 20] [--corrupt 0,ROW,COL] [--reps 9] [--entries 16]
--config babybear: msbb_witness_lookup_balance on the MulAir of the reference's second configuration (BabyBear, Poseidon2; test
parameters) at 2^log-size rows in HBM, 2 messages per row. Part 1: the report (with --corrupt: of the witness with 1 added to that
cell - MulAir's push and pull read the same cells, so it stays balanced whatever they hold; its check() does not). Part 2:
msbb_witness_lookup_balance, msbb_witness_check and msbb_prove alternating on the same witness. Part 3: the balance call alone at
2 x 2^log-size messages on MulAir, on a witness whose tuples are all distinct (two slots pushing (slot, row)) and on one with a
single unbalanced group (push(1, [a, c]) and pull(m, [a, c]) with m = 2 in row 0: the second host wait).
Timing: wall time of each call (all return synchronised, with their result on the host), alternating inside every repetition
after two warm-up rounds; median, minimum and maximum are printed. No figure here is a share of peak."""
import argparse
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
ap.add_argument("--log-size", type=int, default=20)
ap.add_argument("--corrupt", default="1,5,0", help="CIRCUIT,ROW,COL: that cell's lowest bit is flipped (part 1 when given, part 3 always)")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--entries", type=int, default=16)
args = ap.parse_args()
corrupt_given = any(a.startswith("--corrupt") for a in sys.argv[1:])

pkg = load_package()
fe = pkg.frontend
ctx = pkg.Context(0)
n = 1 << args.log_size


def timed(fns, reps):
    out = [[] for _ in fns]
    for i in range(reps + 2):
        for fn, o in zip(fns, out):
            ctx.sync()
            t = time.perf_counter()
            fn()
            dt = 1e3 * (time.perf_counter() - t)
            if i >= 2:
                o.append(dt)
    return out


def line(what, v):
    print("%-44s median %9.3f ms  (min %.3f, max %.3f, %d calls)" % (what, statistics.median(v), min(v), max(v), len(v)), flush=True)


def babybear():
    bb = pkg.babybear
    k = fe.poseidon2_constants()
    bb.set_poseidon2(ctx, k)
    p = fe.BABYBEAR["P"]
    with fe.field(fe.BABYBEAR):
        E, params, none = fe.Expr, fe.test_params(), fe.pack_claims([])
        system = bb.System.new(ctx, params, fe.mul_air_inputs(), k)
        trace = fe.mul_air_trace(n)
        # all distinct at the same message count: 2 slots x 2^log-size rows
        distinct = bb.System.new(ctx, params, [fe.CircuitInputs(1, None, [], [], [fe.Lookup.push(E.const(1), [E.const(j), E.main(0)]) for j in range(2)])], k)
        # MulAir's lookups with the pull's multiplicity in a column: one group left unbalanced
        ac = [E.main(0), E.main(2)]
        one_off = bb.System.new(ctx, params, [fe.CircuitInputs(4, None, [], [], [fe.Lookup.push(E.const(1), ac), fe.Lookup.pull(E.main(3), ac)])], k)
    if corrupt_given:
        ci, row, col = (int(x) for x in args.corrupt.split(","))
        trace[row, col] = (int(trace[row, col]) + 1) % p
    w = system.witness([trace], none)
    w_distinct = distinct.witness([(np.arange(1, n + 1, dtype=np.uint64) % np.uint64(p)).reshape(n, 1)], none)
    m = np.ones((n, 1), dtype=np.uint64)
    m[0, 0] = 2
    w_one = one_off.witness([np.concatenate([trace, m], axis=1)], none)

    rep = w.lookup_balance(entries=args.entries, names=["MulAir"])
    print("mul_air at 2^%d rows%s: %d messages, %d groups, %d unbalanced" % (
        args.log_size, " with 1 added to cell (%d, %d, %d)" % (ci, row, col) if corrupt_given else "", rep.messages, rep.groups, rep.unbalanced))
    print(rep)
    print("check(): verdict %d" % w.check().verdict, flush=True)

    print("\n# the same device-resident witness, calls alternating")
    t_bal, t_check, t_prove = timed([lambda: w.lookup_balance(entries=args.entries), lambda: w.check(), lambda: system.prove_multiple_claims(w)], args.reps)
    line("msbb_witness_lookup_balance", t_bal)
    line("msbb_witness_check", t_check)
    line("msbb_prove", t_prove)
    print("balance / prove = %.3f, balance / check = %.2f" % (statistics.median(t_bal) / statistics.median(t_prove), statistics.median(t_bal) / statistics.median(t_check)))

    print("\n# msbb_witness_lookup_balance at %d messages, calls alternating" % (2 * n))
    t_mul, t_dist, t_one = timed([lambda: w.lookup_balance(entries=args.entries), lambda: w_distinct.lookup_balance(entries=args.entries),
                                  lambda: w_one.lookup_balance(entries=args.entries)], args.reps)
    line("MulAir (every tuple twice, balanced)", t_mul)
    line("all tuples distinct (every group unbalanced)", t_dist)
    rep = w_one.lookup_balance(entries=args.entries)
    line("one unbalanced group of %d (second host wait)" % rep.groups, t_one)
    assert rep.unbalanced == 1 and w_distinct.lookup_balance(entries=0).unbalanced == 2 * n


if args.config == "babybear":
    babybear()
    sys.exit(0)

names = ["ByteTable", "U32Add"]
system = pkg.System.new(ctx, fe.bench_params(), fe.u32_add_system_inputs())
w = system.bench_witness_on_device(n)

# the same witness with one cell changed: traces read back, claims rebuilt from the rows, uploaded again
byte, add = w.trace(0), w.trace(1)
word = lambda c: sum(add[:, c + k] << np.uint64(8 * k) for k in range(4))  # noqa: E731
claims = np.stack([np.ones(len(add), dtype=np.uint64), word(0), word(4), word(8)], axis=1)[add[:, 13] == 1]
ci, row, col = (int(x) for x in args.corrupt.split(","))
bad_traces = [byte, add]
bad_traces[ci][row, col] ^= np.uint64(1)
w_bad = system.witness(bad_traces, fe.pack_claims(claims))

# all distinct at the same message count: 14 slots x 2^log-size rows
E = fe.Expr
distinct = pkg.System.new(ctx, fe.bench_params(), [fe.CircuitInputs(1, None, [], [], [fe.Lookup.push(E.const(1), [E.const(j), E.main(0)]) for j in range(14)])])
w_distinct = distinct.witness([np.arange(1, n + 1, dtype=np.uint64).reshape(n, 1)], fe.pack_claims([]))

rep = (w_bad if corrupt_given else w).lookup_balance(entries=args.entries, names=names)
print("u32add at 2^%d additions%s: %d messages, %d groups, %d unbalanced" % (
    args.log_size, " with cell (%d, %d, %d) changed" % (ci, row, col) if corrupt_given else "", rep.messages, rep.groups, rep.unbalanced))
print(rep, flush=True)


print("\n# the same device-resident witness, calls alternating")
t_bal, t_check, t_prove = timed([lambda: w.lookup_balance(entries=args.entries), lambda: w.check(), lambda: system.prove_multiple_claims(w)], args.reps)
line("ms_witness_lookup_balance", t_bal)
line("ms_witness_check", t_check)
line("ms_prove", t_prove)
print("balance / prove = %.3f, balance / check = %.2f" % (statistics.median(t_bal) / statistics.median(t_prove), statistics.median(t_bal) / statistics.median(t_check)))

print("\n# ms_witness_lookup_balance at about %d messages, calls alternating" % (14 * n))
t_hot, t_dist, t_one = timed([lambda: w.lookup_balance(entries=args.entries), lambda: w_distinct.lookup_balance(entries=args.entries),
                              lambda: w_bad.lookup_balance(entries=args.entries)], args.reps)
line("bench witness (256 hot byte tuples)", t_hot)
line("all tuples distinct (every group unbalanced)", t_dist)
line("bench witness, one cell changed", t_one)
