"""ms_witness_derive_multiplicities from the command line: the bench workload ([ByteTable, U32Add]) generated in HBM at a chosen
size; derive ByteTable's multiplicity column on the device, print the report and time the call.
  python tools/derive_multiplicities.py [--log-size 20] [--reps 9] [--entries 16]
Part 1: the report, and the derived column compared with np.bincount over the byte columns read back.
Part 2: ms_witness_derive_multiplicities, ms_witness_lookup_balance (its closest relative: the same table, the same messages plus
the 256 of the table's own slot) and ms_prove alternating on the SAME device-resident witness.
Part 3: the host route the call replaces, step by step: the U32Add trace read back (ms_witness_trace reads whole traces: 14
columns for the 12 byte columns), np.bincount over the byte columns, and the witness uploaded again through ms_witness_create
(which takes every trace, not the table's alone, and runs from_stage_1).
  python tools/derive_multiplicities.py --config babybear [--log-size 20] [--reps 9] [--entries 16]
--config babybear: msbb_witness_derive_multiplicities on the same workload authored over BabyBear (Poseidon2, test parameters; the
claims' u32 words reduced mod p). There is no BabyBear generator in HBM: the witness is built on the host and uploaded once, with 7
in every cell of the table's column. Part 1: the report and the derived column against np.bincount. Part 2:
msbb_witness_derive_multiplicities, msbb_witness_lookup_balance and msbb_prove alternating on that witness. Part 3: the host route
it replaces: msbb_witness_trace of U32Add, np.bincount, msbb_witness_create.
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
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--entries", type=int, default=16)
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
    with fe.field(fe.BABYBEAR):
        system = bb.System.new(ctx, fe.test_params(), fe.u32_add_system_inputs(), k)
        (byte, add), claims = fe.u32_add_bench_witness(n)
        claims = fe.pack_claims(claims)  # (a 2-D array: reduced mod p)
    print("slot (0, 0): %s" % system.multiplicity_slot(0, 0))
    counts = np.bincount(add[:, :12].astype(np.int64).ravel(), minlength=256).astype(np.uint64).reshape(256, 1)
    assert np.array_equal(byte, counts)

    # the table column overwritten, then derived; this witness serves the timed calls too (deriving again writes the same bytes)
    w = system.witness([np.full((256, 1), 7, dtype=np.uint64), add], claims)
    rep = w.derive_multiplicities(TARGETS, entries=args.entries)
    print("u32add over BabyBear at 2^%d additions, ByteTable column 0 derived from 7 everywhere:" % args.log_size)
    print(rep)
    same = bool(np.array_equal(w.trace(0), counts))
    print("derived column equals np.bincount of the byte columns: %s; lookup_balance().ok: %s" % (same, w.lookup_balance().ok), flush=True)
    assert same and rep.ok

    print("\n# the same device-resident witness, calls alternating")
    t_dm, t_bal, t_prove = timed([lambda: w.derive_multiplicities(TARGETS, entries=args.entries), lambda: w.lookup_balance(entries=args.entries),
                                  lambda: system.prove_multiple_claims(w)], args.reps)
    line("msbb_witness_derive_multiplicities", t_dm)
    line("msbb_witness_lookup_balance", t_bal)
    line("msbb_prove", t_prove)
    print("derive / balance = %.3f, derive / prove = %.3f" % (statistics.median(t_dm) / statistics.median(t_bal), statistics.median(t_dm) / statistics.median(t_prove)))
    assert np.array_equal(w.trace(0), counts)

    print("\n# the host route: read back, np.bincount, msbb_witness_create; steps alternating")
    state = {}

    def read_back():
        state["add"] = w.trace(1)

    def histogram():
        state["byte"] = np.bincount(state["add"][:, :12].astype(np.int64).ravel(), minlength=256).astype(np.uint32).reshape(256, 1)

    def create():
        state["w"] = None  # (the previous upload's memory goes back first)
        state["w"] = system.witness([state["byte"], state["add"]], claims)

    t_read, t_hist, t_create = timed([read_back, histogram, create], args.reps)
    line("msbb_witness_trace of U32Add (14 columns)", t_read)
    line("np.bincount over 12 x 2^%d bytes" % args.log_size, t_hist)
    line("msbb_witness_create (both traces)", t_create)
    total = [a + b + c for a, b, c in zip(t_read, t_hist, t_create)]
    line("host route, the three steps together", total)
    print("host route / derive = %.1f" % (statistics.median(total) / statistics.median(t_dm)))
    assert state["w"].lookup_balance(entries=0).ok


if args.config == "babybear":
    babybear()
    sys.exit(0)

system = pkg.System.new(ctx, fe.bench_params(), fe.u32_add_system_inputs())
print("slot (0, 0): %s" % system.multiplicity_slot(0, 0))
w = system.bench_witness_on_device(n)
add = w.trace(1)
counts = np.bincount(add[:, :12].astype(np.int64).ravel(), minlength=256).astype(np.uint64).reshape(256, 1)
word = lambda c: sum(add[:, c + k] << np.uint64(8 * k) for k in range(4))  # noqa: E731
claims = fe.pack_claims(np.stack([np.ones(len(add), dtype=np.uint64), word(0), word(4), word(8)], axis=1)[add[:, 13] == 1])

# the table column overwritten, then derived
w_garbage = system.witness([np.full((256, 1), 7, dtype=np.uint64), add], claims)
rep = w_garbage.derive_multiplicities(TARGETS, entries=args.entries)
print("u32add at 2^%d additions, ByteTable column 0 derived from 7 everywhere:" % args.log_size)
print(rep)
same = bool(np.array_equal(w_garbage.trace(0), counts)) and bool(np.array_equal(w.trace(0), counts))
print("derived column equals np.bincount of the byte columns: %s; lookup_balance().ok: %s" % (same, w_garbage.lookup_balance().ok), flush=True)
assert same and rep.ok
del w_garbage

print("\n# the same device-resident witness, calls alternating")
t_dm, t_bal, t_prove = timed([lambda: w.derive_multiplicities(TARGETS, entries=args.entries), lambda: w.lookup_balance(entries=args.entries),
                              lambda: system.prove_multiple_claims(w)], args.reps)
line("ms_witness_derive_multiplicities", t_dm)
line("ms_witness_lookup_balance", t_bal)
line("ms_prove", t_prove)
print("derive / balance = %.3f, derive / prove = %.3f" % (statistics.median(t_dm) / statistics.median(t_bal), statistics.median(t_dm) / statistics.median(t_prove)))
assert np.array_equal(w.trace(0), counts)

print("\n# the host route: read back, np.bincount, ms_witness_create; steps alternating")
state = {}


def read_back():
    state["add"] = w.trace(1)


def histogram():
    state["byte"] = np.bincount(state["add"][:, :12].astype(np.int64).ravel(), minlength=256).astype(np.uint64).reshape(256, 1)


def create():
    state["w"] = None  # (the previous upload's memory goes back first)
    state["w"] = system.witness([state["byte"], state["add"]], claims)


t_read, t_hist, t_create = timed([read_back, histogram, create], args.reps)
line("ms_witness_trace of U32Add (14 columns)", t_read)
line("np.bincount over 12 x 2^%d bytes" % args.log_size, t_hist)
line("ms_witness_create (both traces, from_stage_1)", t_create)
total = [a + b + c for a, b, c in zip(t_read, t_hist, t_create)]
line("host route, the three steps together", total)
print("host route / derive = %.1f" % (statistics.median(total) / statistics.median(t_dm)))
