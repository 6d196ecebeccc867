"""ms_witness_argsort from the command line: the sorting permutation of a memory log's rows made on the device, against the host
route it replaces and against a tuned library sort, timed alternately in one run.
  python tools/witness_argsort.py [--log-size 20] [--reps 9]
One circuit of four columns (addr, val, s_addr, s_val) at 2^log-size rows, the witness in HBM; addr is random below 2^20 (at most
the height), val random over the field. Every route ends in a synchronisation and is timed by the host clock around it:
  argsort, field key     ms_witness_argsort on val: eight digit passes
  argsort, address key   ms_witness_argsort on addr: the digits above the addresses are skipped
  argsort, two keys      ms_witness_argsort on (addr, val)
  host                   ms_witness_trace, np.lexsort on addr, ms_witness_create of the trace with the permutation in it - each part
                         timed, and their sum
  torch.sort             a stable torch.sort of val as a device int64 tensor with the sign bit flipped (the order of the unsigned
                         words): the yardstick of a tuned library sort, keys and indices only - no trace is read or written
The results of the three calls are compared with numpy before anything is timed."""
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
ap.add_argument("--log-size", type=int, default=20)
ap.add_argument("--reps", type=int, default=9)
args = ap.parse_args()

pkg = load_package()
fe = pkg.frontend
ctx = pkg.Context(0)
n = 1 << args.log_size
P = (1 << 64) - (1 << 32) + 1
ADDR, VAL, S_ADDR, S_VAL = 0, 1, 2, 3


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


def memory_air():
    E = fe.Expr

    def ev(b):
        local, nxt = b.main()
        d = nxt[S_ADDR] - local[S_ADDR]
        b.when_transition().assert_zero(d * (d - 1))

    return fe.lookup_air(4, ev, [fe.Lookup.push(1, [E.const(7), E.main(ADDR), E.main(VAL)]), fe.Lookup.pull(1, [E.const(7), E.main(S_ADDR), E.main(S_VAL)])])


rng = np.random.default_rng(20)
trace = np.zeros((n, 4), dtype=np.uint64)
trace[:, ADDR] = rng.integers(0, min(n, 1 << 20), size=n, dtype=np.uint64)
trace[:, VAL] = rng.integers(0, P, size=n, dtype=np.uint64)
system = pkg.System.new(ctx, fe.test_params(), [memory_air()])
packed = fe.pack_claims([])
w = system.witness_from_device([torch.from_numpy(trace.view(np.int64)).cuda()], packed)
print("sort info (rows per tile, bits per digit, counts per offsets round, largest n_keys): %s" % (pkg.sort_info(),))

ok = True
for keys, dst in (([VAL], S_VAL), ([ADDR], S_ADDR), ([ADDR, VAL], S_VAL)):
    rep = w.argsort(0, keys, dst)
    want = np.lexsort([trace[:, k] for k in reversed(keys)]).astype(np.uint64)
    same = bool(np.array_equal(w.trace(0)[:, dst], want))
    ok = ok and same
    print("2^%d rows, keys %s -> column %d: %s; equals np.lexsort: %s" % (args.log_size, keys, dst, rep, same), flush=True)
assert ok

flipped = torch.from_numpy((trace[:, VAL] ^ np.uint64(1 << 63)).view(np.int64)).cuda()
state = {}


def sort_field():
    w.argsort(0, [VAL], S_VAL)
    ctx.sync()


def sort_addr():
    w.argsort(0, [ADDR], S_ADDR)
    ctx.sync()


def sort_two():
    w.argsort(0, [ADDR, VAL], S_VAL)
    ctx.sync()


def host_trace():
    state["t"] = w.trace(0)


def host_sort():
    t = state["t"]
    t[:, S_ADDR] = np.lexsort([t[:, ADDR]]).astype(np.uint64)


def host_create():
    state["host"] = None  # (the previous upload's memory goes back first)
    state["host"] = system.witness([state["t"]], packed)


def torch_sort():
    state["sorted"] = torch.sort(flipped, stable=True)
    torch.cuda.synchronize()


print("\n# the routes, alternating")
t_f, t_a, t_2, t_tr, t_so, t_cr, t_to = timed([sort_field, sort_addr, sort_two, host_trace, host_sort, host_create, torch_sort], args.reps)
line("ms_witness_argsort, one key over the field", t_f)
line("ms_witness_argsort, one 20-bit address key", t_a)
line("ms_witness_argsort, two keys (address, field)", t_2)
line("host: ms_witness_trace", t_tr)
line("host: np.lexsort", t_so)
line("host: ms_witness_create", t_cr)
total = [a + b + c for a, b, c in zip(t_tr, t_so, t_cr)]
line("host route, the three steps together", total)
line("torch.sort, stable, int64 keys of the field column", t_to)
assert np.array_equal(state["sorted"][1].cpu().numpy().astype(np.uint64), np.lexsort([trace[:, VAL]]).astype(np.uint64))
m = statistics.median
state.clear()
del w, system  # (before the interpreter takes the library's module apart)
print("host route / argsort on the address key = %.1f; argsort over the field / torch.sort = %.2f" % (m(total) / m(t_a), m(t_f) / m(t_to)))
