"""ms_witness_argsort / msbb_witness_argsort from the command line: the sorting permutation of a memory log's rows made on the
device, against the host route it replaces and against a tuned library sort, timed alternately in one run.
  python tools/witness_argsort.py [--config goldilocks|babybear] [--log-size 20] [--reps 9]
One circuit of four columns (addr, val, s_addr, s_val) at 2^log-size rows, the witness in HBM; addr is random below 2^20 (at most
the height), val random over the field. Every route ends in a synchronisation and is timed by the host clock around it:
  argsort, field key     the call on val: every digit pass (eight over Goldilocks, four over BabyBear)
  argsort, address key   the call on addr: the digits above the addresses are skipped
  argsort, two keys      the call on (addr, val)
  host                   witness_trace, np.lexsort on addr, witness_create of the trace with the permutation in it - each part
                         timed, and their sum
  torch.sort             a stable torch.sort of val on the device, the yardstick of a tuned library sort, keys and indices only -
                         no trace is read or written. Goldilocks: int64 keys with the sign bit flipped (the order of the unsigned
                         words); BabyBear: the canonical values as int32 (below 2^31: the signed order is the canonical one)
--config babybear times the three Goldilocks calls in the same alternating run as well, on a witness of the same shape, so that
the two fields' figures come from one session. The results of the calls are compared with numpy before anything is timed."""
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
ap.add_argument("--config", choices=["goldilocks", "babybear"], default="goldilocks")
ap.add_argument("--log-size", type=int, default=20)
ap.add_argument("--reps", type=int, default=9)
args = ap.parse_args()

pkg = load_package()
fe = pkg.frontend
bb = pkg.babybear
ctx = pkg.Context(0)
n = 1 << args.log_size
GL_P = (1 << 64) - (1 << 32) + 1
ADDR, VAL, S_ADDR, S_VAL = 0, 1, 2, 3
BABYBEAR = args.config == "babybear"


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


def memory_log(rng, p):
    trace = np.zeros((n, 4), dtype=np.uint64)
    trace[:, ADDR] = rng.integers(0, min(n, 1 << 20), size=n, dtype=np.uint64)
    trace[:, VAL] = rng.integers(0, p, size=n, dtype=np.uint64)
    return trace


def checked(name, w, trace):
    """the three calls against np.lexsort"""
    for keys, dst in (([VAL], S_VAL), ([ADDR], S_ADDR), ([ADDR, VAL], S_VAL)):
        rep = w.argsort(0, keys, dst)
        want = np.lexsort([trace[:, k] for k in reversed(keys)]).astype(np.uint64)
        same = bool(np.array_equal(w.trace(0)[:, dst].astype(np.uint64), want))
        print("%s, 2^%d rows, keys %s -> column %d: %s; equals np.lexsort: %s" % (name, args.log_size, keys, dst, rep, same), flush=True)
        assert same


def calls(w):
    """the three timed calls on witness w"""
    def sort_field():
        w.argsort(0, [VAL], S_VAL)
        ctx.sync()

    def sort_addr():
        w.argsort(0, [ADDR], S_ADDR)
        ctx.sync()

    def sort_two():
        w.argsort(0, [ADDR, VAL], S_VAL)
        ctx.sync()

    return [sort_field, sort_addr, sort_two]


rng = np.random.default_rng(20)
gl_trace = memory_log(rng, GL_P)
gl_system = pkg.System.new(ctx, fe.test_params(), [memory_air()])
gl_packed = fe.pack_claims([])
gl_w = gl_system.witness_from_device([torch.from_numpy(gl_trace.view(np.int64)).cuda()], gl_packed)
print("ms_sort_info (rows per tile, bits per digit, counts per offsets round, largest n_keys): %s" % (pkg.sort_info(),))
checked("ms_witness_argsort", gl_w, gl_trace)
if BABYBEAR:
    K = fe.poseidon2_constants()
    bb.set_poseidon2(ctx, K)
    trace = memory_log(rng, bb.P)
    with fe.field(fe.BABYBEAR):
        system = bb.System.new(ctx, fe.test_params(), [memory_air()], K)
        packed = fe.pack_claims([])
    w = system.witness_from_device([torch.from_numpy(trace.astype(np.uint32).view(np.int32)).cuda()], packed)
    print("msbb_sort_info: %s" % (bb.sort_info(),))
    checked("msbb_witness_argsort", w, trace)
    call, host_dtype = "msbb_witness_argsort", np.uint32
    lib_keys, lib_name = torch.from_numpy(trace[:, VAL].astype(np.uint32).view(np.int32)).cuda(), "int32"
else:
    trace, system, packed, w = gl_trace, gl_system, gl_packed, gl_w
    call, host_dtype = "ms_witness_argsort", np.uint64
    lib_keys, lib_name = torch.from_numpy((trace[:, VAL] ^ np.uint64(1 << 63)).view(np.int64)).cuda(), "int64"
state = {}


def host_trace():
    state["t"] = w.trace(0)


def host_sort():
    t = state["t"]
    t[:, S_ADDR] = np.lexsort([t[:, ADDR]]).astype(host_dtype)


def host_create():
    state["host"] = None  # (the previous upload's memory goes back first)
    state["host"] = system.witness([state["t"]], packed)


def torch_sort():
    state["sorted"] = torch.sort(lib_keys, stable=True)
    torch.cuda.synchronize()


print("\n# the routes, alternating")
routes = calls(w) + [host_trace, host_sort, host_create, torch_sort] + (calls(gl_w) if BABYBEAR else [])
times = timed(routes, args.reps)
t_f, t_a, t_2, t_tr, t_so, t_cr, t_to = times[:7]
line("%s, one key over the field" % call, t_f)
line("%s, one 20-bit address key" % call, t_a)
line("%s, two keys (address, field)" % call, t_2)
prefix = "msbb" if BABYBEAR else "ms"
line("host: %s_witness_trace" % prefix, t_tr)
line("host: np.lexsort", t_so)
line("host: %s_witness_create" % prefix, t_cr)
total = [a + b + c for a, b, c in zip(t_tr, t_so, t_cr)]
line("host route, the three steps together", total)
line("torch.sort, stable, %s keys of the field column" % lib_name, t_to)
assert np.array_equal(state["sorted"][1].cpu().numpy().astype(np.uint64), np.lexsort([trace[:, VAL]]).astype(np.uint64))
m = statistics.median
print("host route / argsort on the address key = %.1f; argsort over the field / torch.sort = %.2f" % (m(total) / m(t_a), m(t_f) / m(t_to)))
if BABYBEAR:
    g_f, g_a, g_2 = times[7:]
    line("ms_witness_argsort, one key over the field", g_f)
    line("ms_witness_argsort, one 20-bit address key", g_a)
    line("ms_witness_argsort, two keys (address, field)", g_2)
    print("BabyBear / Goldilocks: field key %.2f, address key %.2f, two keys %.2f" % (m(t_f) / m(g_f), m(t_a) / m(g_a), m(t_2) / m(g_2)))
state.clear()
routes.clear()  # (the timed closures hold the witnesses)
del w, system, gl_w, gl_system  # (before the interpreter takes the library's module apart)
