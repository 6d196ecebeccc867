"""What a witness costs to create when the trace already lies in HBM (System.witness_from_device, ms_witness_create_device)
against today's route through host memory (System.witness, ms_witness_create), on the bench system [ByteTable, U32Add]:
  python tools/device_witness_bench.py [log2 additions = 20] [repetitions = 9]
Per route the median and the spread of the wall time of the call (every call returns synchronised; the witness of the call
before is destroyed first, so device blocks are reused), routes alternating inside each repetition, after two warm-up rounds.
Then the ingest kernels' own time from ms_ctx_kernel_stats (class `transpose`), next to everything that class records during
commit_stage1 of that witness in the same run: for this system exactly the transpose_in launches on the same two matrices (the
same bytes read and written, rows bit-reversed) - the launch count is printed so that the figure can be read for what it is.
The upload route's figure is the yardstick; no figure here is a share of peak."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

import torch  # noqa: E402

log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
pkg = load_package()
fe = pkg.frontend
ctx = pkg.Context(0)
system = pkg.System.new(ctx, fe.bench_params(), fe.u32_add_system_inputs())
traces, claims = fe.u32_add_bench_witness(1 << log_n)
packed = fe.pack_claims(claims)
cells = sum(t.size for t in traces)
print("bench system, 2^%d additions: traces %s, %.1f MB as 64-bit words, %d claims; device %s" % (
    log_n, [t.shape for t in traces], cells * 8 / 1e6, len(packed[0]) - 1, torch.cuda.get_device_name(0)), flush=True)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])).cuda()


def narrowest(a):
    for dt in (np.uint8, np.uint16, np.uint32):
        if int(a.max()) <= np.iinfo(dt).max:
            return a.astype(dt)
    return a


row64 = [dev(t) for t in traces]
row8 = [dev(narrowest(t)) for t in traces]
col64 = [t.t().contiguous().t() for t in row64]
torch.cuda.synchronize()
routes = [
    ("ms_witness_create from numpy (upload route)", lambda: system.witness(traces, packed)),
    ("witness_from_device, u64 row-major", lambda: system.witness_from_device(row64, packed)),
    ("witness_from_device, uint%d row-major" % (8 * row8[1].element_size()), lambda: system.witness_from_device(row8, packed)),
    ("witness_from_device, u64 column-major", lambda: system.witness_from_device(col64, packed)),
]
want = system.prove_multiple_claims(routes[0][1]()).to_bytes()
for name, make in routes[1:]:
    assert system.prove_multiple_claims(make()).to_bytes() == want, name  # same proof bytes from every route, at this size

times = {name: [] for name, _ in routes}
for rep in range(reps + 2):
    for name, make in routes:
        ctx.sync()
        t = time.perf_counter()
        w = make()
        dt = 1e3 * (time.perf_counter() - t)
        del w
        if rep >= 2:
            times[name].append(dt)
base = statistics.median(times[routes[0][0]])
for name, _ in routes:
    v = times[name]
    print("%-46s median %8.3f ms  (min %.3f, max %.3f, %d calls)  %5.1fx the upload route's speed" % (
        name, statistics.median(v), min(v), max(v), len(v), base / statistics.median(v)), flush=True)

# kernel time: HIP events around every launch of the class (profiling serialises nothing else here, but it is a run of its own)
ctx.set_profile(["transpose"])
hs, ws = [t.shape[0] for t in traces], [t.shape[1] for t in traces]
for name, make in routes[1:]:
    ms_ingest, ms_tr = [], []
    for rep in range(reps + 1):
        ctx.reset_stats()
        w = make()
        a = ctx.kernel_stats()["transpose"]
        ctx.reset_stats()
        c = w.commit_stage1(hs, ws)
        b = ctx.kernel_stats()["transpose"]
        del c, w
        if rep >= 1:
            ms_ingest.append(a["ms"])
            ms_tr.append(b["ms"])
    print("%-46s ingest kernels %7.3f ms (%d launches, %.0f MB moved, %.0f GB/s)   class `transpose` during commit_stage1 of it (transpose_in of the same matrices) %7.3f ms (%d launches, %.0f MB)" % (
        name, statistics.median(ms_ingest), a["launches"], a["alg_bytes"] / 1e6, a["alg_bytes"] / 1e6 / statistics.median(ms_ingest),
        statistics.median(ms_tr), b["launches"], b["alg_bytes"] / 1e6), flush=True)
