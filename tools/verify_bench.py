"""Verification throughput: a loop of ms_verify against ms_verify_batch on the same proof bytes, in one process.

The bench workload (u32_add + byte table, bench parameters) is proved once at 2^16 and at 2^20 additions; each proof is then
verified N = 1, 8, 64 times per call, as a loop of System.verify and as one System.verify_batch. Per configuration: the median
of REPS timed repetitions after a warm-up, proofs/s, the GPU time of the batch's two launches (ms_ctx_kernel_stats, taken in a
separate profiled pass) and the share of the batch call that is not kernel time (host part, upload, read-back).

--config babybear: the same comparison for the second configuration (msbb_verify / msbb_verify_batch, BabyBear / Poseidon2),
on the u32_add + byte table workload at the bench parameters; --logs defaults to 12,16 there.

usage: python3 tools/verify_bench.py [--config goldilocks|babybear] [--reps 10] [--logs 16,20] [--batches 1,8,64] [--json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402


def _median_ms(fn, reps):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--config", choices=["goldilocks", "babybear"], default="goldilocks")
    ap.add_argument("--logs", default=None)
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    reps = max(a.reps, 10)
    pkg = load_package()
    fe = pkg.frontend
    ctx = pkg.Context(0)
    babybear = a.config == "babybear"
    names = ("msbb_verify", "msbb_verify_batch") if babybear else ("ms_verify", "ms_verify_batch")
    if babybear:
        with fe.field(fe.BABYBEAR):
            g = pkg.babybear.System.new(ctx, fe.bench_params(), fe.u32_add_system_inputs(), fe.poseidon2_constants())
    else:
        g = pkg.System.new(ctx, fe.bench_params(), fe.u32_add_system_inputs())
    rows = []
    for log_n in [int(x) for x in (a.logs or ("12,16" if babybear else "16,20")).split(",")]:
        if babybear:
            with fe.field(fe.BABYBEAR):
                traces, claims = fe.u32_add_bench_witness(1 << log_n)
                packed = fe.pack_claims(claims)
        else:
            traces, claims = fe.u32_add_bench_witness(1 << log_n)
            packed = fe.pack_claims(claims)
        proof = g.prove_multiple_claims(g.witness(traces, packed)).to_bytes()
        assert g.verify(packed, proof) == 0
        for n in [int(x) for x in a.batches.split(",")]:
            items = [(packed, proof)] * n

            def loop():
                for c, p in items:
                    assert g.verify(c, p) == 0

            def batch():
                assert g.verify_batch(items) == [0] * n

            t_loop, t_batch = _median_ms(loop, reps), _median_ms(batch, reps)
            ctx.set_profile(["compress_layer", "other"])
            ctx.reset_stats()
            batch()
            st = ctx.kernel_stats()
            ctx.set_profile([])
            # the claims of this workload go through the device in both paths (hash and accumulator: "other" launches of
            # the host part are counted with the batch's arithmetic launch)
            gpu_ms = st["compress_layer"]["ms"] + st["other"]["ms"]
            rows.append({"log_adds": log_n, "proof_bytes": len(proof), "batch": n, "loop_ms": t_loop, "batch_ms": t_batch,
                         "loop_proofs_per_s": 1e3 * n / t_loop, "batch_proofs_per_s": 1e3 * n / t_batch, "gpu_ms": gpu_ms,
                         "paths_ms": st["compress_layer"]["ms"], "non_kernel_share": max(0.0, 1 - gpu_ms / t_batch)})
    if a.json:
        print(json.dumps(rows))
        return
    print("| additions | proof bytes | batch | loop of %s: ms (proofs/s) | %s: ms (proofs/s) | GPU kernels ms (paths) | not kernel time |" % names)
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print("| 2^%d | %d | %d | %.2f (%.0f) | %.2f (%.0f) | %.3f (%.3f) | %.0f %% |" % (
            r["log_adds"], r["proof_bytes"], r["batch"], r["loop_ms"], r["loop_proofs_per_s"], r["batch_ms"], r["batch_proofs_per_s"],
            r["gpu_ms"], r["paths_ms"], 100 * r["non_kernel_share"]))


if __name__ == "__main__":
    main()
