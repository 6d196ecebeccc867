"""The reference's BLAKE3 compression system (multi-stark_amd/blake3_circuit.py; src/test_circuits/blake3.rs) at scale: every
compression of the hash of an n-byte input as a claim of the 2625-column compression circuit, proved on the GPU, compared with the
oracle's proof and timed - a wide system (nine circuits, 73 lookups in one of them, the interpreter kernels for its 6952-node
program) next to the bench's tall one.
  python tools/blake3_bench.py [bytes = 65536] [proofs = 5] [--no-oracle] [--device-witness [--no-python]]
--device-witness: the witness is generated in HBM (System.blake3_witness_on_device) from the compression inputs alone; the line
reports the generation time (wall clock around the call, which returns synchronised) beside the proof time, and - unless
--no-python skips the Python witness - the Python generation time and whether both witnesses give the same proof bytes."""
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_package  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 65536
reps = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[2].isdigit() else 5
pkg = load_package()
fe = pkg.frontend
b3 = importlib.import_module("multi_stark_amd.blake3_circuit")
device_witness, python_witness = "--device-witness" in sys.argv, "--no-python" not in sys.argv
data = bytes((i * 13 + 5) & 255 for i in range(n))
if device_witness:
    t = time.perf_counter()
    states, digest = b3.compression_states(data)
    host_ms = 1e3 * (time.perf_counter() - t)
    py_s = None
    if python_witness:
        t = time.time()
        claims = [b3.compression_claim(i) for i in b3.blake3_compressions(data)[0]]
        traces = b3.blake3_witness(claims)
        packed = fe.pack_claims(claims)
        py_s = time.time() - t
    H = 1 << (len(states) - 1).bit_length()
    print("BLAKE3 of %d bytes: %d compressions (enumerated by the library's host code in %.2f ms), compression trace %d x 2625" % (n, len(states), host_ms, H),
          flush=True)
    ctx = pkg.Context(0)
    system = pkg.System.new(ctx, fe.test_params(), b3.blake3_system_inputs())
    t = time.perf_counter()
    w = system.blake3_witness_on_device(states)
    first_ms = 1e3 * (time.perf_counter() - t)
    gen = []
    for _ in range(reps):  # every call generates the whole witness again; the device blocks of the one before are reused
        del w
        t = time.perf_counter()
        w = system.blake3_witness_on_device(states)
        gen.append(1e3 * (time.perf_counter() - t))
    proof = system.prove_multiple_claims(w).to_bytes()
    for _ in range(2):
        system.prove_multiple_claims(w)
    ctx.sync()
    t = time.perf_counter()
    for _ in range(reps):
        system.prove_multiple_claims(w)
    ms = 1e3 * (time.perf_counter() - t) / reps
    line = "device witness, test parameters: generation %.2f ms (first call %.2f ms, then %s), %d rows; proof %.2f ms (%d bytes)" % (
        min(gen), first_ms, " ".join("%.2f" % g for g in gen), w.rows, ms, len(proof))
    if python_witness:
        t = time.time()
        pw = system.witness(traces, packed)
        up_s = time.time() - t
        same = system.prove_multiple_claims(pw).to_bytes() == proof
        line += "; Python witness %.1f s + %.1f s upload and host lookup values; proof bytes %s" % (py_s, up_s, "IDENTICAL" if same else "DIFFER")
        assert same
        assert system.verify_multiple_claims(packed, proof) == 0
    print(line, flush=True)
    sys.exit(0)
t = time.time()
infos, digest = b3.blake3_compressions(data)
claims = [b3.compression_claim(i) for i in infos]
traces = b3.blake3_witness(claims)
packed = fe.pack_claims(claims)
rows = sum(tr.shape[0] for tr in traces)
cells = sum(tr.shape[0] * tr.shape[1] for tr in traces)
print("BLAKE3 of %d bytes: %d compressions; traces %s = %d rows, %.1f M cells (witness generation in Python: %.1f s)" % (
    n, len(infos), [tr.shape for tr in traces], rows, cells / 1e6, time.time() - t), flush=True)
ctx = pkg.Context(0)
for name, params in (("test parameters (blowup 2, 64 queries)", fe.test_params()), ("bench parameters (blowup 4, 100 queries, 10 + 10 PoW bits)", fe.bench_params())):
    system = pkg.System.new(ctx, params, b3.blake3_system_inputs())
    w = system.witness(traces, packed)
    proof = system.prove_multiple_claims(w).to_bytes()
    assert system.verify_multiple_claims(packed, proof) == 0
    for _ in range(2):
        system.prove_multiple_claims(w)
    ctx.sync()
    t = time.perf_counter()
    for _ in range(reps):
        system.prove_multiple_claims(w)
    ms = 1e3 * (time.perf_counter() - t) / reps
    st = system.prove_multiple_claims(w, want_times=True).stage_ms
    line = "%s: %.2f ms per proof (%d bytes), %.1f M trace cells/s, %.0f compressions/s; stages %s" % (
        name, ms, len(proof), cells / ms / 1e3, len(infos) / ms * 1e3, {k: round(v, 2) for k, v in st.items()})
    if "--no-oracle" not in sys.argv:
        import oracle

        oracle.set_threads(min(16, oracle.max_threads()))
        t = time.time()
        want = oracle.System(system.blob).prove(traces, packed)
        line += "; oracle (16 threads) %.1f s, bytes %s" % (time.time() - t, "IDENTICAL" if want == proof else "DIFFER")
        assert want == proof
    print(line, flush=True)
