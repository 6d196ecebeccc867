"""CPU check of the batched BabyBear verifier before any GPU run: tools/bb_verify_host_check.hip compiles the BabyBear
verifier (csrc/bb_verifier.hip, with the host collection of csrc/verify_batch.h) and both kernel bodies of
csrc/bb_verify_dev.h as host code, with the address and undefined-behaviour sanitizers, into a stand-alone program, and
compares them with verify() on proofs the oracle makes on the CPU (arity 1, 2, 3 and 6, caps above 0, a height-1 trace,
lookups with a claim, an inactive circuit, an inactive circuit with a preprocessed trace) and on mutations of them; on the
last one also the directed mutation that sends a proof down the collector's host path. The sponge in a thread is compared
with hash_words for 0 .. 40 words. Needs the built library (the system types of csrc/bb_host.h hold device buffers and
compiled kernels, whose destructors live there; none of them is called with anything to release) and no GPU.

usage: python3 tools/bb_verify_host_check.py [--mutations 150] [--keep DIR]"""
import argparse
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_package  # noqa: E402


def scenarios(out):
    import oracle_bb as ob
    import proof_codec as pc

    pkg = load_package()
    fe = pkg.frontend
    k = fe.poseidon2_constants()
    ob.set_poseidon2(k)

    def emit(name, params, inputs, traces, claims, widen_unopened_row=False):
        compiled = [fe.compile_circuit(c) for c in inputs]
        blob = fe.system_blob(params, compiled, k)
        packed = fe.pack_claims(claims)
        o = ob.System(blob)
        proof = o.prove(traces, packed)
        assert o.verify(packed, proof) == 0, name
        open(os.path.join(out, name + ".blob"), "wb").write(blob)
        open(os.path.join(out, name + ".proof"), "wb").write(proof)
        open(os.path.join(out, name + ".precommit"), "wb").write(o.preprocessed_commit() or b"")
        if widen_unopened_row:  # the preprocessed round comes last; its only matrix is opened at no point
            t = pc.parse(proof, 4, 4)
            rows = t["opening_proof"]["query_proofs"][1]["input_proof"][-1]["opened_values"]
            assert t["preprocessed_opened_values"] == [[]] and len(rows) == 1
            rows[0].append(0)
            open(os.path.join(out, name + ".width.proof"), "wb").write(pc.serialize(t, 4, 4))
        offs, data = packed
        with open(os.path.join(out, name + ".claims"), "wb") as f:
            f.write(struct.pack("<Q", len(offs) - 1))
            f.write(np.asarray(offs, dtype=np.uint64).tobytes())
            f.write(np.asarray(data, dtype=np.uint32).tobytes())

    with fe.field(fe.BABYBEAR):
        mul, tr7 = fe.mul_air_inputs(), [fe.mul_air_trace(1 << 7)]
        emit("arity1", fe.Params(1, 0, 0, 1, 16, 0, 0), mul, tr7, [])
        emit("arity2", fe.Params(1, 1, 1, 2, 10, 2, 2), mul, tr7, [])
        emit("arity3", fe.Params(2, 0, 0, 3, 12, 3, 4), mul, tr7, [])
        emit("arity6", fe.Params(1, 0, 0, 6, 8, 0, 0), mul, tr7, [])
        emit("caps_final", fe.Params(2, 2, 2, 1, 10, 3, 4), mul, tr7, [])
        emit("evenodd", fe.Params(1, 0, 0, 1, 12, 0, 0), fe.even_odd_inputs(), fe.even_odd_traces(), [[0, 4, 1]])
        emit("evenodd_dead", fe.Params(2, 1, 0, 2, 12, 0, 0), fe.even_odd_inputs(with_dead=True),
             fe.even_odd_traces() + [np.zeros((0, 6), dtype=np.uint64)], [[0, 4, 1]])
        emit("evenodd_dead_table", fe.Params(2, 1, 0, 2, 12, 0, 0), fe.even_odd_inputs() + [fe.squares_inputs()[0]],
             fe.even_odd_traces() + [np.zeros((0, 1), dtype=np.uint64)], [[0, 4, 1]], widen_unopened_row=True)
        one_row = [np.tile(np.array([[3, 4, 5]], dtype=np.uint64), (32, 1)), np.array([[4, 2, 3, 1, 10, 10]], dtype=np.uint64)]
        emit("height1", fe.Params(2, 1, 0, 3, 10, 0, 0), fe.verifier_test_inputs(), one_row, [])
        emit("squares_mixed", fe.Params(2, 1, 0, 2, 10, 0, 0), fe.verifier_test_inputs(), fe.verifier_test_traces(0), [])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mutations", type=int, default=150)
    ap.add_argument("--keep", default=None)
    a = ap.parse_args()
    pkg = load_package()
    work = a.keep or tempfile.mkdtemp(prefix="bb_verify_host_check_")
    os.makedirs(work, exist_ok=True)
    scenarios(work)
    exe = os.path.join(work, "bb_verify_host_check")
    lib_dir = os.path.dirname(pkg.LIB_PATH)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-omit-frame-pointer", "-Wno-unused-function", os.path.join(ROOT, "tools", "bb_verify_host_check.hip"), "-o", exe,
                           "-L" + lib_dir, "-lmstark_hip", "-Wl,-rpath," + lib_dir])
    sys.exit(subprocess.call([exe, work, str(a.mutations)]))


if __name__ == "__main__":
    main()
