"""`-m gpu`: the BLAKE3 compression system's witness generated on the device (ms_witness_blake3_compressions, csrc/witness_gen.hip)
against blake3_circuit.blake3_witness - `Blake3CompressionClaims::witness`, src/test_circuits/blake3.rs:1511-2213 - cell for cell,
trace by trace, and the proofs made from it against the proofs of the uploaded Python witness and of the oracle."""
import importlib

import numpy as np
import pytest

NAMES = ["byte pairs", "u32_xor", "u32_add", "rot8", "rot16", "rot12", "rot7", "g", "compression"]


@pytest.fixture(scope="module")
def b3(pkg):
    return importlib.import_module("multi_stark_amd.blake3_circuit")


@pytest.fixture(scope="module")
def compiled(pkg, fe, b3):
    inputs = b3.blake3_system_inputs()
    return inputs, [fe.compile_circuit(ci) for ci in inputs]


def _system(pkg, fe, ctx, compiled, params):
    s = pkg.System(ctx, fe.system_blob(params, compiled[1]), 9)
    s.params = params
    return s


@pytest.fixture(scope="module")
def system(pkg, fe, ctx, compiled):
    return _system(pkg, fe, ctx, compiled, fe.test_params())  # blowup 2, 64 queries, no proof of work


def _states_of_hash(b3, data):
    return [b3.compression_claim(i)[1:33] for i in b3.blake3_compressions(data)[0]]


_CASES = {
    "n1_reference_vector": lambda b3: [b3.all_claims_cases()[-1][1][0][1:33]],          # H = 1: no compression padding, 8 zero rows under G
    "n3_129_bytes": lambda b3: _states_of_hash(b3, bytes((3 * i + 1) & 255 for i in range(129))),  # H = 4: one padding compression row
    "n49_3000_bytes": lambda b3: _states_of_hash(b3, bytes(range(256)) * 11 + bytes(184)),        # traces (64, 2625) and (4096, 81)
    "n2_all_zero": lambda b3: [[0] * 32] * 2,                                             # every byte pair lands in bin (0, 0)
    "n2_all_ones": lambda b3: [[0xFFFFFFFF] * 32] * 2,                                    # the carry column
}
_reference = {}


def _case(b3, fe, name):
    """(states_in, claims, the Python witness, packed claims): computed once per case and left unchanged"""
    if name not in _reference:
        states = [[int(x) for x in s] for s in _CASES[name](b3)]
        claims = [[b3.COMPRESSION] + s for s in states]
        for c, s in zip(claims, states):  # state_out by the Python rounds on the full 32-word state (words 8..11 are free)
            st = list(s)
            b3._rounds(st)
            c += [st[i] ^ st[i + 8] for i in range(8)] + [st[i + 8] ^ s[i] for i in range(8)]
        _reference[name] = (np.array(states, dtype=np.uint32), claims, b3.blake3_witness(claims), fe.pack_claims(claims))
    return _reference[name]


def _check_traces(w, traces):
    for ci, want in enumerate(traces):
        got = w.trace(ci)
        assert got.shape == want.shape, (NAMES[ci], got.shape, want.shape)
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            r, c = (int(x) for x in bad[0])
            raise AssertionError("%s: %d cells differ, the first at row %d column %d: %d, expected %d" % (NAMES[ci], len(bad), r, c, got[r, c], want[r, c]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(_CASES))
def test_device_witness_equals_the_python_witness(pkg, fe, b3, system, oracle, name):
    states, claims, traces, packed = _case(b3, fe, name)
    n = len(claims)
    H = 1 << (n - 1).bit_length()
    assert [t.shape[0] for t in traces] == [65536, 512 * H, 512 * H, 64 * H, 64 * H, 64 * H, 64 * H, 64 * H, H]
    w = system.blake3_witness_on_device(states)
    assert w.rows == sum(t.shape[0] for t in traces)
    assert np.array_equal(w.states_out, np.array([c[33:] for c in claims], dtype=np.uint32))
    if name == "n1_reference_vector":
        assert claims == b3.all_claims_cases()[-1][1]  # its known state_out
        assert not traces[7][56:].any() and traces[7][:56, 0].all()
    if name == "n3_129_bytes":
        assert H == 4 and not traces[8][3].any() and traces[7][3 * 56:4 * 56, 0].all() and not traces[7][3 * 56:, 1:].any()  # multiplicity-1 zero work
    if name == "n2_all_ones":
        assert traces[2][:, 12].any()
    _check_traces(w, traces)
    proof = system.prove_multiple_claims(w).to_bytes()
    assert proof == system.prove_multiple_claims(system.witness(traces, packed)).to_bytes()
    assert system.verify_multiple_claims(packed, proof) == 0
    if name == "n3_129_bytes":
        assert proof == oracle.System(system.blob).prove(traces, packed)
    assert system.prove_multiple_claims(w).to_bytes() == proof  # the witness is not consumed


@pytest.mark.gpu
@pytest.mark.parametrize("no_jit", [False, True])
def test_bench_parameters_and_interpreter_kernels(pkg, fe, b3, ctx, compiled, monkeypatch, no_jit):
    """n = 49 again with the bench parameters (blowup 4, proof of work), and with MSAMD_NO_JIT=1: no circuit has a trace-fed stage-2
    kernel then, so the small circuits' lookup values come from lookup_values_device and the compression circuit's from the
    generator"""
    states, claims, traces, packed = _case(b3, fe, "n49_3000_bytes")
    if no_jit:
        monkeypatch.setenv("MSAMD_NO_JIT", "1")  # acts at System::new
    g = _system(pkg, fe, ctx, compiled, fe.bench_params())
    if no_jit:
        assert [g.circuit_kernels(ci) for ci in range(9)] == [0] * 9
    w = g.blake3_witness_on_device(states)
    _check_traces(w, traces)
    proof = g.prove_multiple_claims(w).to_bytes()
    assert proof == g.prove_multiple_claims(g.witness(traces, packed)).to_bytes()
    assert g.verify_multiple_claims(packed, proof) == 0


@pytest.mark.gpu
def test_refusals(pkg, fe, b3, ctx, system):
    with pytest.raises(pkg.MstarkError, match="bad size"):
        system.blake3_witness_on_device(np.zeros((0, 32), dtype=np.uint32))
    bench = pkg.System.new(ctx, fe.test_params(), fe.u32_add_system_inputs())  # [ByteTable, U32Add]
    with pytest.raises(pkg.MstarkError, match="not the nine-circuit BLAKE3"):
        bench.blake3_witness_on_device(np.zeros((2, 32), dtype=np.uint32))
    # 2^17 + 1 claims: the u32 traces would be 2^27 rows, above NTT_MAX_LOG = 26. Refused before any allocation: an allocation
    # would raise the injected failure instead
    ctx.debug_fail_alloc(1)
    try:
        with pytest.raises(pkg.MstarkError, match="bad size"):
            system.blake3_witness_on_device(np.zeros(((1 << 17) + 1, 32), dtype=np.uint32))
    finally:
        ctx.debug_fail_alloc(0)
    # a host-resident witness has no device traces to read back
    states, claims, traces, packed = _case(b3, fe, "n1_reference_vector")
    hw = system.host_witness(traces, packed)
    with pytest.raises(pkg.MstarkError, match="host-resident"):
        hw.trace(0)
    # and the uploaded one gives back what was uploaded
    assert np.array_equal(system.witness(traces, packed).trace(7), traces[7])
