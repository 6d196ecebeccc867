"""CPU tests of ms_blake3_compressions (host code of the library, no device): every compression of BLAKE3(data) as the 32-word
rows that ms_witness_blake3_compressions takes, in the order of blake3_circuit.blake3_compressions (`blake3_new_update_finalize`,
src/test_circuits/blake3.rs:32-352), and the digest."""
import ctypes as C
import importlib

import numpy as np
import pytest

LENGTHS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 3000, 5000, 8192)  # those of test_hasher_against_the_oracles_blake3


@pytest.fixture(scope="module")
def b3(pkg):
    return importlib.import_module("multi_stark_amd.blake3_circuit")


def _data(n):
    return bytes((i * 7 + 3) & 255 for i in range(n))


@pytest.mark.parametrize("n", LENGTHS)
def test_rows_and_digest_equal_the_python_hasher(b3, oracle, n):
    data = _data(n)
    infos, dig = b3.blake3_compressions(data)
    states, digest = b3.compression_states(data)
    assert states.dtype == np.uint32 and states.shape == (len(infos), 32)
    want = np.array([b3.compression_claim(i)[1:33] for i in infos], dtype=np.uint32)
    assert np.array_equal(states, want)
    assert digest == dig == oracle.hash_bytes(data)


def _call(pkg, data, cap_rows, want_digest=True):
    u8p, u32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    buf = np.frombuffer(data + b"\0", dtype=np.uint8)
    rows = np.full((max(cap_rows, 1), 32), 0xA5A5A5A5, dtype=np.uint32)
    digest = np.zeros(32, dtype=np.uint8)
    n = C.c_size_t(12345)
    rc = pkg.lib().ms_blake3_compressions(buf.ctypes.data_as(u8p), C.c_size_t(len(data)), rows.ctypes.data_as(u32p) if cap_rows else None,
                                          C.c_size_t(cap_rows), C.byref(n), digest.ctypes.data_as(u8p) if want_digest else None)
    return rc, n.value, rows, digest.tobytes()


def test_buffer_size_protocol(pkg, b3):
    data = _data(3000)
    infos, dig = b3.blake3_compressions(data)
    want = np.array([b3.compression_claim(i)[1:33] for i in infos], dtype=np.uint32)
    # no room at all: the needed number of rows is reported
    rc, n, _, _ = _call(pkg, data, 0)
    assert (rc, n) == (-3, len(infos)) == (-3, 49)
    # one row short: MS_ERR_BUFFER again, nothing written past the capacity
    rc, n, rows, _ = _call(pkg, data, 48)
    assert (rc, n) == (-3, 49) and np.array_equal(rows[:48], want[:48])
    # exactly enough, and more than enough (the rest of the buffer is left alone); the digest is optional
    rc, n, rows, digest = _call(pkg, data, 49)
    assert (rc, n) == (0, 49) and np.array_equal(rows, want) and digest == dig
    rc, n, rows, _ = _call(pkg, data, 60, want_digest=False)
    assert (rc, n) == (0, 49) and np.array_equal(rows[:49], want) and (rows[49:] == 0xA5A5A5A5).all()
    # a null count is an error, not a crash
    assert pkg.lib().ms_blake3_compressions(None, C.c_size_t(0), None, C.c_size_t(0), None, None) == -1
    assert b"null" in pkg.lib().ms_last_error()
