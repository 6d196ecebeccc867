"""msbb_witness_argsort in numpy: tests/argsort_model.py restated for the BabyBear configuration (the definition is the "sorting
permutation" section of include/mstark.h read over p = 2^31 - 2^27 + 1; include/mstark_bb.h lists what differs). Traces are the
CANONICAL values, as msbb_witness_trace shows them, held as uint64: the uint64 comparison of values below 2^31 is the canonical
order, so `permutation` and `run` are the other model's. A key has four 8-bit digits: the bytes above the fourth are constant
zero, never run in the 8-digit model, and are not counted here."""
import numpy as np

import argsort_model as am

P = (1 << 31) - (1 << 27) + 1
R = (1 << 32) % P  # the Montgomery word of a canonical x is x * R mod p
MAX_KEYS = am.MAX_KEYS
DIGITS = 4

permutation = am.permutation
run = am.run


def passes(trace, keys):
    """(digit passes run, digit passes skipped) with four 8-bit digits per key column"""
    trace = np.ascontiguousarray(trace, dtype=np.uint64)
    assert int(trace[:, list(keys)].max()) < P
    ran = am.passes(trace, keys)[0]
    return ran, DIGITS * len(keys) - ran


def monty(values):
    """the Montgomery words of canonical values, as they lie in device memory"""
    return (np.asarray(values, dtype=np.uint64) * np.uint64(R)) % np.uint64(P)  # (below 2^31 * 2^28: no overflow)
