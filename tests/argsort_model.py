"""ms_witness_argsort in numpy (the definition is in include/mstark.h): row i comes before row j iff the tuple
(trace[i][k_0], ..., trace[i][k_{m-1}], i) is lexicographically smaller, the cells compared as unsigned 64-bit integers. The
row index is the last component: the order is total, the sort stable, the result unique.
  perm: trace[t][dst] = the row at sorted position t;  rank: trace[r][dst] = the sorted position of row r.
np.lexsort over the uint64 columns with the primary key LAST is that order: it is stable, and uint64 compares unsigned."""
import numpy as np

MAX_KEYS = 8


def permutation(trace, keys):
    """the rows of `trace` (n x width, uint64) in sorted order"""
    trace = np.ascontiguousarray(trace, dtype=np.uint64)
    assert 1 <= len(keys) <= MAX_KEYS and all(0 <= k < trace.shape[1] for k in keys)
    return np.lexsort([trace[:, k] for k in reversed(list(keys))]).astype(np.uint64)


def run(trace, keys, dst, rank=False):
    """the trace after the call: a copy with column dst written, every other cell as it was"""
    assert 0 <= dst < trace.shape[1] and dst not in keys
    perm = permutation(trace, keys)
    out = np.array(trace, dtype=np.uint64, copy=True)
    if rank:
        out[perm.astype(np.int64), dst] = np.arange(trace.shape[0], dtype=np.uint64)
    else:
        out[:, dst] = perm
    return out


def passes(trace, keys):
    """(digit passes run, digit passes skipped) with 8-bit digits: a digit in which all rows share one value is skipped"""
    ran = 0
    for k in keys:
        col = np.ascontiguousarray(trace[:, k], dtype=np.uint64)
        for d in range(8):
            byte = (col >> np.uint64(8 * d)) & np.uint64(0xFF)
            ran += int((byte != byte[0]).any())
    return ran, 8 * len(keys) - ran
