"""CPU tests: the numpy model of ms_witness_argsort (tests/argsort_model.py) against the definition written out in plain Python,
and the parts of the call that need no device: ms_sort_info and the names in the header, the export list and the Rust binding."""
import os
import re

import numpy as np

import argsort_model as am

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = (1 << 64) - (1 << 32) + 1


def by_definition(trace, keys):
    rows = [[int(x) for x in r] for r in trace]
    return sorted(range(len(rows)), key=lambda i: (tuple(rows[i][k] for k in keys), i))


def cases():
    rng = np.random.default_rng(5)
    out = []
    for n, width, keys in [(1, 2, [0]), (2, 2, [1]), (7, 3, [2, 0]), (64, 3, [0]), (65, 4, [3, 1, 0]), (200, 9, list(range(8))), (300, 3, [1, 1]),
                           (257, 3, [0, 1])]:
        t = rng.integers(0, 1 << 64, size=(n, width), dtype=np.uint64)  # any 64-bit word: about half have bit 63 set
        out.append(("random", t, keys))
        few = rng.integers(0, 3, size=(n, width), dtype=np.uint64)
        few[:, keys[0]] |= rng.integers(0, 2, size=n, dtype=np.uint64) << np.uint64(63)  # ties, and bit 63 decides
        out.append(("ties", few, keys))
    return out


def test_model_is_the_definition():
    for name, t, keys in cases():
        want = by_definition(t, keys)
        assert am.permutation(t, keys).tolist() == want, (name, t.shape, keys)
        dst = [c for c in range(t.shape[1]) if c not in keys]
        if not dst:
            continue
        perm, rank = am.run(t, keys, dst[0]), am.run(t, keys, dst[0], rank=True)
        assert perm[:, dst[0]].tolist() == want
        assert [int(rank[r, dst[0]]) for r in want] == list(range(len(want)))
        keep = [c for c in range(t.shape[1]) if c != dst[0]]
        assert np.array_equal(perm[:, keep], t[:, keep]) and np.array_equal(rank[:, keep], t[:, keep])


def test_unsigned_and_stable():
    t = np.array([[1 << 63, 0], [1, 0], [1 << 63, 0], [P - 1, 0], [0, 0], [1, 0]], dtype=np.uint64)
    assert am.permutation(t, [0]).tolist() == [4, 1, 5, 0, 2, 3]
    assert am.run(t, [0], 1, rank=True)[:, 1].tolist() == [3, 1, 4, 5, 0, 2]


def test_model_pass_counts():
    t = np.zeros((10, 3), dtype=np.uint64)
    t[:, 0] = 77
    t[:, 1] = np.arange(10)
    t[3, 2] = 1 << 56
    assert am.passes(t, [0]) == (0, 8) and am.passes(t, [1]) == (1, 7) and am.passes(t, [0, 1, 2]) == (2, 22)


def test_sort_info(pkg):
    info = pkg.sort_info()
    assert len(info) == 4 and all(isinstance(x, int) and x >= 0 for x in info)
    T, bits, R, max_keys = info
    assert bits == 8 and max_keys == 8 == am.MAX_KEYS
    assert T >= 64 and T & (T - 1) == 0


def test_names_in_header_exports_and_binding(pkg):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mstark.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "bindings", "rust", "mstark_sys.rs")).read()
    for name in ("ms_witness_argsort", "ms_sort_info"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in pkg.exported_symbols() and hasattr(pkg.lib(), name), name
        assert re.search(r"pub fn %s\(" % name, rs), name
    assert "MS_SORT_PERM 0" in header and "MS_SORT_RANK 1" in header
    assert (pkg.SORT_PERM, pkg.SORT_RANK) == (0, 1) and hasattr(pkg.SystemWitness, "argsort")
    names = [pkg.lib().ms_kernel_name(i).decode() for i in range(pkg.lib().ms_kernel_count())]
    assert "witness_argsort" in names
