"""CPU tests: the numpy model of msbb_witness_argsort (tests/argsort_model_bb.py) against the definition written out in plain
Python, and the parts of the call that need no device: msbb_sort_info and the names in the header, the export list and the
Rust binding. The counterpart of test_argsort_model.py."""
import os
import re

import numpy as np

import argsort_model_bb as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = (1 << 31) - (1 << 27) + 1
R = (1 << 32) % P


def by_definition(trace, keys):
    rows = [[int(x) for x in r] for r in trace]
    return sorted(range(len(rows)), key=lambda i: (tuple(rows[i][k] for k in keys), i))


def cases():
    rng = np.random.default_rng(6)
    out = []
    for n, width, keys in [(1, 2, [0]), (2, 2, [1]), (64, 3, [0]), (64, 4, [3, 1, 0]), (300, 9, list(range(8))), (300, 3, [1, 1]), (300, 3, [0, 1])]:
        t = rng.integers(0, P, size=(n, width), dtype=np.uint64)
        t.reshape(-1)[: min(t.size, 4)] = np.array([P - 1, 0, 1 << 27, P - 2], dtype=np.uint64)[: min(t.size, 4)]
        out.append(("random", t, keys))
        few = rng.integers(0, 3, size=(n, width), dtype=np.uint64)
        few[:, keys[0]] |= rng.integers(0, 2, size=n, dtype=np.uint64) << np.uint64(30)  # ties, and the top digit decides
        out.append(("ties", few, keys))
    return out


def test_model_is_the_definition():
    seen = set()
    for name, t, keys in cases():
        seen.add(t.shape[0])
        assert int(t.max()) < P
        want = by_definition(t, keys)
        assert bm.permutation(t, keys).tolist() == want, (name, t.shape, keys)
        dst = [c for c in range(t.shape[1]) if c not in keys]
        if not dst:
            continue
        perm, rank = bm.run(t, keys, dst[0]), bm.run(t, keys, dst[0], rank=True)
        assert perm[:, dst[0]].tolist() == want
        assert [int(rank[r, dst[0]]) for r in want] == list(range(len(want)))
        keep = [c for c in range(t.shape[1]) if c != dst[0]]
        assert np.array_equal(perm[:, keep], t[:, keep]) and np.array_equal(rank[:, keep], t[:, keep])
    assert seen == {1, 2, 64, 300}


def test_canonical_order_is_not_the_order_of_the_montgomery_words():
    """x -> x R mod p with R = 2^32 mod p = 2^28 - 2 is no monotone map: 1 -> R, 8 -> 8 R - p = 2^27 - 17 < R. A column of
    such values sorts one way by what it means and another way by the words in memory; the model sorts by what it means."""
    assert R == (1 << 28) - 2
    col = np.array([8, 1, 9, 0, P - 1, 16, 1, 8], dtype=np.uint64)
    words = np.array([(int(x) * R) % P for x in col], dtype=np.uint64)
    assert np.array_equal(bm.monty(col), words) and int(words.max()) < P
    assert words[1] == R and words[0] == 8 * R - P and words[0] < words[1]
    t = np.stack([col, np.zeros_like(col)], axis=1)
    by_value = bm.permutation(t, [0]).tolist()
    by_word = bm.permutation(np.stack([words, np.zeros_like(col)], axis=1), [0]).tolist()
    assert by_value == [3, 1, 6, 0, 7, 2, 5, 4] == by_definition(t, [0])
    assert by_word != by_value
    assert bm.run(t, [0], 1, rank=True)[:, 1].tolist() == [3, 1, 5, 0, 7, 6, 2, 4]


def test_model_pass_counts():
    t = np.zeros((10, 3), dtype=np.uint64)
    t[:, 0] = 77
    t[:, 1] = np.arange(10)
    t[3, 2] = 0x77 << 24
    assert bm.passes(t, [0]) == (0, 4) and bm.passes(t, [1]) == (1, 3) and bm.passes(t, [0, 1, 2]) == (2, 10)
    t[:, 1] = np.uint64(P - 1) - np.arange(10, dtype=np.uint64) * np.uint64(0x01010101)
    assert bm.passes(t, [1]) == (4, 0) and bm.passes(t, [1, 1]) == (8, 0)


def test_sort_info(pkg):
    info = pkg.babybear.sort_info()
    assert len(info) == 4 and all(isinstance(x, int) and x >= 0 for x in info)
    T, bits, R_, max_keys = info
    assert bits == 8 and max_keys == 8 == bm.MAX_KEYS
    assert T >= 64 and T & (T - 1) == 0


def test_names_in_header_exports_and_binding(pkg):
    bb = pkg.babybear
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mstark_bb.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "bindings", "rust", "mstark_sys.rs")).read()
    for name in ("msbb_witness_argsort", "msbb_sort_info"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in bb.exported_symbols() and hasattr(pkg.lib(), name), name
        assert re.search(r"pub fn %s\(" % name, rs), name
    assert hasattr(bb.Witness, "argsort") and callable(bb.sort_info)
