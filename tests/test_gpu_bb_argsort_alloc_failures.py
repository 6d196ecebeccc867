"""`-m gpu`: an allocation failure at every allocation point of msbb_witness_argsort (csrc/bb_argsort.hip), with the sweep of
tests/alloc_failure_sweep.py on a context of its own, as test_gpu_alloc_failures.py does for the other witness-building calls.
After every injected failure the traces are byte-identical; after the success they equal the model
(tests/argsort_model_bb.py)."""
import numpy as np
import pytest
import torch  # (before the library opens the device)

import argsort_model_bb as bm
from alloc_failure_sweep import own_cache, sweep
from test_gpu_alloc_failures import actx  # noqa: F401  (a context for sweeps alone, with the BabyBear permutation set)

pytestmark = pytest.mark.gpu

# The device allocations of witness_argsort, csrc/bb_argsort.hip: keys_a (l. 113), slots and d_hist (l. 114) before the call's
# host wait (l. 121); keys_b (l. 136), idx_a and idx_b (l. 137) and counts (l. 138) after it, and only when some digit pass
# runs. The first write to the trace is the last launch (bas_final_k, l. 157).
SORT_BEFORE_WAIT, SORT_AFTER_WAIT = 3, 4


@pytest.mark.parametrize("keys", ["field", "constant"])
def test_bb_argsort(pkg, actx, keys):
    import test_gpu_bb_witness_argsort as ta

    bb = pkg.babybear
    n = 2 * bb.sort_info()[0]
    with own_cache(ta):
        s = ta.lab_system(actx)  # (its systems are keyed without the context: this one stays out of that module's way)
    rng = np.random.default_rng(3300)
    start = [rng.integers(0, bm.P, size=(n, w), dtype=np.uint64) for w in ta.WIDTHS]
    if keys == "constant":
        start[2][:, 13] = 0x01234567
    ci, cols, dst, rank = 2, [13], 7, keys == "constant"
    want = [bm.run(t, cols, dst, rank) if c == ci else t for c, t in enumerate(start)]
    passes, skipped = bm.passes(start[ci], cols)
    assert passes == (4 if keys == "field" else 0)
    at_least = SORT_BEFORE_WAIT + (SORT_AFTER_WAIT if passes else 0)
    w = s.witness_from_device([ta.dev32(t) for t in start], ta.pack([]))

    def unchanged(state, when):
        for c, t in enumerate(state):
            assert ta.same(w.trace(c), t), "trace differs %s: circuit %d" % (when, c)

    def success(rep):
        unchanged(want, "after the successful call")
        assert rep.fields() == (n, len(cols), passes, skipped), str(rep)

    unchanged(start, "before the first call")
    sweep(pkg, actx, "bb argsort %d rows %s key" % (n, keys), lambda: w.argsort(ci, cols, dst, rank=rank),
          lambda nth: unchanged(start, "after a failed call (allocation %d)" % nth), success, at_least)
