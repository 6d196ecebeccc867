"""`-m gpu`: an allocation failure at every allocation point of msbb_witness_claims_fill (csrc/claims_fill.h, csrc/bb_fill.hip) on
a call with an input matrix, a keep expression and two compaction tiles, in append mode, with the sweep of
tests/alloc_failure_sweep.py on a context of its own. After every injected failure the claims and the traces are byte-identical
to the start; after the success the claims equal the model's (tests/claims_model_bb.py) and the traces are still what they were."""
import numpy as np
import pytest
import torch  # (before the library opens the device)

import claims_model_bb as cb
from alloc_failure_sweep import own_cache, sweep
from test_gpu_alloc_failures import actx  # noqa: F401  (a context for sweeps alone, with the BabyBear permutation set)

pytestmark = pytest.mark.gpu

# The device allocations of the call, cl_witness_claims_fill in csrc/claims_fill.h - the driver of both fields, so the count is
# the one of tests/test_gpu_claims_alloc_failures.py. In front of the first launch: the code, the output table, the constants and
# the two read-back words, always; the temporary of the pass with the tile counts and the tile offsets, for a keep expression over
# more than one tile; the ingested inputs. Behind the first host wait, when the kept total is known: the new offset and data
# arrays. The witness changes only after the last of them.
ALWAYS, KEEP_TWO_TILES, INPUTS, NEW_ARRAYS = 4, 3, 1, 2


def test_bb_claims_fill_with_inputs_keep_and_two_tiles_appending(pkg, fe, actx):
    import test_gpu_bb_witness_claims as tc

    E = fe.Expr
    n = 2 * tc.TILE
    with own_cache(tc):
        s, pres = tc.lab_system(actx)  # (its systems are keyed without the context: this one stays out of that module's way)
    rng = np.random.default_rng(9700)
    traces = tc.lab_traces(rng, [n, 0])
    start = [[5, 6, 7], [], [cb.P - 1]]
    w = s.witness_from_device([tc.dev32(traces[0]), None], tc.pack(start))
    inputs = np.stack([tc.rand_field(rng, n), rng.integers(0, 3, size=n, dtype=np.uint64)], axis=1)
    prog = tc.lab_program(keep=E.input(1))
    d_inputs = tc.dev32(inputs)
    before = w.claims()
    assert before[0].tolist() == [0, 3, 3, 4] and before[1].tolist() == [5, 6, 7, cb.P - 1]
    want = cb.claims(prog.blob, traces[0], None, inputs, n, before)
    assert len(want[0]) - len(before[0]) == int((inputs[:, 1] != 0).sum()) > tc.TILE  # kept rows in both tiles
    at_least = ALWAYS + KEEP_TWO_TILES + INPUTS + NEW_ARRAYS
    assert at_least == 10

    def unchanged(when):
        got = w.claims()
        assert np.array_equal(got[0], before[0]) and np.array_equal(got[1], before[1]), "claims differ %s" % when
        assert np.array_equal(w.trace(0).astype(np.uint64), traces[0]), "trace differs %s" % when

    def success(rep):
        got = w.claims()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(w.trace(0).astype(np.uint64), traces[0])
        info = pkg.babybear.claims_program_info(prog)
        assert rep.fields() == (n, len(want[0]) - len(before[0]), info["instructions"], info["lds_lanes"]), str(rep)

    unchanged("before the first call")
    sweep(pkg, actx, "bb claims fill with inputs, keep and two tiles, appending, %d rows" % n, lambda: w.fill_claims(0, prog, n, d_inputs, append=True),
          lambda nth: unchanged("after a failed call (allocation %d)" % nth), success, at_least)
