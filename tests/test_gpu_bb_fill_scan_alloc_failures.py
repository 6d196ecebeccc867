"""`-m gpu`: an allocation failure at every allocation point of msbb_witness_fill with scan steps (csrc/bb_fill.hip), with the
sweep of tests/alloc_failure_sweep.py on a context of its own, as test_gpu_alloc_failures.py does for the other
witness-building calls. After every injected failure the traces are byte-identical to the start; after the success they equal
the model (tests/fill_scan_model_bb.py)."""
import numpy as np
import pytest
import torch  # (before the library opens the device)

import fill_scan_model_bb as bsm
from alloc_failure_sweep import own_cache, sweep
from test_gpu_alloc_failures import actx  # noqa: F401  (a context for sweeps alone, with the BabyBear permutation set)

pytestmark = pytest.mark.gpu

# The device allocations of the call, fl_witness_fill in csrc/fill_dev.h (with BbFill of csrc/bb_fill.hip): d_code, d_outs and
# d_consts always; scratch when a group's slot file goes to the global scratch; tmp when there is a scan, and aggs and starts
# when the height is above one scan tile; inp and bad when the program reads inputs. All of them precede the first launch that
# writes the trace (the group loop).
FILL_ALWAYS, FILL_SCRATCH, FILL_SCAN, FILL_TILES, FILL_INPUTS = 3, 1, 1, 2, 2


def test_bb_fill_with_scans(pkg, actx):
    import test_gpu_bb_witness_fill_scan as ts

    bb, fe = pkg.babybear, pkg.frontend
    E = fe.Expr
    T = ts.tile()
    n = 2 * T  # two scan tiles: every temporary of the call exists
    with own_cache(ts):
        s = ts.lab_system(actx)  # (its systems are keyed without the context: this one stays out of that module's way)
    with fe.field(fe.BABYBEAR):
        m, x = E.input(0), E.input(1)
        leaves = [fe.bits(x + k, k % 25, 1 + k // 50) for k in range(300)]  # 300 live leaves: the coefficient pass leaves LDS
        add = leaves[-1]
        for leaf in reversed(leaves[:-1]):
            add = leaf - add
        # group 0 overwrites column 0 with a function of itself - a second run gives another witness - and the scan, a later
        # group, reads what group 0 wrote; a last group reads the scan's next row
        prog = bb.compile_fill(2, 0, 2, [(0, E.main(0) * m + 1), (1, fe.scan(E.main(0), add, init=5)), (0, E.main_next(1) - E.main(0))])
    assert bb.fill_scan_info(prog) == (1, 3, 0, T) and bb.fill_program_info(prog)["lds_lanes"] == 0
    at_least = FILL_ALWAYS + FILL_SCRATCH + FILL_SCAN + FILL_TILES + FILL_INPUTS
    assert at_least == 9
    rng = np.random.default_rng(3400)
    start = [rng.integers(0, bsm.P, size=(n, w), dtype=np.uint64) for w in ts.WIDTHS]
    ci = 1
    inputs = ts.operands(rng, n, 2, T)
    once_run = bsm.run(prog.blob, start[ci], None, inputs.astype(np.uint64))
    assert not np.array_equal(bsm.run(prog.blob, once_run, None, inputs.astype(np.uint64)), once_run)  # not idempotent
    want = [once_run if c == ci else t for c, t in enumerate(start)]
    w = s.witness_from_device([ts.dev32(t) for t in start], ts.pack([]))
    d_inputs = ts.dev(inputs)

    def unchanged(state, when):
        for c, t in enumerate(state):
            assert ts.same(w.trace(c), t), "trace differs %s: circuit %d" % (when, c)

    def success(rep):
        unchanged(want, "after the successful call")
        info = bb.fill_program_info(prog)
        assert rep.fields() == (n, len(prog.steps), info["instructions"], 0), str(rep)

    unchanged(start, "before the first call")
    sweep(pkg, actx, "bb fill with scans %d rows" % n, lambda: w.fill(ci, prog, d_inputs),
          lambda nth: unchanged(start, "after a failed call (allocation %d)" % nth), success, at_least)
