"""`-m gpu`: an allocation failure at every allocation point of ms_witness_fill on a program with a peer read, an input matrix
and a scan (csrc/fill.hip), with the sweep of tests/alloc_failure_sweep.py on a context of its own, as
test_gpu_bb_fill_scan_alloc_failures.py does for the other field. After every injected failure the traces of ALL circuits are
byte-identical to the start and the text names the bytes; after the success the filled circuit equals the model
(tests/fill_peer_model.py) and the peers are still what they were."""
import numpy as np
import pytest
import torch  # (before the library opens the device)

import fill_peer_model as pm
from alloc_failure_sweep import own_cache, sweep

pytestmark = pytest.mark.gpu

# The device allocations of the call, fl_witness_fill in csrc/fill_dev.h: d_code, d_outs and d_consts always; tmp when there is a scan, and aggs
# and starts when the height is above one scan tile; inp and bad when the program reads inputs. Resolving the peers allocates
# nothing. All of them precede the first launch that writes the trace.
FILL_ALWAYS, FILL_SCAN, FILL_TILES, FILL_INPUTS = 3, 1, 2, 2


@pytest.fixture(scope="module")
def actx(pkg):
    """the context of the sweep"""
    c = pkg.Context(0)
    yield c
    c.debug_fail_alloc(0)


def test_fill_with_a_peer_read_inputs_and_a_scan(pkg, fe, actx):
    import test_gpu_witness_fill_peers as tp

    E = fe.Expr
    T = pkg.fill_scan_info(fe.compile_fill(1, 0, 0, []))[3]
    n = 2 * T  # two scan tiles: every temporary of the call exists
    with own_cache(tp):
        s, pres = tp.lab_system(pkg, fe, actx)  # (its systems are keyed without the context: this one stays out of that module's way)
    ci = 1
    m, x = E.input(0), E.input(1)
    # group 0 overwrites column 0 with a function of itself and of a peer - a second run gives another witness - and the scan, a
    # later group, reads what group 0 wrote next to a taller peer at a computed row; a last group reads the scan's next row
    prog = fe.compile_fill(3, 0, 2, [(0, E.main(0) * m + E.peer(2, 13)), (1, fe.scan(E.main(0), E.peer_at(5, 3, x), init=5)), (0, E.main_next(1) - E.peer_next(0, 0))],
                           peers=s.fill_peers())
    assert pkg.fill_scan_info(prog) == (1, 3, 0, T) and prog.peers == [(0, 1, 1), (2, 1, 14), (5, 1, 14)]
    at_least = FILL_ALWAYS + FILL_SCAN + FILL_TILES + FILL_INPUTS
    assert at_least == 8
    rng = np.random.default_rng(3500)
    heights = [n // 2, n, n, 0, 0, 2 * n, 0, 0]
    start = [rng.integers(0, pm.GOLDILOCKS_P, size=(h, tp.ALL_WIDTHS[c]), dtype=np.uint64) if h else None for c, h in enumerate(heights)]
    inputs = np.stack([rng.integers(0, pm.GOLDILOCKS_P, size=n, dtype=np.uint64), rng.integers(0, 3 * n, size=n, dtype=np.uint64)], axis=1)
    once_run = pm.run(prog.blob, ci, start, pres, inputs)
    again = [once_run if c == ci else t for c, t in enumerate(start)]
    assert not np.array_equal(pm.run(prog.blob, ci, again, pres, inputs), once_run)  # not idempotent
    w = s.witness_from_device([None if t is None else tp.dev(t) for t in start], fe.pack_claims([]))
    d_inputs = tp.dev(inputs)

    def unchanged(state, when):
        for c, t in enumerate(state):
            if t is not None:
                assert np.array_equal(w.trace(c), t), "trace differs %s: circuit %d" % (when, c)

    def success(rep):
        unchanged(again, "after the successful call")
        info = pkg.fill_program_info(prog)
        assert rep.fields() == (n, len(prog.steps), info["instructions"], info["lds_lanes"]), str(rep)

    unchanged(start, "before the first call")
    sweep(pkg, actx, "fill with a peer read, inputs and a scan %d rows" % n, lambda: w.fill(ci, prog, d_inputs),
          lambda nth: unchanged(start, "after a failed call (allocation %d)" % nth), success, at_least)
