"""The sweep of tests/test_gpu_alloc_failures.py: one call made again and again with Context.debug_fail_alloc(nth) armed for
nth = 1, 2, ... - the nth device allocation from then on throws on the host, before hipMalloc - until the call needs fewer than
nth allocations and returns. Nothing here opens a device."""
import contextlib
import re
import time

ERROR_TEXT = re.compile(r"injected allocation failure|cannot allocate the \d+ bytes of ")
LAST_NTH = 200  # the sweep has to end by a success at some nth <= 200
TIMES = {}      # label -> (failing points, seconds), for the figures of a run (printed by each case)


def sweep(pkg, ctx, label, call, after_failure, after_success, at_least, before=None):
    """call() under every nth. A call that raises must raise pkg.MstarkError (anything else propagates and fails the test) with
    the text of an allocation failure; after_failure(nth) then runs unarmed. The first call that returns ends the sweep:
    after_success(result) runs unarmed. `at_least`: the device allocations on the path the case names - fewer failing points
    mean the case did not take it. before() (optional) runs unarmed in front of every call. -> the number of failing points"""
    t0 = time.perf_counter()
    failures = 0
    for nth in range(1, LAST_NTH + 1):
        error = None
        if before:
            before()
        ctx.debug_fail_alloc(nth)
        try:
            result = call()
        except pkg.MstarkError as e:
            error = e
        finally:
            ctx.debug_fail_alloc(0)
        if error is None:
            after_success(result)
            TIMES[label] = (failures, time.perf_counter() - t0)
            print("%s: %d failing points, %.2f s" % (label, failures, TIMES[label][1]))
            assert failures >= at_least, "%s: %d failing points, the path has %d allocations" % (label, failures, at_least)
            return failures
        assert ERROR_TEXT.search(str(error)), "%s, allocation %d: %s" % (label, nth, error)
        failures += 1
        after_failure(nth)
    raise AssertionError("%s: no success up to allocation %d" % (label, LAST_NTH))


@contextlib.contextmanager
def own_cache(*modules):
    """the GPU modules of these calls keep their systems in a module-level dictionary, keyed without the context, and take the
    context as an argument. Inside this block such a module sees an empty dictionary: what it builds here, on the context of
    the sweeps, stays out of its own tests' way, and what its own tests built on theirs is not handed to the sweeps."""
    saved = [(m, name, getattr(m, name)) for m in modules for name in ("_CACHE", "_SYS") if hasattr(m, name)]
    for m, name, _ in saved:
        setattr(m, name, {})
    try:
        yield
    finally:
        for m, name, value in saved:
            setattr(m, name, value)
