"""Pcs::open at free opening points and at the kernel dispatch edges of the Goldilocks opening (ms_pcs_open: csrc/prover.hip
pcs_open, csrc/open_plan.h, csrc/open.hip), against the oracle. tests/test_gpu_kernels.py::_pcs_scenario and every whole proof
open at the prover's own pattern - zeta, or (zeta, zeta g) on every matrix; here the points are free: unrelated pairs, a second
matrix that demotes a next pair, reversed pairs, generators of other heights, a one-row trace, matrices / heights / rounds
without points, three points at a height (refused) - and the shapes sit on the dispatch thresholds: the fast route of the
inverse denominators, the row blocks and batches of the barycentric sums, the column loops of both reduced-opening kernels,
the wide kernel with the leaf hashing, the side stream. The case table and what each case reaches: tests/pcs_plan_model.py,
guarded by tests/test_pcs_plan_model.py.

Every case: commit each round on the device and in the oracle (equal caps), observe the caps, sample z, a, b on both
transcripts (equal), open on both: equal opened values, equal FRI bytes, equal transcript state afterwards; both verifiers
accept the device's output and reject it with one word flipped in the opened values of any one matrix."""
import zlib

import numpy as np
import pytest

import pcs_plan_model as M
from __graft_entry__ import load_package
from conftest import P, rand_field

pytestmark = pytest.mark.gpu
_fe = load_package().frontend


def _assert_same_bytes(got, want, what):
    """(asserting on two byte strings themselves makes a failing pytest diff them, which takes minutes: compare first)"""
    same = got == want
    where = "" if same else "lengths %d / %d" % (len(got), len(want)) if len(got) != len(want) else "first at byte %d" % next(
        i for i in range(len(got)) if got[i] != want[i])
    assert same, "%s: bytes differ, %s" % (what, where)


def _params(case):
    return _fe.Params(*case.params)


def _matrices(case, seed):
    shapes = [[(m.log_n, m.width) for m in r] for r in case.rounds]
    rng = np.random.default_rng(zlib.crc32(repr((shapes, seed)).encode()))
    return [[rand_field(rng, (1 << ln, w)) for ln, w in r] for r in shapes]


def _value(oracle, p, base):
    """a symbolic point's value: base * g(k)^e, kept as the fraction e / 2^k of a full turn"""
    z = base[p.base]
    if not p.turn:
        return z
    g = pow(oracle.lib().mso_gl_two_adic_generator(p.turn.denominator.bit_length() - 1), p.turn.numerator, P)
    return (z[0] * g % P, z[1] * g % P)


def _points(oracle, case, base):
    return [[[_value(oracle, p, base) for p in m.points] for m in r] for r in case.rounds]


def _observe_and_sample(ch, caps):
    for cap in caps:
        ch.observe_digests(cap)
    return {"z": ch.sample_ext(), "a": ch.sample_ext(), "b": ch.sample_ext()}


# the oracle's side of a case is computed once and shared between the knob values (and the refusal tests' good case)
_commits, _opens = {}, {}


def _oracle_commit(oracle, case, seed):
    key = (case.params[0], case.params[1], tuple(tuple((m.log_n, m.width) for m in r) for r in case.rounds), seed)
    if key not in _commits:
        while len(_commits) >= 2:  # (the 4096 x 512 cases are 32 MB each: keep the latest two)
            _commits.pop(next(iter(_commits)))
        mats = _matrices(case, seed)
        _commits[key] = (mats, [oracle.Mmcs([oracle.coset_lde_bitrev(m, case.params[0]) for m in r], case.params[1]) for r in mats])
    return _commits[key]


def _oracle_open(oracle, case, seed):
    mats, o_rounds = _oracle_commit(oracle, case, seed)
    if (case.name, seed) not in _opens:
        oc = oracle.Challenger.for_params(_params(case))
        base = _observe_and_sample(oc, [o.cap for o in o_rounds])
        pts = _points(oracle, case, base)
        o_open, o_fri = oracle.pcs_open(_params(case), list(zip(o_rounds, pts)), oc)
        _opens[case.name, seed] = (base, pts, o_open, o_fri, oc.sample_bits(20))
    return (mats, o_rounds) + _opens[case.name, seed]


def _fresh(pkg, oracle, case, caps, base, lib_side):
    c = pkg.Challenger(_params(case)) if lib_side else oracle.Challenger.for_params(_params(case))
    assert _observe_and_sample(c, caps) == base
    return c


def check_once(ctx, pkg, oracle, case, seed=0):
    params = _params(case)
    mats, o_rounds, base, pts, o_open, o_fri, o_bits = _oracle_open(oracle, case, seed)
    g_rounds = [pkg.PcsCommitment(ctx, r, params.log_blowup, params.cap_height) for r in mats]
    caps = [g.cap for g in g_rounds]
    assert caps == [o.cap for o in o_rounds]
    gc = pkg.Challenger(params)
    assert _observe_and_sample(gc, caps) == base
    g_open, g_fri = pkg.pcs_open(ctx, params, list(zip(g_rounds, pts)), gc)
    if not np.array_equal(g_open, o_open):
        bad = np.flatnonzero(g_open != o_open) if g_open.shape == o_open.shape else []
        raise AssertionError("%s: opened values differ (%d of %d words, first at word %s)" % (case.name, len(bad), o_open.size, bad[:1]))
    _assert_same_bytes(g_fri, o_fri, case.name + ": FriProof")
    assert gc.sample_bits(20) == o_bits, "the transcripts end in different states"
    desc = [(cap, [(m.log_n, m.width) for m in r], per) for cap, r, per in zip(caps, case.rounds, pts)]
    assert pkg.pcs_verify(params, desc, g_open, g_fri, _fresh(pkg, oracle, case, caps, base, True)), "the library's verifier rejects"
    assert oracle.pcs_verify(params, desc, g_open, g_fri, _fresh(pkg, oracle, case, caps, base, False)), "the oracle's verifier rejects"
    off = 0
    for r in case.rounds:
        for m in r:
            if m.points:
                bad = g_open.copy()
                bad[off] ^= 1
                assert not pkg.pcs_verify(params, desc, bad, g_fri, _fresh(pkg, oracle, case, caps, base, True)), "flipped word %d: library accepts" % off
                assert not oracle.pcs_verify(params, desc, bad, g_fri, _fresh(pkg, oracle, case, caps, base, False)), "flipped word %d: oracle accepts" % off
            off += 2 * len(m.points) * m.width


def check(ctx, pkg, oracle, monkeypatch, case, knob=None):
    for name, value in M.KNOBS[knob or "none"].items():
        monkeypatch.setenv(name, value)
    # (the side-stream cases alternate two matrix sets: a stale buffer must never pass for this call's values)
    for seed in ((0, 1, 0, 1) if case.alternate else (0,)):
        check_once(ctx, pkg, oracle, case, seed)


@pytest.mark.parametrize("run", [r for r in M.RUNS if not r[0].refused], ids=M.run_id)
def test_open_at_free_points(ctx, pkg, oracle, monkeypatch, run):
    check(ctx, pkg, oracle, monkeypatch, *run)


@pytest.mark.parametrize("case", [c for c in M.CASES if c.refused], ids=lambda c: c.name)
def test_three_points_at_one_height_are_refused(ctx, pkg, oracle, case):
    """ms_pcs_open takes at most two distinct points per LDE height over all rounds, a pair (z, z g) counting as two: a third is
    an error that names the limit (the oracle, like Plonky3, accepts it). The context survives: a good case on it afterwards
    gives the oracle's bytes - from a fresh challenger, the refused call has advanced its own."""
    params = _params(case)
    mats, o_rounds, base, pts, o_open, o_fri, _ = _oracle_open(oracle, case, 0)
    caps = [o.cap for o in o_rounds]
    desc = [(cap, [(m.log_n, m.width) for m in r], per) for cap, r, per in zip(caps, case.rounds, pts)]
    assert oracle.pcs_verify(params, desc, o_open, o_fri, _fresh(pkg, oracle, case, caps, base, False))
    g_rounds = [pkg.PcsCommitment(ctx, r, params.log_blowup, params.cap_height) for r in mats]
    assert [g.cap for g in g_rounds] == caps
    gc = pkg.Challenger(params)
    assert _observe_and_sample(gc, caps) == base
    with pytest.raises(pkg.MstarkError, match=M.REFUSAL_TEXT):
        pkg.pcs_open(ctx, params, list(zip(g_rounds, pts)), gc)
    good = next(c for c in M.CASES if c.name == "unrelated-p%s" % case.name[-1])
    check_once(ctx, pkg, oracle, good)
