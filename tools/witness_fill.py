"""ms_witness_fill from the command line: the bench workload ([ByteTable, U32Add]) made three ways at a chosen size, timed
alternately in one run.
  python tools/witness_fill.py [--log-size 20] [--reps 9]
Part 1: a witness of zero traces in HBM is filled from an n x 2 uint32 tensor of (x, y) pairs by the U32Add fill program
(frontend.u32_add_fill_program), ByteTable's column is derived (ms_witness_derive_multiplicities), and the result is compared with
the host builder's traces and, proof bytes against proof bytes, with the witness of the hand-written generator.
Part 2, three routes to the same witness, alternating inside every repetition:
  fill      ms_witness_fill of U32Add from the tensor, then ms_witness_derive_multiplicities; the witness (zero traces, the
            claims) exists beforehand, as it does for a caller who fills one witness again and again
  generator ms_witness_u32_add_bench: the hand-written kernel, which also makes the pairs, the claims and the witness itself
  host      frontend._u32_add_traces (numpy) and ms_witness_create (upload, from_stage_1); the pairs exist beforehand
ms_witness_fill alone (followed by a synchronisation) is a line of its own.
  python tools/witness_fill.py --config babybear [--log-size 20] [--reps 9]
--config babybear: msbb_witness_fill on the same workload authored over BabyBear (Poseidon2, test parameters; the claims' u32
words reduced mod p). U32Add is filled from an n x 4 uint16 tensor of the pairs' 16-bit halves by
frontend.u32_add_halves_fill_program (a field below 2^31 cannot hold x + y), ByteTable's column is derived
(msbb_witness_derive_multiplicities), and the result is compared with the host builder's traces and, proof bytes against proof
bytes, with the host-built witness. There is no BabyBear generator in HBM, so two routes alternate: fill + derive (and
msbb_witness_fill alone) against the host route, frontend._u32_add_traces (numpy) and msbb_witness_create.
  python tools/witness_fill.py --scan [--log-size 20] [--reps 9]
--scan: the price of scan steps. A test circuit of 16 columns is filled by the U32Add program plus a Horner accumulator
(acc' = acc * alpha + the sum word) and a running sum of the carries; the routes alternate: ms_witness_fill with the two scans,
the same program without them (the difference is what the scans cost), the running sum alone in the additive form (multiplier
the constant 1) and in the affine form (multiplier an input column of ones), and the host route the scans replace -
ms_witness_trace, one sequential loop over the rows, ms_witness_create.
  python tools/witness_fill.py --scan --config babybear [--log-size 20] [--reps 9]
the same leg over BabyBear (msbb_witness_fill): the halves program plus a base-field Horner accumulator and a running sum of the
carries, with and without the scans, the running sum alone in both forms (no inputs: the multiplier of the affine form is the
activity column, all ones), and the host route - msbb_witness_trace, numpy and one sequential loop, msbb_witness_create. The
bytes each scan moves by its layout (28 per row in the affine form, 16 in the additive, plus what its coefficient pass reads)
over the measured time is printed next to them; it is no share of a peak.
  python tools/witness_fill.py --gather [--config babybear] [--log-size 20] [--reps 9]
--gather: the price of an indexed read (frontend.Expr.main_at). A test circuit of 4 columns - a value, the identity index, a
random permutation, and the column that is written - is filled by three one-step programs in turn: the value through the
identity index, the value through the permutation, and the ordinary offset-0 copy. None reads inputs, so a call is the program
upload and one launch of the fill kernel.
  python tools/witness_fill.py --alone [--log-size 20] [--reps 9]
--alone: ms_witness_fill of U32Add from the pairs and nothing else in the process: the line by which two builds are compared,
one process each, in turn.
  python tools/witness_fill.py --peers [--log-size 20] [--reps 9]
--peers: the price of a peer read (frontend.Expr.peer / peer_at). A lab system of two circuits: A holds a value and a random
permutation, B the same two columns and the column that is written. One-step programs fill B's column in turn: A's value at the
thread's row (peer), A's value through the permutation (peer_at), the same two reads of B's own columns (main, main_at), and
the host route the peer reads replace - ms_witness_trace of A, the upload of that matrix, and input_at through the permutation.
Each result is compared with numpy.
  python tools/witness_fill.py --claims [--log-size 20] [--reps 9]
--claims: the claims of the bench workload, [1, x, y, z] per addition, built on the device from the filled trace
(ms_witness_claims_fill with frontend.u32_add_claims_program). The routes alternate: fill_claims alone without a keep expression
(the pass writes the claims where they stay) and with an all-ones keep (the activity column: every row is kept, so the compaction
moves the most it can); the whole device route, fill + fill_claims + derive_multiplicities; the host route it replaces -
ms_witness_trace, numpy, and a new ms_witness_create_device from the traces in HBM with the claims given by the host; and the
hand-written generator. The compaction's time is the difference of the two fill_claims lines, printed next to the bytes its
layout states (8 (W + 1) written and read and 8 W written per kept row); it is no share of a peak.
  python tools/witness_fill.py --claims --config babybear [--log-size 20] [--reps 9] [--width 4|49]
the same call over BabyBear (msbb_witness_claims_fill): the route on the bench workload, checked against the host builder and the
host-built witness's proof; then, in a lab circuit of 14 + W columns (W = 4: the bench claims, W = 49: as wide as the BLAKE3
system's), the claims call without keep next to msbb_witness_fill assigning the same W expressions to W columns - one
interpreter, row-major stores W words apart against contiguous column-major ones - and next to the read-back of the list alone;
then the keep compaction at densities 1/64, 1/2 and 1 (profile class witness_claims) against its stated bytes. --width runs one
width alone, so that a kernel trace of the run tells the two passes apart by name.
Timing: wall time of each route (all return synchronised), alternating after two warm-up rounds; median, minimum and maximum are
printed. No figure here is a share of peak."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="goldilocks", choices=["goldilocks", "babybear"])
ap.add_argument("--log-size", type=int, default=20)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--scan", action="store_true", help="the scan-step leg (both configurations)")
ap.add_argument("--gather", action="store_true", help="the indexed-read leg (both configurations)")
ap.add_argument("--peers", action="store_true", help="the peer-read leg (Goldilocks)")
ap.add_argument("--claims", action="store_true", help="ms_witness_claims_fill on the bench workload (--config babybear: msbb_witness_claims_fill)")
ap.add_argument("--width", type=int, default=0, choices=[0, 4, 49], help="--claims --config babybear: one claim width alone (for a kernel trace)")
ap.add_argument("--alone", action="store_true", help="ms_witness_fill of U32Add alone in the process (Goldilocks)")
args = ap.parse_args()

pkg = load_package()
fe = pkg.frontend
ctx = pkg.Context(0)
n = 1 << args.log_size
TARGETS = [(0, 0)]


def timed(fns, reps):
    out = [[] for _ in fns]
    for i in range(reps + 2):
        for fn, o in zip(fns, out):
            ctx.sync()
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            dt = 1e3 * (time.perf_counter() - t)
            if i >= 2:
                o.append(dt)
    return out


def line(what, v):
    print("%-52s median %9.3f ms  (min %.3f, max %.3f, %d calls)" % (what, statistics.median(v), min(v), max(v), len(v)), flush=True)


def babybear():
    bb = pkg.babybear
    k = fe.poseidon2_constants()
    bb.set_poseidon2(ctx, k)
    xs, ys = fe.xorshift_pairs(n)
    with fe.field(fe.BABYBEAR):
        system = bb.System.new(ctx, fe.test_params(), fe.u32_add_system_inputs(), k)
        traces, claims = fe._u32_add_traces(xs, ys, n)
        packed = fe.pack_claims(claims)  # (a 2-D array: reduced mod p)
        prog = fe.u32_add_halves_fill_program(n)
    print("fill program: %d nodes, %d steps; %s" % (len(prog.nodes), len(prog.steps), bb.fill_program_info(prog)))
    m16, s16 = np.uint64(0xFFFF), np.uint64(16)
    halves = torch.from_numpy(np.stack([xs & m16, xs >> s16, ys & m16, ys >> s16], axis=1).astype(np.uint16).view(np.int16)).cuda()
    w = system.witness_from_device([torch.zeros(t.shape, dtype=torch.int32, device="cuda") for t in traces], packed)

    rep = w.fill(1, prog, halves)
    dm = w.derive_multiplicities(TARGETS)
    print("u32add over BabyBear at 2^%d additions, U32Add filled from the halves: %s" % (args.log_size, rep))
    print(dm)
    same = bool(np.array_equal(w.trace(0), traces[0])) and bool(np.array_equal(w.trace(1), traces[1]))
    host = system.witness(traces, packed)
    proof = system.prove_multiple_claims(w).to_bytes()
    same_proof = proof == system.prove_multiple_claims(host).to_bytes()
    print("traces equal the host builder's: %s; proof equals the host-built witness's: %s; check().verdict: %d" % (same, same_proof, w.check().verdict),
          flush=True)
    assert same and same_proof and dm.ok
    del host

    print("\n# two routes to the same witness, alternating")
    state = {}

    def fill_route():
        w.fill(1, prog, halves)
        w.derive_multiplicities(TARGETS)

    def fill_alone():
        w.fill(1, prog, halves)
        ctx.sync()

    def host_traces():
        state["traces"] = fe._u32_add_traces(xs, ys, n)[0]

    def host_create():
        state["host"] = None  # (the previous upload's memory goes back first)
        state["host"] = system.witness(state["traces"], packed)

    t_fill, t_alone, t_tr, t_cr = timed([fill_route, fill_alone, host_traces, host_create], args.reps)
    line("fill: msbb_witness_fill + derive_multiplicities", t_fill)
    line("      msbb_witness_fill alone", t_alone)
    line("host: frontend._u32_add_traces", t_tr)
    line("host: msbb_witness_create (both traces)", t_cr)
    total = [a + b for a, b in zip(t_tr, t_cr)]
    line("host route, the two steps together", total)
    print("host route / fill route = %.1f" % (statistics.median(total) / statistics.median(t_fill)))
    assert np.array_equal(w.trace(1), traces[1]) and np.array_equal(w.trace(0), traces[0])
    state.clear()  # witnesses go before their system


def scan_leg():
    """--scan: what scan steps cost. One circuit of 16 columns: the 14 of U32Add, a Horner accumulator over the sum words
    (column 14) and a running sum of the carries (column 15)."""
    E = fe.Expr
    alpha = (1 << 32) + 3
    x, y, one = E.input(0), E.input(1), E.input(2)
    s = x + y
    plain = [(k, fe.bits(x, 8 * k, 8)) for k in range(4)] + [(4 + k, fe.bits(y, 8 * k, 8)) for k in range(4)]
    plain += [(8 + k, fe.bits(s, 8 * k, 8)) for k in range(4)] + [(12, fe.bits(s, 32, 1)), (13, fe.lt(E.row(), n))]
    z = E.main(8) + E.main(9) * 256 + E.main(10) * 65536 + E.main(11) * (1 << 24)
    scans = [(14, fe.scan(alpha, z)), (15, fe.running_sum(E.main(12)))]
    prog_scans, prog_plain = fe.compile_fill(16, 0, 3, plain + scans), fe.compile_fill(16, 0, 3, plain)
    sum_additive = fe.compile_fill(16, 0, 3, [(15, fe.running_sum(E.main(12)))])
    sum_affine = fe.compile_fill(16, 0, 3, [(15, fe.scan(one, E.main(12)))])  # the multiplier as a column of ones: the affine form
    for name, p in (("with the two scans", prog_scans), ("without them", prog_plain), ("running sum, additive", sum_additive),
                    ("running sum, affine", sum_affine)):
        print("program %-24s %d steps; %s; scan info %s" % (name + ":", len(p.steps), pkg.fill_program_info(p), pkg.fill_scan_info(p)))
    system = pkg.System.new(ctx, fe.bench_params(), [fe.CircuitInputs(16, None, [E.main(12) * E.main(12) - E.main(12)], [], [])])
    xs, ys = fe.xorshift_pairs(n)
    packed = fe.pack_claims([])
    inputs = torch.from_numpy(np.stack([xs, ys, np.ones_like(xs)], axis=1).astype(np.uint32).view(np.int32)).cuda()
    w = system.witness_from_device([torch.zeros((n, 16), dtype=torch.int64, device="cuda")], packed)

    def host_loop(t):
        """the two columns as the host makes them: one sequential loop over the rows"""
        zs = (t[:, 8] + t[:, 9] * 256 + t[:, 10] * 65536 + t[:, 11] * (1 << 24)).tolist()
        cs = t[:, 12].tolist()
        acc, run, p = 0, 0, fe.P
        h, r = [0] * n, [0] * n
        for i in range(n):
            h[i], r[i] = acc, run
            acc, run = (alpha * acc + zs[i]) % p, run + cs[i]
        t[:, 14], t[:, 15] = np.array(h, dtype=np.uint64), np.array(r, dtype=np.uint64)
        return t

    rep = w.fill(0, prog_scans, inputs)
    print("2^%d rows, filled with the scans: %s" % (args.log_size, rep))
    want = np.zeros((n, 16), dtype=np.uint64)
    want[:, :14] = fe._u32_add_traces(xs, ys, n)[0][1]
    want = host_loop(want)
    same = bool(np.array_equal(w.trace(0), want))
    w.fill(0, sum_affine, inputs)
    same_affine = bool(np.array_equal(w.trace(0), want))
    print("trace equals the host's: %s; the running sum again in the affine form: %s" % (same, same_affine), flush=True)
    assert same and same_affine

    print("\n# the routes, alternating")
    state = {}

    def fill(prog):
        def run():
            w.fill(0, prog, inputs)
            ctx.sync()
        return run

    def host_read():
        state["t"] = w.trace(0)

    def host_scan():
        state["t"] = host_loop(state["t"])

    def host_create():
        state["host"] = None  # (the previous upload's memory goes back first)
        state["host"] = system.witness([state["t"]], packed)

    t_sc, t_pl, t_add, t_aff, t_rd, t_lp, t_cr = timed([fill(prog_scans), fill(prog_plain), fill(sum_additive), fill(sum_affine), host_read, host_scan,
                                                        host_create], args.reps)
    line("ms_witness_fill with the two scans", t_sc)
    line("ms_witness_fill without them", t_pl)
    line("running sum alone, additive form", t_add)
    line("running sum alone, affine form (multiplier column)", t_aff)
    line("host: ms_witness_trace", t_rd)
    line("host: the sequential loop (Python integers)", t_lp)
    line("host: ms_witness_create", t_cr)
    total = [a + b + c for a, b, c in zip(t_rd, t_lp, t_cr)]
    moved = [a + c for a, c in zip(t_rd, t_cr)]
    line("host route, the three steps together", total)
    line("host route without its loop (read back + create)", moved)
    m = statistics.median
    print("the two scans cost %.3f ms; host route / fill = %.0f, without the loop %.1f; affine / additive = %.2f" % (
        m(t_sc) - m(t_pl), m(total) / m(t_sc), m(moved) / m(t_sc), m(t_aff) / m(t_add)))
    assert np.array_equal(w.trace(0), want)
    state.clear()  # witnesses go before their system


def scan_leg_bb():
    """--scan --config babybear: what scan steps cost over BabyBear. One circuit of 16 columns: the 14 of U32Add from the 16-bit
    halves, a Horner accumulator over the sum words (column 14) and a running sum of the carries (column 15)."""
    bb = pkg.babybear
    k = fe.poseidon2_constants()
    bb.set_poseidon2(ctx, k)
    E = fe.Expr
    p = fe.BABYBEAR["P"]
    alpha = (1 << 27) + 3
    with fe.field(fe.BABYBEAR):
        plain = list(zip([d for d, _ in fe.u32_add_halves_fill_program(n).steps], halves_roots(n)))
        z = E.main(8) + E.main(9) * 256 + E.main(10) * 65536 + E.main(11) * (1 << 24)
        scans = [(14, fe.scan(alpha, z)), (15, fe.running_sum(E.main(12)))]
        prog_scans, prog_plain = bb.compile_fill(16, 0, 4, plain + scans), bb.compile_fill(16, 0, 4, plain)
        sum_additive = bb.compile_fill(16, 0, 0, [(15, fe.running_sum(E.main(12)))])
        sum_affine = bb.compile_fill(16, 0, 0, [(15, fe.scan(E.main(13), E.main(12)))])  # the multiplier as a column of ones: the affine form
        system = bb.System.new(ctx, fe.test_params(), [fe.CircuitInputs(16, None, [E.main(12) * E.main(12) - E.main(12)], [], [])], k)
        packed = fe.pack_claims([])
    for name, pr in (("with the two scans", prog_scans), ("without them", prog_plain), ("running sum, additive", sum_additive),
                     ("running sum, affine", sum_affine)):
        print("program %-24s %d steps; %s; scan info %s" % (name + ":", len(pr.steps), bb.fill_program_info(pr), bb.fill_scan_info(pr)))
    xs, ys = fe.xorshift_pairs(n)
    m16, s16 = np.uint64(0xFFFF), np.uint64(16)
    inputs = torch.from_numpy(np.stack([xs & m16, xs >> s16, ys & m16, ys >> s16], axis=1).astype(np.uint16).view(np.int16)).cuda()
    w = system.witness_from_device([torch.zeros((n, 16), dtype=torch.int32, device="cuda")], packed)

    def host_loop(t):
        """the two columns as the host makes them: numpy for the sum words and the running sum, one sequential loop for Horner"""
        t = t.astype(np.uint64)
        zs = ((t[:, 8] + t[:, 9] * 256 + t[:, 10] * 65536 + t[:, 11] * (1 << 24)) % p).tolist()
        acc, h = 0, [0] * n
        for i in range(n):
            h[i] = acc
            acc = (alpha * acc + zs[i]) % p
        t[:, 14] = np.array(h, dtype=np.uint64)
        t[1:, 15] = np.cumsum(t[:-1, 12]) % p
        t[0, 15] = 0
        return t

    rep = w.fill(0, prog_scans, inputs)
    print("2^%d rows, filled with the scans: %s" % (args.log_size, rep))
    with fe.field(fe.BABYBEAR):
        want = np.zeros((n, 16), dtype=np.uint64)
        want[:, :14] = fe._u32_add_traces(xs, ys, n)[0][1]
    want = host_loop(want)
    same = bool(np.array_equal(w.trace(0).astype(np.uint64), want))
    w.fill(0, sum_affine)
    same_affine = bool(np.array_equal(w.trace(0).astype(np.uint64), want))
    print("trace equals the host's: %s; the running sum again in the affine form: %s" % (same, same_affine), flush=True)
    assert same and same_affine

    print("\n# babybear, 2^%d rows: the routes, alternating" % args.log_size)
    state = {}

    def fill(prog, inp):
        def run():
            w.fill(0, prog, inp)
            ctx.sync()
        return run

    def host_read():
        state["t"] = w.trace(0)

    def host_scan():
        state["t"] = host_loop(state["t"])

    def host_create():
        state["host"] = None  # (the previous upload's memory goes back first)
        state["host"] = system.witness([state["t"]], packed)

    t_sc, t_pl, t_add, t_aff, t_rd, t_lp, t_cr = timed([fill(prog_scans, inputs), fill(prog_plain, inputs), fill(sum_additive, None), fill(sum_affine, None),
                                                        host_read, host_scan, host_create], args.reps)
    line("msbb_witness_fill with the two scans", t_sc)
    line("msbb_witness_fill without them", t_pl)
    line("running sum alone, additive form (no inputs)", t_add)
    line("running sum alone, affine form (multiplier column)", t_aff)
    line("host: msbb_witness_trace", t_rd)
    line("host: numpy and the sequential loop (Python integers)", t_lp)
    line("host: msbb_witness_create", t_cr)
    total = [a + b + c for a, b, c in zip(t_rd, t_lp, t_cr)]
    moved = [a + c for a, c in zip(t_rd, t_cr)]
    line("host route, the three steps together", total)
    line("host route without its loop (read back + create)", moved)
    m = statistics.median
    cost = m(t_sc) - m(t_pl)
    print("the two scans cost %.3f ms; host route / fill = %.0f, without the loop %.1f; affine / additive = %.2f" % (
        cost, m(total) / m(t_sc), m(moved) / m(t_sc), m(t_aff) / m(t_add)))
    # bytes by the layout: affine 28 per row and additive 16; the Horner pass reads 4 columns (16), the sum's pass 1 (4)
    both, add_b, aff_b = (28 + 16 + 16 + 4) * n, (16 + 4) * n, (28 + 8) * n
    print("bytes by the layout / time: the two scans %d B/row in %.3f ms = %.0f GB/s; additive alone %d B/row, whole call %.3f ms = %.0f GB/s; "
          "affine alone %d B/row, whole call %.3f ms = %.0f GB/s" % (
              both // n, cost, both / cost / 1e6 if cost > 0 else float("nan"), add_b // n, m(t_add), add_b / m(t_add) / 1e6,
              aff_b // n, m(t_aff), aff_b / m(t_aff) / 1e6))
    assert np.array_equal(w.trace(0).astype(np.uint64), want)
    state.clear()  # witnesses go before their system


def halves_roots(num_adds):
    """the right-hand sides of frontend.u32_add_halves_fill_program, in its order of steps (call under field(BABYBEAR))"""
    E = fe.Expr
    x_lo, x_hi, y_lo, y_hi = (E.input(k) for k in range(4))
    s_lo = x_lo + y_lo
    s_hi = x_hi + y_hi + fe.bits(s_lo, 16, 1)
    roots = []
    for lo, hi in ((x_lo, x_hi), (y_lo, y_hi), (s_lo, s_hi)):
        roots += [fe.bits(lo, 0, 8), fe.bits(lo, 8, 8), fe.bits(hi, 0, 8), fe.bits(hi, 8, 8)]
    return roots + [fe.bits(s_hi, 16, 1), fe.lt(E.row(), num_adds)]


def gather_leg():
    """--gather: what an indexed read costs. One circuit of 4 columns (value, identity index, a random permutation, out); three
    one-step programs write `out` and alternate: the value through the identity index, through the permutation, and as the
    ordinary offset-0 copy. No inputs, so no ingest and no host wait: the call is program upload and one launch."""
    E = fe.Expr
    bb_cfg = args.config == "babybear"
    rng = np.random.default_rng(1)
    if bb_cfg:
        api = pkg.babybear
        k = fe.poseidon2_constants()
        api.set_poseidon2(ctx, k)
        p = fe.BABYBEAR["P"]
    else:
        api, p = pkg, fe.P
    value = rng.integers(0, p, size=n, dtype=np.uint64)
    perm = rng.permutation(n).astype(np.uint64)
    trace = np.stack([value, np.arange(n, dtype=np.uint64), perm, np.zeros(n, dtype=np.uint64)], axis=1)
    with fe.field(fe.BABYBEAR if bb_cfg else fe.GOLDILOCKS):
        inputs = [fe.CircuitInputs(4, None, [E.main(3) * E.main(3) - E.main(3)], [], [])]
        system = api.System.new(ctx, fe.bench_params() if not bb_cfg else fe.test_params(), inputs, *([k] if bb_cfg else []))
        progs = [("identity index: out = main_at(0, main(1))", fe.compile_fill(4, 0, 0, [(3, E.main_at(0, E.main(1)))]), value),
                 ("random permutation: out = main_at(0, main(2))", fe.compile_fill(4, 0, 0, [(3, E.main_at(0, E.main(2)))]), value[perm.astype(np.int64)]),
                 ("ordinary copy: out = main(0)", fe.compile_fill(4, 0, 0, [(3, E.main(0))]), value)]
        packed = fe.pack_claims([])
    on_dev = torch.from_numpy(trace.astype(np.uint32).view(np.int32) if bb_cfg else trace.view(np.int64)).cuda()
    w = system.witness_from_device([on_dev], packed)
    for name, prog, want in progs:
        rep = w.fill(0, prog)
        got = w.trace(0)
        ok = bool(np.array_equal(got[:, 3].astype(np.uint64), want)) and bool(np.array_equal(got[:, :3].astype(np.uint64), trace[:, :3]))
        print("%-48s %s; %s; equals numpy: %s" % (name, api.fill_program_info(prog), rep, ok), flush=True)
        assert ok

    def fill(prog):
        def run():
            w.fill(0, prog)
            ctx.sync()
        return run

    print("\n# %s, 2^%d rows: the three routes, alternating" % (args.config, args.log_size))
    times = timed([fill(prog) for _, prog, _ in progs], args.reps)
    call = "msbb_witness_fill" if bb_cfg else "ms_witness_fill"
    for (name, _, _), t in zip(progs, times):
        line("%s, %s" % (call, name.split(":")[0]), t)
    m = statistics.median
    print("identity / copy = %.2f, permutation / copy = %.2f, permutation / identity = %.2f" % (
        m(times[0]) / m(times[2]), m(times[1]) / m(times[2]), m(times[1]) / m(times[0])))
    del w


def peers_leg():
    """--peers: what a read of another circuit's trace costs, next to the same read of the circuit's own and to the host route"""
    E = fe.Expr
    A, B = 0, 1
    rng = np.random.default_rng(1)
    value = rng.integers(0, fe.P, size=n, dtype=np.uint64)
    perm = rng.permutation(n).astype(np.uint64)
    ta = np.stack([value, perm], axis=1)
    tb = np.stack([value, perm, np.zeros(n, dtype=np.uint64)], axis=1)
    placeholder = lambda w: fe.CircuitInputs(w, None, [E.main(0) * E.main(0) - E.main(0)], [], [])
    system = pkg.System.new(ctx, fe.bench_params(), [placeholder(2), placeholder(3)])
    peers = system.fill_peers()
    permuted = value[perm.astype(np.int64)]
    progs = [("peer: out = peer(A, 0)", fe.compile_fill(3, 0, 0, [(2, E.peer(A, 0))], peers=peers), value),
             ("peer_at: out = peer_at(A, 0, main(1))", fe.compile_fill(3, 0, 0, [(2, E.peer_at(A, 0, E.main(1)))], peers=peers), permuted),
             ("main: out = main(0)", fe.compile_fill(3, 0, 0, [(2, E.main(0))]), value),
             ("main_at: out = main_at(0, main(1))", fe.compile_fill(3, 0, 0, [(2, E.main_at(0, E.main(1)))]), permuted)]
    host_prog = fe.compile_fill(3, 0, 2, [(2, E.input_at(0, E.main(1)))])
    w = system.witness_from_device([torch.from_numpy(ta.view(np.int64)).cuda(), torch.from_numpy(tb.view(np.int64)).cuda()], fe.pack_claims([]))

    def clear():
        w.fill(B, fe.compile_fill(3, 0, 0, [(2, E.const(0))]))

    def host_route():
        a = w.trace(A)                                    # device -> host
        w.fill(B, host_prog, torch.from_numpy(a.view(np.int64)).cuda())  # host -> device, and the indexed read of the inputs
        ctx.sync()

    for name, prog, want in progs + [("host: trace(A), upload, input_at(0, main(1))", None, permuted)]:
        clear()
        if prog is None:
            host_route()
            rep, info = "", pkg.fill_program_info(host_prog)
        else:
            rep, info = w.fill(B, prog), pkg.fill_program_info(prog)
        got = w.trace(B)
        ok = bool(np.array_equal(got[:, 2], want)) and bool(np.array_equal(got[:, :2], tb[:, :2])) and bool(np.array_equal(w.trace(A), ta))
        print("%-48s %s; %s; peers %s; equals numpy: %s" % (name, info, rep, pkg.fill_peer_info(prog or host_prog), ok), flush=True)
        assert ok

    def fill(prog):
        def run():
            w.fill(B, prog)
            ctx.sync()
        return run

    print("\n# goldilocks, 2^%d rows: the routes, alternating" % args.log_size)
    times = timed([fill(prog) for _, prog, _ in progs] + [host_route], args.reps)
    for (name, _, _), t in zip(progs, times):
        line("ms_witness_fill, %s" % name.split(":")[0], t)
    line("host route: ms_witness_trace, upload, input_at", times[4])
    m = statistics.median
    print("peer / main = %.2f, peer_at / main_at = %.2f, host route / peer_at = %.1f" % (
        m(times[0]) / m(times[2]), m(times[1]) / m(times[3]), m(times[4]) / m(times[1])))
    del w


def alone_leg():
    """--alone: ms_witness_fill of U32Add from the pairs and nothing else in the process - the figure to compare two builds by"""
    system = pkg.System.new(ctx, fe.bench_params(), fe.u32_add_system_inputs())
    xs, ys = fe.xorshift_pairs(n)
    prog = fe.u32_add_fill_program(n)
    pairs = torch.from_numpy(np.stack([xs, ys], axis=1).astype(np.uint32).view(np.int32)).cuda()
    w = system.witness_from_device([torch.zeros((256, 1), dtype=torch.int64, device="cuda"), torch.zeros((n, 14), dtype=torch.int64, device="cuda")],
                                   fe.pack_claims([]))

    def fill_alone():
        w.fill(1, prog, pairs)
        ctx.sync()

    line("ms_witness_fill alone", timed([fill_alone], args.reps)[0])
    del w


def claims_leg():
    """--claims: what building the claims on the device costs, next to the host round trip it replaces"""
    E = fe.Expr
    system = pkg.System.new(ctx, fe.bench_params(), fe.u32_add_system_inputs())
    xs, ys = fe.xorshift_pairs(n)
    traces, claims = fe._u32_add_traces(xs, ys, n)
    packed = fe.pack_claims(claims)
    fill_prog, plain = fe.u32_add_fill_program(n), fe.u32_add_claims_program()
    word = lambda i: sum((E.main(i + k) * E.const(256 ** k) for k in range(1, 4)), E.main(i))
    kept = fe.compile_claims(14, 0, 0, [E.const(1), word(0), word(4), word(8)], keep=E.main(13))
    for name, p in (("without keep", plain), ("keep = the activity column", kept)):
        print("claim program %-28s %d nodes; %s" % (name + ":", len(p.nodes), pkg.claims_program_info(p)))
    pairs = torch.from_numpy(np.stack([xs, ys], axis=1).astype(np.uint32).view(np.int32)).cuda()
    zeros = lambda: [torch.zeros(t.shape, dtype=torch.int64, device="cuda") for t in traces]
    w = system.witness_from_device(zeros(), fe.pack_claims([]))
    w.fill(1, fill_prog, pairs)
    for p in (kept, plain):
        rep = w.fill_claims(1, p, rows=n)
        offs, data = w.claims()
        same = bool(np.array_equal(offs, packed[0])) and bool(np.array_equal(data, packed[1]))
        print("2^%d additions, %s: %s; claims equal the host builder's: %s" % (args.log_size, "with keep" if p.has_keep else "without keep", rep, same), flush=True)
        assert same
    dm = w.derive_multiplicities(TARGETS)
    gen = system.bench_witness_on_device(n)
    proof = system.prove_multiple_claims(w).to_bytes()
    same_proof = proof == system.prove_multiple_claims(gen).to_bytes()
    g = gen.claims()
    same_gen = bool(np.array_equal(g[0], packed[0])) and bool(np.array_equal(g[1], packed[1]))
    print("proof equals the generator's witness's: %s; the generator's claims are the same: %s; check().verdict: %d" % (same_proof, same_gen, w.check().verdict),
          flush=True)
    assert dm.ok and same_proof and same_gen
    del gen
    on_dev = [torch.from_numpy(np.ascontiguousarray(t).view(np.int64)).cuda() for t in traces]  # the host route's traces stay in HBM

    print("\n# goldilocks, 2^%d additions: the routes, alternating" % args.log_size)
    state = {}

    def claims_alone(p):
        def run():
            w.fill_claims(1, p, rows=n)  # (returns synchronised: its last step is the host copy)
        return run

    def device_route():
        w.fill(1, fill_prog, pairs)
        w.fill_claims(1, plain, rows=n)
        w.derive_multiplicities(TARGETS)

    def host_read():
        state["t"] = w.trace(1)

    def host_numpy():
        t = state["t"]
        word = lambda i: t[:, i] | (t[:, i + 1] << np.uint64(8)) | (t[:, i + 2] << np.uint64(16)) | (t[:, i + 3] << np.uint64(24))
        state["claims"] = fe.pack_claims(np.stack([np.ones(n, dtype=np.uint64), word(0), word(4), word(8)], axis=1))

    def host_create():
        state["host"] = None  # (the previous witness's memory goes back first)
        state["host"] = system.witness_from_device(on_dev, state["claims"])

    def generator():
        state["gen"] = None
        state["gen"] = system.bench_witness_on_device(n)
        ctx.sync()

    t_pl, t_kp, t_dev, t_rd, t_np, t_cr, t_gen = timed([claims_alone(plain), claims_alone(kept), device_route, host_read, host_numpy, host_create, generator],
                                                       args.reps)
    line("fill_claims alone, without keep", t_pl)
    line("fill_claims alone, keep = all ones", t_kp)
    line("device route: fill + fill_claims + derive", t_dev)
    line("host: ms_witness_trace", t_rd)
    line("host: numpy (the words from their bytes, pack)", t_np)
    line("host: ms_witness_create_device, host claims", t_cr)
    total = [a + b + c for a, b, c in zip(t_rd, t_np, t_cr)]
    line("host route, the three steps together", total)
    line("generator: ms_witness_u32_add_bench", t_gen)
    m = statistics.median
    W = plain.width
    stated = n * (2 * 8 * (W + 1) + 8 * W)
    print("host route / fill_claims = %.1f; device route / generator = %.2f" % (m(total) / m(t_pl), m(t_dev) / m(t_gen)))
    # the compaction by itself: its launches between two events (the profile class witness_claims), one call at a time
    ctx.set_profile(["witness_claims"])
    t_cp = []
    for i in range(args.reps + 2):
        ctx.reset_stats()
        w.fill_claims(1, kept, rows=n)
        st = ctx.kernel_stats()["witness_claims"]
        if i >= 2:
            t_cp.append(st["ms"])
    ctx.set_profile([])
    line("compaction launches of one call (device time)", t_cp)
    print("compaction: %d stated bytes per row (8 (W + 1) written by the pass, 8 (W + 1) read, 8 W written; every row kept), %.1f MB in all; the "
          "launches move the last two, %.1f MB, in %.3f ms = %.0f GB/s" % (stated // n, stated / 1e6, (stated - 8 * (W + 1) * n) / 1e6, m(t_cp),
                                                                          (stated - 8 * (W + 1) * n) / m(t_cp) / 1e6))
    assert np.array_equal(state["host"].claims()[1], packed[1]) and np.array_equal(w.claims()[1], packed[1])
    state.clear()  # witnesses go before their system
    del w


def claims_leg_bb():
    """--claims --config babybear: msbb_witness_claims_fill. The route on the bench workload; the price of the row-major store,
    the claims pass next to msbb_witness_fill evaluating the same expressions as steps into as many columns; the compaction."""
    bb = pkg.babybear
    E = fe.Expr
    k = fe.poseidon2_constants()
    bb.set_poseidon2(ctx, k)
    xs, ys = fe.xorshift_pairs(n)
    with fe.field(fe.BABYBEAR):
        system = bb.System.new(ctx, fe.test_params(), fe.u32_add_system_inputs(), k)
        traces, claims = fe._u32_add_traces(xs, ys, n)
        packed = fe.pack_claims(claims)  # (a 2-D array: reduced mod p)
        fill_prog, plain = fe.u32_add_halves_fill_program(n), fe.u32_add_claims_program()
    print("claim program of the bench workload: %d nodes; %s" % (len(plain.nodes), bb.claims_program_info(plain)))
    m16, s16 = np.uint64(0xFFFF), np.uint64(16)
    halves = torch.from_numpy(np.stack([xs & m16, xs >> s16, ys & m16, ys >> s16], axis=1).astype(np.uint16).view(np.int16)).cuda()
    w = system.witness_from_device([torch.zeros(t.shape, dtype=torch.int32, device="cuda") for t in traces], fe.pack_claims([]))
    w.fill(1, fill_prog, halves)
    rep = w.fill_claims(1, plain, rows=n)
    offs, data = w.claims()
    same = bool(np.array_equal(offs, packed[0])) and bool(np.array_equal(data, packed[1]))
    dm = w.derive_multiplicities(TARGETS)
    proof = system.prove_multiple_claims(w).to_bytes()
    same_proof = proof == system.prove_multiple_claims(system.witness(traces, packed)).to_bytes()
    print("u32add over BabyBear at 2^%d additions: %s; claims equal the host builder's mod p: %s; proof equals the host-built witness's: %s; "
          "check().verdict: %d" % (args.log_size, rep, same, same_proof, w.check().verdict), flush=True)
    assert same and same_proof and dm.ok
    del w

    # the lab system: per width W a circuit of 14 + W columns, the first 14 those of U32Add. The claim program's W elements read
    # columns 0 .. 13; the fill program assigns the same W expressions to columns 14 .. 14 + W - 1: one interpreter, one program
    # body, row-major 4-byte stores W words apart against column-major contiguous ones.
    widths = [args.width] if args.width else [4, 49]
    with fe.field(fe.BABYBEAR):
        word = lambda i: sum((E.main(i + j) * E.const(256 ** j) for j in range(1, 4)), E.main(i))
        elements = {4: [E.const(1), word(0), word(4), word(8)], 49: [E.main(j % 14) * (j + 2) + E.main_next((j + 5) % 14) for j in range(49)]}
        ph = [E.main(0) * E.main(0) - E.main(0)]
        lab = bb.System.new(ctx, fe.test_params(), [fe.CircuitInputs(14 + W, None, ph, [], []) for W in widths], k)
        progs = {W: (fe.compile_claims(14 + W, 0, 0, elements[W]), fe.compile_fill(14 + W, 0, 0, [(14 + j, e) for j, e in enumerate(elements[W])]),
                     fe.compile_claims(14 + W, 0, 0, elements[W], keep=E.main(13))) for W in widths}
    t1 = torch.from_numpy(np.ascontiguousarray(traces[1]).astype(np.uint32).view(np.int32)).cuda()
    lw = lab.witness_from_device([torch.cat([t1, torch.zeros((n, W), dtype=torch.int32, device="cuda")], dim=1) for W in widths], fe.pack_claims([]))
    del t1
    fns, names = [], []
    for ci, W in enumerate(widths):
        cl, fl, _ = progs[W]
        print("W = %d: claim program %s; fill program %s" % (W, bb.claims_program_info(cl), bb.fill_program_info(fl)))
        lw.fill(ci, fl)
        lw.fill_claims(ci, cl, rows=n)
        got = lw.claims()[1].reshape(n, W)
        assert np.array_equal(got, lw.trace(ci)[:, 14:]), "the claims are the filled columns, row by row"
        if W == 4:
            assert np.array_equal(got.reshape(-1), packed[1])

        def claims_call(ci=ci, cl=cl):
            lw.fill_claims(ci, cl, rows=n)  # (returns synchronised: its last step is the host copy)

        def fill_call(ci=ci, fl=fl):
            lw.fill(ci, fl)
            ctx.sync()

        def copy_alone(ci=ci):
            lw.claims()  # the read-back of the list and nothing else: what the host copy of the call costs at least

        fns += [claims_call, fill_call, copy_alone]
        names += ["W = %d: msbb_witness_claims_fill, no keep" % W, "W = %d: msbb_witness_fill, the same %d expressions" % (W, W),
                  "W = %d: Witness.claims() alone (the list read back)" % W]
    print("\n# babybear, 2^%d rows: the claims pass next to the fill, alternating (wall time; the claims call ends in its host copy)" % args.log_size)
    for name, t in zip(names, timed(fns, args.reps)):
        line(name, t)

    # the compaction: its launches between two events (the profile class witness_claims), one call at a time, W = 4
    if 4 in widths:
        ci, (_, _, kept) = widths.index(4), progs[4]
        S, W = 4, 4
        print("\n# the keep compaction at W = 4: device time of its launches against the bytes the layout states")
        ctx.set_profile(["witness_claims"])
        for name, dens in (("1/64", 64), ("1/2", 2), ("1", 1)):
            act = (torch.arange(n, device="cuda") % dens == 0).to(torch.int32)
            tr = torch.from_numpy(lw.trace(ci).view(np.int32)).cuda()
            tr[:, 13] = act
            cw = lab.witness_from_device([tr if c == ci else None for c in range(len(widths))], fe.pack_claims([]))
            n_kept = int(act.sum().item())
            t_cp = []
            for i in range(args.reps + 2):
                ctx.reset_stats()
                assert cw.fill_claims(ci, kept, rows=n).claims == n_kept
                if i >= 2:
                    t_cp.append(ctx.kernel_stats()["witness_claims"]["ms"])
            moved = 2 * S * n + 2 * S * W * n_kept  # the flag read by the count and by the scatter; each kept row read and written
            line("density %s: compaction launches of one call" % name, t_cp)
            print("    stated bytes: %d x 2 x %d (flags) + %d x 2 x %d (kept rows) = %.1f MB -> %.0f GB/s (no share of a peak: the flag reads "
                  "touch one 32-byte sector per row)" % (n, S, n_kept, S * W, moved / 1e6, moved / statistics.median(t_cp) / 1e6), flush=True)
            del cw
        ctx.set_profile([])
    del lw


if args.claims:
    claims_leg_bb() if args.config == "babybear" else claims_leg()
    sys.exit(0)
if args.gather:
    gather_leg()
    sys.exit(0)
if args.peers:
    peers_leg()
    sys.exit(0)
if args.alone:
    alone_leg()
    sys.exit(0)
if args.scan and args.config == "babybear":
    scan_leg_bb()
    sys.exit(0)
if args.config == "babybear":
    babybear()
    sys.exit(0)
if args.scan:
    scan_leg()
    sys.exit(0)

system = pkg.System.new(ctx, fe.bench_params(), fe.u32_add_system_inputs())
xs, ys = fe.xorshift_pairs(n)
traces, claims = fe._u32_add_traces(xs, ys, n)
packed = fe.pack_claims(claims)
prog = fe.u32_add_fill_program(n)
print("fill program: %d nodes, %d steps; %s" % (len(prog.nodes), len(prog.steps), pkg.fill_program_info(prog)))
pairs = torch.from_numpy(np.stack([xs, ys], axis=1).astype(np.uint32).view(np.int32)).cuda()
w = system.witness_from_device([torch.zeros(t.shape, dtype=torch.int64, device="cuda") for t in traces], packed)

rep = w.fill(1, prog, pairs)
dm = w.derive_multiplicities(TARGETS)
print("u32add at 2^%d additions, U32Add filled from the pairs: %s" % (args.log_size, rep))
print(dm)
same = bool(np.array_equal(w.trace(0), traces[0])) and bool(np.array_equal(w.trace(1), traces[1]))
gen = system.bench_witness_on_device(n)
proof = system.prove_multiple_claims(w).to_bytes()
same_proof = proof == system.prove_multiple_claims(gen).to_bytes()
print("traces equal the host builder's: %s; proof equals the generator's witness's: %s; check().verdict: %d" % (same, same_proof, w.check().verdict),
      flush=True)
assert same and same_proof and dm.ok
del gen

print("\n# three routes to the same witness, alternating")
state = {}


def fill_route():
    w.fill(1, prog, pairs)
    w.derive_multiplicities(TARGETS)


def fill_alone():
    w.fill(1, prog, pairs)
    ctx.sync()


def generator():
    state["gen"] = None  # (the previous witness's memory goes back first)
    state["gen"] = system.bench_witness_on_device(n)
    ctx.sync()


def host_traces():
    state["traces"] = fe._u32_add_traces(xs, ys, n)[0]


def host_create():
    state["host"] = None
    state["host"] = system.witness(state["traces"], packed)


t_fill, t_alone, t_gen, t_tr, t_cr = timed([fill_route, fill_alone, generator, host_traces, host_create], args.reps)
line("fill: ms_witness_fill + derive_multiplicities", t_fill)
line("      ms_witness_fill alone", t_alone)
line("generator: ms_witness_u32_add_bench", t_gen)
line("host: frontend._u32_add_traces", t_tr)
line("host: ms_witness_create (both traces, from_stage_1)", t_cr)
total = [a + b for a, b in zip(t_tr, t_cr)]
line("host route, the two steps together", total)
m = statistics.median
print("fill route / generator = %.2f, host route / fill route = %.1f" % (m(t_fill) / m(t_gen), m(total) / m(t_fill)))
assert np.array_equal(w.trace(1), traces[1]) and np.array_equal(w.trace(0), traces[0])
state.clear()  # witnesses go before their system, and both before the interpreter takes the module apart
del w
del system
