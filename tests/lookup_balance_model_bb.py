"""Model of msbb_witness_lookup_balance (include/mstark_bb.h; the definition is the "Lookup balance" section of include/mstark.h
read over BabyBear): helper for the tests, not a test. The counterpart of lookup_balance_model.py.

A dict over the tuples with trailing zeros stripped, filled in origin order - the claims by index (multiplicity 1), then for
every active circuit the oracle's lookup values (oracle_bb.System.compute_lookup_values) row-major, slot last; messages of
multiplicity 0 are skipped. The report has the fields of the device's: see `Report.fields`."""
import numpy as np

P = (1 << 31) - (1 << 27) + 1
D = 4


def strip(t):
    t = [int(x) % P for x in t]
    while t and t[-1] == 0:
        t.pop()
    return tuple(t)


class Report:
    def __init__(self, messages, groups, unbalanced, entries, slot_counts, claims_count):
        self.messages, self.groups, self.unbalanced, self.entries = messages, groups, unbalanced, entries
        self.slot_counts, self.claims_count, self.ok = slot_counts, claims_count, unbalanced == 0

    def fields(self):
        """the same tuple as multi_stark_amd.LookupBalanceReport.fields()"""
        return (self.messages, self.groups, self.unbalanced, self.entries, self.slot_counts, self.claims_count)


def _active(compiled, traces):
    for ci, cc in enumerate(compiled):
        tr = traces[ci]
        if tr is not None and len(tr) and cc.lookups:
            yield ci, cc, np.asarray(tr, dtype=np.uint64)


def messages(osys, compiled, traces, claims_packed):
    """every message of non-zero multiplicity in origin order: (origin, source, multiplicity, stripped tuple); source = (circuit,
    slot) or "claims" """
    offs, data = claims_packed
    for i in range(len(offs) - 1):
        yield ("claims", i, 0), "claims", 1, strip(data[int(offs[i]):int(offs[i + 1])])
    for ci, cc, tr in _active(compiled, traces):
        mult, args = osys.compute_lookup_values(ci, tr)
        o = np.cumsum([0] + [len(a) for _, a in cc.lookups]).tolist()
        L = len(cc.lookups)
        rows, slots = np.nonzero(mult % np.uint64(P))  # row-major: rows ascending, slots ascending within a row
        for r, j in zip(rows.tolist(), slots.tolist()):
            yield (ci, r, j), (ci, j), int(mult[r, j]) % P, strip(args[r, o[j]:o[j + 1]].tolist())
        assert L == mult.shape[1]


def balance(osys, compiled, traces, claims_packed, entries=64):
    groups = {}  # tuple -> [net, members, first origin, sources]; dicts keep insertion order = order of first origin
    n = 0
    for origin, source, m, t in messages(osys, compiled, traces, claims_packed):
        n += 1
        g = groups.setdefault(t, [0, 0, origin, []])
        g[0] = (g[0] + m) % P
        g[1] += 1
        g[3].append(source)
    slot_counts = [[0] * len(cc.lookups) for cc in compiled]
    claims_count, bad = 0, []
    for t, (net, members, origin, sources) in groups.items():
        if net == 0:
            continue
        bad.append((origin, net, members, list(t)))
        for s in sources:
            if s == "claims":
                claims_count += 1
            else:
                slot_counts[s[0]][s[1]] += 1
    return Report(n, len(groups), len(bad), bad[:entries], slot_counts, claims_count)


def accumulator_is_zero(oracle_bb, osys, compiled, traces, claims_packed, beta, gamma):
    """the verifier's balance: the oracle's accumulator (four coordinates) chained over the claims and every active circuit, as
    the prover chains it"""
    beta, gamma = [int(x) for x in beta], [int(x) for x in gamma]
    assert len(beta) == D and len(gamma) == D
    acc = tuple(oracle_bb.claims_accumulator(claims_packed, beta, gamma)) if len(claims_packed[0]) > 1 else (0,) * D
    for ci, cc, tr in _active(compiled, traces):
        mult, args = osys.compute_lookup_values(ci, tr)
        offs = np.cumsum([0] + [len(a) for _, a in cc.lookups]).astype(np.uint64)
        _, acc = oracle_bb.stage2_trace(mult, offs, args, beta, gamma, acc)
    return tuple(int(x) for x in acc) == (0,) * D
