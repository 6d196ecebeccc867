"""Model of ms_witness_derive_multiplicities (include/mstark.h, "Table multiplicity columns"): helper for the tests, not a test.

Eligibility is read from the compiled circuit (cc.lookups and cc.nodes, tuples (kind, source, offset, a, b)). The demand is a dict
over the stripped tuples built from lookup_balance_model.messages, restricted to the sources that are no target (the derived
columns are zeroed first, so a target's messages do not exist for it either); the target rows' tuples come from the oracle's
compute_lookup_values; the first target row of a tuple in origin order is its provider. -> the traces with the derived columns
rewritten, and a report with the fields of the device's."""
import numpy as np

import lookup_balance_model as lm

P = lm.P
N_VAR, N_ADD, N_SUB, N_MUL, N_NEG, SRC_MAIN = 1, 6, 7, 8, 9, 1  # the system-blob encoding (multi_stark_amd.frontend)


class Misuse(Exception):
    pass


class Report:
    def __init__(self, demand_messages, demand_groups, served, unserved, duplicates, entries):
        self.demand_messages, self.demand_groups, self.served, self.unserved = demand_messages, demand_groups, served, unserved
        self.duplicates, self.entries, self.ok = duplicates, entries, unserved == 0

    def fields(self):
        """the same tuple as multi_stark_amd.MultiplicityReport.fields()"""
        return (self.demand_messages, self.demand_groups, self.served, self.unserved, self.duplicates, self.entries)


def _reach(nodes, root, seen):
    todo = [root]
    while todo:
        n = todo.pop()
        if n in seen:
            continue
        seen.add(n)
        kind, _, _, a, b = nodes[n]
        if kind in (N_ADD, N_SUB, N_MUL):
            todo += [a, b]
        elif kind == N_NEG:
            todo.append(a)


def classify(cc, slot):
    """(eligibility, column, pull) of ms_system_multiplicity_slot for lookup slot `slot` of the compiled circuit"""
    n = cc.lookups[slot][0]
    pull = cc.nodes[n][0] == N_NEG
    if pull:
        n = cc.nodes[n][3]
    kind, source, offset, col, _ = cc.nodes[n]
    if kind != N_VAR or source != SRC_MAIN or offset != 0:
        return (1, 0, False)
    seen = set()
    for j, (m, args) in enumerate(cc.lookups):
        if j != slot:
            _reach(cc.nodes, m, seen)
        for a in args:
            _reach(cc.nodes, a, seen)
    read = any(cc.nodes[k][0] == N_VAR and cc.nodes[k][1] == SRC_MAIN and cc.nodes[k][3] == col for k in seen)
    return (2 if read else 0, col, pull)


def derive(osys, compiled, traces, claims_packed, targets, entries=64):
    """-> ([trace per circuit, derived columns rewritten], Report); Misuse for what the call refuses"""
    cols = {}
    for (c, j) in targets:
        if c >= len(compiled) or j >= len(compiled[c].lookups):
            raise Misuse("out of range")
        code, col, pull = classify(compiled[c], j)
        if code:
            raise Misuse("not eligible: %d" % code)
        if (c, col) in [(c2, v[0]) for (c2, _), v in cols.items()]:
            raise Misuse("shared derived column")
        cols[(c, j)] = (col, pull)
    out = [None if t is None or len(t) == 0 else np.array(t, dtype=np.uint64) for t in traces]
    for (c, j), (col, _) in cols.items():
        if out[c] is not None:
            out[c][:, col] = 0
    demand = {}  # tuple -> [D, members, first origin]; insertion order = order of first origin
    n = 0
    for origin, source, m, t in lm.messages(osys, compiled, out, claims_packed):
        if source in cols:
            continue
        n += 1
        g = demand.setdefault(t, [0, 0, origin])
        g[0] = (g[0] + m) % P
        g[1] += 1
    rows = []  # the target rows in origin order: circuit, row, slot
    for c in sorted({c for c, _ in cols}):
        if out[c] is None:
            continue
        cc = compiled[c]
        _, args = osys.compute_lookup_values(c, out[c])
        args = args.tolist()
        o = np.cumsum([0] + [len(a) for _, a in cc.lookups]).tolist()
        slots = sorted(j for c2, j in cols if c2 == c)
        for r in range(len(args)):
            for j in slots:
                rows.append((c, r, j, lm.strip(args[r][o[j]:o[j + 1]])))
    provider, duplicates = set(), 0
    for c, r, j, t in rows:
        if t in provider:
            duplicates += 1
            continue
        provider.add(t)
        col, pull = cols[(c, j)]
        d = demand[t][0] if t in demand else 0
        out[c][r, col] = d if pull else (P - d) % P
    served = sum(1 for t, g in demand.items() if g[0] and t in provider)
    unserved = [(g[2], g[0], g[1], list(t)) for t, g in demand.items() if g[0] and t not in provider]
    return out, Report(n, len(demand), served, len(unserved), duplicates, unserved[:entries])
