"""Model of msbb_witness_derive_multiplicities (include/mstark_bb.h; the definition is the "Table multiplicity columns" section of
include/mstark.h read over BabyBear): helper for the tests, not a test. The counterpart of multiplicity_model.py.

Eligibility does not depend on the field: `classify` is multiplicity_model's. The demand is a dict over the stripped tuples built
from lookup_balance_model_bb.messages, restricted to the sources that are no target (the derived columns are zeroed first, so a
target's messages do not exist for it either); the target rows' tuples come from oracle_bb's compute_lookup_values; the first
target row of a tuple in origin order is its provider. -> the traces with the derived columns rewritten (canonical, uint64), and
a report with the fields of the device's."""
import numpy as np

import lookup_balance_model_bb as lm
from multiplicity_model import Misuse, Report, classify  # noqa: F401  (re-exported: the tests take them from here)

P = lm.P


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
        args = np.asarray(args).tolist()
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
