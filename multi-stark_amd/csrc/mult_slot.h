// The classifier of ms_system_multiplicity_slot / msbb_system_multiplicity_slot (include/mstark.h, "Table multiplicity columns"):
// may a lookup slot be a target of the derive-multiplicities calls? Host code over a circuit's node vector and lookup list, which
// HCircuit (host.h) and BCircuit (bb_host.h) hold in the same types, so both configurations run this one function: the answer
// depends on the node program only, never on the field.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <utility>
#include <vector>

#include "program.h"

namespace msamd {

typedef std::vector<std::pair<uint32_t, std::vector<uint32_t>>> SlotLookups;  // per slot: multiplicity node, argument nodes

// every node a lookup expression rooted at `root` reads
inline void dm_reach(const std::vector<PNode>& nodes, uint32_t root, std::vector<uint8_t>& seen) {
  std::vector<uint32_t> todo{root};
  while (!todo.empty()) {
    const uint32_t n = todo.back();
    todo.pop_back();
    if (n >= nodes.size() || seen[n]) continue;
    seen[n] = 1;
    const PNode& nd = nodes[n];
    if (nd.kind == OP_ADD || nd.kind == OP_SUB || nd.kind == OP_MUL) todo.push_back((uint32_t)nd.a), todo.push_back((uint32_t)nd.b);
    if (nd.kind == OP_NEG) todo.push_back((uint32_t)nd.a);
  }
}

// out3 = [eligibility, column, pull]
inline void multiplicity_slot(const std::vector<PNode>& nodes, const SlotLookups& lookups, size_t slot, uint64_t out3[3]) {
  if (slot >= lookups.size()) throw std::runtime_error("lookup slot out of range");
  out3[0] = 1, out3[1] = 0, out3[2] = 0;
  uint32_t n = lookups[slot].first;
  if (n < nodes.size() && nodes[n].kind == OP_NEG) out3[2] = 1, n = (uint32_t)nodes[n].a;
  if (n >= nodes.size()) return;
  const PNode& var = nodes[n];
  if (var.kind != OP_VAR || var.source != 1 || var.offset != 0) {
    out3[2] = 0;
    return;
  }
  out3[1] = var.a;
  // the other lookup expressions of the circuit: every argument of every slot, every other slot's multiplicity
  std::vector<uint8_t> seen(nodes.size(), 0);
  for (size_t j = 0; j < lookups.size(); j++) {
    if (j != slot) dm_reach(nodes, lookups[j].first, seen);
    for (uint32_t a : lookups[j].second) dm_reach(nodes, a, seen);
  }
  out3[0] = 0;
  for (size_t k = 0; k < nodes.size(); k++)
    if (seen[k] && nodes[k].kind == OP_VAR && nodes[k].source == 1 && nodes[k].a == var.a) out3[0] = 2;  // (at either offset)
}

}  // namespace msamd
