// Exact lookup balance on the device for the BabyBear configuration (msbb_witness_lookup_balance): the definition of the "Lookup
// balance" section of include/mstark.h over p = 2^31 - 2^27 + 1. The kernels and the call are balance_dev.h's, on the grouping
// table of lb_dev.h, for BabyBear as bb_lb.h describes it (with the sweep of the lookup values, which the witness does not hold).
#include "balance_dev.h"
#include "bb_lb.h"

namespace msbb {

size_t lookup_balance_slots(const BSystem& sys) {
  size_t n = 0;
  for (auto& c : sys.circuits) n += c.num_lookups;
  return n;
}

void witness_lookup_balance(BSystem& sys, BWitness& wit, u64 summary[4], u64* entries, size_t entries_cap, u32* args_out, size_t args_cap,
                            u64* slot_counts) {
  msamd::lb_balance<BbLookup>(sys, wit, lookup_balance_slots(sys), summary, entries, entries_cap, args_out, args_cap, slot_counts);
}

}  // namespace msbb
