// Exact lookup balance on the device (ms_witness_lookup_balance): the kernels and the call are balance_dev.h's, on the grouping
// table of lb_dev.h, for Goldilocks as gl_lb.h describes it.
#include "balance_dev.h"
#include "gl_lb.h"

namespace msamd {

size_t lookup_balance_slots(const HSystem& sys) {
  size_t n = 0;
  for (auto& c : sys.circuits) n += c.num_lookups;
  return n;
}

void witness_lookup_balance(HSystem& sys, HWitness& wit, u64 summary[4], u64* entries, size_t entries_cap, u64* args_out, size_t args_cap,
                            u64* slot_counts) {
  lb_balance<GlLookup>(sys, wit, lookup_balance_slots(sys), summary, entries, entries_cap, args_out, args_cap, slot_counts);
}

}  // namespace msamd
