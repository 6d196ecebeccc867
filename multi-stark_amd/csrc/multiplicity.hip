// Table multiplicity columns derived on the device (ms_witness_derive_multiplicities): the kernels and the call are
// multiplicity_dev.h's, on the grouping table of lb_dev.h, for Goldilocks as gl_lb.h describes it. Here: where a target's derived
// cells lie. The trace is row-major, and a witness that holds its lookup values holds the target's multiplicities too: the
// provider writes v into the trace cell and s v = -D into the held multiplicity, so both stay consistent.
#include "gl_lb.h"
#include "mult_slot.h"
#include "multiplicity_dev.h"

namespace msamd {

// the classifier is host code over the node program alone (mult_slot.h), shared with the BabyBear configuration
void multiplicity_slot(const HCircuit& c, size_t slot, u64 out3[3]) { multiplicity_slot(c.nodes, c.lookups, slot, out3); }

void witness_derive_multiplicities(HSystem& sys, HWitness& wit, const ms_mult_target* targets, size_t n_targets, u64 summary[MS_DM_SUMMARY_WORDS],
                                   u64* entries, size_t entries_cap, u64* args_out, size_t args_cap) {
  dm_derive<GlLookup>(
      sys, wit, targets, n_targets, summary, entries, entries_cap, args_out, args_cap,
      [](const HCircuit&, size_t, const std::string&) {},  // (an eligible column lies in the main trace: nothing further)
      [&](size_t ci, size_t column, size_t, GlLookup::Cell& cell) {
        cell.trace = wit.traces[ci].p, cell.held = wit.lookups[ci].mult.p;
        cell.W = (u32)sys.circuits[ci].main_width, cell.m = (u32)column;
        return cell.trace != nullptr;
      });
}

}  // namespace msamd
