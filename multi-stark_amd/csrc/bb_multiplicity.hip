// Table multiplicity columns derived on the device for the BabyBear configuration (msbb_witness_derive_multiplicities; the
// definition is the "Table multiplicity columns" section of include/mstark.h read over p = 2^31 - 2^27 + 1): the kernels and the
// call are multiplicity_dev.h's, on the grouping table of lb_dev.h, for BabyBear as bb_lb.h describes it. Here: where a target's
// derived cells lie. The library's trace is a column-major Montgomery BMat, so the provider's cell is buf[m * ld + r] =
// bb_to_monty(v). The witness holds no lookup values - each call sweeps them from the traces into temporaries - so there is
// nothing held to keep consistent: the next call that needs them sweeps the column this one wrote.
#include "bb_lb.h"
#include "mult_slot.h"
#include "multiplicity_dev.h"

namespace msbb {

// the classifier is host code over the node program alone (mult_slot.h), shared with the Goldilocks configuration
void multiplicity_slot(const BCircuit& c, size_t slot, u64 out3[3]) { msamd::multiplicity_slot(c.nodes, c.lookups, slot, out3); }

void witness_derive_multiplicities(BSystem& sys, BWitness& wit, const ms_mult_target* targets, size_t n_targets, u64 summary[MS_DM_SUMMARY_WORDS],
                                   u64* entries, size_t entries_cap, u32* args_out, size_t args_cap) {
  msamd::dm_derive<BbLookup>(
      sys, wit, targets, n_targets, summary, entries, entries_cap, args_out, args_cap,
      [](const BCircuit& c, size_t column, const std::string& target) {
        if (column >= c.main_width) throw std::runtime_error(target + " is not eligible: its column is beyond the main trace");
      },
      [&](size_t ci, size_t column, size_t rows, BbLookup::Cell& cell) {
        BMat& tr = wit.traces[ci];
        if (!tr.buf.p || tr.ld < rows) return false;  // (the sources have checked h and w)
        cell.col = tr.col(column);
        return true;
      });
}

}  // namespace msbb
