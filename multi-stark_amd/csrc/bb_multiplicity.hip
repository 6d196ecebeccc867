// Table multiplicity columns derived on the device for the BabyBear configuration (msbb_witness_derive_multiplicities; the
// definition is the "Table multiplicity columns" section of include/mstark.h read over p = 2^31 - 2^27 + 1): the caller names the
// lookup slots that act as providers (TARGETS: their multiplicity is one main-trace column, optionally negated), every other
// message of the witness is DEMAND, and the call writes into each target's column what makes the demand cancel. The grouping is
// that of msbb_witness_lookup_balance (bb_lb_dev.h), followed by a write instead of a report. The design is multiplicity.hip's.
// What differs from it:
//   - the library's trace is a column-major Montgomery BMat: the provider's cell is buf[m * ld + r] = bb_to_monty(v);
//   - a group's demand is one plain 64-bit sum of canonical multiplicities (fewer than 2^32 messages, the host refuses more),
//     reduced modulo p when it is read: no small / big split;
//   - the witness holds no lookup values. Each call sweeps them from the traces into temporaries (bl_sources), so there is
//     nothing held to keep consistent: the next call that needs them sweeps the column this one wrote.
//
// All launches go to the context's stream, in this order:
//   dm_zero_k    zeroes the multiplicity of every target row in the swept temporaries: multiplicity 0 does not exist for
//                bl_insert_k, so the table receives the demand only
//   bl_init_k, bl_insert_k   the demand grouped and summed (bb_lb_dev.h)
//   dm_probe_k   serve, pass 1: one thread per target row. A read-only probe finds the group of the row's tuple (the swept
//                arguments, Montgomery words compared as they lie); a row that finds one takes a 64-bit atomicMin on the slot's
//                `first_target` word with its origin and keeps the slot in slot_of[row]. A row whose tuple has no group claims
//                nothing here
//   dm_claim_k   the rows left over - target tuples nobody demands - are inserted into the SAME table by the claiming probe of
//                bl_insert_k (a separate launch, so that no read-only probe runs beside a claim; owners are learnt only from the
//                value the CAS returns), as groups of no members and net 0, and take the same atomicMin. Equal tuples among them
//                meet in one slot: which of them is a duplicate is decided by origin, not by who came first. The table has room:
//                cap >= 2 x messages counts the target rows
//   dm_report_k  walks the demand again: messages, groups, served and unserved groups of non-zero demand; marks the first origins
//                of the unserved groups in the bitmap the compaction of bb_lb_dev.h reads
//   dm_write_k   serve, pass 2: one thread per target row. The row whose origin is its slot's first_target is the provider and
//                writes bb_to_monty(v), v = D for a pull, (p - D) mod p for a push; every other row writes 0 and is counted as a
//                duplicate, one ballot and one atomic per wave. Consecutive threads are consecutive rows of one column, so the
//                stores of a wave are contiguous
// Nothing depends on thread order or on the hash: origins decide providers, sums are exact, marks lie at fixed positions. Bounded
// loops raise the flag of bb_lb_dev.h, which the host turns into MS_ERR (the derived columns are unspecified then).
#include "bb_lb_dev.h"
#include "mult_slot.h"

namespace msbb {
namespace {

constexpr const char* DM_CALL = "msbb_witness_derive_multiplicities";
enum { DM_C_SERVED = BL_C_WORDS, DM_C_DUPLICATES, DM_C_WORDS };  // after the four counters of bb_lb_dev.h ([2]: unserved groups)

struct DmTgt {  // one target slot of an active circuit; its rows are the target rows from row0 up to the next target's row0
  u64 row0, msg_base;  // msg_base: the circuit's first message (BlSrc::base)
  u32 *col, *mult;     // the derived column (buf + m * ld, Montgomery); the swept multiplicities bl_msg reads
  u32 L, j, pull, pad;
};

// target row k -> its target, row and message index (origin)
__device__ const DmTgt& dm_row(const DmTgt* tg, u32 nt, u64 k, u64& r, u64& i) {
  u32 lo = 0, hi = nt;
  while (hi - lo > 1) {
    const u32 mid = (lo + hi) >> 1;
    if (tg[mid].row0 <= k) lo = mid; else hi = mid;
  }
  const DmTgt& g = tg[lo];
  r = k - g.row0;
  i = g.msg_base + r * g.L + g.j;
  return g;
}

__global__ __launch_bounds__(256) void dm_zero_k(const DmTgt* tg, u32 nt, u64 n_rows) {
  const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
  if (k >= n_rows) return;
  u64 r, i;
  const DmTgt& g = dm_row(tg, nt, k, r, i);
  g.mult[r * g.L + g.j] = 0;
}

__global__ __launch_bounds__(256) void dm_probe_k(BlTab t, const BlSrc* srcs, u32 ns, const DmTgt* tg, u32 nt, u64 n_rows, u64* first_target,
                                                  u64* slot_of) {
  const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
  if (k >= n_rows) return;
  u64 r, i, s;
  dm_row(tg, nt, k, r, i);
  const BlMsg m = bl_msg(srcs, ns, i);
  if (bl_lookup(t, srcs, ns, i, m, s)) {
    atomicMin((unsigned long long*)&first_target[s], (unsigned long long)i);
    slot_of[k] = s;
  } else {
    slot_of[k] = BL_EMPTY;
  }
}

__global__ __launch_bounds__(256) void dm_claim_k(BlTab t, const BlSrc* srcs, u32 ns, const DmTgt* tg, u32 nt, u64 n_rows, u64* first_target,
                                                  u64* slot_of, u64* counters) {
  const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
  if (k >= n_rows || slot_of[k] != BL_EMPTY) return;
  u64 r, i, s;
  dm_row(tg, nt, k, r, i);
  const BlMsg m = bl_msg(srcs, ns, i);
  if (!bl_claim(t, srcs, ns, i, m, bl_hash(m, t.hash_mask), s)) {
    atomicOr((unsigned long long*)&counters[BL_C_FLAG], 4ull);
    return;
  }
  atomicMin((unsigned long long*)&first_target[s], (unsigned long long)i);
  slot_of[k] = s;
}

__global__ __launch_bounds__(BL_T) void dm_report_k(BlTab t, const BlSrc* srcs, u32 ns, const u64* first_target, u64* counters, u64* marks,
                                                    u32* wg_counts) {
  __shared__ u32 tot[4];
  if (threadIdx.x < 4) tot[threadIdx.x] = 0;
  __syncthreads();
  u32 n_msgs = 0, n_groups = 0, n_served = 0, n_unserved = 0;
  bool failed = false;
  for (u32 it = 0; it < BL_PER; it++) {
    const u64 i = (u64)blockIdx.x * BL_BLOCK + it * BL_T + threadIdx.x;
    bool mark = false;
    if (i < t.n_msgs) {
      const BlMsg m = bl_msg(srcs, ns, i);
      if (m.mult != 0) {  // (the target rows have none: dm_zero_k)
        n_msgs++;
        u64 s;
        if (!bl_lookup(t, srcs, ns, i, m, s)) {
          failed = true;
        } else if (t.first[s] == i) {
          n_groups++;
          if (bl_net(t, s) != 0) {
            mark = first_target[s] == BL_EMPTY;
            n_served += !mark;
            n_unserved += mark;
          }
        }
      }
    }
    const unsigned long long b = __ballot(mark);  // the wave's 64 messages are consecutive and start at a multiple of 64
    if ((threadIdx.x & 63) == 0) marks[(size_t)blockIdx.x * BL_WORDS + it * (BL_T / 64) + (threadIdx.x >> 6)] = b;
  }
  if (n_msgs) atomicAdd(&tot[0], n_msgs);
  if (n_groups) atomicAdd(&tot[1], n_groups);
  if (n_unserved) atomicAdd(&tot[2], n_unserved);
  if (n_served) atomicAdd(&tot[3], n_served);
  if (failed) atomicOr((unsigned long long*)&counters[BL_C_FLAG], 2ull);
  __syncthreads();
  if (threadIdx.x < 3 && tot[threadIdx.x]) atomicAdd((unsigned long long*)&counters[threadIdx.x], (unsigned long long)tot[threadIdx.x]);
  if (threadIdx.x == 3 && tot[3]) atomicAdd((unsigned long long*)&counters[DM_C_SERVED], (unsigned long long)tot[3]);
  if (threadIdx.x == 0) wg_counts[blockIdx.x] = tot[2];
}

__global__ __launch_bounds__(256) void dm_write_k(BlTab t, const DmTgt* tg, u32 nt, u64 n_rows, const u64* first_target, const u64* slot_of,
                                                  u64* counters) {
  const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
  bool dup = false;
  if (k < n_rows) {
    u64 r, i;
    const DmTgt& g = dm_row(tg, nt, k, r, i);
    const u64 s = slot_of[k];
    if (s != BL_EMPTY) {  // (all-ones: dm_claim_k found the table full and raised the flag)
      const bool provider = first_target[s] == i;
      const u32 d = provider ? (u32)bl_net(t, s) : 0;
      g.col[r] = bb_to_monty(g.pull ? d : (d ? BB_P - d : 0));
      dup = !provider;
    }
  }
  const unsigned long long b = __ballot(dup);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd((unsigned long long*)&counters[DM_C_DUPLICATES], (unsigned long long)__popcll(b));
}

}  // namespace

// the classifier is host code over the node program alone (mult_slot.h), shared with the Goldilocks configuration
void multiplicity_slot(const BCircuit& c, size_t slot, u64 out3[3]) { msamd::multiplicity_slot(c.nodes, c.lookups, slot, out3); }

void witness_derive_multiplicities(BSystem& sys, BWitness& wit, const ms_mult_target* targets, size_t n_targets, u64 summary[MS_DM_SUMMARY_WORDS],
                                   u64* entries, size_t entries_cap, u32* args_out, size_t args_cap) {
  Ctx& ctx = *sys.ctx;
  const std::string name(DM_CALL);
  bl_accept(sys, wit, DM_CALL);
  const size_t C = sys.circuits.size();
  for (int k = 0; k < MS_DM_SUMMARY_WORDS; k++) summary[k] = 0;

  // misuse of targets, before anything is launched
  struct Named {
    size_t c, j, m;
    bool pull;
  };
  std::vector<Named> named;
  for (size_t k = 0; k < n_targets; k++) {
    const size_t c = targets[k].circuit, j = targets[k].slot;
    const std::string what = "target (" + std::to_string(c) + ", " + std::to_string(j) + ")";
    if (c >= C || j >= sys.circuits[c].lookups.size()) throw std::runtime_error(name + ": " + what + " is out of range");
    u64 o[3];
    multiplicity_slot(sys.circuits[c], j, o);
    if (o[0] == 1) throw std::runtime_error(name + ": " + what + " is not eligible: its multiplicity is not one main-trace column at offset 0 (optionally negated)");
    if (o[0] == 2)
      throw std::runtime_error(name + ": " + what + " is not eligible: column " + std::to_string(o[1]) + " is read by another lookup expression of the circuit");
    if (o[1] >= sys.circuits[c].main_width) throw std::runtime_error(name + ": " + what + " is not eligible: its column is beyond the main trace");
    for (auto& e : named)
      if (e.c == c && e.m == o[1]) throw std::runtime_error(name + ": " + what + " shares the derived column " + std::to_string(o[1]) + " with an earlier target");
    named.push_back({c, j, (size_t)o[1], o[2] != 0});
  }

  // (bl_sources writes temporaries of the call only: an error it raises leaves the witness as it was)
  std::vector<BlSrc> srcs;
  std::vector<DBuf<u32>> keep;
  size_t max_len = 0;
  const size_t M = bl_sources(sys, wit, DM_CALL, srcs, keep, max_len);
  if (M == 0) return;

  // the target slots of active circuits, in the order they were named (the order does not matter: origins decide)
  std::vector<DmTgt> tg;
  u64 n_rows = 0;
  for (auto& e : named) {
    const size_t h = wit.heights[e.c];
    if (!h) continue;  // an inactive target circuit has no rows
    const BlSrc* src = nullptr;
    for (auto& s : srcs)
      if (s.mult && s.circuit == e.c) src = &s;
    BMat& tr = wit.traces[e.c];
    if (!src || !tr.buf.p || tr.ld < h) throw std::runtime_error(name + ": an active circuit has no trace on this device");  // (bl_sources has checked h and w)
    DmTgt g{};
    g.row0 = n_rows, g.msg_base = src->base;
    g.col = tr.col(e.m), g.mult = const_cast<u32*>(src->mult);  // (src->mult: a temporary of this call)
    g.L = src->L, g.j = (u32)e.j, g.pull = e.pull ? 1 : 0;
    tg.push_back(g);
    n_rows += h;
  }

  size_t cap = 64;
  while (cap < 2 * M) cap <<= 1;
  const size_t n_blocks = (M + BL_BLOCK - 1) / BL_BLOCK, row_blocks = (size_t)((n_rows + 255) / 256);
  // four arrays of bb_lb_dev.h and first_target: the smallest origin of a target row with the slot's tuple (all-ones: none)
  DBuf<u64> table = bl_alloc<u64>(ctx, 5 * cap, DM_CALL, "its grouping table, 40 bytes x " + std::to_string(cap) + " slots");
  DBuf<u64> slot_of = bl_alloc<u64>(ctx, std::max<size_t>(n_rows, 1), DM_CALL, "one word per target row");
  DBuf<u64> rep = bl_alloc<u64>(ctx, DM_C_WORDS, DM_CALL, "its counters"), marks = bl_alloc<u64>(ctx, n_blocks * BL_WORDS, DM_CALL, "its mark bitmap"),
            wg_prefix = bl_alloc<u64>(ctx, n_blocks, DM_CALL, "its per-workgroup offsets");
  DBuf<u32> wg_counts = bl_alloc<u32>(ctx, n_blocks, DM_CALL, "its per-workgroup counts");
  DBuf<BlSrc> d_srcs = bl_alloc<BlSrc>(ctx, srcs.size(), DM_CALL, "its source table");
  DBuf<DmTgt> d_tg = bl_alloc<DmTgt>(ctx, std::max<size_t>(tg.size(), 1), DM_CALL, "its target table");
  // the buffers of the second phase, at the caller's capacities: no allocation may follow the first write to the witness (dm_zero_k and
  // dm_write_k), so that an allocation failure leaves it as it was
  for (auto& cl : wit.claims) max_len = std::max(max_len, cl.size());
  const size_t args_room = std::min(args_out ? args_cap : 0, entries_cap * max_len);
  DBuf<u64> d_entries;
  DBuf<u32> d_args;
  if (entries_cap) {
    d_entries = bl_alloc<u64>(ctx, entries_cap * MS_LB_ENTRY_WORDS, DM_CALL, "its entries");
    d_args = bl_alloc<u32>(ctx, std::max<size_t>(args_room, 1), DM_CALL, "its tuples");
  }
  ctx.h2d(d_srcs.p, srcs.data(), srcs.size() * sizeof(BlSrc));
  if (!tg.empty()) ctx.h2d(d_tg.p, tg.data(), tg.size() * sizeof(DmTgt));
  BlTab t;
  t.owner = table.p, t.sum = table.p + cap, t.members = table.p + 2 * cap, t.first = table.p + 3 * cap;
  t.cap_mask = cap - 1, t.hash_mask = bl_hash_mask(), t.n_msgs = M;
  u64* first_target = table.p + 4 * cap;
  const u32 ns = (u32)srcs.size(), nt = (u32)tg.size();
  HIP_CHECK(hipMemsetAsync(first_target, 0xff, cap * 8, ctx.stream));
  if (n_rows) hipLaunchKernelGGL(dm_zero_k, dim3((unsigned)row_blocks), dim3(256), 0, ctx.stream, d_tg.p, nt, n_rows);
  hipLaunchKernelGGL(bl_init_k, dim3((unsigned)((std::max(cap, rep.n) + 255) / 256)), dim3(256), 0, ctx.stream, t, rep.p, rep.n);
  hipLaunchKernelGGL(bl_insert_k, dim3((unsigned)n_blocks), dim3(BL_T), 0, ctx.stream, t, d_srcs.p, ns, rep.p);
  if (n_rows) {
    hipLaunchKernelGGL(dm_probe_k, dim3((unsigned)row_blocks), dim3(256), 0, ctx.stream, t, d_srcs.p, ns, d_tg.p, nt, n_rows, first_target, slot_of.p);
    hipLaunchKernelGGL(dm_claim_k, dim3((unsigned)row_blocks), dim3(256), 0, ctx.stream, t, d_srcs.p, ns, d_tg.p, nt, n_rows, first_target, slot_of.p,
                       rep.p);
  }
  hipLaunchKernelGGL(dm_report_k, dim3((unsigned)n_blocks), dim3(BL_T), 0, ctx.stream, t, d_srcs.p, ns, first_target, rep.p, marks.p, wg_counts.p);
  if (n_rows)
    hipLaunchKernelGGL(dm_write_k, dim3((unsigned)row_blocks), dim3(256), 0, ctx.stream, t, d_tg.p, nt, n_rows, first_target, slot_of.p, rep.p);
  HIP_CHECK(hipGetLastError());
  // first host wait: the counters
  u64 h[DM_C_WORDS];
  ctx.d2h(h, rep.p, sizeof(h));
  if (h[BL_C_FLAG]) throw std::runtime_error(name + ": internal error (a probe sequence of the grouping table reached its bound)");
  summary[0] = h[BL_C_MSGS], summary[1] = h[BL_C_GROUPS], summary[2] = h[DM_C_SERVED], summary[3] = h[BL_C_UNBALANCED], summary[4] = h[DM_C_DUPLICATES];
  const size_t n_out = (size_t)std::min<u64>(summary[3], entries_cap);
  summary[5] = n_out;
  if (!n_out) return;

  // some demand is unserved: its first n_out groups, in origin order, and their tuples - the second host wait
  const size_t n_args = std::min(args_out ? args_cap : 0, n_out * max_len);  // (<= args_room: n_out <= entries_cap)
  HIP_CHECK(hipMemsetAsync(d_args.p, 0, std::max<size_t>(n_args, 1) * 4, ctx.stream));
  HIP_CHECK(hipMemsetAsync(d_entries.p, 0, n_out * MS_LB_ENTRY_WORDS * 8, ctx.stream));  // (bl_args_k reads every entry, written or not)
  hipLaunchKernelGGL(bl_scan_k, dim3(1), dim3(BL_T), 0, ctx.stream, wg_counts.p, wg_prefix.p, n_blocks);
  hipLaunchKernelGGL(bl_entries_k, dim3((unsigned)n_blocks), dim3(64), 0, ctx.stream, t, d_srcs.p, ns, marks.p, wg_counts.p, wg_prefix.p, d_entries.p,
                     (u64)n_out, rep.p);
  hipLaunchKernelGGL(bl_args_k, dim3(1), dim3(BL_T), 0, ctx.stream, d_srcs.p, ns, d_entries.p, (u64)n_out, rep.p, d_args.p, (u64)n_args);
  HIP_CHECK(hipGetLastError());
  u64 flag = 0;
  ctx.d2h_queue(&flag, rep.p + BL_C_FLAG, 8);
  if (n_args) ctx.d2h_queue(args_out, d_args.p, n_args * 4);
  ctx.d2h(entries, d_entries.p, n_out * MS_LB_ENTRY_WORDS * 8);
  if (flag) throw std::runtime_error(name + ": internal error (an unserved group was not found in the grouping table)");
}

}  // namespace msbb
