// Table multiplicity columns derived on the device (ms_witness_derive_multiplicities; the definition is in include/mstark.h): the
// caller names the lookup slots that act as providers (TARGETS: their multiplicity is one main-trace column, optionally negated),
// every other message of the witness is DEMAND, and the call writes into each target's column what makes the demand cancel - what
// witness builders compute on the host with a histogram. The grouping is that of ms_witness_lookup_balance (lb_dev.h: the
// open-addressed table in HBM, LDS pre-aggregation, exact sums modulo p), followed by a write instead of a report.
//
// All launches go to the context's stream, in this order:
//   dm_zero_k    zeroes the multiplicity of every target row in the lookup values (held by the witness, or the temporaries
//                computed from its traces): multiplicity 0 does not exist for lb_insert_k, so the table receives the demand only
//   lb_init_k, lb_insert_k   the demand grouped and summed (lb_dev.h)
//   dm_probe_k   serve, pass 1: one thread per target row. A read-only probe finds the group of the row's tuple; a row that
//                finds one takes a 64-bit atomicMin on the slot's `first_target` word with its origin and keeps the slot in
//                slot_of[row]. A row whose tuple has no group claims nothing here
//   dm_claim_k   the rows left over - target tuples nobody demands - are inserted into the SAME table by the claiming probe of
//                lb_insert_k (a separate launch, so that no read-only probe runs beside a claim; owners are learnt only from the
//                value the CAS returns), as groups of no members and net 0, and take the same atomicMin. Equal tuples among them
//                meet in one slot: which of them is a duplicate is decided by origin, not by who came first. The table has room:
//                cap >= 2 x messages counts the target rows
//   dm_report_k  walks the demand again: messages, groups, served and unserved groups of non-zero demand; marks the first origins
//                of the unserved groups in the bitmap the compaction of lb_dev.h reads
//   dm_write_k   serve, pass 2: one thread per target row. The row whose origin is its slot's first_target is the provider and
//                writes v (D for a pull, p - D for a push) into the row-major trace cell and s v = -D into the held multiplicity;
//                every other row writes 0 to both and is counted as a duplicate, one ballot and one atomic per wave
// Nothing depends on thread order or on the hash: origins decide providers, sums are exact, marks lie at fixed positions. Bounded
// loops raise the flag of lb_dev.h, which the host turns into MS_ERR (the derived columns are unspecified then).
#include <algorithm>

#include "lb_dev.h"
#include "mult_slot.h"

namespace msamd {
namespace {

constexpr const char* DM_CALL = "ms_witness_derive_multiplicities";
enum { DM_C_SERVED = LB_C_WORDS, DM_C_DUPLICATES, DM_C_WORDS };  // after the four counters of lb_dev.h ([2]: unserved groups)

struct DmTgt {  // one target slot of an active circuit; its rows are the target rows from row0 up to the next target's row0
  u64 row0, msg_base;        // msg_base: the circuit's first message (LbSrc::base)
  u64 *trace, *mult, *held;  // row-major trace; the multiplicities lb_msg reads; the witness's own (nullptr: it holds none)
  u32 L, j, W, m, pull, pad;
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

__global__ __launch_bounds__(256) void dm_probe_k(LbTab t, const LbSrc* srcs, u32 ns, const DmTgt* tg, u32 nt, u64 n_rows, u64* first_target,
                                                  u64* slot_of) {
  const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
  if (k >= n_rows) return;
  u64 r, i, s;
  dm_row(tg, nt, k, r, i);
  const LbMsg m = lb_msg(srcs, ns, i);
  if (lb_lookup(t, srcs, ns, i, m, s)) {
    atomicMin((unsigned long long*)&first_target[s], (unsigned long long)i);
    slot_of[k] = s;
  } else {
    slot_of[k] = LB_EMPTY;
  }
}

__global__ __launch_bounds__(256) void dm_claim_k(LbTab t, const LbSrc* srcs, u32 ns, const DmTgt* tg, u32 nt, u64 n_rows, u64* first_target,
                                                  u64* slot_of, u64* counters) {
  const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
  if (k >= n_rows || slot_of[k] != LB_EMPTY) return;
  u64 r, i, s;
  dm_row(tg, nt, k, r, i);
  const LbMsg m = lb_msg(srcs, ns, i);
  if (!lb_claim(t, srcs, ns, i, m, lb_hash(m, t.hash_mask), s)) {
    atomicOr((unsigned long long*)&counters[LB_C_FLAG], 4ull);
    return;
  }
  atomicMin((unsigned long long*)&first_target[s], (unsigned long long)i);
  slot_of[k] = s;
}

__global__ __launch_bounds__(LB_T) void dm_report_k(LbTab t, const LbSrc* srcs, u32 ns, const u64* first_target, u64* counters, u64* marks,
                                                    u32* wg_counts) {
  __shared__ u32 tot[4];
  if (threadIdx.x < 4) tot[threadIdx.x] = 0;
  __syncthreads();
  u32 n_msgs = 0, n_groups = 0, n_served = 0, n_unserved = 0;
  bool failed = false;
  for (u32 it = 0; it < LB_PER; it++) {
    const u64 i = (u64)blockIdx.x * LB_BLOCK + it * LB_T + threadIdx.x;
    bool mark = false;
    if (i < t.n_msgs) {
      const LbMsg m = lb_msg(srcs, ns, i);
      if (m.mult != 0) {  // (the target rows have none: dm_zero_k)
        n_msgs++;
        u64 s;
        if (!lb_lookup(t, srcs, ns, i, m, s)) {
          failed = true;
        } else if (t.first[s] == i) {
          n_groups++;
          if (lb_net(t, s) != 0) {
            mark = first_target[s] == LB_EMPTY;
            n_served += !mark;
            n_unserved += mark;
          }
        }
      }
    }
    const unsigned long long b = __ballot(mark);  // the wave's 64 messages are consecutive and start at a multiple of 64
    if ((threadIdx.x & 63) == 0) marks[(size_t)blockIdx.x * LB_WORDS + it * (LB_T / 64) + (threadIdx.x >> 6)] = b;
  }
  if (n_msgs) atomicAdd(&tot[0], n_msgs);
  if (n_groups) atomicAdd(&tot[1], n_groups);
  if (n_unserved) atomicAdd(&tot[2], n_unserved);
  if (n_served) atomicAdd(&tot[3], n_served);
  if (failed) atomicOr((unsigned long long*)&counters[LB_C_FLAG], 2ull);
  __syncthreads();
  if (threadIdx.x < 3 && tot[threadIdx.x]) atomicAdd((unsigned long long*)&counters[threadIdx.x], (unsigned long long)tot[threadIdx.x]);
  if (threadIdx.x == 3 && tot[3]) atomicAdd((unsigned long long*)&counters[DM_C_SERVED], (unsigned long long)tot[3]);
  if (threadIdx.x == 0) wg_counts[blockIdx.x] = tot[2];
}

__global__ __launch_bounds__(256) void dm_write_k(LbTab t, const DmTgt* tg, u32 nt, u64 n_rows, const u64* first_target, const u64* slot_of,
                                                  u64* counters) {
  const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
  bool dup = false;
  if (k < n_rows) {
    u64 r, i;
    const DmTgt& g = dm_row(tg, nt, k, r, i);
    const u64 s = slot_of[k];
    if (s != LB_EMPTY) {  // (all-ones: dm_claim_k found the table full and raised the flag)
      const bool provider = first_target[s] == i;
      const u64 d = provider ? lb_net(t, s) : 0, minus_d = d ? GL_P - d : 0;
      g.trace[r * g.W + g.m] = g.pull ? d : minus_d;
      if (g.held) g.held[r * g.L + g.j] = minus_d;
      dup = !provider;
    }
  }
  const unsigned long long b = __ballot(dup);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd((unsigned long long*)&counters[DM_C_DUPLICATES], (unsigned long long)__popcll(b));
}

}  // namespace

// the classifier is host code over the node program alone (mult_slot.h), shared with the BabyBear configuration
void multiplicity_slot(const HCircuit& c, size_t slot, u64 out3[3]) { multiplicity_slot(c.nodes, c.lookups, slot, out3); }

void witness_derive_multiplicities(HSystem& sys, HWitness& wit, const ms_mult_target* targets, size_t n_targets, u64 summary[MS_DM_SUMMARY_WORDS],
                                   u64* entries, size_t entries_cap, u64* args_out, size_t args_cap) {
  Ctx& ctx = *sys.ctx;
  const std::string name(DM_CALL);
  lb_accept(sys, wit, DM_CALL);
  const size_t C = sys.circuits.size(), n_claims = wit.claim_offsets.size() - 1;
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
    for (auto& e : named)
      if (e.c == c && e.m == o[1]) throw std::runtime_error(name + ": " + what + " shares the derived column " + std::to_string(o[1]) + " with an earlier target");
    named.push_back({c, j, (size_t)o[1], o[2] != 0});
  }

  // (lb_sources writes temporaries of the call only: an error it raises leaves the witness as it was)
  std::vector<LbSrc> srcs;
  std::vector<DBuf<u64>> keep;
  size_t max_len = 0;
  const size_t M = lb_sources(sys, wit, DM_CALL, srcs, keep, max_len);
  if (M == 0) return;
  if (M >> 40) throw std::runtime_error(name + ": more than 2^40 messages");

  // the target slots of active circuits, in origin order of their circuits (the order does not matter: origins decide)
  std::vector<DmTgt> tg;
  u64 n_rows = 0;
  for (auto& e : named) {
    const size_t h = wit.heights[e.c];
    if (!h) continue;  // an inactive target circuit has no rows
    const LbSrc* src = nullptr;
    for (auto& s : srcs)
      if (s.mult && s.circuit == e.c) src = &s;
    if (!src || !wit.traces[e.c].p) throw std::runtime_error(name + ": an active circuit has no trace on this device");
    DmTgt g{};
    g.row0 = n_rows, g.msg_base = src->base;
    g.trace = wit.traces[e.c].p, g.mult = const_cast<u64*>(src->mult), g.held = wit.lookups[e.c].mult.p;  // (src->mult: held or a temporary of this call)
    g.L = src->L, g.j = (u32)e.j, g.W = (u32)sys.circuits[e.c].main_width, g.m = (u32)e.m, g.pull = e.pull ? 1 : 0;
    tg.push_back(g);
    n_rows += h;
  }

  size_t cap = 64;
  while (cap < 2 * M) cap <<= 1;
  const size_t n_blocks = (M + LB_BLOCK - 1) / LB_BLOCK, row_blocks = (size_t)((n_rows + 255) / 256);
  // five arrays of lb_dev.h and first_target: the smallest origin of a target row with the slot's tuple (all-ones: none)
  DBuf<u64> table = lb_alloc(ctx, 6 * cap, DM_CALL, ("its grouping table, 48 bytes x " + std::to_string(cap) + " slots").c_str());
  DBuf<u64> slot_of = lb_alloc(ctx, std::max<size_t>(n_rows, 1), DM_CALL, "one word per target row");
  DBuf<u64> rep(ctx, DM_C_WORDS), marks(ctx, n_blocks * LB_WORDS), wg_prefix(ctx, n_blocks);
  DBuf<u32> wg_counts(ctx, n_blocks);
  DBuf<LbSrc> d_srcs(ctx, srcs.size());
  DBuf<DmTgt> d_tg(ctx, std::max<size_t>(tg.size(), 1));
  // the buffers of the second phase, at the caller's capacities: no allocation may follow the first write to the witness (dm_zero_k), so that
  // an allocation failure leaves it as it was
  for (size_t i = 0; i < n_claims; i++) max_len = std::max<size_t>(max_len, wit.claim_offsets[i + 1] - wit.claim_offsets[i]);
  const size_t args_room = std::min(args_out ? args_cap : 0, entries_cap * max_len);
  DBuf<u64> d_entries, d_args;
  if (entries_cap) {
    d_entries = lb_alloc(ctx, entries_cap * MS_LB_ENTRY_WORDS, DM_CALL, "its entries");
    d_args = lb_alloc(ctx, std::max<size_t>(args_room, 1), DM_CALL, "its tuples");
  }
  ctx.h2d(d_srcs.p, srcs.data(), srcs.size() * sizeof(LbSrc));
  if (!tg.empty()) ctx.h2d(d_tg.p, tg.data(), tg.size() * sizeof(DmTgt));
  LbTab t;
  t.owner = table.p, t.small = table.p + cap, t.big = table.p + 2 * cap, t.members = table.p + 3 * cap, t.first = table.p + 4 * cap;
  t.cap_mask = cap - 1, t.hash_mask = lb_hash_mask(), t.n_msgs = M;
  u64* first_target = table.p + 5 * cap;
  const u32 ns = (u32)srcs.size(), nt = (u32)tg.size();
  HIP_CHECK(hipMemsetAsync(first_target, 0xff, cap * 8, ctx.stream));
  if (n_rows) hipLaunchKernelGGL(dm_zero_k, dim3((unsigned)row_blocks), dim3(256), 0, ctx.stream, d_tg.p, nt, n_rows);
  hipLaunchKernelGGL(lb_init_k, dim3((unsigned)((std::max(cap, rep.n) + 255) / 256)), dim3(256), 0, ctx.stream, t, rep.p, rep.n);
  hipLaunchKernelGGL(lb_insert_k, dim3((unsigned)n_blocks), dim3(LB_T), 0, ctx.stream, t, d_srcs.p, ns, rep.p);
  if (n_rows) {
    hipLaunchKernelGGL(dm_probe_k, dim3((unsigned)row_blocks), dim3(256), 0, ctx.stream, t, d_srcs.p, ns, d_tg.p, nt, n_rows, first_target, slot_of.p);
    hipLaunchKernelGGL(dm_claim_k, dim3((unsigned)row_blocks), dim3(256), 0, ctx.stream, t, d_srcs.p, ns, d_tg.p, nt, n_rows, first_target, slot_of.p,
                       rep.p);
  }
  hipLaunchKernelGGL(dm_report_k, dim3((unsigned)n_blocks), dim3(LB_T), 0, ctx.stream, t, d_srcs.p, ns, first_target, rep.p, marks.p, wg_counts.p);
  if (n_rows)
    hipLaunchKernelGGL(dm_write_k, dim3((unsigned)row_blocks), dim3(256), 0, ctx.stream, t, d_tg.p, nt, n_rows, first_target, slot_of.p, rep.p);
  HIP_CHECK(hipGetLastError());
  // first host wait: the counters
  u64 h[DM_C_WORDS];
  ctx.d2h(h, rep.p, sizeof(h));
  if (h[LB_C_FLAG]) throw std::runtime_error(name + ": internal error (a probe sequence of the grouping table reached its bound)");
  summary[0] = h[LB_C_MSGS], summary[1] = h[LB_C_GROUPS], summary[2] = h[DM_C_SERVED], summary[3] = h[LB_C_UNBALANCED], summary[4] = h[DM_C_DUPLICATES];
  const size_t n_out = (size_t)std::min<u64>(summary[3], entries_cap);
  summary[5] = n_out;
  if (!n_out) return;

  // some demand is unserved: its first n_out groups, in origin order, and their tuples - the second host wait
  const size_t n_args = std::min(args_out ? args_cap : 0, n_out * max_len);  // (<= args_room: n_out <= entries_cap)
  HIP_CHECK(hipMemsetAsync(d_args.p, 0, std::max<size_t>(n_args, 1) * 8, ctx.stream));
  HIP_CHECK(hipMemsetAsync(d_entries.p, 0, n_out * MS_LB_ENTRY_WORDS * 8, ctx.stream));  // (lb_args_k reads every entry, written or not)
  hipLaunchKernelGGL(lb_scan_k, dim3(1), dim3(LB_T), 0, ctx.stream, wg_counts.p, wg_prefix.p, n_blocks);
  hipLaunchKernelGGL(lb_entries_k, dim3((unsigned)n_blocks), dim3(64), 0, ctx.stream, t, d_srcs.p, ns, marks.p, wg_counts.p, wg_prefix.p, d_entries.p,
                     (u64)n_out, rep.p);
  hipLaunchKernelGGL(lb_args_k, dim3(1), dim3(LB_T), 0, ctx.stream, d_srcs.p, ns, d_entries.p, (u64)n_out, rep.p, d_args.p, (u64)n_args);
  HIP_CHECK(hipGetLastError());
  u64 flag = 0;
  ctx.d2h_queue(&flag, rep.p + LB_C_FLAG, 8);
  if (n_args) ctx.d2h_queue(args_out, d_args.p, n_args * 8);
  ctx.d2h(entries, d_entries.p, n_out * MS_LB_ENTRY_WORDS * 8);
  if (flag) throw std::runtime_error(name + ": internal error (an unserved group was not found in the grouping table)");
}

}  // namespace msamd
