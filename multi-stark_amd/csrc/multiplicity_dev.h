// Table multiplicity columns derived on the device, the part that is one text in both fields (ms_witness_derive_multiplicities
// in multiplicity.hip, msbb_witness_derive_multiplicities in bb_multiplicity.hip; the definition is in include/mstark.h): the
// caller names the lookup slots that act as providers (TARGETS: their multiplicity is one main-trace column, optionally negated),
// every other message of the witness is DEMAND, and the call writes into each target's column what makes the demand cancel - what
// witness builders compute on the host with a histogram. The grouping is that of the lookup balance (lb_dev.h: the open-addressed
// table in HBM, LDS pre-aggregation, exact sums modulo p, the policy F that describes a field), followed by a write instead of a
// report.
//
// All launches go to the context's stream, in this order:
//   dm_zero_k    zeroes the multiplicity of every target row in the lookup values the sources read (held by the witness, or
//                temporaries of the call): multiplicity 0 does not exist for lb_insert_k, so the table receives the demand only
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
//                stores the group's demand D through the policy (F::store: v = D for a pull, p - D for a push, into the cell
//                as the field's trace keeps it); every other row stores 0 and is counted as a duplicate, one ballot and one
//                atomic per wave
// Nothing depends on thread order or on the hash: origins decide providers, sums are exact, marks lie at fixed positions. Bounded
// loops raise the flag of lb_dev.h, which the host turns into MS_ERR (the derived columns are unspecified then).
#pragma once
#include <algorithm>

#include "lb_dev.h"

namespace msamd {
namespace {

enum { DM_C_SERVED = LB_C_WORDS, DM_C_DUPLICATES, DM_C_WORDS };  // after the four counters of lb_dev.h ([2]: unserved groups)

template <class F>
struct DmTgt {  // one target slot of an active circuit; its rows are the target rows from row0 up to the next target's row0
  u64 row0, msg_base;      // msg_base: the circuit's first message (LbSrc::base)
  typename F::Word* mult;  // the multiplicities lb_msg reads
  u32 L, j, pull, pad;
  typename F::Cell cell;   // where the derived column lies
};

// target row k -> its target, row and message index (origin)
template <class F>
__device__ const DmTgt<F>& dm_row(const DmTgt<F>* tg, u32 nt, u64 k, u64& r, u64& i) {
  u32 lo = 0, hi = nt;
  while (hi - lo > 1) {
    const u32 mid = (lo + hi) >> 1;
    if (tg[mid].row0 <= k) lo = mid; else hi = mid;
  }
  const DmTgt<F>& g = tg[lo];
  r = k - g.row0;
  i = g.msg_base + r * g.L + g.j;
  return g;
}

template <class F>
__global__ __launch_bounds__(256) void dm_zero_k(const DmTgt<F>* tg, u32 nt, u64 n_rows) {
  const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
  if (k >= n_rows) return;
  u64 r, i;
  const DmTgt<F>& g = dm_row(tg, nt, k, r, i);
  g.mult[r * g.L + g.j] = 0;
}

template <class F>
__global__ __launch_bounds__(256) void dm_probe_k(LbTab<F> t, const LbSrc<F>* srcs, u32 ns, const DmTgt<F>* tg, u32 nt, u64 n_rows, u64* first_target,
                                                  u64* slot_of) {
  const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
  if (k >= n_rows) return;
  u64 r, i, s;
  dm_row(tg, nt, k, r, i);
  const LbMsg<F> m = lb_msg(srcs, ns, i);
  if (lb_lookup(t, srcs, ns, i, m, s)) {
    atomicMin((unsigned long long*)&first_target[s], (unsigned long long)i);
    slot_of[k] = s;
  } else {
    slot_of[k] = LB_EMPTY;
  }
}

template <class F>
__global__ __launch_bounds__(256) void dm_claim_k(LbTab<F> t, const LbSrc<F>* srcs, u32 ns, const DmTgt<F>* tg, u32 nt, u64 n_rows, u64* first_target,
                                                  u64* slot_of, u64* counters) {
  const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
  if (k >= n_rows || slot_of[k] != LB_EMPTY) return;
  u64 r, i, s;
  dm_row(tg, nt, k, r, i);
  const LbMsg<F> m = lb_msg(srcs, ns, i);
  if (!lb_claim(t, srcs, ns, i, m, lb_hash(m, t.hash_mask), s)) {
    atomicOr((unsigned long long*)&counters[LB_C_FLAG], 4ull);
    return;
  }
  atomicMin((unsigned long long*)&first_target[s], (unsigned long long)i);
  slot_of[k] = s;
}

template <class F>
__global__ __launch_bounds__(LB_T) void dm_report_k(LbTab<F> t, const LbSrc<F>* srcs, u32 ns, const u64* first_target, u64* counters, u64* marks,
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
      const LbMsg<F> m = lb_msg(srcs, ns, i);
      if (m.mult != 0) {  // (the target rows have none: dm_zero_k)
        n_msgs++;
        u64 s;
        if (!lb_lookup(t, srcs, ns, i, m, s)) {
          failed = true;
        } else if (t.first[s] == i) {
          n_groups++;
          if (F::net(t, s) != 0) {
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

template <class F>
__global__ __launch_bounds__(256) void dm_write_k(LbTab<F> t, const DmTgt<F>* tg, u32 nt, u64 n_rows, const u64* first_target, const u64* slot_of,
                                                  u64* counters) {
  const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
  bool dup = false;
  if (k < n_rows) {
    u64 r, i;
    const DmTgt<F>& g = dm_row(tg, nt, k, r, i);
    const u64 s = slot_of[k];
    if (s != LB_EMPTY) {  // (all-ones: dm_claim_k found the table full and raised the flag)
      const bool provider = first_target[s] == i;
      F::store(g, r, provider ? F::net(t, s) : 0);
      dup = !provider;
    }
  }
  const unsigned long long b = __ballot(dup);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd((unsigned long long*)&counters[DM_C_DUPLICATES], (unsigned long long)__popcll(b));
}

// The call. Two things are the field's own and come as callables:
//   refuse(circuit, column, what)      a further reason why the target `what`, otherwise eligible, is refused (throws)
//   place(circuit index, column, rows, cell) -> false: the circuit has no trace on this device; else cell is where its column lies
template <class F, class Sys, class Wit, class Refuse, class Place>
void dm_derive(Sys& sys, Wit& wit, const ms_mult_target* targets, size_t n_targets, u64 summary[MS_DM_SUMMARY_WORDS], u64* entries,
               size_t entries_cap, typename F::Word* args_out, size_t args_cap, Refuse refuse, Place place) {
  using Word = typename F::Word;
  Ctx& ctx = *sys.ctx;
  const char* call = F::call_derive;
  const std::string name(call);
  F::accept(sys, wit, call);
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
    refuse(sys.circuits[c], (size_t)o[1], name + ": " + what);
    for (auto& e : named)
      if (e.c == c && e.m == o[1]) throw std::runtime_error(name + ": " + what + " shares the derived column " + std::to_string(o[1]) + " with an earlier target");
    named.push_back({c, j, (size_t)o[1], o[2] != 0});
  }

  // (the sources are read or swept into temporaries of the call only: an error raised there leaves the witness as it was)
  std::vector<LbSrc<F>> srcs;
  std::vector<DBuf<Word>> keep;
  size_t max_len = 0;
  const size_t M = F::sources(sys, wit, call, srcs, keep, max_len);
  if (M == 0) return;

  // the target slots of active circuits, in the order they were named (the order does not matter: origins decide)
  std::vector<DmTgt<F>> tg;
  u64 n_rows = 0;
  for (auto& e : named) {
    const size_t h = wit.heights[e.c];
    if (!h) continue;  // an inactive target circuit has no rows
    const LbSrc<F>* src = nullptr;
    for (auto& s : srcs)
      if (s.mult && s.circuit == e.c) src = &s;
    DmTgt<F> g{};
    if (!src || !place(e.c, e.m, h, g.cell)) throw std::runtime_error(name + ": an active circuit has no trace on this device");
    g.row0 = n_rows, g.msg_base = src->base;
    g.mult = const_cast<Word*>(src->mult);  // (held by the witness or a temporary of this call)
    g.L = src->L, g.j = (u32)e.j, g.pull = e.pull ? 1 : 0;
    tg.push_back(g);
    n_rows += h;
  }

  const size_t row_blocks = (size_t)((n_rows + 255) / 256);
  // the arrays of lb_dev.h and first_target: the smallest origin of a target row with the slot's tuple (all-ones: none)
  LbRun<F> run;
  run.alloc_table(ctx, call, M, 1);
  DBuf<u64> slot_of = lb_alloc<u64>(ctx, std::max<size_t>(n_rows, 1), call, "one word per target row");
  run.alloc_rest(ctx, call, DM_C_WORDS, srcs.size());
  DBuf<DmTgt<F>> d_tg = lb_alloc<DmTgt<F>>(ctx, std::max<size_t>(tg.size(), 1), call, "its target table");
  // the buffers of the second phase, at the caller's capacities: no allocation may follow the first write to the witness
  // (dm_zero_k, where the witness holds the lookup values, and dm_write_k), so that an allocation failure leaves it as it was
  max_len = std::max(max_len, F::max_claim_len(wit));
  const size_t args_room = std::min(args_out ? args_cap : 0, entries_cap * max_len);
  DBuf<u64> d_entries;
  DBuf<Word> d_args;
  if (entries_cap) {
    d_entries = lb_alloc<u64>(ctx, entries_cap * MS_LB_ENTRY_WORDS, call, "its entries");
    d_args = lb_alloc<Word>(ctx, std::max<size_t>(args_room, 1), call, "its tuples");
  }
  ctx.h2d(run.d_srcs.p, srcs.data(), srcs.size() * sizeof(LbSrc<F>));
  if (!tg.empty()) ctx.h2d(d_tg.p, tg.data(), tg.size() * sizeof(DmTgt<F>));
  const LbTab<F>& t = run.t;
  u64* first_target = run.extra;
  const u32 ns = run.ns, nt = (u32)tg.size();
  const dim3 rows_grid((unsigned)row_blocks), msgs_grid((unsigned)run.n_blocks);
  HIP_CHECK(hipMemsetAsync(first_target, 0xff, run.cap * 8, ctx.stream));
  if (n_rows) hipLaunchKernelGGL(dm_zero_k<F>, rows_grid, dim3(256), 0, ctx.stream, d_tg.p, nt, n_rows);
  run.insert(ctx);
  if (n_rows) {
    hipLaunchKernelGGL(dm_probe_k<F>, rows_grid, dim3(256), 0, ctx.stream, t, run.d_srcs.p, ns, d_tg.p, nt, n_rows, first_target, slot_of.p);
    hipLaunchKernelGGL(dm_claim_k<F>, rows_grid, dim3(256), 0, ctx.stream, t, run.d_srcs.p, ns, d_tg.p, nt, n_rows, first_target, slot_of.p, run.rep.p);
  }
  hipLaunchKernelGGL(dm_report_k<F>, msgs_grid, dim3(LB_T), 0, ctx.stream, t, run.d_srcs.p, ns, first_target, run.rep.p, run.marks.p, run.wg_counts.p);
  if (n_rows) hipLaunchKernelGGL(dm_write_k<F>, rows_grid, dim3(256), 0, ctx.stream, t, d_tg.p, nt, n_rows, first_target, slot_of.p, run.rep.p);
  HIP_CHECK(hipGetLastError());
  // first host wait: the counters
  u64 h[DM_C_WORDS];
  ctx.d2h(h, run.rep.p, sizeof(h));
  if (h[LB_C_FLAG]) throw std::runtime_error(name + ": internal error (a probe sequence of the grouping table reached its bound)");
  summary[0] = h[LB_C_MSGS], summary[1] = h[LB_C_GROUPS], summary[2] = h[DM_C_SERVED], summary[3] = h[LB_C_UNBALANCED], summary[4] = h[DM_C_DUPLICATES];
  const size_t n_out = (size_t)std::min<u64>(summary[3], entries_cap);
  summary[5] = n_out;
  if (!n_out) return;

  // some demand is unserved: its first n_out groups, in origin order, and their tuples - the second host wait
  const size_t n_args = std::min(args_out ? args_cap : 0, n_out * max_len);  // (<= args_room: n_out <= entries_cap)
  run.entries(ctx, call, "an unserved group", n_out, n_args, d_entries, d_args, entries, args_out);
}

}  // namespace
}  // namespace msamd
