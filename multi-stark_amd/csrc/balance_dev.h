// Exact lookup balance on the device, the part that is one text in both fields (ms_witness_lookup_balance in balance.hip,
// msbb_witness_lookup_balance in bb_balance.hip): every message of the witness - each claim, each (active circuit, row, lookup
// slot) with a non-zero multiplicity - is grouped by its tuple (trailing zeros stripped, as the Horner fingerprint of
// src/lookup.rs:373-384 does not see them), the multiplicities of a group are summed modulo p, and the groups whose sum is not
// zero are reported with where they came from. No challenges: what the witness check reports as one bit, located.
//
// The grouping table, its insertion kernel and the order-preserving compaction are in lb_dev.h, with the policy F that describes
// a field. Here:
//   lb_report_k  walks the messages again, finds each one's slot read-only, counts messages / groups / unbalanced groups
//                and per-source messages of unbalanced groups, and marks the first origins of unbalanced groups in a bitmap
//                (one 64-bit ballot per wave, at a fixed position: nothing depends on a race)
//   lb_balance   the call: refusals and sources (the policy's), the table, init / insert / report, the first host wait for the
//                counters, and - when some group is unbalanced and the caller has room - the entries behind a second one
#pragma once
#include "lb_dev.h"

namespace msamd {
namespace {

constexpr unsigned LB_HIST = 1024;  // per-source counters up to this many are summed in LDS first

template <class F>
__global__ __launch_bounds__(LB_T) void lb_report_k(LbTab<F> t, const LbSrc<F>* srcs, u32 ns, u64* counters, u64* slot_counts, u32 n_slot_words,
                                                    u64* marks, u32* wg_counts) {
  __shared__ u32 hist[LB_HIST];
  __shared__ u32 tot[4];
  const bool use_hist = n_slot_words <= LB_HIST;
  if (use_hist)
    for (u32 e = threadIdx.x; e < n_slot_words; e += LB_T) hist[e] = 0;
  if (threadIdx.x < 4) tot[threadIdx.x] = 0;
  __syncthreads();
  u32 n_msgs = 0, n_groups = 0, n_unb = 0;
  bool failed = false;
  for (u32 it = 0; it < LB_PER; it++) {
    const u64 i = (u64)blockIdx.x * LB_BLOCK + it * LB_T + threadIdx.x;
    bool mark = false;
    if (i < t.n_msgs) {
      const LbMsg<F> m = lb_msg(srcs, ns, i);
      if (m.mult != 0) {
        n_msgs++;
        u64 s;
        if (!lb_lookup(t, srcs, ns, i, m, s)) {
          failed = true;
        } else {
          const bool unb = F::net(t, s) != 0, is_first = t.first[s] == i;
          n_groups += is_first;
          mark = unb && is_first;
          n_unb += mark;
          if (unb) {
            const LbSrc<F>& src = srcs[m.src];
            const u32 word = src.mult ? src.slot0 + (u32)((typename F::Idx)(i - src.base) % src.L) : n_slot_words - 1;
            if (use_hist) atomicAdd(&hist[word], 1u);
            else atomicAdd((unsigned long long*)&slot_counts[word], 1ull);
          }
        }
      }
    }
    const unsigned long long b = __ballot(mark);  // the wave's 64 messages are consecutive and start at a multiple of 64
    if ((threadIdx.x & 63) == 0) marks[(size_t)blockIdx.x * LB_WORDS + it * (LB_T / 64) + (threadIdx.x >> 6)] = b;
  }
  if (n_msgs) atomicAdd(&tot[0], n_msgs);
  if (n_groups) atomicAdd(&tot[1], n_groups);
  if (n_unb) atomicAdd(&tot[2], n_unb);
  if (failed) atomicOr((unsigned long long*)&counters[LB_C_FLAG], 2ull);
  __syncthreads();
  if (threadIdx.x < 3 && tot[threadIdx.x]) atomicAdd((unsigned long long*)&counters[threadIdx.x], (unsigned long long)tot[threadIdx.x]);
  if (threadIdx.x == 0) wg_counts[blockIdx.x] = tot[2];
  if (use_hist)
    for (u32 e = threadIdx.x; e < n_slot_words; e += LB_T)
      if (hist[e]) atomicAdd((unsigned long long*)&slot_counts[e], (unsigned long long)hist[e]);
}

// n_slots: the lookup slots of the system, lookup_balance_slots(sys)
template <class F, class Sys, class Wit>
void lb_balance(Sys& sys, Wit& wit, size_t n_slots, u64 summary[4], u64* entries, size_t entries_cap, typename F::Word* args_out, size_t args_cap,
                u64* slot_counts) {
  using Word = typename F::Word;
  Ctx& ctx = *sys.ctx;
  const char* call = F::call_balance;
  const std::string name(call);
  F::accept(sys, wit, call);
  for (int k = 0; k < 4; k++) summary[k] = 0;
  if (slot_counts) memset(slot_counts, 0, (n_slots + 1) * 8);
  if (n_slots + 1 > 0xffffffffu) throw std::runtime_error(name + ": too many lookup slots");

  std::vector<LbSrc<F>> srcs;
  std::vector<DBuf<Word>> keep;
  size_t max_len = 0;
  const size_t M = F::sources(sys, wit, call, srcs, keep, max_len);
  if (M == 0) return;

  LbRun<F> run;
  run.alloc_table(ctx, call, M, 0);
  run.alloc_rest(ctx, call, LB_C_WORDS + n_slots + 1, srcs.size());  // [4 counters | n_slots + 1 per-source counts]
  ctx.h2d(run.d_srcs.p, srcs.data(), srcs.size() * sizeof(LbSrc<F>));
  run.insert(ctx);
  hipLaunchKernelGGL(lb_report_k<F>, dim3((unsigned)run.n_blocks), dim3(LB_T), 0, ctx.stream, run.t, run.d_srcs.p, run.ns, run.rep.p,
                     run.rep.p + LB_C_WORDS, (u32)(n_slots + 1), run.marks.p, run.wg_counts.p);
  HIP_CHECK(hipGetLastError());
  // first host wait: the counters and the per-source counts
  std::vector<u64> h(run.rep.n);
  ctx.d2h(h.data(), run.rep.p, run.rep.n * 8);
  if (h[LB_C_FLAG]) throw std::runtime_error(name + ": internal error (a probe sequence of the grouping table reached its bound)");
  summary[0] = h[LB_C_MSGS], summary[1] = h[LB_C_GROUPS], summary[2] = h[LB_C_UNBALANCED];
  if (slot_counts) memcpy(slot_counts, h.data() + LB_C_WORDS, (n_slots + 1) * 8);
  const size_t n_out = (size_t)std::min<u64>(summary[2], entries_cap);
  summary[3] = n_out;
  if (!n_out) return;

  // the witness is unbalanced: its first n_out offenders, in origin order, and their tuples - the second host wait
  max_len = std::max(max_len, F::max_claim_len(wit));
  const size_t n_args = std::min(args_out ? args_cap : 0, n_out * max_len);
  DBuf<u64> d_entries = lb_alloc<u64>(ctx, n_out * MS_LB_ENTRY_WORDS, call, "its entries");
  DBuf<Word> d_args = lb_alloc<Word>(ctx, std::max<size_t>(n_args, 1), call, "its tuples");
  run.entries(ctx, call, "an offender", n_out, n_args, d_entries, d_args, entries, args_out);
}

}  // namespace
}  // namespace msamd
