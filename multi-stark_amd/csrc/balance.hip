// Exact lookup balance on the device (ms_witness_lookup_balance): every message of the witness - each claim, each (active circuit,
// row, lookup slot) with a non-zero multiplicity - is grouped by its tuple (trailing zeros stripped, as the Horner fingerprint
// of src/lookup.rs:373-384 does not see them), the multiplicities of a group are summed modulo p, and the groups whose sum is
// not zero are reported with where they came from. No challenges: what ms_witness_check reports as one bit, located.
//
// The grouping table, its insertion kernel lb_insert_k and the order-preserving compaction (lb_scan_k, lb_entries_k, lb_args_k)
// are in lb_dev.h, which ms_witness_derive_multiplicities (multiplicity.hip) shares. Here:
//   lb_report_k  walks the messages again, finds each one's slot read-only, counts messages / groups / unbalanced groups
//                and per-source messages of unbalanced groups, and marks the first origins of unbalanced groups in a bitmap
//                (one 64-bit ballot per wave, at a fixed position: nothing depends on a race)
#include "lb_dev.h"

namespace msamd {
namespace {

constexpr unsigned LB_HIST = 1024;       // per-source counters up to this many are summed in LDS first
constexpr const char* LB_CALL = "ms_witness_lookup_balance";

__global__ __launch_bounds__(LB_T) void lb_report_k(LbTab t, const LbSrc* srcs, u32 ns, u64* counters, u64* slot_counts, u32 n_slot_words,
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
      const LbMsg m = lb_msg(srcs, ns, i);
      if (m.mult != 0) {
        n_msgs++;
        u64 s;
        if (!lb_lookup(t, srcs, ns, i, m, s)) {
          failed = true;
        } else {
          const bool unb = lb_net(t, s) != 0, is_first = t.first[s] == i;
          n_groups += is_first;
          mark = unb && is_first;
          n_unb += mark;
          if (unb) {
            const LbSrc& src = srcs[m.src];
            const u32 word = src.mult ? src.slot0 + (u32)((i - src.base) % src.L) : n_slot_words - 1;
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

}  // namespace

size_t lookup_balance_slots(const HSystem& sys) {
  size_t n = 0;
  for (auto& c : sys.circuits) n += c.num_lookups;
  return n;
}

void witness_lookup_balance(HSystem& sys, HWitness& wit, u64 summary[4], u64* entries, size_t entries_cap, u64* args_out, size_t args_cap,
                            u64* slot_counts) {
  Ctx& ctx = *sys.ctx;
  lb_accept(sys, wit, LB_CALL);
  const size_t n_slots = lookup_balance_slots(sys), n_claims = wit.claim_offsets.size() - 1;
  for (int k = 0; k < 4; k++) summary[k] = 0;
  if (slot_counts) memset(slot_counts, 0, (n_slots + 1) * 8);

  std::vector<LbSrc> srcs;
  std::vector<DBuf<u64>> keep;
  size_t max_len = 0;
  const size_t M = lb_sources(sys, wit, LB_CALL, srcs, keep, max_len);
  if (M == 0) return;
  if (M >> 40) throw std::runtime_error("ms_witness_lookup_balance: more than 2^40 messages");
  if (n_slots + 1 > 0xffffffffu) throw std::runtime_error("ms_witness_lookup_balance: too many lookup slots");

  size_t cap = 64;
  while (cap < 2 * M) cap <<= 1;
  const u64 hash_mask = lb_hash_mask();
  const size_t n_blocks = (M + LB_BLOCK - 1) / LB_BLOCK;
  DBuf<u64> table = lb_alloc(ctx, 5 * cap, LB_CALL, ("its grouping table, 40 bytes x " + std::to_string(cap) + " slots").c_str());
  // [4 counters | n_slots + 1 per-source counts], the mark bitmap, the per-workgroup counts and their scan
  DBuf<u64> rep(ctx, LB_C_WORDS + n_slots + 1), marks(ctx, n_blocks * LB_WORDS), wg_prefix(ctx, n_blocks);
  DBuf<u32> wg_counts(ctx, n_blocks);
  DBuf<LbSrc> d_srcs(ctx, srcs.size());
  ctx.h2d(d_srcs.p, srcs.data(), srcs.size() * sizeof(LbSrc));
  LbTab t;
  t.owner = table.p, t.small = table.p + cap, t.big = table.p + 2 * cap, t.members = table.p + 3 * cap, t.first = table.p + 4 * cap;
  t.cap_mask = cap - 1, t.hash_mask = hash_mask, t.n_msgs = M;
  const u32 ns = (u32)srcs.size();
  hipLaunchKernelGGL(lb_init_k, dim3((unsigned)((std::max(cap, rep.n) + 255) / 256)), dim3(256), 0, ctx.stream, t, rep.p, rep.n);
  hipLaunchKernelGGL(lb_insert_k, dim3((unsigned)n_blocks), dim3(LB_T), 0, ctx.stream, t, d_srcs.p, ns, rep.p);
  hipLaunchKernelGGL(lb_report_k, dim3((unsigned)n_blocks), dim3(LB_T), 0, ctx.stream, t, d_srcs.p, ns, rep.p, rep.p + LB_C_WORDS, (u32)(n_slots + 1),
                     marks.p, wg_counts.p);
  HIP_CHECK(hipGetLastError());
  // first host wait: the counters and the per-source counts
  std::vector<u64> h(rep.n);
  ctx.d2h(h.data(), rep.p, rep.n * 8);
  if (h[LB_C_FLAG]) throw std::runtime_error("ms_witness_lookup_balance: internal error (a probe sequence of the grouping table reached its bound)");
  summary[0] = h[LB_C_MSGS], summary[1] = h[LB_C_GROUPS], summary[2] = h[LB_C_UNBALANCED];
  if (slot_counts) memcpy(slot_counts, h.data() + LB_C_WORDS, (n_slots + 1) * 8);
  const size_t n_out = (size_t)std::min<u64>(summary[2], entries_cap);
  summary[3] = n_out;
  if (!n_out) return;

  // the witness is unbalanced: its first n_out offenders, in origin order, and their tuples - the second host wait
  for (size_t i = 0; i < n_claims; i++) max_len = std::max<size_t>(max_len, wit.claim_offsets[i + 1] - wit.claim_offsets[i]);
  const size_t n_args = std::min(args_out ? args_cap : 0, n_out * max_len);
  DBuf<u64> d_entries(ctx, n_out * MS_LB_ENTRY_WORDS), d_args(ctx, std::max<size_t>(n_args, 1));
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
  if (flag) throw std::runtime_error("ms_witness_lookup_balance: internal error (an offender was not found in the grouping table)");
}

}  // namespace msamd
