// Exact lookup balance on the device for the BabyBear configuration (msbb_witness_lookup_balance): the definition of the "Lookup
// balance" section of include/mstark.h over p = 2^31 - 2^27 + 1. Every message of the witness - each claim, each (active
// circuit, row, lookup slot) with a non-zero multiplicity - is grouped by its tuple (trailing zeros stripped, as the Horner
// fingerprint of src/lookup.rs:373-384 does not see them), the multiplicities of a group are summed modulo p, and the groups
// whose sum is not zero are reported with where they came from. The design is balance.hip's, re-derived for this field's data.
//
// The grouping table, the sweep of the lookup values the witness does not hold, the compaction of the entries and the invariants
// they rest on are in bb_lb_dev.h, which msbb_witness_derive_multiplicities (bb_multiplicity.hip) shares. Here:
//   bl_report_k  walks the messages again, finds each one's slot read-only, counts messages / groups / unbalanced groups
//                and per-source messages of unbalanced groups, and marks the first origins of unbalanced groups in a bitmap
//                (one 64-bit ballot per wave, at a fixed position: nothing depends on a race)
#include "bb_lb_dev.h"

namespace msbb {
namespace {

constexpr const char* BL_CALL = "msbb_witness_lookup_balance";
constexpr unsigned BL_HIST = 1024;       // per-source counters up to this many are summed in LDS first

__global__ __launch_bounds__(BL_T) void bl_report_k(BlTab t, const BlSrc* srcs, u32 ns, u64* counters, u64* slot_counts, u32 n_slot_words,
                                                    u64* marks, u32* wg_counts) {
  __shared__ u32 hist[BL_HIST];
  __shared__ u32 tot[4];
  const bool use_hist = n_slot_words <= BL_HIST;
  if (use_hist)
    for (u32 e = threadIdx.x; e < n_slot_words; e += BL_T) hist[e] = 0;
  if (threadIdx.x < 4) tot[threadIdx.x] = 0;
  __syncthreads();
  u32 n_msgs = 0, n_groups = 0, n_unb = 0;
  bool failed = false;
  for (u32 it = 0; it < BL_PER; it++) {
    const u64 i = (u64)blockIdx.x * BL_BLOCK + it * BL_T + threadIdx.x;
    bool mark = false;
    if (i < t.n_msgs) {
      const BlMsg m = bl_msg(srcs, ns, i);
      if (m.mult != 0) {
        n_msgs++;
        u64 s;
        if (!bl_lookup(t, srcs, ns, i, m, s)) {
          failed = true;
        } else {
          const bool unb = bl_net(t, s) != 0, is_first = t.first[s] == i;
          n_groups += is_first;
          mark = unb && is_first;
          n_unb += mark;
          if (unb) {
            const BlSrc& src = srcs[m.src];
            const u32 word = src.mult ? src.slot0 + (u32)(i - src.base) % src.L : n_slot_words - 1;
            if (use_hist) atomicAdd(&hist[word], 1u);
            else atomicAdd((unsigned long long*)&slot_counts[word], 1ull);
          }
        }
      }
    }
    const unsigned long long b = __ballot(mark);  // the wave's 64 messages are consecutive and start at a multiple of 64
    if ((threadIdx.x & 63) == 0) marks[(size_t)blockIdx.x * BL_WORDS + it * (BL_T / 64) + (threadIdx.x >> 6)] = b;
  }
  if (n_msgs) atomicAdd(&tot[0], n_msgs);
  if (n_groups) atomicAdd(&tot[1], n_groups);
  if (n_unb) atomicAdd(&tot[2], n_unb);
  if (failed) atomicOr((unsigned long long*)&counters[BL_C_FLAG], 2ull);
  __syncthreads();
  if (threadIdx.x < 3 && tot[threadIdx.x]) atomicAdd((unsigned long long*)&counters[threadIdx.x], (unsigned long long)tot[threadIdx.x]);
  if (threadIdx.x == 0) wg_counts[blockIdx.x] = tot[2];
  if (use_hist)
    for (u32 e = threadIdx.x; e < n_slot_words; e += BL_T)
      if (hist[e]) atomicAdd((unsigned long long*)&slot_counts[e], (unsigned long long)hist[e]);
}

}  // namespace

size_t lookup_balance_slots(const BSystem& sys) {
  size_t n = 0;
  for (auto& c : sys.circuits) n += c.num_lookups;
  return n;
}

void witness_lookup_balance(BSystem& sys, BWitness& wit, u64 summary[4], u64* entries, size_t entries_cap, u32* args_out, size_t args_cap,
                            u64* slot_counts) {
  Ctx& ctx = *sys.ctx;
  bl_accept(sys, wit, BL_CALL);
  const size_t n_slots = lookup_balance_slots(sys);
  for (int k = 0; k < 4; k++) summary[k] = 0;
  if (slot_counts) memset(slot_counts, 0, (n_slots + 1) * 8);

  // the sources in origin order; each active circuit's lookup values are swept into temporaries of the call
  std::vector<BlSrc> srcs;
  std::vector<DBuf<u32>> keep;
  size_t max_len = 0;
  if (n_slots + 1 > 0xffffffffu) throw std::runtime_error("msbb_witness_lookup_balance: too many lookup slots");
  const size_t M = bl_sources(sys, wit, BL_CALL, srcs, keep, max_len);
  if (M == 0) return;

  size_t cap = 64;
  while (cap < 2 * M) cap <<= 1;
  const size_t n_blocks = (M + BL_BLOCK - 1) / BL_BLOCK;
  DBuf<u64> table = bl_alloc<u64>(ctx, 4 * cap, BL_CALL, "its grouping table, 32 bytes x " + std::to_string(cap) + " slots");
  // [4 counters | n_slots + 1 per-source counts], the mark bitmap, the per-workgroup counts and their scan
  DBuf<u64> rep = bl_alloc<u64>(ctx, BL_C_WORDS + n_slots + 1, BL_CALL, "its counters"),
            marks = bl_alloc<u64>(ctx, n_blocks * BL_WORDS, BL_CALL, "its mark bitmap"),
            wg_prefix = bl_alloc<u64>(ctx, n_blocks, BL_CALL, "its per-workgroup offsets");
  DBuf<u32> wg_counts = bl_alloc<u32>(ctx, n_blocks, BL_CALL, "its per-workgroup counts");
  DBuf<BlSrc> d_srcs = bl_alloc<BlSrc>(ctx, srcs.size(), BL_CALL, "its source table");
  ctx.h2d(d_srcs.p, srcs.data(), srcs.size() * sizeof(BlSrc));
  BlTab t;
  t.owner = table.p, t.sum = table.p + cap, t.members = table.p + 2 * cap, t.first = table.p + 3 * cap;
  t.cap_mask = cap - 1, t.hash_mask = bl_hash_mask(), t.n_msgs = M;
  const u32 ns = (u32)srcs.size();
  hipLaunchKernelGGL(bl_init_k, dim3((unsigned)((std::max(cap, rep.n) + 255) / 256)), dim3(256), 0, ctx.stream, t, rep.p, rep.n);
  hipLaunchKernelGGL(bl_insert_k, dim3((unsigned)n_blocks), dim3(BL_T), 0, ctx.stream, t, d_srcs.p, ns, rep.p);
  hipLaunchKernelGGL(bl_report_k, dim3((unsigned)n_blocks), dim3(BL_T), 0, ctx.stream, t, d_srcs.p, ns, rep.p, rep.p + BL_C_WORDS, (u32)(n_slots + 1),
                     marks.p, wg_counts.p);
  HIP_CHECK(hipGetLastError());
  // first host wait: the counters and the per-source counts
  std::vector<u64> h(rep.n);
  ctx.d2h(h.data(), rep.p, rep.n * 8);
  if (h[BL_C_FLAG]) throw std::runtime_error("msbb_witness_lookup_balance: internal error (a probe sequence of the grouping table reached its bound)");
  summary[0] = h[BL_C_MSGS], summary[1] = h[BL_C_GROUPS], summary[2] = h[BL_C_UNBALANCED];
  if (slot_counts) memcpy(slot_counts, h.data() + BL_C_WORDS, (n_slots + 1) * 8);
  const size_t n_out = (size_t)std::min<u64>(summary[2], entries_cap);
  summary[3] = n_out;
  if (!n_out) return;

  // the witness is unbalanced: its first n_out offenders, in origin order, and their tuples - the second host wait
  for (auto& cl : wit.claims) max_len = std::max(max_len, cl.size());
  const size_t n_args = std::min(args_out ? args_cap : 0, n_out * max_len);
  DBuf<u64> d_entries = bl_alloc<u64>(ctx, n_out * MS_LB_ENTRY_WORDS, BL_CALL, "its entries");
  DBuf<u32> d_args = bl_alloc<u32>(ctx, std::max<size_t>(n_args, 1), BL_CALL, "its tuples");
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
  if (flag) throw std::runtime_error("msbb_witness_lookup_balance: internal error (an offender was not found in the grouping table)");
}

}  // namespace msbb
