// The grouping table of the exact lookup calls, one text for both fields: ms_witness_lookup_balance / msbb_witness_lookup_balance
// (balance_dev.h: report the groups that do not cancel) and ms_witness_derive_multiplicities / msbb_witness_derive_multiplicities
// (multiplicity_dev.h: write what makes them cancel). Include it from a .hip file only; everything lives in an unnamed namespace, so
// each translation unit compiles the kernels it launches for itself, for its own field. A field describes itself by a plain
// policy struct F (GlLookup in gl_lb.h, BbLookup in bb_lb.h):
//   using Word, Idx             the stored word (8 or 4 bytes); the integer that holds a message's index WITHIN its source - the
//                               row and slot of a message are one divide of that width (64-bit where a call takes 2^40
//                               messages, 32-bit where it refuses 2^32)
//   key / mult / report(word)   a stored word as it is stripped, hashed and compared; as the canonical multiplicity that is
//                               summed; as the canonical value a reported tuple shows
//   SUMS                        the number of 8-byte sum arrays of a slot (all start at zero)
//   lds_value(mult, v)          whether this multiplicity may be summed in the LDS table first, and as which 64-bit value v
//   add(t, s, mult)             one message's multiplicity into slot s; false: a bounded loop reached its bound
//   flush(t, s, v)              an LDS entry's sum into slot s
//   net(t, s)                   the group's sum modulo p, canonical (plain loads: a later launch)
//   Cell, store(g, r, d)        multiplicity_dev.h: where a derived cell lies, and the write of the demand d into target row r
//   call_balance, call_derive, accept, sources, max_claim_len   the host side: names for the error texts, the refusals, the
//                               source list with the lookup values found or swept, the longest claim
//
// Messages are numbered in ORIGIN order: claims by index, then the circuits in system order, row-major, slot last. The
// grouping table is open-addressed, in HBM, 3 + SUMS 8-byte arrays of `cap` slots (cap = the power of two >= max(64, 2 x messages)):
//   owner    the message index that claimed the slot (all-ones: free) - its tuple IS the slot's key
//   sum[]    the policy's sums of the group's multiplicities
//   members  number of messages of the group
//   first    smallest message index of the group (atomicMin)
// A slot is claimed by a 64-bit atomicCAS on `owner`, and inside a launch that claims the value that CAS returns is the only
// way a thread learns an owner: no plain load of the word there (another CU's L1 may hold the line from before the claim). Keys
// are never copied: equality is decided on the two messages' tuples, input data written by earlier launches. The hash picks the
// first slot only. What bounds the loops: a probe sequence visits at most `cap` slots and the table holds at most cap / 2
// groups; a policy's own loop has a bound of its own. A loop that reaches its bound raises a flag the host turns into MS_ERR;
// nothing spins.
//   lb_insert_k  groups the messages of non-zero multiplicity. Equal tuples of a workgroup's 1024 consecutive messages are
//                first summed in a 512-entry table in LDS (the bench witness puts 12 x 2^20 byte messages on 256 tuples: one
//                global atomic per message would queue them on a few L2 addresses), which is then flushed, one global insertion
//                per entry; a message that finds no room within 8 LDS probes, or whose multiplicity the policy keeps out of
//                LDS, is inserted directly
//   lb_lookup    read-only probe of a later launch (plain loads)
//   lb_scan_k, lb_entries_k, lb_args_k  order-preserving compaction of the first entries_cap marks of a bitmap over the
//                messages (one word per 64 consecutive messages, LB_WORDS words per workgroup of the marking kernel, whose
//                per-workgroup mark counts are scanned): entries written at fixed positions, then the tuples packed in entry
//                order. counters[LB_C_UNBALANCED] holds the number of marks, counters[LB_C_FLAG] the error flag
#pragma once
#include <cstdlib>
#include <string>

#include "../../include/mstark.h"
#include "msamd.h"

namespace msamd {
namespace {

constexpr u64 LB_EMPTY = ~u64(0);
constexpr unsigned LB_T = 256, LB_PER = 4, LB_BLOCK = LB_T * LB_PER;  // a workgroup owns LB_BLOCK consecutive messages
constexpr unsigned LB_WORDS = LB_BLOCK / 64;                           // ... = that many words of the mark bitmap
constexpr unsigned LB_LDS = 512, LB_LDS_PROBES = 8;

template <class F>
struct LbSrc {  // one source of messages: the claims (mult == nullptr, offs = u64 offsets) or one circuit's lookup values
  u64 base, count;
  const typename F::Word *mult, *args;
  const void* offs;
  u32 L, aw, circuit, slot0;
};
template <class F>
struct LbTab {
  u64 *owner, *sum[F::SUMS], *members, *first;
  u64 cap_mask, hash_mask, n_msgs;
  // the arrays in one allocation of (3 + SUMS) x cap words, in this order -> where a caller's own arrays may follow
  u64* place(u64* p, size_t cap) {
    owner = p, p += cap;
    for (unsigned a = 0; a < F::SUMS; a++) sum[a] = p, p += cap;
    members = p, first = p + cap;
    return p + 2 * cap;
  }
};
template <class F>
struct LbMsg {
  const typename F::Word* p;  // as stored
  typename F::Word mult;      // canonical
  u32 len, src;
};
enum { LB_C_MSGS = 0, LB_C_GROUPS, LB_C_UNBALANCED, LB_C_FLAG, LB_C_WORDS };

template <class F>
__device__ LbMsg<F> lb_msg(const LbSrc<F>* srcs, u32 ns, u64 i) {
  using Idx = typename F::Idx;
  u32 lo = 0, hi = ns;
  while (hi - lo > 1) {
    const u32 mid = (lo + hi) >> 1;
    if (srcs[mid].base <= i) lo = mid; else hi = mid;
  }
  const LbSrc<F>& s = srcs[lo];
  const Idx k = (Idx)(i - s.base);
  LbMsg<F> m;
  m.src = lo;
  if (!s.mult) {
    const u64* off = (const u64*)s.offs;
    const u64 a = off[k];
    m.p = s.args + a;
    m.len = (u32)(off[k + 1] - a);
    m.mult = 1;
  } else {
    const Idx r = k / s.L;
    const u32 j = (u32)(k - r * s.L);
    const u32* off = (const u32*)s.offs;
    m.p = s.args + (size_t)r * s.aw + off[j];
    m.len = off[j + 1] - off[j];
    m.mult = F::mult(s.mult[k]);
  }
  while (m.len && F::key(m.p[m.len - 1]) == 0) m.len--;
  return m;
}

template <class F>
__device__ u64 lb_hash(const LbMsg<F>& m, u64 hash_mask) {
  u64 h = (u64(m.len) + 1) * 0x9E3779B97F4A7C15ULL;
  for (u32 k = 0; k < m.len; k++) {
    h = (h ^ F::key(m.p[k])) * 0xFF51AFD7ED558CCDULL;
    h ^= h >> 29;
  }
  h *= 0xC4CEB9FE1A85EC53ULL;
  h ^= h >> 32;
  return h & hash_mask;
}

template <class F>
__device__ bool lb_eq(const LbMsg<F>& a, const LbMsg<F>& b) {
  if (a.len != b.len) return false;
  for (u32 k = 0; k < a.len; k++)
    if (F::key(a.p[k]) != F::key(b.p[k])) return false;
  return true;
}

// the slot of message i's group, claimed for i when no equal tuple owns one yet; false: the table is full (cannot happen at
// cap >= 2 x messages; the caller raises the flag)
template <class F>
__device__ bool lb_claim(const LbTab<F>& t, const LbSrc<F>* srcs, u32 ns, u64 i, const LbMsg<F>& m, u64 h, u64& slot) {
  u64 s = h & t.cap_mask;
  for (u64 step = 0; step <= t.cap_mask; step++, s = (s + 1) & t.cap_mask) {
    const u64 prev = atomicCAS((unsigned long long*)&t.owner[s], (unsigned long long)LB_EMPTY, (unsigned long long)i);
    if (prev == LB_EMPTY || prev == i || lb_eq(lb_msg(srcs, ns, prev), m)) {
      slot = s;
      return true;
    }
  }
  return false;
}

template <class F>
__device__ void lb_count(const LbTab<F>& t, u64 s, u64 members, u64 first) {
  atomicAdd((unsigned long long*)&t.members[s], (unsigned long long)members);
  atomicMin((unsigned long long*)&t.first[s], (unsigned long long)first);
}

template <class F>
__global__ void lb_init_k(LbTab<F> t, u64* zeros, size_t n_zeros) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= t.cap_mask) {
    t.owner[i] = LB_EMPTY;
    t.first[i] = LB_EMPTY;
    for (unsigned a = 0; a < F::SUMS; a++) t.sum[a][i] = 0;
    t.members[i] = 0;
  }
  if (i < n_zeros) zeros[i] = 0;
}

template <class F>
__global__ __launch_bounds__(LB_T) void lb_insert_k(LbTab<F> t, const LbSrc<F>* srcs, u32 ns, u64* counters) {
  __shared__ u64 l_key[LB_LDS], l_sum[LB_LDS], l_min[LB_LDS];
  __shared__ u32 l_cnt[LB_LDS];
  for (u32 e = threadIdx.x; e < LB_LDS; e += LB_T) l_key[e] = LB_EMPTY, l_sum[e] = 0, l_min[e] = LB_EMPTY, l_cnt[e] = 0;
  __syncthreads();
  bool failed = false;
  for (u32 it = 0; it < LB_PER; it++) {
    const u64 i = (u64)blockIdx.x * LB_BLOCK + it * LB_T + threadIdx.x;
    if (i >= t.n_msgs) break;
    const LbMsg<F> m = lb_msg(srcs, ns, i);
    if (m.mult == 0) continue;
    const u64 h = lb_hash(m, t.hash_mask);
    u64 v;
    bool done = false;
    if (F::lds_value(m.mult, v)) {
      u32 ls = (u32)h & (LB_LDS - 1);
      for (u32 probe = 0; probe < LB_LDS_PROBES && !done; probe++, ls = (ls + 1) & (LB_LDS - 1)) {
        const u64 prev = atomicCAS((unsigned long long*)&l_key[ls], (unsigned long long)LB_EMPTY, (unsigned long long)i);
        if (prev == LB_EMPTY || prev == i || lb_eq(lb_msg(srcs, ns, prev), m)) {
          atomicAdd((unsigned long long*)&l_sum[ls], (unsigned long long)v);
          atomicMin((unsigned long long*)&l_min[ls], (unsigned long long)i);
          atomicAdd(&l_cnt[ls], 1u);
          done = true;
        }
      }
    }
    if (!done) {
      u64 s;
      if (lb_claim(t, srcs, ns, i, m, h, s)) {
        lb_count(t, s, 1, i);
        if (!F::add(t, s, m.mult)) failed = true;
      } else {
        failed = true;
      }
    }
  }
  __syncthreads();
  for (u32 e = threadIdx.x; e < LB_LDS; e += LB_T) {
    const u64 rep = l_key[e];
    if (rep == LB_EMPTY) continue;
    const LbMsg<F> m = lb_msg(srcs, ns, rep);
    u64 s;
    if (lb_claim(t, srcs, ns, rep, m, lb_hash(m, t.hash_mask), s)) {
      lb_count(t, s, l_cnt[e], l_min[e]);
      F::flush(t, s, l_sum[e]);
    } else {
      failed = true;
    }
  }
  if (failed) atomicOr((unsigned long long*)&counters[LB_C_FLAG], 1ull);
}

// read-only: the slot that holds message i's group (written by an earlier launch: plain loads)
template <class F>
__device__ bool lb_lookup(const LbTab<F>& t, const LbSrc<F>* srcs, u32 ns, u64 i, const LbMsg<F>& m, u64& slot) {
  u64 s = lb_hash(m, t.hash_mask) & t.cap_mask;
  for (u64 step = 0; step <= t.cap_mask; step++, s = (s + 1) & t.cap_mask) {
    const u64 o = t.owner[s];
    if (o == LB_EMPTY) return false;
    if (o == i || lb_eq(lb_msg(srcs, ns, o), m)) {
      slot = s;
      return true;
    }
  }
  return false;
}

// exclusive scan of the per-workgroup mark counts, one workgroup: a contiguous chunk per thread, the 256 chunk sums by thread 0
__global__ __launch_bounds__(LB_T) void lb_scan_k(const u32* wg_counts, u64* wg_prefix, size_t n_blocks) {
  __shared__ u64 part[LB_T];
  const size_t chunk = (n_blocks + LB_T - 1) / LB_T, a = threadIdx.x * chunk, b = a + chunk < n_blocks ? a + chunk : n_blocks;
  u64 sum = 0;
  for (size_t k = a; k < b; k++) sum += wg_counts[k];
  part[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 run = 0;
    for (u32 k = 0; k < LB_T; k++) {
      const u64 v = part[k];
      part[k] = run;
      run += v;
    }
  }
  __syncthreads();
  u64 run = part[threadIdx.x];
  for (size_t k = a; k < b; k++) {
    wg_prefix[k] = run;
    run += wg_counts[k];
  }
}

// one wave per workgroup of the marking kernel: lane w < LB_WORDS takes bitmap word w; entry e goes to position prefix + rank
template <class F>
__global__ __launch_bounds__(64) void lb_entries_k(LbTab<F> t, const LbSrc<F>* srcs, u32 ns, const u64* marks, const u32* wg_counts,
                                                   const u64* wg_prefix, u64* entries, u64 cap, u64* counters) {
  if (wg_counts[blockIdx.x] == 0 || wg_prefix[blockIdx.x] >= cap || threadIdx.x >= LB_WORDS) return;
  const u64* words = marks + (size_t)blockIdx.x * LB_WORDS;
  u64 pos = wg_prefix[blockIdx.x];
  for (u32 w = 0; w < threadIdx.x; w++) pos += __popcll(words[w]);
  u64 bits = words[threadIdx.x];
  for (u32 k = 0; k < 64 && bits && pos < cap; k++, pos++) {
    const u32 bit = __ffsll((unsigned long long)bits) - 1;
    bits &= bits - 1;
    const u64 i = ((u64)blockIdx.x * LB_WORDS + threadIdx.x) * 64 + bit;
    const LbMsg<F> m = lb_msg(srcs, ns, i);
    const LbSrc<F>& src = srcs[m.src];
    u64 s = 0;
    if (!lb_lookup(t, srcs, ns, i, m, s)) {
      atomicOr((unsigned long long*)&counters[LB_C_FLAG], 2ull);
      return;
    }
    u64* e = entries + pos * MS_LB_ENTRY_WORDS;
    const typename F::Idx k_in = (typename F::Idx)(i - src.base);
    e[0] = src.mult ? src.circuit : MS_LB_CLAIMS;
    e[1] = src.mult ? k_in / src.L : k_in;
    e[2] = src.mult ? k_in % src.L : 0;
    e[3] = F::net(t, s);
    e[4] = t.members[s];
    e[5] = m.len;
    e[6] = ~u64(0);
    e[7] = i;  // for lb_args_k, which puts the reserved zero here
  }
}

// offsets of the tuples in entry order and the tuples themselves (canonical), one workgroup: 256 entries per round, their
// lengths scanned by thread 0
template <class F>
__global__ __launch_bounds__(LB_T) void lb_args_k(const LbSrc<F>* srcs, u32 ns, u64* entries, u64 cap, const u64* counters,
                                                  typename F::Word* args_out, u64 args_cap) {
  __shared__ u64 off[LB_T];
  __shared__ u64 carry;
  const u64 n = counters[LB_C_UNBALANCED] < cap ? counters[LB_C_UNBALANCED] : cap;
  if (threadIdx.x == 0) carry = 0;
  for (u64 base = 0; base < n; base += LB_T) {
    const u64 k = base + threadIdx.x;
    u64* e = entries + k * MS_LB_ENTRY_WORDS;
    off[threadIdx.x] = k < n ? e[5] : 0;
    __syncthreads();
    if (threadIdx.x == 0) {
      u64 run = carry;
      for (u32 q = 0; q < LB_T; q++) {
        const u64 v = off[q];
        off[q] = run;
        run += v;
      }
      carry = run;
    }
    __syncthreads();
    if (k < n) {
      const u64 o = off[threadIdx.x], len = e[5];
      if (o + len <= args_cap) {
        const LbMsg<F> m = lb_msg(srcs, ns, e[7]);
        for (u64 q = 0; q < len; q++) args_out[o + q] = F::report(m.p[q]);
        e[6] = o;
      }
      e[7] = 0;
    }
    __syncthreads();
  }
}

// ---- host side, common to both calls; `call` names the entry point in the error texts
// an allocation failure of a call is an error that names the call and the bytes
template <class T>
DBuf<T> lb_alloc(Ctx& ctx, size_t count, const char* call, const std::string& what) {
  try {
    return DBuf<T>(ctx, count);
  } catch (const std::exception&) {
    (void)hipGetLastError();
    throw std::runtime_error(std::string(call) + ": cannot allocate the " + std::to_string(count * sizeof(T)) + " bytes of " + what);
  }
}

// MSAMD_LB_HASH_BITS=k (diagnostics, read per call): keep the low k bits of the hash (0: every probe sequence starts at slot 0)
u64 lb_hash_mask() {
  if (const char* e = getenv("MSAMD_LB_HASH_BITS")) {
    const long k = atol(e);
    if (k >= 0 && k < 64) return (u64(1) << k) - 1;
  }
  return ~u64(0);
}

// The state both calls set up the same way: the table (with `extra` arrays of the caller behind it), the counters, the mark
// bitmap and its scan, the source table on the device. Allocations in this order: table, [between], counters, marks, offsets,
// counts, sources - `between` is where the derive call takes its word per target row.
template <class F>
struct LbRun {
  size_t cap = 64, n_blocks;
  u32 ns;
  LbTab<F> t;
  u64* extra;
  DBuf<u64> table, rep, marks, wg_prefix;
  DBuf<u32> wg_counts;
  DBuf<LbSrc<F>> d_srcs;

  void alloc_table(Ctx& ctx, const char* call, size_t M, unsigned n_extra) {
    while (cap < 2 * M) cap <<= 1;
    n_blocks = (M + LB_BLOCK - 1) / LB_BLOCK;
    const size_t arrays = 3 + F::SUMS + n_extra;
    table = lb_alloc<u64>(ctx, arrays * cap, call, "its grouping table, " + std::to_string(8 * arrays) + " bytes x " + std::to_string(cap) + " slots");
    extra = t.place(table.p, cap);
    t.cap_mask = cap - 1, t.hash_mask = lb_hash_mask(), t.n_msgs = M;
  }
  void alloc_rest(Ctx& ctx, const char* call, size_t rep_words, size_t n_srcs) {
    rep = lb_alloc<u64>(ctx, rep_words, call, "its counters");
    marks = lb_alloc<u64>(ctx, n_blocks * LB_WORDS, call, "its mark bitmap");
    wg_prefix = lb_alloc<u64>(ctx, n_blocks, call, "its per-workgroup offsets");
    wg_counts = lb_alloc<u32>(ctx, n_blocks, call, "its per-workgroup counts");
    d_srcs = lb_alloc<LbSrc<F>>(ctx, n_srcs, call, "its source table");
    ns = (u32)n_srcs;
  }
  // the demand grouped and summed
  void insert(Ctx& ctx) {
    hipLaunchKernelGGL(lb_init_k<F>, dim3((unsigned)((std::max(cap, rep.n) + 255) / 256)), dim3(256), 0, ctx.stream, t, rep.p, rep.n);
    hipLaunchKernelGGL(lb_insert_k<F>, dim3((unsigned)n_blocks), dim3(LB_T), 0, ctx.stream, t, d_srcs.p, ns, rep.p);
  }
  // the first n_out marked messages, in origin order, and their tuples - the second host wait of a call. `what`: what a mark
  // is, for the error text
  void entries(Ctx& ctx, const char* call, const char* what, size_t n_out, size_t n_args, DBuf<u64>& d_entries, DBuf<typename F::Word>& d_args,
               u64* entries_out, typename F::Word* args_out) {
    constexpr size_t W = sizeof(typename F::Word);
    HIP_CHECK(hipMemsetAsync(d_args.p, 0, std::max<size_t>(n_args, 1) * W, ctx.stream));
    HIP_CHECK(hipMemsetAsync(d_entries.p, 0, n_out * MS_LB_ENTRY_WORDS * 8, ctx.stream));  // (lb_args_k reads every entry, written or not)
    hipLaunchKernelGGL(lb_scan_k, dim3(1), dim3(LB_T), 0, ctx.stream, wg_counts.p, wg_prefix.p, n_blocks);
    hipLaunchKernelGGL(lb_entries_k<F>, dim3((unsigned)n_blocks), dim3(64), 0, ctx.stream, t, d_srcs.p, ns, marks.p, wg_counts.p, wg_prefix.p,
                       d_entries.p, (u64)n_out, rep.p);
    hipLaunchKernelGGL(lb_args_k<F>, dim3(1), dim3(LB_T), 0, ctx.stream, d_srcs.p, ns, d_entries.p, (u64)n_out, rep.p, d_args.p, (u64)n_args);
    HIP_CHECK(hipGetLastError());
    u64 flag = 0;
    ctx.d2h_queue(&flag, rep.p + LB_C_FLAG, 8);
    if (n_args) ctx.d2h_queue(args_out, d_args.p, n_args * W);
    ctx.d2h(entries_out, d_entries.p, n_out * MS_LB_ENTRY_WORDS * 8);
    if (flag) throw std::runtime_error(std::string(call) + ": internal error (" + what + " was not found in the grouping table)");
  }
};

}  // namespace
}  // namespace msamd
