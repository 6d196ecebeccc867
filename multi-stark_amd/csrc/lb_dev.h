// The grouping table of the exact lookup calls, shared by balance.hip (ms_witness_lookup_balance: report the groups that do not
// cancel) and multiplicity.hip (ms_witness_derive_multiplicities: write what makes them cancel). Include it from a .hip file only;
// everything lives in an unnamed namespace, so each translation unit compiles the kernels it launches for itself.
//
// Messages are numbered in ORIGIN order: claims by index, then the circuits in system order, row-major, slot last. The
// grouping table is open-addressed, in HBM, five 8-byte arrays of `cap` slots (cap = the power of two >= 2 x messages):
//   owner    the message index that claimed the slot (all-ones: free) - its tuple IS the slot's key
//   small    wrapping signed sum of the multiplicities in (0, 2^20) and of -(p - m) for those in (p - 2^20, p)
//   big      sum modulo p of every other multiplicity (a compare-and-swap loop; rare)
//   members  number of messages of the group
//   first    smallest message index of the group (atomicMin)
// A slot is claimed by a 64-bit atomicCAS on `owner`, and inside a launch that claims the value that CAS returns is the only
// way a thread learns an owner: no plain load of the word there (another CU's L1 may hold the line from before the claim). Keys
// are never copied: equality is decided on the two messages' tuples, input data written by earlier launches. The hash picks the
// first slot only. What bounds the loops: a probe sequence visits at most `cap` slots and the table holds at most cap / 2
// groups; the compare-and-swap loop of `big` gives up after as many rounds as there are messages (each lost round is another
// message's completed add). A loop that reaches its bound raises a flag the host turns into MS_ERR.
//   lb_insert_k  groups the messages of non-zero multiplicity. Equal tuples of a workgroup's 1024 consecutive messages are
//                first summed in a 512-entry table in LDS (the bench witness puts 12 x 2^20 byte messages on 256 tuples: one
//                global atomic per message would queue them on a few L2 addresses), which is then flushed, one global insertion
//                per entry; a message that finds no room within 8 LDS probes, or whose multiplicity is not small, is inserted
//                directly
//   lb_lookup    read-only probe of a later launch (plain loads)
//   lb_scan_k, lb_entries_k, lb_args_k  order-preserving compaction of the first entries_cap marks of a bitmap over the
//                messages (one word per 64 consecutive messages, LB_WORDS words per workgroup of the marking kernel, whose
//                per-workgroup mark counts are scanned): entries written at fixed positions, then the tuples packed in entry
//                order. counters[LB_C_UNBALANCED] holds the number of marks, counters[LB_C_FLAG] the error flag
#pragma once
#include <cstdlib>
#include <string>

#include "host.h"

namespace msamd {
namespace {

constexpr u64 LB_EMPTY = ~u64(0);
constexpr u64 LB_SMALL = u64(1) << 20;   // multiplicities below it (or above p - it) go to the wrapping counter
constexpr unsigned LB_T = 256, LB_PER = 4, LB_BLOCK = LB_T * LB_PER;  // a workgroup owns LB_BLOCK consecutive messages
constexpr unsigned LB_WORDS = LB_BLOCK / 64;                           // ... = that many words of the mark bitmap
constexpr unsigned LB_LDS = 512, LB_LDS_PROBES = 8;

struct LbSrc {  // one source of messages: the claims (mult == nullptr, offs = u64 offsets) or one circuit's LookupValues
  u64 base, count;
  const u64 *mult, *args;
  const void* offs;
  u32 L, aw, circuit, slot0;
};
struct LbTab {
  u64 *owner, *small, *big, *members, *first;
  u64 cap_mask, hash_mask, n_msgs;
};
struct LbMsg {
  const u64* p;
  u64 mult;
  u32 len, src;
};
enum { LB_C_MSGS = 0, LB_C_GROUPS, LB_C_UNBALANCED, LB_C_FLAG, LB_C_WORDS };

__device__ __forceinline__ u64 lb_canon(u64 v) { return v >= GL_P ? v - GL_P : v; }

__device__ LbMsg lb_msg(const LbSrc* srcs, u32 ns, u64 i) {
  u32 lo = 0, hi = ns;
  while (hi - lo > 1) {
    const u32 mid = (lo + hi) >> 1;
    if (srcs[mid].base <= i) lo = mid; else hi = mid;
  }
  const LbSrc& s = srcs[lo];
  const u64 k = i - s.base;
  LbMsg m;
  m.src = lo;
  if (!s.mult) {
    const u64* off = (const u64*)s.offs;
    const u64 a = off[k];
    m.p = s.args + a;
    m.len = (u32)(off[k + 1] - a);
    m.mult = 1;
  } else {
    const u64 r = k / s.L;
    const u32 j = (u32)(k - r * s.L);
    const u32* off = (const u32*)s.offs;
    m.p = s.args + r * s.aw + off[j];
    m.len = off[j + 1] - off[j];
    m.mult = lb_canon(s.mult[k]);
  }
  while (m.len && lb_canon(m.p[m.len - 1]) == 0) m.len--;
  return m;
}

__device__ u64 lb_hash(const LbMsg& m, u64 hash_mask) {
  u64 h = (u64(m.len) + 1) * 0x9E3779B97F4A7C15ULL;
  for (u32 k = 0; k < m.len; k++) {
    h = (h ^ lb_canon(m.p[k])) * 0xFF51AFD7ED558CCDULL;
    h ^= h >> 29;
  }
  h *= 0xC4CEB9FE1A85EC53ULL;
  h ^= h >> 32;
  return h & hash_mask;
}

__device__ bool lb_eq(const LbMsg& a, const LbMsg& b) {
  if (a.len != b.len) return false;
  for (u32 k = 0; k < a.len; k++)
    if (lb_canon(a.p[k]) != lb_canon(b.p[k])) return false;
  return true;
}

// the slot of message i's group, claimed for i when no equal tuple owns one yet; false: the table is full (cannot happen at
// cap >= 2 x messages; the caller raises the flag)
__device__ bool lb_claim(const LbTab& t, const LbSrc* srcs, u32 ns, u64 i, const LbMsg& m, u64 h, u64& slot) {
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

__device__ bool lb_add(const LbTab& t, u64 s, u64 small_sum, u64 big, u64 members, u64 first) {
  atomicAdd((unsigned long long*)&t.members[s], (unsigned long long)members);
  atomicMin((unsigned long long*)&t.first[s], (unsigned long long)first);
  if (small_sum) atomicAdd((unsigned long long*)&t.small[s], (unsigned long long)small_sum);
  if (!big) return true;
  u64 old = 0;
  for (u64 round = 0; round <= t.n_msgs; round++) {
    u64 sum = old + big;
    if (sum < old || sum >= GL_P) sum -= GL_P;
    const u64 got = atomicCAS((unsigned long long*)&t.big[s], (unsigned long long)old, (unsigned long long)sum);
    if (got == old) return true;
    old = got;
  }
  return false;
}

__global__ void lb_init_k(LbTab t, u64* zeros, size_t n_zeros) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= t.cap_mask) {
    t.owner[i] = LB_EMPTY;
    t.first[i] = LB_EMPTY;
    t.small[i] = 0;
    t.big[i] = 0;
    t.members[i] = 0;
  }
  if (i < n_zeros) zeros[i] = 0;
}

__global__ __launch_bounds__(LB_T) void lb_insert_k(LbTab t, const LbSrc* srcs, u32 ns, u64* counters) {
  __shared__ u64 l_key[LB_LDS], l_sum[LB_LDS], l_min[LB_LDS];
  __shared__ u32 l_cnt[LB_LDS];
  for (u32 e = threadIdx.x; e < LB_LDS; e += LB_T) l_key[e] = LB_EMPTY, l_sum[e] = 0, l_min[e] = LB_EMPTY, l_cnt[e] = 0;
  __syncthreads();
  bool failed = false;
  for (u32 it = 0; it < LB_PER; it++) {
    const u64 i = (u64)blockIdx.x * LB_BLOCK + it * LB_T + threadIdx.x;
    if (i >= t.n_msgs) break;
    const LbMsg m = lb_msg(srcs, ns, i);
    if (m.mult == 0) continue;
    const u64 h = lb_hash(m, t.hash_mask);
    const bool pos = m.mult < LB_SMALL, neg = m.mult > GL_P - LB_SMALL;
    const u64 sv = pos ? m.mult : neg ? u64(0) - (GL_P - m.mult) : 0;
    bool done = false;
    if (pos || neg) {
      u32 ls = (u32)h & (LB_LDS - 1);
      for (u32 probe = 0; probe < LB_LDS_PROBES && !done; probe++, ls = (ls + 1) & (LB_LDS - 1)) {
        const u64 prev = atomicCAS((unsigned long long*)&l_key[ls], (unsigned long long)LB_EMPTY, (unsigned long long)i);
        if (prev == LB_EMPTY || prev == i || lb_eq(lb_msg(srcs, ns, prev), m)) {
          atomicAdd((unsigned long long*)&l_sum[ls], (unsigned long long)sv);
          atomicMin((unsigned long long*)&l_min[ls], (unsigned long long)i);
          atomicAdd(&l_cnt[ls], 1u);
          done = true;
        }
      }
    }
    if (!done) {
      u64 s;
      if (!lb_claim(t, srcs, ns, i, m, h, s) || !lb_add(t, s, sv, (pos || neg) ? 0 : m.mult, 1, i)) failed = true;
    }
  }
  __syncthreads();
  for (u32 e = threadIdx.x; e < LB_LDS; e += LB_T) {
    const u64 rep = l_key[e];
    if (rep == LB_EMPTY) continue;
    const LbMsg m = lb_msg(srcs, ns, rep);
    u64 s;
    if (!lb_claim(t, srcs, ns, rep, m, lb_hash(m, t.hash_mask), s) || !lb_add(t, s, l_sum[e], 0, l_cnt[e], l_min[e])) failed = true;
  }
  if (failed) atomicOr((unsigned long long*)&counters[LB_C_FLAG], 1ull);
}

// read-only: the slot that holds message i's group (written by an earlier launch: plain loads)
__device__ bool lb_lookup(const LbTab& t, const LbSrc* srcs, u32 ns, u64 i, const LbMsg& m, u64& slot) {
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

__device__ u64 lb_net(const LbTab& t, u64 s) {
  const long long sm = (long long)t.small[s];  // |sm| < 2^20 x messages < 2^62 (the host checks the message count)
  const u64 a = sm >= 0 ? (u64)sm : GL_P - (u64)(-sm);
  u64 sum = a + t.big[s];
  if (sum < a || sum >= GL_P) sum -= GL_P;
  return sum;
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
__global__ __launch_bounds__(64) void lb_entries_k(LbTab t, const LbSrc* srcs, u32 ns, const u64* marks, const u32* wg_counts, const u64* wg_prefix,
                                                   u64* entries, u64 cap, u64* counters) {
  if (wg_counts[blockIdx.x] == 0 || wg_prefix[blockIdx.x] >= cap || threadIdx.x >= LB_WORDS) return;
  const u64* words = marks + (size_t)blockIdx.x * LB_WORDS;
  u64 pos = wg_prefix[blockIdx.x];
  for (u32 w = 0; w < threadIdx.x; w++) pos += __popcll(words[w]);
  u64 bits = words[threadIdx.x];
  for (u32 k = 0; k < 64 && bits && pos < cap; k++, pos++) {
    const u32 bit = __ffsll((unsigned long long)bits) - 1;
    bits &= bits - 1;
    const u64 i = ((u64)blockIdx.x * LB_WORDS + threadIdx.x) * 64 + bit;
    const LbMsg m = lb_msg(srcs, ns, i);
    const LbSrc& src = srcs[m.src];
    u64 s = 0;
    if (!lb_lookup(t, srcs, ns, i, m, s)) {
      atomicOr((unsigned long long*)&counters[LB_C_FLAG], 2ull);
      return;
    }
    u64* e = entries + pos * MS_LB_ENTRY_WORDS;
    const u64 k_in = i - src.base;
    e[0] = src.mult ? src.circuit : MS_LB_CLAIMS;
    e[1] = src.mult ? k_in / src.L : k_in;
    e[2] = src.mult ? k_in % src.L : 0;
    e[3] = lb_net(t, s);
    e[4] = t.members[s];
    e[5] = m.len;
    e[6] = ~u64(0);
    e[7] = i;  // for lb_args_k, which puts the reserved zero here
  }
}

// offsets of the tuples in entry order and the tuples themselves, one workgroup: 256 entries per round, their lengths scanned by thread 0
__global__ __launch_bounds__(LB_T) void lb_args_k(const LbSrc* srcs, u32 ns, u64* entries, u64 cap, const u64* counters, u64* args_out, u64 args_cap) {
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
        const LbMsg m = lb_msg(srcs, ns, e[7]);
        for (u64 q = 0; q < len; q++) args_out[o + q] = lb_canon(m.p[q]);
        e[6] = o;
      }
      e[7] = 0;
    }
    __syncthreads();
  }
}

// ---- host side, common to both calls; `call` names the entry point in the error texts
// an allocation failure of the call is an error that names the bytes
DBuf<u64> lb_alloc(Ctx& ctx, size_t words, const char* call, const char* what) {
  try {
    return DBuf<u64>(ctx, words);
  } catch (const std::exception&) {
    (void)hipGetLastError();
    throw std::runtime_error(std::string(call) + ": cannot allocate the " + std::to_string(words * 8) + " bytes of " + what);
  }
}

// what every exact lookup call refuses before it launches anything
void lb_accept(const HSystem& sys, const HWitness& wit, const char* call) {
  if (wit.sys != &sys || wit.heights.size() != sys.circuits.size()) throw std::runtime_error("witness does not belong to this system");
  if (wit.host_resident)
    throw std::runtime_error(std::string(call) + " takes a device-resident witness (ms_witness_create, ms_witness_create_device, the generators)");
  if (wit.has_remote || wit.claims_partial) throw std::runtime_error(std::string(call) + ": this witness lacks traces that another rank computes");
}

// the sources in origin order; lookup values a witness does not hold (its stage 2 reads the trace) are computed into
// temporaries that `keep` owns. -> the number of messages M; max_len: the longest tuple a circuit's slot can have
size_t lb_sources(HSystem& sys, HWitness& wit, const char* call, std::vector<LbSrc>& srcs, std::vector<DBuf<u64>>& keep, size_t& max_len) {
  Ctx& ctx = *sys.ctx;
  const std::string name(call);
  const size_t C = sys.circuits.size(), n_claims = wit.claim_offsets.size() - 1;
  size_t M = 0, slot0 = 0;
  if (n_claims) {
    if (wit.claim_data.size() >> 32) throw std::runtime_error(name + ": more than 2^32 claim elements");
    LbSrc s{};
    s.base = 0, s.count = n_claims, s.mult = nullptr, s.args = wit.d_claim_data.p, s.offs = wit.d_claim_offsets.p, s.L = 1;
    srcs.push_back(s);
    M += n_claims;
  }
  for (size_t ci = 0; ci < C; ci++) {
    const HCircuit& c = sys.circuits[ci];
    const size_t h = wit.heights[ci], L = c.num_lookups;
    if (h && L) {
      const DLookups& lk = wit.lookups[ci];
      const u64 *mult = lk.mult.p, *args = lk.args.p;
      if (!mult) {
        if (!wit.traces[ci].p) throw std::runtime_error(name + ": an active circuit has no trace on this device");
        keep.push_back(lb_alloc(ctx, h * L, call, "a circuit's multiplicities"));
        keep.push_back(lb_alloc(ctx, std::max<size_t>(h * c.args_width, 1), call, "a circuit's lookup arguments"));
        u64 *tm = keep[keep.size() - 2].p, *ta = keep.back().p;
        if (!c.prefix_on_device || !lookup_values_device(ctx, c.prefix_prog, wit.traces[ci].p, c.pre_width ? c.d_preprocessed.p : nullptr, h,
                                                         c.main_width, c.pre_width, c.args_width, tm, ta))
          throw std::runtime_error("device-resident witness: this circuit's lookup prefix does not fit the device sweep");
        mult = tm, args = ta;
      }
      LbSrc s{};
      s.base = M, s.count = h * L, s.mult = mult, s.args = args, s.offs = lk.arg_offsets.p;
      s.L = (u32)L, s.aw = (u32)c.args_width, s.circuit = (u32)ci, s.slot0 = (u32)slot0;
      srcs.push_back(s);
      M += h * L;
      for (auto& l : c.lookups) max_len = std::max(max_len, l.second.size());
    }
    slot0 += L;
  }
  return M;
}

// MSAMD_LB_HASH_BITS=k (diagnostics, read per call): keep the low k bits of the hash (0: every probe sequence starts at slot 0)
u64 lb_hash_mask() {
  u64 hash_mask = ~u64(0);
  if (const char* e = getenv("MSAMD_LB_HASH_BITS")) {
    const long k = atol(e);
    if (k >= 0 && k < 64) hash_mask = (u64(1) << k) - 1;
  }
  return hash_mask;
}

}  // namespace
}  // namespace msamd
