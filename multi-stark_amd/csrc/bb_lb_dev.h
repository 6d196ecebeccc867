// The grouping table of the exact lookup calls of the BabyBear configuration, shared by bb_balance.hip (msbb_witness_lookup_balance:
// report the groups that do not cancel) and bb_multiplicity.hip (msbb_witness_derive_multiplicities: write what makes them cancel).
// Include it from a .hip file only; everything lives in an unnamed namespace, so each translation unit compiles the kernels it
// launches for itself. The counterpart of lb_dev.h.
//
// INVARIANT: every word read here is a Montgomery word that is a reduced representative (< p): the upload converts canonical
// values with bb_to_monty, the sweep's constants come from bb_to_monty, and bb_add / bb_sub / bb_mul / bb_neg return values
// below p. Montgomery form is a bijection on [0, p) that fixes 0, so equality and zero tests on the words ARE equality and zero
// tests on the values: tuples are stripped, hashed and compared as they lie, and nothing is canonicalised first. bb_from_monty
// is applied only to what is summed (the multiplicities) and to what is reported (the tuples; the net is a sum of canonical values).
//
// Messages are numbered in ORIGIN order: claims by index, then the circuits in system order, row-major, slot last. The
// grouping table is open-addressed, in HBM, four 8-byte arrays of `cap` slots (cap = the power of two >= max(64, 2 x messages)):
//   owner    the message index that claimed the slot (all-ones: free) - its tuple IS the slot's key
//   sum      plain 64-bit sum of the canonical multiplicities: fewer than 2^32 messages (the host refuses more) of values
//            below 2^31 stay below 2^63, so one atomicAdd per insertion is exact and the net is sum mod p when it is read
//   members  number of messages of the group
//   first    smallest message index of the group (atomicMin)
// A slot is claimed by a 64-bit atomicCAS on `owner`, and inside a launch that claims the value that CAS returns is the only way
// a thread learns an owner: no plain load of the word there (another CU's L1 may hold the line from before the claim). Keys are
// never copied: equality is decided on the two messages' tuples, input data written by earlier launches. The hash picks the
// first slot only. What bounds the loops: a probe sequence visits at most `cap` slots and the table holds at most cap / 2
// groups. A loop that reaches its bound raises a flag the host turns into MS_ERR; nothing spins.
//   bl_insert_k  groups the messages of non-zero multiplicity. Equal tuples of a workgroup's 1024 consecutive messages are first
//                summed in a 512-entry table in LDS (same three sums), which is then flushed, one global insertion per entry; a
//                message that finds no room within 8 LDS probes is inserted directly
//   bl_lookup    read-only probe of a later launch (plain loads)
//   bl_scan_k, bl_entries_k, bl_args_k  order-preserving compaction of the first entries_cap marks of a bitmap over the messages
//                (one word per 64 consecutive messages, BL_WORDS words per workgroup of the marking kernel, whose per-workgroup
//                mark counts are scanned): entries written at fixed positions, then the tuples packed in entry order.
//                counters[BL_C_UNBALANCED] holds the number of marks, counters[BL_C_FLAG] the error flag
// Host side: bl_accept and bl_sources are the source setup both calls share - the refusals, the message count and the sweep of
// each active circuit's lookup values (bb_lookup_values_async, bb_kernels.hip) into temporaries of the call, row-major
// (multiplicities h x L, arguments h x args_width), so that the 64 consecutive messages of a wave - 64 / L rows x L slots - read
// one contiguous run of each. The claims are read where the witness keeps them.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/mstark_bb.h"
#include "bb_host.h"

namespace msbb {
namespace {

constexpr u64 BL_EMPTY = ~u64(0);
constexpr unsigned BL_T = 256, BL_PER = 4, BL_BLOCK = BL_T * BL_PER;  // a workgroup owns BL_BLOCK consecutive messages
constexpr unsigned BL_WORDS = BL_BLOCK / 64;                           // ... = that many words of the mark bitmap
constexpr unsigned BL_LDS = 512, BL_LDS_PROBES = 8;


struct BlSrc {  // one source of messages: the claims (mult == nullptr, offs = u64 offsets) or one circuit's lookup values
  u64 base, count;
  const u32 *mult, *args;
  const void* offs;
  u32 L, aw, circuit, slot0;
};
struct BlTab {
  u64 *owner, *sum, *members, *first;
  u64 cap_mask, hash_mask, n_msgs;
};
struct BlMsg {
  const u32* p;  // Montgomery words
  u32 mult;      // canonical
  u32 len, src;
};
enum { BL_C_MSGS = 0, BL_C_GROUPS, BL_C_UNBALANCED, BL_C_FLAG, BL_C_WORDS };

__device__ BlMsg bl_msg(const BlSrc* srcs, u32 ns, u64 i) {
  u32 lo = 0, hi = ns;
  while (hi - lo > 1) {
    const u32 mid = (lo + hi) >> 1;
    if (srcs[mid].base <= i) lo = mid; else hi = mid;
  }
  const BlSrc& s = srcs[lo];
  const u64 k = i - s.base;
  BlMsg m;
  m.src = lo;
  if (!s.mult) {
    const u64* off = (const u64*)s.offs;
    const u64 a = off[k];
    m.p = s.args + a;
    m.len = (u32)(off[k + 1] - a);
    m.mult = 1;
  } else {
    const u32 r = (u32)k / s.L;  // (k < messages < 2^32)
    const u32 j = (u32)k - r * s.L;
    const u32* off = (const u32*)s.offs;
    m.p = s.args + (size_t)r * s.aw + off[j];
    m.len = off[j + 1] - off[j];
    m.mult = bb_from_monty(s.mult[k]);
  }
  while (m.len && m.p[m.len - 1] == 0) m.len--;
  return m;
}

__device__ u64 bl_hash(const BlMsg& m, u64 hash_mask) {
  u64 h = (u64(m.len) + 1) * 0x9E3779B97F4A7C15ULL;
  for (u32 k = 0; k < m.len; k++) {
    h = (h ^ m.p[k]) * 0xFF51AFD7ED558CCDULL;
    h ^= h >> 29;
  }
  h *= 0xC4CEB9FE1A85EC53ULL;
  h ^= h >> 32;
  return h & hash_mask;
}

__device__ bool bl_eq(const BlMsg& a, const BlMsg& b) {
  if (a.len != b.len) return false;
  for (u32 k = 0; k < a.len; k++)
    if (a.p[k] != b.p[k]) return false;
  return true;
}

// the slot of message i's group, claimed for i when no equal tuple owns one yet; false: the table is full (cannot happen at
// cap >= 2 x messages; the caller raises the flag)
__device__ bool bl_claim(const BlTab& t, const BlSrc* srcs, u32 ns, u64 i, const BlMsg& m, u64 h, u64& slot) {
  u64 s = h & t.cap_mask;
  for (u64 step = 0; step <= t.cap_mask; step++, s = (s + 1) & t.cap_mask) {
    const u64 prev = atomicCAS((unsigned long long*)&t.owner[s], (unsigned long long)BL_EMPTY, (unsigned long long)i);
    if (prev == BL_EMPTY || prev == i || bl_eq(bl_msg(srcs, ns, prev), m)) {
      slot = s;
      return true;
    }
  }
  return false;
}

__device__ void bl_add(const BlTab& t, u64 s, u64 sum, u64 members, u64 first) {
  atomicAdd((unsigned long long*)&t.sum[s], (unsigned long long)sum);
  atomicAdd((unsigned long long*)&t.members[s], (unsigned long long)members);
  atomicMin((unsigned long long*)&t.first[s], (unsigned long long)first);
}

__global__ void bl_init_k(BlTab t, u64* zeros, size_t n_zeros) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= t.cap_mask) {
    t.owner[i] = BL_EMPTY;
    t.first[i] = BL_EMPTY;
    t.sum[i] = 0;
    t.members[i] = 0;
  }
  if (i < n_zeros) zeros[i] = 0;
}

__global__ __launch_bounds__(BL_T) void bl_insert_k(BlTab t, const BlSrc* srcs, u32 ns, u64* counters) {
  __shared__ u64 l_key[BL_LDS], l_sum[BL_LDS], l_min[BL_LDS];
  __shared__ u32 l_cnt[BL_LDS];
  for (u32 e = threadIdx.x; e < BL_LDS; e += BL_T) l_key[e] = BL_EMPTY, l_sum[e] = 0, l_min[e] = BL_EMPTY, l_cnt[e] = 0;
  __syncthreads();
  bool failed = false;
  for (u32 it = 0; it < BL_PER; it++) {
    const u64 i = (u64)blockIdx.x * BL_BLOCK + it * BL_T + threadIdx.x;
    if (i >= t.n_msgs) break;
    const BlMsg m = bl_msg(srcs, ns, i);
    if (m.mult == 0) continue;
    const u64 h = bl_hash(m, t.hash_mask);
    bool done = false;
    u32 ls = (u32)h & (BL_LDS - 1);
    for (u32 probe = 0; probe < BL_LDS_PROBES && !done; probe++, ls = (ls + 1) & (BL_LDS - 1)) {
      const u64 prev = atomicCAS((unsigned long long*)&l_key[ls], (unsigned long long)BL_EMPTY, (unsigned long long)i);
      if (prev == BL_EMPTY || prev == i || bl_eq(bl_msg(srcs, ns, prev), m)) {
        atomicAdd((unsigned long long*)&l_sum[ls], (unsigned long long)m.mult);
        atomicMin((unsigned long long*)&l_min[ls], (unsigned long long)i);
        atomicAdd(&l_cnt[ls], 1u);
        done = true;
      }
    }
    if (!done) {
      u64 s;
      if (bl_claim(t, srcs, ns, i, m, h, s)) bl_add(t, s, m.mult, 1, i);
      else failed = true;
    }
  }
  __syncthreads();
  for (u32 e = threadIdx.x; e < BL_LDS; e += BL_T) {
    const u64 rep = l_key[e];
    if (rep == BL_EMPTY) continue;
    const BlMsg m = bl_msg(srcs, ns, rep);
    u64 s;
    if (bl_claim(t, srcs, ns, rep, m, bl_hash(m, t.hash_mask), s)) bl_add(t, s, l_sum[e], l_cnt[e], l_min[e]);
    else failed = true;
  }
  if (failed) atomicOr((unsigned long long*)&counters[BL_C_FLAG], 1ull);
}

// read-only: the slot that holds message i's group (written by bl_insert_k, an earlier launch: plain loads)
__device__ bool bl_lookup(const BlTab& t, const BlSrc* srcs, u32 ns, u64 i, const BlMsg& m, u64& slot) {
  u64 s = bl_hash(m, t.hash_mask) & t.cap_mask;
  for (u64 step = 0; step <= t.cap_mask; step++, s = (s + 1) & t.cap_mask) {
    const u64 o = t.owner[s];
    if (o == BL_EMPTY) return false;
    if (o == i || bl_eq(bl_msg(srcs, ns, o), m)) {
      slot = s;
      return true;
    }
  }
  return false;
}

__device__ __forceinline__ u64 bl_net(const BlTab& t, u64 s) { return t.sum[s] % BB_P; }

// exclusive scan of the per-workgroup mark counts, one workgroup: a contiguous chunk per thread, the 256 chunk sums by thread 0
__global__ __launch_bounds__(BL_T) void bl_scan_k(const u32* wg_counts, u64* wg_prefix, size_t n_blocks) {
  __shared__ u64 part[BL_T];
  const size_t chunk = (n_blocks + BL_T - 1) / BL_T, a = threadIdx.x * chunk, b = a + chunk < n_blocks ? a + chunk : n_blocks;
  u64 sum = 0;
  for (size_t k = a; k < b; k++) sum += wg_counts[k];
  part[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 run = 0;
    for (u32 k = 0; k < BL_T; k++) {
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

// one wave per workgroup of bl_report_k: lane w < BL_WORDS takes bitmap word w; entry e goes to position prefix + rank
__global__ __launch_bounds__(64) void bl_entries_k(BlTab t, const BlSrc* srcs, u32 ns, const u64* marks, const u32* wg_counts, const u64* wg_prefix,
                                                   u64* entries, u64 cap, u64* counters) {
  if (wg_counts[blockIdx.x] == 0 || wg_prefix[blockIdx.x] >= cap || threadIdx.x >= BL_WORDS) return;
  const u64* words = marks + (size_t)blockIdx.x * BL_WORDS;
  u64 pos = wg_prefix[blockIdx.x];
  for (u32 w = 0; w < threadIdx.x; w++) pos += __popcll(words[w]);
  u64 bits = words[threadIdx.x];
  for (u32 k = 0; k < 64 && bits && pos < cap; k++, pos++) {
    const u32 bit = __ffsll((unsigned long long)bits) - 1;
    bits &= bits - 1;
    const u64 i = ((u64)blockIdx.x * BL_WORDS + threadIdx.x) * 64 + bit;
    const BlMsg m = bl_msg(srcs, ns, i);
    const BlSrc& src = srcs[m.src];
    u64 s = 0;
    if (!bl_lookup(t, srcs, ns, i, m, s)) {
      atomicOr((unsigned long long*)&counters[BL_C_FLAG], 2ull);
      return;
    }
    u64* e = entries + pos * MS_LB_ENTRY_WORDS;
    const u32 k_in = (u32)(i - src.base);
    e[0] = src.mult ? src.circuit : MS_LB_CLAIMS;
    e[1] = src.mult ? k_in / src.L : k_in;
    e[2] = src.mult ? k_in % src.L : 0;
    e[3] = bl_net(t, s);
    e[4] = t.members[s];
    e[5] = m.len;
    e[6] = ~u64(0);
    e[7] = i;  // for bl_args_k, which puts the reserved zero here
  }
}

// offsets of the tuples in entry order and the tuples themselves (canonical), one workgroup: 256 entries per round, their
// lengths scanned by thread 0
__global__ __launch_bounds__(BL_T) void bl_args_k(const BlSrc* srcs, u32 ns, u64* entries, u64 cap, const u64* counters, u32* args_out, u64 args_cap) {
  __shared__ u64 off[BL_T];
  __shared__ u64 carry;
  const u64 n = counters[BL_C_UNBALANCED] < cap ? counters[BL_C_UNBALANCED] : cap;
  if (threadIdx.x == 0) carry = 0;
  for (u64 base = 0; base < n; base += BL_T) {
    const u64 k = base + threadIdx.x;
    u64* e = entries + k * MS_LB_ENTRY_WORDS;
    off[threadIdx.x] = k < n ? e[5] : 0;
    __syncthreads();
    if (threadIdx.x == 0) {
      u64 run = carry;
      for (u32 q = 0; q < BL_T; q++) {
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
        const BlMsg m = bl_msg(srcs, ns, e[7]);
        for (u64 q = 0; q < len; q++) args_out[o + q] = bb_from_monty(m.p[q]);
        e[6] = o;
      }
      e[7] = 0;
    }
    __syncthreads();
  }
}

// an allocation failure of a call is an error that names the call and the bytes
template <class T>
DBuf<T> bl_alloc(Ctx& ctx, size_t count, const char* call, const std::string& what) {
  try {
    return DBuf<T>(ctx, count);
  } catch (const std::exception&) {
    (void)hipGetLastError();
    throw std::runtime_error(std::string(call) + ": cannot allocate the " + std::to_string(count * sizeof(T)) + " bytes of " + what);
  }
}

// MSAMD_LB_HASH_BITS=k (diagnostics, read per call): keep the low k bits of the hash (0: every probe sequence starts at slot 0)
inline u64 bl_hash_mask() {
  if (const char* e = getenv("MSAMD_LB_HASH_BITS")) {
    const long k = atol(e);
    if (k >= 0 && k < 64) return (u64(1) << k) - 1;
  }
  return ~u64(0);
}

// the witnesses both calls take: of this system, and device-resident
inline void bl_accept(const BSystem& sys, const BWitness& wit, const char* call) {
  const size_t C = sys.circuits.size();
  if (wit.sys != &sys || wit.heights.size() != C || wit.traces.size() != C) throw std::runtime_error("witness does not belong to this system");
  if (wit.host_resident)
    throw std::runtime_error(std::string(call) + " takes a device-resident witness (msbb_witness_create, msbb_witness_create_device)");
}

// The sources of the witness's messages in origin order -> the message count M (0: no claims and no active circuit with
// lookups; nothing was launched). The count comes first: nothing is allocated or launched for a call that is refused. Then each
// active circuit's lookup values are swept into temporaries of the call, which `keep` owns (two per source of a circuit:
// multiplicities, arguments). max_len: the longest tuple of a circuit's lookups.
inline size_t bl_sources(BSystem& sys, BWitness& wit, const char* call, std::vector<BlSrc>& srcs, std::vector<DBuf<u32>>& keep, size_t& max_len) {
  Ctx& ctx = *sys.ctx;
  const std::string name(call);
  const size_t C = sys.circuits.size(), n_claims = wit.claims.size();
  size_t M = n_claims;
  for (size_t ci = 0; ci < C; ci++) {
    const BCircuit& c = sys.circuits[ci];
    const size_t h = wit.heights[ci];
    if (!h || !c.num_lookups) continue;
    const BMat& t = wit.traces[ci];
    if (!t.buf.p || t.h != h || t.w != c.main_width) throw std::runtime_error(name + ": an active circuit has no trace on this device");
    if (c.pre_width && (h != c.pre_height || !c.pre.buf.p)) throw std::runtime_error("main trace height must equal preprocessed trace height");
    if (h > (~size_t(0) >> 1) / c.num_lookups) throw std::runtime_error(name + ": 2^32 messages or more");
    M += h * c.num_lookups;
    for (auto& l : c.lookups) max_len = std::max(max_len, l.second.size());
  }
  if (M == 0) return 0;
  if (M >> 32) throw std::runtime_error(name + ": 2^32 messages or more (the 64-bit sums would no longer be exact)");

  size_t base = 0, slot0 = 0;
  if (n_claims) {
    BlSrc s{};
    s.base = 0, s.count = n_claims, s.mult = nullptr, s.args = wit.d_claim_data.p, s.offs = wit.d_claim_offs.p, s.L = 1;
    srcs.push_back(s);
    base += n_claims;
  }
  for (size_t ci = 0; ci < C; ci++) {
    const BCircuit& c = sys.circuits[ci];
    const size_t h = wit.heights[ci], L = c.num_lookups;
    if (h && L) {
      keep.push_back(bl_alloc<u32>(ctx, h * L, call, "a circuit's multiplicities"));
      keep.push_back(bl_alloc<u32>(ctx, std::max<size_t>(h * c.args_width, 1), call, "a circuit's lookup arguments"));
      u32 *tm = keep[keep.size() - 2].p, *ta = keep.back().p;
      {
        DBuf<u32> scratch = bl_alloc<u32>(ctx, std::max<size_t>(c.lookup_prefix_len, 1) * h, call, "a circuit's sweep scratch");
        bb_lookup_values_async(ctx, c.prog, c.lookup_prefix_len, c.lk, c.args_width, wit.traces[ci], c.pre_width ? &c.pre : nullptr, scratch.p, tm, ta);
      }  // (released behind the launch: the pool hands a block on in stream order)
      BlSrc s{};
      s.base = base, s.count = h * L, s.mult = tm, s.args = ta, s.offs = c.lk.arg_off.p;
      s.L = (u32)L, s.aw = (u32)c.args_width, s.circuit = (u32)ci, s.slot0 = (u32)slot0;
      srcs.push_back(s);
      base += h * L;
    }
    slot0 += L;
  }
  HIP_CHECK(hipGetLastError());
  return M;
}

}  // namespace
}  // namespace msbb
