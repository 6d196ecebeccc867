// What the grouping table of lb_dev.h and the two exact lookup calls built on it (balance.hip, multiplicity.hip) need to know of
// Goldilocks. Words are 64-bit and not necessarily canonical (p <= w < 2^64 stands for w - p), so a word is canonicalised
// wherever it is a key, a multiplicity or a reported value. A call takes up to 2^40 messages: indices within a source are 64-bit.
//
// The sum of a group: two arrays. `small` is a wrapping signed counter that takes the multiplicities in (0, 2^20) and -(p - m)
// for those in (p - 2^20, p) - one atomicAdd each, and only these go through the LDS table of lb_insert_k; |small| <
// 2^20 x messages < 2^62. `big` is the sum modulo p of every other multiplicity, by a compare-and-swap loop (rare) that gives up
// after as many rounds as there are messages: each lost round is another message's completed add.
//
// Host side: a witness may hold its lookup values (mult, args per circuit); where it holds none (its stage 2 reads the trace)
// they are computed into two temporaries per circuit by lookup_values_device.
#pragma once
#include "host.h"
#include "lb_dev.h"

namespace msamd {
namespace {

__device__ __forceinline__ u64 lb_canon(u64 v) { return v >= GL_P ? v - GL_P : v; }

struct GlLookup {
  using Word = u64;
  using Idx = u64;
  using Tab = LbTab<GlLookup>;
  using Src = LbSrc<GlLookup>;
  static constexpr unsigned SUMS = 2;  // small, big
  static constexpr u64 SMALL = u64(1) << 20;
  static constexpr const char *call_balance = "ms_witness_lookup_balance", *call_derive = "ms_witness_derive_multiplicities";

  static __device__ __forceinline__ u64 key(u64 w) { return lb_canon(w); }
  static __device__ __forceinline__ u64 mult(u64 w) { return lb_canon(w); }
  static __device__ __forceinline__ u64 report(u64 w) { return lb_canon(w); }

  static __device__ __forceinline__ bool lds_value(u64 m, u64& v) {
    const bool pos = m < SMALL, neg = m > GL_P - SMALL;
    v = pos ? m : neg ? u64(0) - (GL_P - m) : 0;
    return pos || neg;
  }
  static __device__ __forceinline__ void flush(const Tab& t, u64 s, u64 v) {
    if (v) atomicAdd((unsigned long long*)&t.sum[0][s], (unsigned long long)v);
  }
  static __device__ bool add(const Tab& t, u64 s, u64 m) {
    u64 v;
    if (lds_value(m, v)) {
      flush(t, s, v);
      return true;
    }
    u64 old = 0;
    for (u64 round = 0; round <= t.n_msgs; round++) {
      u64 sum = old + m;
      if (sum < old || sum >= GL_P) sum -= GL_P;
      const u64 got = atomicCAS((unsigned long long*)&t.sum[1][s], (unsigned long long)old, (unsigned long long)sum);
      if (got == old) return true;
      old = got;
    }
    return false;
  }
  static __device__ u64 net(const Tab& t, u64 s) {
    const long long sm = (long long)t.sum[0][s];  // |sm| < 2^20 x messages < 2^62 (the host checks the message count)
    const u64 a = sm >= 0 ? (u64)sm : GL_P - (u64)(-sm);
    u64 sum = a + t.sum[1][s];
    if (sum < a || sum >= GL_P) sum -= GL_P;
    return sum;
  }

  // a derived cell: the row-major trace cell, and the multiplicity the witness holds (nullptr: it holds none)
  struct Cell {
    u64 *trace, *held;
    u32 W, m;
  };
  template <class Tgt>
  static __device__ __forceinline__ void store(const Tgt& g, u64 r, u64 d) {
    const u64 minus_d = d ? GL_P - d : 0;
    g.cell.trace[r * g.cell.W + g.cell.m] = g.pull ? d : minus_d;
    if (g.cell.held) g.cell.held[r * g.L + g.j] = minus_d;
  }

  // what every exact lookup call refuses before it launches anything
  static void accept(const HSystem& sys, const HWitness& wit, const char* call) {
    if (wit.sys != &sys || wit.heights.size() != sys.circuits.size()) throw std::runtime_error("witness does not belong to this system");
    if (wit.host_resident)
      throw std::runtime_error(std::string(call) + " takes a device-resident witness (ms_witness_create, ms_witness_create_device, the generators)");
    if (wit.has_remote || wit.claims_partial) throw std::runtime_error(std::string(call) + ": this witness lacks traces that another rank computes");
  }

  // the sources in origin order; lookup values a witness does not hold are computed into temporaries that `keep` owns.
  // -> the number of messages M; max_len: the longest tuple a circuit's slot can have
  static size_t sources(HSystem& sys, HWitness& wit, const char* call, std::vector<Src>& srcs, std::vector<DBuf<u64>>& keep, size_t& max_len) {
    Ctx& ctx = *sys.ctx;
    const std::string name(call);
    const size_t C = sys.circuits.size(), n_claims = wit.claim_offsets.size() - 1;
    size_t M = 0, slot0 = 0;
    if (n_claims) {
      if (wit.claim_data.size() >> 32) throw std::runtime_error(name + ": more than 2^32 claim elements");
      Src s{};
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
          keep.push_back(lb_alloc<u64>(ctx, h * L, call, "a circuit's multiplicities"));
          keep.push_back(lb_alloc<u64>(ctx, std::max<size_t>(h * c.args_width, 1), call, "a circuit's lookup arguments"));
          u64 *tm = keep[keep.size() - 2].p, *ta = keep.back().p;
          if (!c.prefix_on_device || !lookup_values_device(ctx, c.prefix_prog, wit.traces[ci].p, c.pre_width ? c.d_preprocessed.p : nullptr, h,
                                                           c.main_width, c.pre_width, c.args_width, tm, ta))
            throw std::runtime_error("device-resident witness: this circuit's lookup prefix does not fit the device sweep");
          mult = tm, args = ta;
        }
        Src s{};
        s.base = M, s.count = h * L, s.mult = mult, s.args = args, s.offs = lk.arg_offsets.p;
        s.L = (u32)L, s.aw = (u32)c.args_width, s.circuit = (u32)ci, s.slot0 = (u32)slot0;
        srcs.push_back(s);
        M += h * L;
        for (auto& l : c.lookups) max_len = std::max(max_len, l.second.size());
      }
      slot0 += L;
    }
    if (M >> 40) throw std::runtime_error(name + ": more than 2^40 messages");
    return M;
  }

  static size_t max_claim_len(const HWitness& wit) {
    size_t len = 0;
    for (size_t i = 0; i + 1 < wit.claim_offsets.size(); i++) len = std::max<size_t>(len, wit.claim_offsets[i + 1] - wit.claim_offsets[i]);
    return len;
  }
};

}  // namespace
}  // namespace msamd
