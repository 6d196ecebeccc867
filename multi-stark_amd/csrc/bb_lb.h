// What the grouping table of lb_dev.h and the two exact lookup calls built on it (bb_balance.hip, bb_multiplicity.hip) need to
// know of BabyBear.
//
// INVARIANT: every word read here is a Montgomery word that is a reduced representative (< p): the upload converts canonical
// values with bb_to_monty, the sweep's constants come from bb_to_monty, and bb_add / bb_sub / bb_mul / bb_neg return values
// below p. Montgomery form is a bijection on [0, p) that fixes 0, so equality and zero tests on the words ARE equality and zero
// tests on the values: tuples are stripped, hashed and compared as they lie, and nothing is canonicalised first. bb_from_monty
// is applied only to what is summed (the multiplicities) and to what is reported (the tuples; the net is a sum of canonical values).
//
// The sum of a group: one array, the plain 64-bit sum of the canonical multiplicities. Fewer than 2^32 messages (the host
// refuses more, before anything is allocated or launched) of values below 2^31 stay below 2^63, so one atomicAdd per insertion
// is exact, every multiplicity may go through the LDS table of lb_insert_k, and the net is sum mod p when it is read. The same
// limit keeps a message's index within its source in 32 bits: its row and slot are one 32-bit divide.
//
// Host side: the witness holds no lookup values. The count comes first; then each active circuit's lookup values are swept
// (bb_lookup_values_async, bb_kernels.hip) into temporaries of the call, row-major (multiplicities h x L, arguments h x
// args_width), so that the 64 consecutive messages of a wave - 64 / L rows x L slots - read one contiguous run of each. The
// claims are read where the witness keeps them.
#pragma once
#include "../../include/mstark_bb.h"
#include "bb_host.h"
#include "lb_dev.h"

namespace msbb {
namespace {

struct BbLookup {
  using Word = u32;
  using Idx = u32;
  using Tab = msamd::LbTab<BbLookup>;
  using Src = msamd::LbSrc<BbLookup>;
  static constexpr unsigned SUMS = 1;
  static constexpr const char *call_balance = "msbb_witness_lookup_balance", *call_derive = "msbb_witness_derive_multiplicities";

  static __device__ __forceinline__ u32 key(u32 w) { return w; }
  static __device__ __forceinline__ u32 mult(u32 w) { return bb_from_monty(w); }
  static __device__ __forceinline__ u32 report(u32 w) { return bb_from_monty(w); }

  static __device__ __forceinline__ bool lds_value(u32 m, u64& v) {
    v = m;
    return true;
  }
  static __device__ __forceinline__ void flush(const Tab& t, u64 s, u64 v) { atomicAdd((unsigned long long*)&t.sum[0][s], (unsigned long long)v); }
  static __device__ __forceinline__ bool add(const Tab& t, u64 s, u32 m) {
    flush(t, s, m);
    return true;
  }
  static __device__ __forceinline__ u64 net(const Tab& t, u64 s) { return t.sum[0][s] % BB_P; }

  // a derived cell: row r of the derived column (buf + m * ld, column-major, Montgomery). Consecutive threads are consecutive
  // rows, so the stores of a wave are contiguous; nothing is held
  struct Cell {
    u32* col;
  };
  template <class Tgt>
  static __device__ __forceinline__ void store(const Tgt& g, u64 r, u64 demand) {
    const u32 d = (u32)demand;  // (a net: below p)
    g.cell.col[r] = bb_to_monty(g.pull ? d : (d ? BB_P - d : 0));
  }

  // the witnesses both calls take: of this system, and device-resident
  static void accept(const BSystem& sys, const BWitness& wit, const char* call) {
    const size_t C = sys.circuits.size();
    if (wit.sys != &sys || wit.heights.size() != C || wit.traces.size() != C) throw std::runtime_error("witness does not belong to this system");
    if (wit.host_resident)
      throw std::runtime_error(std::string(call) + " takes a device-resident witness (msbb_witness_create, msbb_witness_create_device)");
  }

  // The sources of the witness's messages in origin order -> the message count M (0: no claims and no active circuit with
  // lookups; nothing was launched). The count comes first: nothing is allocated or launched for a call that is refused. Then each
  // active circuit's lookup values are swept into temporaries of the call, which `keep` owns (two per source of a circuit:
  // multiplicities, arguments). max_len: the longest tuple of a circuit's lookups.
  static size_t sources(BSystem& sys, BWitness& wit, const char* call, std::vector<Src>& srcs, std::vector<DBuf<u32>>& keep, size_t& max_len) {
    using msamd::lb_alloc;
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
      Src s{};
      s.base = 0, s.count = n_claims, s.mult = nullptr, s.args = wit.d_claim_data.p, s.offs = wit.d_claim_offs.p, s.L = 1;
      srcs.push_back(s);
      base += n_claims;
    }
    for (size_t ci = 0; ci < C; ci++) {
      const BCircuit& c = sys.circuits[ci];
      const size_t h = wit.heights[ci], L = c.num_lookups;
      if (h && L) {
        keep.push_back(lb_alloc<u32>(ctx, h * L, call, "a circuit's multiplicities"));
        keep.push_back(lb_alloc<u32>(ctx, std::max<size_t>(h * c.args_width, 1), call, "a circuit's lookup arguments"));
        u32 *tm = keep[keep.size() - 2].p, *ta = keep.back().p;
        {
          DBuf<u32> scratch = lb_alloc<u32>(ctx, std::max<size_t>(c.lookup_prefix_len, 1) * h, call, "a circuit's sweep scratch");
          bb_lookup_values_async(ctx, c.prog, c.lookup_prefix_len, c.lk, c.args_width, wit.traces[ci], c.pre_width ? &c.pre : nullptr, scratch.p, tm, ta);
        }  // (released behind the launch: the pool hands a block on in stream order)
        Src s{};
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

  static size_t max_claim_len(const BWitness& wit) {
    size_t len = 0;
    for (auto& cl : wit.claims) len = std::max(len, cl.size());
    return len;
  }
};

}  // namespace
}  // namespace msbb
