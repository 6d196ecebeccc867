// msbb_witness_fill (the BabyBear / Poseidon2 configuration): what the shared kernels and driver of fill_dev.h need to know of
// BabyBear (p = 2^31 - 2^27 + 1; what differs in the definition is listed in include/mstark_bb.h).
//
// What differs in this field:
//   - the library's trace and BCircuit::pre are column-major Montgomery matrices with a leading dimension: a cell is
//     buf[c * ld + row], read through bb_from_monty and written once, at the end, as bb_to_monty(slot). Consecutive threads are
//     consecutive rows of one column, so every load and store of a wave is contiguous;
//   - slots are u32 and hold CANONICAL values: bits, lt, xor and and work on them as they lie, add / sub / neg are the modular
//     forms, and mul(a, b) is one bb_to_monty and one Montgomery multiplication (a R * b / R = a b). inv0 is the chain x^(p - 2)
//     on the Montgomery word, which maps 0 to 0;
//   - the slot file takes 4 bytes per word: in LDS at 256 lanes up to 64 slots, 128 up to 128, 64 up to 256;
//   - inputs pass through ingest_babybear into a column-major Montgomery temporary with leading dimension h_in;
//   - the witness holds no lookup values, and there are no peer reads (the third format is refused by the magic);
//   - the scan computes on MONTGOMERY words: the coefficient pass stores them (column-major with leading dimension n: A in
//     tmp[r], B in tmp[n + r]; B alone in tmp[r] in the additive form), (a, b) then (a', b') is (a' a, a' b + b') with bb_mul on
//     the words as they lie - a Montgomery product of two Montgomery words is the Montgomery word of the product - and 1 is BB_R1.
//     A thread's rows r0 .. r0 + 3 need the coefficients of rows r0 - 1 .. r0 + 2: it loads those of its own rows r0 .. r0 + 3,
//     ONE 16-byte load per coefficient column where that address is 16-byte aligned and all four rows lie below n (4-byte loads
//     guarded by n otherwise: the temporary is aligned and r0 a multiple of 4, so that is the tail alone), and takes row r0 - 1
//     from the lane before it (lane 0 of a wave loads it itself). The dst column of a column-major trace is contiguous: the four
//     cells are one 16-byte store under the same two conditions - with ld below 4 (heights 1 and 2) or a dst column that starts
//     off a 16-byte boundary, 4-byte stores. A tile's aggregate lies split: a in aggs[t], b in aggs[n_tiles + t].
//
// CLAIM PROGRAMS (msbb_witness_claims_fill, below the fill): the same interpreter over the first rows of a trace with a row-major
// output, the witness's new claims; the driver is claims_fill.h, shared with Goldilocks.
#include "bb_host.h"
#include "claims_fill.h"

namespace msbb {

namespace {

using namespace msamd;  // fill_dev.h, the node kinds of program.h and fill_program.h, FillCode, the ingest helpers
static_assert(SC_ROWS % 4 == 0, "a thread's rows are whole 16-byte groups");

// One coefficient column (n words) for the rows r0 .. r0 + SC_ROWS - 1 of a thread, r0 a multiple of 4: out[j] = col[r0 + j - 1],
// the coefficient that row r0 + j follows. The thread loads col[r0 ..] - 16 bytes at a time where the address is aligned and
// the four rows lie below n, else word by word under the guard - and col[r0 - 1] is the last word of the lane before it; lane 0
// of a wave loads it itself. A word from n on, or in front of row 0, is never used (those rows carry the identity, or init).
// Every thread of the workgroup takes part in the shuffle.
__device__ __forceinline__ void bsc_load(const u32* col, size_t n, size_t r0, u32 out[SC_ROWS]) {
  u32 v[SC_ROWS];
  for (u32 q = 0; q < SC_ROWS; q += 4) {
    const u32* a = col + r0 + q;
    if (r0 + q + 4 <= n && (reinterpret_cast<uintptr_t>(a) & 15) == 0) {
      const uint4 w = *reinterpret_cast<const uint4*>(a);
      v[q] = w.x, v[q + 1] = w.y, v[q + 2] = w.z, v[q + 3] = w.w;
    } else {
      for (u32 j = 0; j < 4; j++) v[q + j] = r0 + q + j < n ? a[j] : 0;
    }
  }
  u32 prev = sc_up(v[SC_ROWS - 1], 1);
  if ((threadIdx.x & 63) == 0) prev = r0 > 0 && r0 - 1 < n ? col[r0 - 1] : 0;
  out[0] = prev;
  for (u32 j = 1; j < SC_ROWS; j++) out[j] = v[j - 1];
}

struct BbFill {
  using Word = u32;
  static constexpr u32 BITS = 32;
  static constexpr u32 P = BB_P;
  static constexpr bool PEERS = false;
  static constexpr const char* call = "msbb_witness_fill";
  static constexpr FillField magic = FILL_BABYBEAR;
  static __device__ __forceinline__ u32 add(u32 a, u32 b) { return bb_add(a, b); }
  static __device__ __forceinline__ u32 sub(u32 a, u32 b) { return bb_sub(a, b); }
  static __device__ __forceinline__ u32 mul(u32 a, u32 b) { return bb_mul(bb_to_monty(a), b); }  // a R * b / R
  static __device__ __forceinline__ u32 neg(u32 a) { return bb_neg(a); }
  static __device__ __forceinline__ u32 inv0(u32 a) { return bb_from_monty(bb_inv(bb_to_monty(a))); }  // (the chain x^(p - 2) maps 0 to 0)
  static __device__ __forceinline__ u32 load(u32 w) { return bb_from_monty(w); }
  static __device__ __forceinline__ u32 stored(u32 v) { return bb_to_monty(v); }
  static __device__ __forceinline__ u32 row(size_t r) { return (u32)r; }  // (heights are at most 2^27 < p)

  using Column = u32*;  // a scan's dst column: n contiguous Montgomery words
  struct View {
    const u32* d_main;         // main_w columns of leading dimension ld, Montgomery: read
    u32* d_out;                // written, column-major with leading dimension out_ld: the trace (out_ld = ld), or the temporary of a coefficient pass (n)
    size_t out_ld;
    const u32 *d_pre, *d_inp;  // pre_w columns of leading dimension pre_ld; n_in columns of leading dimension h_in
    size_t n, h_in, ld, pre_ld;
    __device__ __forceinline__ const u32& main(size_t row, u32 col) const { return d_main[col * ld + row]; }
    __device__ __forceinline__ const u32& pre(size_t row, u32 col) const { return d_pre[col * pre_ld + row]; }
    __device__ __forceinline__ const u32& inp(size_t row, u32 col) const { return d_inp[col * h_in + row]; }
    __device__ __forceinline__ void store(size_t row, u32 col, u32 v) const { d_out[col * out_ld + row] = v; }
    void to_tmp(u32* tmp, uint32_t) { d_out = tmp, out_ld = n; }
    void inputs(const u32* p, size_t h, size_t) { d_inp = p, h_in = h; }
    Column column(uint32_t dst) const { return d_out + size_t(dst) * ld; }
  };

  // ---- the scan: Montgomery words
  static __device__ __forceinline__ u32 one() { return BB_R1; }
  static __device__ __forceinline__ u32 sc_mul(u32 a, u32 b) { return bb_mul(a, b); }
  // the maps of the thread's rows: (1, init) at row 0, (A(r-1), B(r-1)) behind it, the identity from row n on
  template <bool ADD>
  static __device__ __forceinline__ void rows(const ScParams<BbFill>& p, size_t r0, Aff<BbFill> row[SC_ROWS]) {
    u32 a[SC_ROWS], b[SC_ROWS];
    if (!ADD) bsc_load(p.tmp, p.n, r0, a);
    bsc_load(ADD ? p.tmp : p.tmp + p.n, p.n, r0, b);
    for (u32 j = 0; j < SC_ROWS; j++) {
      const size_t r = r0 + j;
      row[j] = r >= p.n ? Aff<BbFill>{BB_R1, 0} : r == 0 ? Aff<BbFill>{BB_R1, p.init} : Aff<BbFill>{ADD ? BB_R1 : a[j], b[j]};
    }
  }
  static __device__ __forceinline__ void store(const ScParams<BbFill>& p, size_t r0, const u32 cell[SC_ROWS]) {
    for (u32 q = 0; q < SC_ROWS; q += 4) {
      u32* d = p.dst + r0 + q;
      if (r0 + q + 4 <= p.n && (reinterpret_cast<uintptr_t>(d) & 15) == 0) {
        *reinterpret_cast<uint4*>(d) = make_uint4(cell[q], cell[q + 1], cell[q + 2], cell[q + 3]);
      } else {
        for (u32 j = 0; j < 4; j++)
          if (r0 + q + j < p.n) d[j] = cell[q + j];
      }
    }
  }
  static __device__ __forceinline__ Aff<BbFill> agg_get(const ScParams<BbFill>& p, u32 t) {
    return Aff<BbFill>{p.aggs[t], p.aggs[size_t(p.n_tiles) + t]};
  }
  static __device__ __forceinline__ void agg_put(const ScParams<BbFill>& p, u32 t, Aff<BbFill> f) {
    p.aggs[t] = f.a;
    p.aggs[size_t(p.n_tiles) + t] = f.b;
  }

  // ---- the host side
  static void fail(const std::string& what) { fl_fail<BbFill>(what); }
  static View accept(BSystem& sys, BWitness& wit, size_t ci) {
    const size_t C = sys.circuits.size();
    if (wit.sys != &sys || wit.heights.size() != C || wit.traces.size() != C) fail("the witness does not belong to this system");
    if (wit.host_resident) fail("takes a device-resident witness (msbb_witness_create, msbb_witness_create_device)");
    if (ci >= C) fail("circuit " + std::to_string(ci) + " is out of range");
    const size_t n = wit.heights[ci];
    if (!n) fail("circuit " + std::to_string(ci) + " is inactive (height 0)");
    const BCircuit& c = sys.circuits[ci];
    BMat& tr = wit.traces[ci];
    if (!tr.buf.p || tr.h != n || tr.w != c.main_width || tr.ld < n) fail("the circuit has no trace on this device");
    const bool pre = c.pre_width && n == c.pre_height && c.pre.buf.p && c.pre.h == n && c.pre.w == c.pre_width && c.pre.ld >= n;
    View v{};
    v.d_main = v.d_out = tr.buf.p;
    v.out_ld = v.ld = tr.ld;
    v.d_pre = pre ? c.pre.buf.p : nullptr, v.pre_ld = pre ? c.pre.ld : 0;
    v.n = n;
    return v;
  }
  static void resolve_peers(BSystem&, BWitness&, size_t, const FillCode&, View&) {}
  static void held_before(BSystem&, BWitness&, size_t) {}
  static void after(BSystem&, BWitness&, size_t) {}
  static void ingest(Ctx& ctx, const IngestView& in, u32* out, u64* bad) { ingest_babybear(ctx, in, out, bad); }
  static u32 init(u64 v) { return bb_to_monty((u32)v); }  // (init < p: fill_compile)
  static bool too_high(size_t) { return false; }          // (heights are at most 2^27: 2^17 tiles)
};

}  // namespace

void fill_program_info(const uint8_t* program, size_t program_len, u64 out4[4]) {
  fl_program_info<BbFill>(program, program_len, "msbb_fill_program_info", out4);
}

void fill_scan_info(const uint8_t* program, size_t program_len, u64 out4[4]) { fl_scan_info<BbFill>(program, program_len, "msbb_fill_scan_info", out4); }

void witness_fill(BSystem& sys, BWitness& wit, size_t ci, const uint8_t* program, size_t program_len, const ms_dev_matrix* inputs,
                  void* producer_stream, u64 summary[4]) {
  fl_witness_fill<BbFill>(sys, wit, ci, program, program_len, inputs, producer_stream, summary);
}

// ---- msbb_witness_claims_fill: the claims of a witness from its traces (include/mstark_bb.h; the definition is "CLAIM PROGRAMS"
// of include/mstark.h). The driver is cl_witness_claims_fill of claims_fill.h; what BabyBear decides:
//   - the traces are column-major and the claim list is ROW-major (claim k is W consecutive words), so the pass is
//     fill_k<BbClaimFill, *>: BbFill with a View of its own whose store writes d_out[row * out_w + col]. Reads are BbFill's. With
//     W > 1 the 4-byte stores of a wave are W words apart, not contiguous (DESIGN.md has the measured cost);
//   - the words are Montgomery words in [0, p) on the device - what the pass stores (F::stored) is what d_claim_data holds - and
//     a keep flag is compared as the stored word: the Montgomery word of v is 0 exactly when v is 0;
//   - the compaction is claims_dev.h instantiated for u32. Bytes per row with S = 4: the pass writes 4 (W + 1), the count launch
//     reads 4 (the flag; one 32-byte sector where W + 1 >= 8), the scatter reads 4 again and 4 W per kept row and writes 4 W per
//     kept row; counts and offsets stay 16 bytes per tile;
//   - the host copy, BWitness::claims, is one canonical vector per claim (the transcript absorbs them): the new elements are
//     read back once, converted on the host and cut into vectors of W beside the witness's list;
//   - no claims_partial and no has_remote: neither form of witness exists in this configuration.
namespace {

struct BbClaimFill : BbFill {
  struct View : BbFill::View {
    uint32_t out_w;  // d_out is rows x out_w row-major here; out_ld is not used
    __device__ __forceinline__ void store(size_t row, u32 col, u32 v) const { d_out[row * out_w + col] = v; }
    void to_tmp(u32* out, uint32_t cols) { d_out = out, out_w = cols; }
  };
};

struct BbClaims {
  using Fill = BbClaimFill;
  static constexpr const char* call = "msbb_witness_claims_fill";
  static void fail(const std::string& what) { throw std::runtime_error(std::string(call) + ": " + what); }
  static void accept(BSystem& sys, BWitness& wit) {
    const size_t C = sys.circuits.size();
    if (wit.sys != &sys || wit.heights.size() != C || wit.traces.size() != C) fail("the witness does not belong to this system");
    if (wit.host_resident) fail("takes a device-resident witness (msbb_witness_create, msbb_witness_create_device)");
  }
  static BbClaimFill::View trace(BSystem& sys, BWitness& wit, size_t ci) {
    if (ci >= sys.circuits.size()) fail("circuit " + std::to_string(ci) + " is out of range");
    const size_t n = wit.heights[ci];
    if (!n) fail("circuit " + std::to_string(ci) + " is inactive (height 0)");
    const BCircuit& c = sys.circuits[ci];
    const BMat& tr = wit.traces[ci];
    if (!tr.buf.p || tr.h != n || tr.w != c.main_width || tr.ld < n) fail("the circuit has no trace on this device");
    const bool pre = c.pre_width && n == c.pre_height && c.pre.buf.p && c.pre.h == n && c.pre.w == c.pre_width && c.pre.ld >= n;
    BbClaimFill::View v{};
    v.d_main = tr.buf.p, v.ld = tr.ld;
    v.d_pre = pre ? c.pre.buf.p : nullptr, v.pre_ld = pre ? c.pre.ld : 0;
    v.n = n;
    return v;
  }
  static size_t n_claims(const BWitness& wit) { return wit.claims.size(); }
  static size_t n_elems(const BWitness& wit) {
    size_t e = 0;
    for (auto& cl : wit.claims) e += cl.size();
    return e;
  }
  static const u64* d_offs(const BWitness& wit) { return wit.d_claim_offs.p; }
  static const u32* d_data(const BWitness& wit) { return wit.d_claim_data.p; }
  struct Host {
    const BWitness& wit;
    std::vector<std::vector<u32>> claims;  // canonical: the claims that stay, then the new ones
    std::vector<u32> flat;                 // the new elements as they lie on the device
    size_t n_base, W;
    Host(const BWitness& wit, size_t n_base, size_t, size_t kept, size_t W) : wit(wit), flat(kept * W), n_base(n_base), W(W) {
      claims.reserve(n_base + kept);
    }
    void read(Ctx& ctx, const u64*, const u32* d_new_data) {  // (the claims that stay are copied while the device works)
      claims.assign(wit.claims.begin(), wit.claims.begin() + n_base);
      ctx.d2h(flat.data(), d_new_data, flat.size() * 4);
      for (size_t k = 0; k * W < flat.size(); k++) {
        claims.emplace_back(W);
        for (size_t e = 0; e < W; e++) claims.back()[e] = bb_from_monty(flat[k * W + e]);
      }
    }
    void publish(BWitness& wit, DBuf<u64>&& d_new_offs, DBuf<u32>&& d_new_data) {
      wit.claims.swap(claims);
      wit.d_claim_offs = std::move(d_new_offs);
      wit.d_claim_data = std::move(d_new_data);
    }
  };
};

}  // namespace

void claims_program_info(const uint8_t* program, size_t program_len, u64 out4[4]) {
  cl_program_info<BbClaims>(program, program_len, "msbb_claims_program_info", out4);
}

void witness_claims_fill(BSystem& sys, BWitness& wit, size_t ci, const uint8_t* program, size_t program_len, size_t rows, const ms_dev_matrix* inputs,
                         void* producer_stream, uint32_t mode, u64 summary[4]) {
  cl_witness_claims_fill<BbClaims>(sys, wit, ci, program, program_len, rows, inputs, producer_stream, mode, summary);
}

}  // namespace msbb
