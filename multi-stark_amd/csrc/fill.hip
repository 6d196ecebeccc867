// ms_witness_fill (the Goldilocks configuration): what the shared kernels and driver of fill_dev.h need to know of Goldilocks.
//
// What differs in this field: slots are the 8-byte values as they lie in memory, and the scan computes on the same words. The
// trace, the preprocessed trace, the ingested inputs and the temporary of a coefficient pass are row-major, a cell is
// buf[row * width + col]: a scan thread loads the (A, B) of a row with one 16-byte load from the n x 2 temporary (n x 1, B
// alone, in the additive form) and stores each of its four dst cells with a strided 8-byte store, and a tile's aggregate lies
// interleaved, (a, b) at aggs[2 t]. When the witness holds lookup values for the circuit, lookup_values_k recomputes them
// behind the last group.
//
// PEER READS (the third format) exist in this field alone: source 4 + k of OP_VAR / OP_AT reads entry k of View::peers, the
// main or preprocessed trace of ANOTHER circuit of the witness, with that matrix's own height as the bound. resolve_peers
// checks the program's records against the system and the witness and refuses before any launch; the call writes no peer.
//
// CLAIM PROGRAMS (ms_witness_claims_fill, below the fill): the same interpreter over the first rows of a trace, its output the
// witness's new claims; the driver is claims_fill.h, shared with BabyBear, the compaction of a keep mask is claims_dev.h.
#include "claims_fill.h"
#include "host.h"

namespace msamd {

namespace {

struct FlPeer {  // a peer read's matrix: another circuit's main or preprocessed trace, h x w row-major (h = 0: inactive, p unused)
  const u64* p;
  size_t h;
  uint32_t w;
};

struct GlFill {
  using Word = u64;
  static constexpr u32 BITS = 64;
  static constexpr u64 P = GL_P;
  static constexpr bool PEERS = true;
  static constexpr const char* call = "ms_witness_fill";
  static constexpr FillField magic = FILL_GOLDILOCKS;
  static __device__ __forceinline__ u64 add(u64 a, u64 b) { return gl_add(a, b); }
  static __device__ __forceinline__ u64 sub(u64 a, u64 b) { return gl_sub(a, b); }
  static __device__ __forceinline__ u64 mul(u64 a, u64 b) { return gl_mul(a, b); }
  static __device__ __forceinline__ u64 neg(u64 a) { return gl_neg(a); }
  static __device__ __forceinline__ u64 inv0(u64 a) { return gl_inv(a); }  // (the chain x^(p - 2) maps 0 to 0)
  static __device__ __forceinline__ u64 load(u64 w) { return w; }
  static __device__ __forceinline__ u64 stored(u64 v) { return v; }
  static __device__ __forceinline__ u64 row(size_t r) { return (u64)r; }

  struct Column {  // a scan's dst column: cell r at p[r * w + c]
    u64* p;
    uint32_t w, c;
  };
  struct View {
    const u64* d_main;        // n x main_w row-major, read
    u64* d_out;               // n x out_w row-major, written: the trace (out_w = main_w), or the temporary of a coefficient pass
    uint32_t out_w;
    const u64 *d_pre, *d_inp;  // n x pre_w and h_in x n_in, row-major
    size_t n, h_in;
    uint32_t main_w, pre_w, n_in;
    FlPeer peers[FL_MAX_PEERS];  // source 4 + k; indexed by the instruction word alone, so the lookup is wave-uniform
    __device__ __forceinline__ const u64& main(size_t row, u32 col) const { return d_main[row * main_w + col]; }
    __device__ __forceinline__ const u64& pre(size_t row, u32 col) const { return d_pre[row * pre_w + col]; }
    __device__ __forceinline__ const u64& inp(size_t row, u32 col) const { return d_inp[row * n_in + col]; }
    __device__ __forceinline__ u64 peer(u32 k, u64 row, u32 col) const {  // a row from the peer's height on loads nothing
      const FlPeer& q = peers[k];
      return row < (u64)q.h ? q.p[(size_t)row * q.w + col] : 0;
    }
    __device__ __forceinline__ void store(size_t row, u32 col, u64 v) const { d_out[row * out_w + col] = v; }
    void to_tmp(u64* tmp, uint32_t cols) { d_out = tmp, out_w = cols; }
    void inputs(const u64* p, size_t h, size_t w) { d_inp = p, h_in = h, n_in = (uint32_t)w; }
    Column column(uint32_t dst) const { return Column{d_out, main_w, dst}; }
  };

  // ---- the scan: the words as they lie
  static __device__ __forceinline__ u64 one() { return 1; }
  static __device__ __forceinline__ u64 sc_mul(u64 a, u64 b) { return gl_mul(a, b); }
  template <bool ADD>
  static __device__ __forceinline__ void rows(const ScParams<GlFill>& p, size_t r0, Aff<GlFill> row[SC_ROWS]) {
    for (u32 j = 0; j < SC_ROWS; j++) {
      const size_t r = r0 + j;
      if (r >= p.n) {
        row[j] = Aff<GlFill>{1, 0};
      } else if (r == 0) {
        row[j] = Aff<GlFill>{1, p.init};
      } else if (ADD) {
        row[j] = Aff<GlFill>{1, p.tmp[r - 1]};
      } else {
        const ulonglong2 v = reinterpret_cast<const ulonglong2*>(p.tmp)[r - 1];
        row[j] = Aff<GlFill>{v.x, v.y};
      }
    }
  }
  static __device__ __forceinline__ void store(const ScParams<GlFill>& p, size_t r0, const u64 cell[SC_ROWS]) {
    for (u32 j = 0; j < SC_ROWS; j++)
      if (r0 + j < p.n) p.dst.p[(r0 + j) * p.dst.w + p.dst.c] = cell[j];
  }
  static __device__ __forceinline__ Aff<GlFill> agg_get(const ScParams<GlFill>& p, u32 t) {
    return Aff<GlFill>{p.aggs[2 * size_t(t)], p.aggs[2 * size_t(t) + 1]};
  }
  static __device__ __forceinline__ void agg_put(const ScParams<GlFill>& p, u32 t, Aff<GlFill> f) {
    p.aggs[2 * size_t(t)] = f.a;
    p.aggs[2 * size_t(t) + 1] = f.b;
  }

  // ---- the host side
  static void fail(const std::string& what) { fl_fail<GlFill>(what); }
  static View accept(HSystem& sys, HWitness& wit, size_t ci) {
    const size_t C = sys.circuits.size();
    if (wit.sys != &sys || wit.heights.size() != C) fail("the witness does not belong to this system");
    if (wit.host_resident) fail("takes a device-resident witness (ms_witness_create, ms_witness_create_device, the generators)");
    if (wit.has_remote) fail("this witness lacks traces that another rank computes");
    if (ci >= C) fail("circuit " + std::to_string(ci) + " is out of range");
    const size_t n = wit.heights[ci];
    if (!n) fail("circuit " + std::to_string(ci) + " is inactive (height 0)");
    if (!wit.traces[ci].p) fail("the circuit has no trace on this device");
    const HCircuit& c = sys.circuits[ci];
    View v{};
    v.d_main = v.d_out = wit.traces[ci].p;
    v.out_w = v.main_w = (uint32_t)c.main_width, v.pre_w = (uint32_t)c.pre_width;
    v.d_pre = c.pre_width && n == c.pre_height ? c.d_preprocessed.p : nullptr;
    v.n = n;
    return v;
  }
  static void resolve_peers(HSystem& sys, HWitness& wit, size_t ci, const FillCode& fc, View& v) {  // each record against the system and the witness
    const size_t C = sys.circuits.size();
    for (size_t k = 0; k < fc.peers.size(); k++) {
      const FillPeer& r = fc.peers[k];
      FlPeer& q = v.peers[k];
      const std::string at = "peer " + std::to_string(k) + " (circuit " + std::to_string(r.circuit) + ", " + (r.trace ? "main" : "preprocessed") + " trace): ";
      if (r.circuit >= C) fail(at + "the circuit is out of range (the system has " + std::to_string(C) + ")");
      if (r.circuit == ci) fail(at + "a peer is another circuit than the one being filled (use source " + std::to_string(r.trace) + " for circuit " + std::to_string(ci) + " itself)");
      const HCircuit& pc = sys.circuits[r.circuit];
      const size_t have = r.trace ? pc.main_width : pc.pre_width;
      if (r.width != have) fail(at + "the program declares width " + std::to_string(r.width) + ", the circuit has " + std::to_string(have));
      if (r.trace) {
        q.h = wit.heights[r.circuit];
        q.p = wit.traces[r.circuit].p;
        if (q.h && !q.p) fail(at + "the circuit has no trace on this device");
      } else {
        q.h = pc.pre_width ? pc.pre_height : 0;
        q.p = pc.d_preprocessed.p;
        if (q.h && !q.p) fail(at + "the preprocessed trace is not on the device");
      }
      q.w = (uint32_t)r.width;
    }
  }
  static void held_before(HSystem& sys, HWitness& wit, size_t ci) {
    const HCircuit& c = sys.circuits[ci];
    if (wit.lookups[ci].mult.p && (!c.prefix_on_device || c.prefix_prog.n_slots * 64 * 8 > 64 * 1024))
      fail("the witness holds lookup values for circuit " + std::to_string(ci) + " and its lookup prefix does not fit the device sweep");
  }
  // SystemWitness::from_stage_1 again for the values the witness holds (checked in held_before: the sweep fits)
  static void after(HSystem& sys, HWitness& wit, size_t ci) {
    const HCircuit& c = sys.circuits[ci];
    DLookups& lk = wit.lookups[ci];
    if (lk.mult.p && !lookup_values_device(*sys.ctx, c.prefix_prog, wit.traces[ci].p, c.pre_width ? c.d_preprocessed.p : nullptr, wit.heights[ci],
                                           c.main_width, c.pre_width, c.args_width, lk.mult.p, lk.args.p))
      fail("internal error (the lookup prefix was found to fit and does not)");
  }
  static void ingest(Ctx& ctx, const IngestView& in, u64* out, u64* bad) { ingest_goldilocks(ctx, in, out, bad); }
  static u64 init(u64 v) { return v; }
  static bool too_high(size_t n_tiles) { return n_tiles > (size_t(1) << 31); }
};

}  // namespace

void fill_program_info(const uint8_t* program, size_t program_len, u64 out4[4]) {
  fl_program_info<GlFill>(program, program_len, "ms_fill_program_info", out4);
}

size_t fill_peer_info(const uint8_t* program, size_t program_len, u64* out, size_t cap) {
  const FillCode fc = fill_compile(program, program_len, "ms_fill_peer_info", FILL_GOLDILOCKS);
  if (fc.peers.size() <= cap)
    for (size_t k = 0; k < fc.peers.size(); k++) out[3 * k] = fc.peers[k].circuit, out[3 * k + 1] = fc.peers[k].trace, out[3 * k + 2] = fc.peers[k].width;
  return fc.peers.size();
}

void fill_scan_info(const uint8_t* program, size_t program_len, u64 out4[4]) { fl_scan_info<GlFill>(program, program_len, "ms_fill_scan_info", out4); }

void witness_fill(HSystem& sys, HWitness& wit, size_t ci, const uint8_t* program, size_t program_len, const ms_dev_matrix* inputs,
                  void* producer_stream, u64 summary[4]) {
  fl_witness_fill<GlFill>(sys, wit, ci, program, program_len, inputs, producer_stream, summary);
}

// ---- ms_witness_claims_fill: the claims of a witness from its traces (include/mstark.h, "CLAIM PROGRAMS"). The driver is
// cl_witness_claims_fill of claims_fill.h; what Goldilocks decides: a witness that holds only a slice of its claims or lacks
// traces another rank computes is refused, the pass is fill_k<GlFill, *> whose row-major View takes the claim data as it is, and
// the host copy is the flat offset and element vectors of HWitness (short transcripts are hashed from them).
namespace {

struct GlClaims {
  using Fill = GlFill;
  static constexpr const char* call = "ms_witness_claims_fill";
  static void fail(const std::string& what) { throw std::runtime_error(std::string(call) + ": " + what); }
  static void accept(HSystem& sys, HWitness& wit) {
    if (wit.sys != &sys || wit.heights.size() != sys.circuits.size()) fail("the witness does not belong to this system");
    if (wit.claims_partial) fail("this witness holds only a slice of its claims (ms_witness_create_host_sliced)");
    if (wit.host_resident) fail("takes a device-resident witness (ms_witness_create, ms_witness_create_device, the generators)");
    if (wit.has_remote) fail("this witness lacks traces that another rank computes");
  }
  static GlFill::View trace(HSystem& sys, HWitness& wit, size_t ci) {
    if (ci >= sys.circuits.size()) fail("circuit " + std::to_string(ci) + " is out of range");
    const size_t n = wit.heights[ci];
    if (!n) fail("circuit " + std::to_string(ci) + " is inactive (height 0)");
    if (!wit.traces[ci].p) fail("the circuit has no trace on this device");
    const HCircuit& c = sys.circuits[ci];
    GlFill::View v{};
    v.d_main = wit.traces[ci].p, v.main_w = (uint32_t)c.main_width, v.pre_w = (uint32_t)c.pre_width, v.n = n;
    v.d_pre = c.pre_width && n == c.pre_height ? c.d_preprocessed.p : nullptr;
    return v;
  }
  static size_t n_claims(const HWitness& wit) { return wit.claim_offsets.size() - 1; }
  static size_t n_elems(const HWitness& wit) { return wit.claim_data.size(); }
  static const u64* d_offs(const HWitness& wit) { return wit.d_claim_offsets.p; }
  static const u64* d_data(const HWitness& wit) { return wit.d_claim_data.p; }
  struct Host {
    const HWitness& wit;
    std::vector<u64> offs, data;
    size_t n_base, e_base;
    Host(const HWitness& wit, size_t n_base, size_t e_base, size_t kept, size_t W)
        : wit(wit), offs(n_base + kept + 1), data(e_base + kept * W), n_base(n_base), e_base(e_base) {}
    void read(Ctx& ctx, const u64* d_new_offs, const u64* d_new_data) {  // (the claims that stay are copied while the device works)
      std::copy(wit.claim_offsets.begin(), wit.claim_offsets.begin() + n_base, offs.begin());
      std::copy(wit.claim_data.begin(), wit.claim_data.begin() + e_base, data.begin());
      ctx.d2h_queue(offs.data() + n_base, d_new_offs, (offs.size() - n_base) * 8);
      ctx.d2h(data.data() + e_base, d_new_data, (data.size() - e_base) * 8);
    }
    void publish(HWitness& wit, DBuf<u64>&& d_new_offs, DBuf<u64>&& d_new_data) {
      wit.claim_offsets.swap(offs);
      wit.claim_data.swap(data);
      wit.claim_elems_total = wit.claim_data.size();
      wit.d_claim_offsets = std::move(d_new_offs);
      wit.d_claim_data = std::move(d_new_data);
    }
  };
};

}  // namespace

void claims_program_info(const uint8_t* program, size_t program_len, u64 out4[4]) {
  cl_program_info<GlClaims>(program, program_len, "ms_claims_program_info", out4);
}

void witness_claims_fill(HSystem& sys, HWitness& wit, size_t ci, const uint8_t* program, size_t program_len, size_t rows, const ms_dev_matrix* inputs,
                         void* producer_stream, uint32_t mode, u64 summary[4]) {
  cl_witness_claims_fill<GlClaims>(sys, wit, ci, program, program_len, rows, inputs, producer_stream, mode, summary);
}

}  // namespace msamd
