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
// witness's new claims; the compaction of a keep mask is claims_dev.h.
#include "claims_dev.h"
#include "fill_dev.h"
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

// ---- ms_witness_claims_fill: the claims of a witness from its traces (include/mstark.h, "CLAIM PROGRAMS")
//
// The program's one pass is fill_k<GlFill, LDS> as ms_witness_fill launches it, over the first `rows` rows and with
// View::to_tmp as its output: without a keep root straight into the new claim data behind the claims that stay (rows x W,
// row-major: the rows ARE the claims), with one into a temporary of rows x (W + 1) that claims_dev.h compacts. The new offset and
// data arrays are built beside the witness's and change places with them, host copies included, as the last thing the call does:
// until then it writes nothing the witness owns, so every refusal, an allocation failure at any point and the offender word of
// the inputs leave the witness as it was. Host waits: [the offender word and the kept total, one read-back: when there are
// inputs or a keep root], the host copy of the new claims.
void claims_program_info(const uint8_t* program, size_t program_len, u64 out4[4]) {
  const ClaimCode cc = claims_compile(program, program_len, "ms_claims_program_info", GlFill::magic);
  out4[0] = cc.pass.n_instr, out4[1] = cc.pass.n_slots, out4[2] = slot_lds_lanes(cc.pass.n_slots, sizeof(u64), 0);
  out4[3] = cc.width | (u64(cc.has_keep) << 32);
}

void witness_claims_fill(HSystem& sys, HWitness& wit, size_t ci, const uint8_t* program, size_t program_len, size_t rows, const ms_dev_matrix* inputs,
                         void* producer_stream, uint32_t mode, u64 summary[4]) {
  Ctx& ctx = *sys.ctx;
  const std::string name = "ms_witness_claims_fill";
  auto fail = [&](const std::string& what) -> void { throw std::runtime_error(name + ": " + what); };
  const size_t C = sys.circuits.size();
  if (wit.sys != &sys || wit.heights.size() != C) fail("the witness does not belong to this system");
  if (wit.claims_partial) fail("this witness holds only a slice of its claims (ms_witness_create_host_sliced)");
  if (wit.host_resident) fail("takes a device-resident witness (ms_witness_create, ms_witness_create_device, the generators)");
  if (wit.has_remote) fail("this witness lacks traces that another rank computes");
  if (mode != MS_CLAIMS_REPLACE && mode != MS_CLAIMS_APPEND) fail("mode " + std::to_string(mode) + " (MS_CLAIMS_REPLACE = 0, MS_CLAIMS_APPEND = 1)");
  if (ci >= C) fail("circuit " + std::to_string(ci) + " is out of range");
  const size_t n = wit.heights[ci];
  if (!n) fail("circuit " + std::to_string(ci) + " is inactive (height 0)");
  if (!wit.traces[ci].p) fail("the circuit has no trace on this device");
  const HCircuit& c = sys.circuits[ci];
  const ClaimCode cc = claims_compile(program, program_len, name, GlFill::magic);
  if (cc.main_w != c.main_width || cc.pre_w != c.pre_width)
    fail("the program is for main_width " + std::to_string(cc.main_w) + " and preprocessed width " + std::to_string(cc.pre_w) + ", circuit " +
         std::to_string(ci) + " has " + std::to_string(c.main_width) + " and " + std::to_string(c.pre_width));
  if (c.pre_width && (n != c.pre_height || !c.d_preprocessed.p)) fail("main trace height must equal preprocessed trace height");
  if (rows > n) fail("rows " + std::to_string(rows) + " is above the circuit's height " + std::to_string(n));
  IngestView in;
  size_t h_in = 0;
  if (cc.n_inputs) {
    if (!inputs) fail("the program reads " + std::to_string(cc.n_inputs) + " input columns and no input matrix was given");
    if (inputs->height > n) fail("input height " + std::to_string(inputs->height) + " is above the circuit's height " + std::to_string(n));
    h_in = (size_t)inputs->height;
    if (h_in) {
      try {
        in = ingest_check(ctx, *inputs, ci, cc.n_inputs, sizeof(u64));
      } catch (const std::exception& e) {
        fail(std::string("input matrix: ") + e.what());
      }
    }
  }
  const FillPass& pass = cc.pass;
  const bool keep = cc.has_keep;
  const size_t W = cc.width, cols = W + keep;
  const bool append = mode == MS_CLAIMS_APPEND;
  const size_t n_base = append ? wit.claim_offsets.size() - 1 : 0, e_base = append ? wit.claim_data.size() : 0;  // the claims that stay
  if ((e_base + rows * W) >> 60) fail("the last claim offset would be out of range");  // (rows x W < 2^42)
  const unsigned lanes = slot_lds_lanes(pass.n_slots, sizeof(u64), 0);
  const size_t batch = lanes || !rows ? rows : slot_scratch_rows(pass.n_slots, sizeof(u64), rows);
  const size_t n_tiles = (rows + CL_TILE - 1) / CL_TILE;

  // the buffers whose sizes are known now; with a keep root the new arrays follow the kept total
  DBuf<uint32_t> d_code(ctx, pass.code.size()), d_outs(ctx, pass.outs.size());
  DBuf<u64> d_consts(ctx, std::max<size_t>(pass.consts.size(), 1)), scratch, tmp, counts, offsets, packed, new_offs, new_data, fb(ctx, 2), inp;
  if (!lanes && rows) scratch = DBuf<u64>(ctx, batch * pass.n_slots);
  if (keep && rows) {
    tmp = DBuf<u64>(ctx, rows * cols);
    if (n_tiles > 1)
      counts = DBuf<u64>(ctx, n_tiles), offsets = DBuf<u64>(ctx, n_tiles);
    else
      packed = DBuf<u64>(ctx, rows * W);  // (one tile: launch (c) alone, into a buffer of the call, since the total is not known yet)
  }
  if (!keep) new_offs = DBuf<u64>(ctx, n_base + rows + 1), new_data = DBuf<u64>(ctx, std::max<size_t>(e_base + rows * W, 1));
  if (h_in) inp = DBuf<u64>(ctx, h_in * cc.n_inputs);
  ctx.h2d(d_code.p, pass.code.data(), pass.code.size() * 4);
  ctx.h2d(d_outs.p, pass.outs.data(), pass.outs.size() * 4);
  if (!pass.consts.empty()) ctx.h2d(d_consts.p, pass.consts.data(), pass.consts.size() * 8);
  ingest_wait_for_producer(ctx, producer_stream);
  try {
    HIP_CHECK(hipMemsetAsync(fb.p, 0xFF, 16, ctx.stream));  // [the inputs' offender word, the kept total]
    if (h_in) GlFill::ingest(ctx, in, inp.p, fb.p);
    if (rows) {
      FlParams<GlFill> p;
      p.v = GlFill::View{};
      p.v.d_main = wit.traces[ci].p, p.v.main_w = (uint32_t)c.main_width, p.v.pre_w = (uint32_t)c.pre_width, p.v.n = n;
      p.v.d_pre = c.pre_width ? c.d_preprocessed.p : nullptr;
      p.v.inputs(inp.p, h_in, cc.n_inputs);
      p.v.to_tmp(keep ? tmp.p : new_data.p + e_base, (uint32_t)cols);
      p.code = d_code.p, p.consts = d_consts.p, p.outs = d_outs.p;
      p.n_instr = (uint32_t)pass.n_instr, p.n_outs = (uint32_t)(pass.outs.size() / 2);
      p.row0 = 0, p.rows = rows, p.scratch = nullptr;
      if (lanes) {
        hipLaunchKernelGGL((fill_k<GlFill, true>), dim3((unsigned)((rows + lanes - 1) / lanes)), dim3(lanes), pass.n_slots * lanes * sizeof(u64), ctx.stream, p);
      } else {
        p.scratch = scratch.p;
        for (size_t r0 = 0; r0 < rows; r0 += batch) {
          p.row0 = r0;
          p.rows = std::min(batch, rows - r0);
          hipLaunchKernelGGL((fill_k<GlFill, false>), dim3((unsigned)((p.rows + 255) / 256)), dim3(256), 0, ctx.stream, p);
        }
      }
      HIP_CHECK(hipGetLastError());
    }
    ClParams<u64> cp{tmp.p, packed.p, counts.p, nullptr, fb.p + 1, rows, (u32)W, (u32)n_tiles};
    if (keep && rows) {  // (profiled as K_WITNESS_CLAIMS with the bytes the layout states: the flags here, the kept rows with the scatter)
      hipEvent_t ev = ctx.prof_begin(K_WITNESS_CLAIMS);
      if (n_tiles > 1) {
        cp.offsets = offsets.p;
        hipLaunchKernelGGL((claims_count_k<u64>), dim3((unsigned)n_tiles), dim3(CL_THREADS), 0, ctx.stream, cp);
        hipLaunchKernelGGL((claims_offsets_k<u64>), dim3(1), dim3(CL_THREADS), 0, ctx.stream, cp);
      } else {
        hipLaunchKernelGGL((claims_scatter_k<u64>), dim3(1), dim3(CL_THREADS), 0, ctx.stream, cp);
      }
      HIP_CHECK(hipGetLastError());
      ctx.prof_end(K_WITNESS_CLAIMS, ev, 8.0 * double(rows) + 16.0 * double(n_tiles));
    }
    u64 fb_h[2] = {~u64(0), 0};
    if (h_in || (keep && rows)) ctx.d2h(fb_h, fb.p, 16);  // the first host wait: nothing of the witness has been written, and the caller's matrix has been read
    if (h_in && fb_h[0] != ~u64(0))
      fail("non-canonical input value: row " + std::to_string(fb_h[0] / cc.n_inputs) + ", column " + std::to_string(fb_h[0] % cc.n_inputs));
    const size_t kept = !keep ? rows : rows ? (size_t)fb_h[1] : 0;
    if (kept > rows) fail("internal error (more kept rows than rows)");
    if (keep) new_offs = DBuf<u64>(ctx, n_base + kept + 1), new_data = DBuf<u64>(ctx, std::max<size_t>(e_base + kept * W, 1));
    std::vector<u64> h_offs(n_base + kept + 1), h_data(e_base + kept * W);
    if (n_base) HIP_CHECK(hipMemcpyAsync(new_offs.p, wit.d_claim_offsets.p, n_base * 8, hipMemcpyDeviceToDevice, ctx.stream));
    if (e_base) HIP_CHECK(hipMemcpyAsync(new_data.p, wit.d_claim_data.p, e_base * 8, hipMemcpyDeviceToDevice, ctx.stream));
    if (keep && kept) {
      hipEvent_t ev = ctx.prof_begin(K_WITNESS_CLAIMS);
      if (n_tiles > 1) {
        cp.dst = new_data.p + e_base, cp.total = nullptr;
        hipLaunchKernelGGL((claims_scatter_k<u64>), dim3((unsigned)n_tiles), dim3(CL_THREADS), 0, ctx.stream, cp);
      } else {
        HIP_CHECK(hipMemcpyAsync(new_data.p + e_base, packed.p, kept * W * 8, hipMemcpyDeviceToDevice, ctx.stream));
      }
      ctx.prof_end(K_WITNESS_CLAIMS, ev, 8.0 * double(rows) + 16.0 * double(kept) * double(W));
    }
    hipLaunchKernelGGL(claims_arith_offsets_k, dim3((unsigned)((kept + 1 + 255) / 256)), dim3(256), 0, ctx.stream, new_offs.p + n_base, (u64)e_base, (u64)W,
                       kept + 1);
    HIP_CHECK(hipGetLastError());
    std::copy(wit.claim_offsets.begin(), wit.claim_offsets.begin() + n_base, h_offs.begin());
    std::copy(wit.claim_data.begin(), wit.claim_data.begin() + e_base, h_data.begin());
    ctx.d2h_queue(h_offs.data() + n_base, new_offs.p + n_base, (kept + 1) * 8);
    ctx.d2h(h_data.data() + e_base, new_data.p + e_base, kept * W * 8);  // the second host wait: the host copy (short transcripts are hashed from it)
    // the exchange: nothing below throws
    wit.claim_offsets.swap(h_offs);
    wit.claim_data.swap(h_data);
    wit.claim_elems_total = e_base + kept * W;
    wit.d_claim_offsets = std::move(new_offs);
    wit.d_claim_data = std::move(new_data);
    summary[0] = rows, summary[1] = kept, summary[2] = pass.n_instr, summary[3] = lanes;
  } catch (...) {
    (void)hipStreamSynchronize(ctx.stream);  // what has been queued may still be reading the caller's matrix
    abandon_pending();
    throw;
  }
}

}  // namespace msamd
