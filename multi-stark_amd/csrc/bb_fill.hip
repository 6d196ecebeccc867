// Trace columns filled on the device from a program for the BabyBear configuration (msbb_witness_fill; the definition is the
// "Trace columns filled on the device" section of include/mstark.h read over p = 2^31 - 2^27 + 1, what differs is listed in
// include/mstark_bb.h). The design is fill.hip's. The host compiler is the same function (fill_compile, fill_program.h), run
// with this field's magic, modulus and 32-bit values. What differs on the device:
//   - the library's trace and BCircuit::pre are column-major Montgomery matrices with a leading dimension: a cell is
//     buf[c * ld + row], read through bb_from_monty and written once, at the end, as bb_to_monty(slot). Consecutive threads are
//     consecutive rows of one column, so every load and store of a wave is contiguous;
//   - slots are u32 and hold CANONICAL values: bits, lt, xor and and work on them as they lie, add / sub / neg are the modular
//     forms, and mul(a, b) is one bb_to_monty and one Montgomery multiplication (a R * b / R = a b). inv0 is the chain x^(p - 2)
//     on the Montgomery word, which maps 0 to 0;
//   - the slot file [slot][lane] takes 4 bytes per word: in LDS at 256 lanes up to 64 slots, 128 up to 128, 64 up to 256, and in
//     a global scratch walked in row batches beyond. No barrier: every lane owns its column of the file;
//   - inputs pass through ingest_babybear into a column-major Montgomery temporary with leading dimension h_in;
//   - an indexed read (OP_AT) of row i is buf[c * ld + i] with the source's own leading dimension, one scattered 4-byte load
//     guarded by the source's height (n, or h_in for inputs): a row from the height on loads nothing and reads 0;
//   - the witness holds no lookup values, so there is nothing beside the assigned columns to update.
//
// Order on the context's stream: program upload, [wait for the producer's stream, ingest of the inputs with the offender word,
// ONE host wait for that word], bb_fill_k. Every refusal comes before bb_fill_k is launched.
#include <algorithm>

#include "bb_host.h"
#include "fill_program.h"
#include "ingest.h"

namespace msbb {

namespace {

using namespace msamd;  // the node kinds of program.h and fill_program.h, FillCode, the ingest helpers

constexpr const char* FL_CALL = "msbb_witness_fill";

struct BflParams {
  u32* trace;            // main_w columns of leading dimension ld, Montgomery: read and written
  const u32 *pre, *inp;  // pre_w columns of leading dimension pre_ld; n_in columns of leading dimension h_in
  size_t n, h_in, ld, pre_ld;
  const uint32_t* code;
  const u32* consts;  // canonical
  const uint32_t* outs;
  uint32_t n_instr, n_outs;
  size_t row0, rows;
  u32* scratch;
};

template <bool LDS>
__global__ __launch_bounds__(256) void bb_fill_k(BflParams p) {
  extern __shared__ __attribute__((aligned(16))) u32 bfl_sm[];
  const u32 tid = threadIdx.x;
  const size_t t = blockIdx.x * size_t(blockDim.x) + tid;
  if (t >= p.rows) return;  // (no barrier below: every lane owns its column of the slot file)
  const size_t r = p.row0 + t, rn = r + 1 == p.n ? 0 : r + 1;
  u32* slots = LDS ? (bfl_sm + tid) : (p.scratch + t);
  const size_t stride = LDS ? blockDim.x : p.rows;
  for (u32 pc = 0; pc < p.n_instr; pc++) {
    const uint4 ins = reinterpret_cast<const uint4*>(p.code)[pc];
    u32 v;
    switch (ins.x) {
      case OP_CONST: v = p.consts[ins.z]; break;
      case OP_VAR: {
        const u32 src = ins.z & 0xff;
        const size_t row = (ins.z >> 8) ? rn : r;
        if (src == FL_SRC_MAIN)
          v = bb_from_monty(p.trace[ins.w * p.ld + row]);
        else if (src == FL_SRC_PRE)
          v = bb_from_monty(p.pre[ins.w * p.pre_ld + row]);
        else
          v = row < p.h_in ? bb_from_monty(p.inp[ins.w * p.h_in + row]) : 0;
        break;
      }
      case OP_AT: {  // [row slot, source | column << 8]: the bound check is the definition, a row from the height on loads nothing
        const size_t i = slots[ins.z * stride];
        const u32 src = ins.w & 0xff;
        const size_t col = ins.w >> 8;
        v = 0;
        if (i < (src == FL_SRC_INPUT ? p.h_in : p.n))
          v = bb_from_monty(src == FL_SRC_MAIN ? p.trace[col * p.ld + i] : src == FL_SRC_PRE ? p.pre[col * p.pre_ld + i] : p.inp[col * p.h_in + i]);
        break;
      }
      case OP_ROW: v = (u32)r; break;  // (heights are at most 2^27 < p)
      case OP_ADD: v = bb_add(slots[ins.z * stride], slots[ins.w * stride]); break;
      case OP_SUB: v = bb_sub(slots[ins.z * stride], slots[ins.w * stride]); break;
      case OP_MUL: v = bb_mul(bb_to_monty(slots[ins.z * stride]), slots[ins.w * stride]); break;  // a R * b / R
      case OP_NEG: v = bb_neg(slots[ins.z * stride]); break;
      case OP_BITS: {
        const u32 length = ins.w >> 8;
        v = (slots[ins.z * stride] >> (ins.w & 0xff)) & (length == 32 ? ~u32(0) : (u32(1) << length) - 1);  // <= the operand: canonical
        break;
      }
      case OP_INV0: v = bb_from_monty(bb_inv(bb_to_monty(slots[ins.z * stride]))); break;  // (the chain x^(p - 2) maps 0 to 0)
      case OP_LT: v = slots[ins.z * stride] < slots[ins.w * stride] ? 1 : 0; break;
      case OP_XOR: {
        v = slots[ins.z * stride] ^ slots[ins.w * stride];  // < 2^31 < 2 p
        if (v >= BB_P) v -= BB_P;
        break;
      }
      default: v = slots[ins.z * stride] & slots[ins.w * stride]; break;  // OP_AND: <= either operand
    }
    slots[ins.y * stride] = v;
  }
  for (u32 o = 0; o < p.n_outs; o++) p.trace[p.outs[2 * o] * p.ld + r] = bb_to_monty(slots[p.outs[2 * o + 1] * stride]);
}

}  // namespace

void fill_program_info(const uint8_t* program, size_t program_len, u64 out4[4]) {
  const FillCode fc = fill_compile(program, program_len, "msbb_fill_program_info", FILL_BABYBEAR);
  out4[0] = fc.n_instr, out4[1] = fc.n_slots, out4[2] = slot_lds_lanes(fc.n_slots, 4, 0), out4[3] = fc.n_assigned;
}

void witness_fill(BSystem& sys, BWitness& wit, size_t ci, const uint8_t* program, size_t program_len, const ms_dev_matrix* inputs,
                  void* producer_stream, u64 summary[4]) {
  Ctx& ctx = *sys.ctx;
  const std::string name(FL_CALL);
  auto fail = [&](const std::string& what) -> void { throw std::runtime_error(name + ": " + what); };
  const size_t C = sys.circuits.size();
  if (wit.sys != &sys || wit.heights.size() != C || wit.traces.size() != C) fail("the witness does not belong to this system");
  if (wit.host_resident) fail("takes a device-resident witness (msbb_witness_create, msbb_witness_create_device)");
  if (ci >= C) fail("circuit " + std::to_string(ci) + " is out of range");
  const size_t n = wit.heights[ci];
  if (!n) fail("circuit " + std::to_string(ci) + " is inactive (height 0)");
  const BCircuit& c = sys.circuits[ci];
  BMat& tr = wit.traces[ci];
  if (!tr.buf.p || tr.h != n || tr.w != c.main_width || tr.ld < n) fail("the circuit has no trace on this device");
  const FillCode fc = fill_compile(program, program_len, name, FILL_BABYBEAR);
  if (fc.main_w != c.main_width || fc.pre_w != c.pre_width)
    fail("the program is for main_width " + std::to_string(fc.main_w) + " and preprocessed width " + std::to_string(fc.pre_w) + ", circuit " +
         std::to_string(ci) + " has " + std::to_string(c.main_width) + " and " + std::to_string(c.pre_width));
  if (c.pre_width && (n != c.pre_height || !c.pre.buf.p || c.pre.h != n || c.pre.w != c.pre_width || c.pre.ld < n))
    fail("main trace height must equal preprocessed trace height");
  IngestView view;
  size_t h_in = 0;
  if (fc.n_inputs) {
    if (!inputs) fail("the program reads " + std::to_string(fc.n_inputs) + " input columns and no input matrix was given");
    if (inputs->height > n) fail("input height " + std::to_string(inputs->height) + " is above the circuit's height " + std::to_string(n));
    h_in = (size_t)inputs->height;
    if (h_in) {
      try {
        view = ingest_check(ctx, *inputs, ci, fc.n_inputs, 4);
      } catch (const std::exception& e) {
        fail(std::string("input matrix: ") + e.what());
      }
    }
  }
  const unsigned lanes = slot_lds_lanes(fc.n_slots, 4, 0);
  summary[0] = n, summary[1] = fc.n_steps, summary[2] = fc.n_instr, summary[3] = lanes;
  if (fc.outs.empty()) return;  // no step: nothing to write

  std::vector<u32> consts(fc.consts.begin(), fc.consts.end());  // (each below p: fill_compile)
  DBuf<uint32_t> d_code(ctx, fc.code.size()), d_outs(ctx, fc.outs.size());
  DBuf<u32> d_consts(ctx, std::max<size_t>(consts.size(), 1)), scratch;
  size_t batch = n;
  if (!lanes) {
    batch = slot_scratch_rows(fc.n_slots, 4, n);
    scratch = DBuf<u32>(ctx, batch * fc.n_slots);
  }
  ctx.h2d(d_code.p, fc.code.data(), fc.code.size() * 4);
  ctx.h2d(d_outs.p, fc.outs.data(), fc.outs.size() * 4);
  if (!consts.empty()) ctx.h2d(d_consts.p, consts.data(), consts.size() * 4);
  ingest_wait_for_producer(ctx, producer_stream);
  try {
    DBuf<u32> inp;
    DBuf<u64> bad;
    if (h_in) {
      inp = DBuf<u32>(ctx, h_in * fc.n_inputs);
      bad = DBuf<u64>(ctx, 1);
      HIP_CHECK(hipMemsetAsync(bad.p, 0xFF, 8, ctx.stream));
      ingest_babybear(ctx, view, inp.p, bad.p);
      u64 bad_h = ~u64(0);
      ctx.d2h(&bad_h, bad.p, 8);  // the one host wait: nothing has been written yet, and the caller's matrix has been read
      if (bad_h != ~u64(0))
        fail("non-canonical input value: row " + std::to_string(bad_h / fc.n_inputs) + ", column " + std::to_string(bad_h % fc.n_inputs));
    }
    BflParams p;
    p.trace = tr.buf.p;
    p.pre = c.pre_width ? c.pre.buf.p : nullptr;
    p.inp = inp.p;
    p.n = n, p.h_in = h_in, p.ld = tr.ld, p.pre_ld = c.pre_width ? c.pre.ld : 0;
    p.code = d_code.p, p.consts = d_consts.p, p.outs = d_outs.p;
    p.n_instr = (uint32_t)fc.n_instr, p.n_outs = (uint32_t)(fc.outs.size() / 2);
    p.row0 = 0, p.rows = n, p.scratch = nullptr;
    if (lanes) {
      hipLaunchKernelGGL(bb_fill_k<true>, dim3((unsigned)((n + lanes - 1) / lanes)), dim3(lanes), fc.n_slots * lanes * 4, ctx.stream, p);
    } else {
      p.scratch = scratch.p;
      for (size_t r0 = 0; r0 < n; r0 += batch) {
        p.row0 = r0;
        p.rows = std::min(batch, n - r0);
        hipLaunchKernelGGL(bb_fill_k<false>, dim3((unsigned)((p.rows + 255) / 256)), dim3(256), 0, ctx.stream, p);
      }
    }
    HIP_CHECK(hipGetLastError());
  } catch (...) {
    (void)hipStreamSynchronize(ctx.stream);  // what has been queued may still be reading the caller's matrix
    abandon_pending();
    throw;
  }
}

}  // namespace msbb
