// Trace columns filled on the device from a program (ms_witness_fill; the definition is in include/mstark.h): the caller
// authors, in the front end, how each dependent column of one circuit follows from inputs and other columns - an ordered list
// of steps (dst column, expression) over the constraint algebra plus the witness-only nodes row / bits / inv0 / lt / xor / and -
// and the device evaluates it for every row of the witness's row-major trace.
//
// Host side (fill_compile in fill_program.h, no device needed, shared with the BabyBear configuration): the blob is checked in
// full, then linearised into hash-consed instances with slots allocated by liveness; here it runs with the Goldilocks parameters
// (magic, modulus, 64-bit values).
//
// Device side: fill_k, one thread per row. The slot file is [slot][lane] - in LDS at 256 / 128 / 64 lanes per workgroup (lane l
// touches the 8-byte words slot * lanes + l: consecutive lanes, consecutive words, no bank conflict), or, when it does not fit
// 64 KB at 64 lanes, in a global scratch walked in row batches (tiers 1 and 4 of check.hip). Rows are independent: offset-1
// reads of the main trace are refused for every column the program assigns, so no thread reads what another one writes.
//
// Order on the context's stream: program upload, [wait for the producer's stream, ingest of the inputs into a row-major
// temporary with the offender word, ONE host wait for that word], fill_k, lookup_values_k when the witness holds lookup values
// for the circuit. Every refusal comes before fill_k is launched.
#include <algorithm>

#include "fill_program.h"
#include "host.h"
#include "ingest.h"

namespace msamd {

namespace {

constexpr const char* FL_CALL = "ms_witness_fill";

struct FlParams {
  u64* trace;                 // n x main_w row-major, read and written
  const u64 *pre, *inp;       // n x pre_w and h_in x n_in, row-major
  size_t n, h_in;
  uint32_t main_w, pre_w, n_in;
  const uint32_t* code;
  const u64* consts;
  const uint32_t* outs;
  uint32_t n_instr, n_outs;
  size_t row0, rows;
  u64* scratch;
};

template <bool LDS>
__global__ __launch_bounds__(256) void fill_k(FlParams p) {
  extern __shared__ __attribute__((aligned(16))) u64 sm[];
  const u32 tid = threadIdx.x;
  const size_t t = blockIdx.x * size_t(blockDim.x) + tid;
  if (t >= p.rows) return;  // (no barrier below: every lane owns its column of the slot file)
  const size_t r = p.row0 + t, rn = r + 1 == p.n ? 0 : r + 1;
  u64* slots = LDS ? (sm + tid) : (p.scratch + t);
  const size_t stride = LDS ? blockDim.x : p.rows;
  for (u32 pc = 0; pc < p.n_instr; pc++) {
    const uint4 ins = reinterpret_cast<const uint4*>(p.code)[pc];
    u64 v;
    switch (ins.x) {
      case OP_CONST: v = p.consts[ins.z]; break;
      case OP_VAR: {
        const u32 src = ins.z & 0xff;
        const size_t row = (ins.z >> 8) ? rn : r;
        if (src == FL_SRC_MAIN)
          v = p.trace[row * p.main_w + ins.w];
        else if (src == FL_SRC_PRE)
          v = p.pre[row * p.pre_w + ins.w];
        else
          v = row < p.h_in ? p.inp[row * p.n_in + ins.w] : 0;
        break;
      }
      case OP_ROW: v = (u64)r; break;
      case OP_ADD: v = gl_add(slots[ins.z * stride], slots[ins.w * stride]); break;
      case OP_SUB: v = gl_sub(slots[ins.z * stride], slots[ins.w * stride]); break;
      case OP_MUL: v = gl_mul(slots[ins.z * stride], slots[ins.w * stride]); break;
      case OP_NEG: v = gl_neg(slots[ins.z * stride]); break;
      case OP_BITS: {
        const u32 length = ins.w >> 8;
        v = (slots[ins.z * stride] >> (ins.w & 0xff)) & (length == 64 ? ~u64(0) : (u64(1) << length) - 1);  // <= the operand: canonical
        break;
      }
      case OP_INV0: v = gl_inv(slots[ins.z * stride]); break;  // (the chain x^(p - 2) maps 0 to 0)
      case OP_LT: v = slots[ins.z * stride] < slots[ins.w * stride] ? 1 : 0; break;
      case OP_XOR: {
        v = slots[ins.z * stride] ^ slots[ins.w * stride];  // < 2^64 < 2 p
        if (v >= GL_P) v -= GL_P;
        break;
      }
      default: v = slots[ins.z * stride] & slots[ins.w * stride]; break;  // OP_AND: <= either operand
    }
    slots[ins.y * stride] = v;
  }
  for (u32 o = 0; o < p.n_outs; o++) p.trace[r * p.main_w + p.outs[2 * o]] = slots[p.outs[2 * o + 1] * stride];
}

}  // namespace

void fill_program_info(const uint8_t* program, size_t program_len, u64 out4[4]) {
  const FillCode fc = fill_compile(program, program_len, "ms_fill_program_info", FILL_GOLDILOCKS);
  out4[0] = fc.n_instr, out4[1] = fc.n_slots, out4[2] = fill_lds_lanes(fc.n_slots, 8), out4[3] = fc.n_assigned;
}

void witness_fill(HSystem& sys, HWitness& wit, size_t ci, const uint8_t* program, size_t program_len, const ms_dev_matrix* inputs,
                  void* producer_stream, u64 summary[4]) {
  Ctx& ctx = *sys.ctx;
  const std::string name(FL_CALL);
  auto fail = [&](const std::string& what) -> void { throw std::runtime_error(name + ": " + what); };
  const size_t C = sys.circuits.size();
  if (wit.sys != &sys || wit.heights.size() != C) fail("the witness does not belong to this system");
  if (wit.host_resident) fail("takes a device-resident witness (ms_witness_create, ms_witness_create_device, the generators)");
  if (wit.has_remote) fail("this witness lacks traces that another rank computes");
  if (ci >= C) fail("circuit " + std::to_string(ci) + " is out of range");
  const size_t n = wit.heights[ci];
  if (!n) fail("circuit " + std::to_string(ci) + " is inactive (height 0)");
  if (!wit.traces[ci].p) fail("the circuit has no trace on this device");
  const HCircuit& c = sys.circuits[ci];
  const FillCode fc = fill_compile(program, program_len, name, FILL_GOLDILOCKS);
  if (fc.main_w != c.main_width || fc.pre_w != c.pre_width)
    fail("the program is for main_width " + std::to_string(fc.main_w) + " and preprocessed width " + std::to_string(fc.pre_w) + ", circuit " +
         std::to_string(ci) + " has " + std::to_string(c.main_width) + " and " + std::to_string(c.pre_width));
  if (c.pre_width && (n != c.pre_height || !c.d_preprocessed.p)) fail("main trace height must equal preprocessed trace height");
  DLookups& lk = wit.lookups[ci];
  const bool held = lk.mult.p != nullptr;
  if (held && (!c.prefix_on_device || c.prefix_prog.n_slots * 64 * 8 > 64 * 1024))
    fail("the witness holds lookup values for circuit " + std::to_string(ci) + " and its lookup prefix does not fit the device sweep");
  IngestView view;
  size_t h_in = 0;
  if (fc.n_inputs) {
    if (!inputs) fail("the program reads " + std::to_string(fc.n_inputs) + " input columns and no input matrix was given");
    if (inputs->height > n) fail("input height " + std::to_string(inputs->height) + " is above the circuit's height " + std::to_string(n));
    h_in = (size_t)inputs->height;
    if (h_in) {
      try {
        view = ingest_check(ctx, *inputs, ci, fc.n_inputs, 8);
      } catch (const std::exception& e) {
        fail(std::string("input matrix: ") + e.what());
      }
    }
  }
  const unsigned lanes = fill_lds_lanes(fc.n_slots, 8);
  summary[0] = n, summary[1] = fc.n_steps, summary[2] = fc.n_instr, summary[3] = lanes;
  if (fc.outs.empty()) return;  // no step: nothing to write

  DBuf<uint32_t> d_code(ctx, fc.code.size()), d_outs(ctx, fc.outs.size());
  DBuf<u64> d_consts(ctx, std::max<size_t>(fc.consts.size(), 1)), scratch;
  size_t batch = n;
  if (!lanes) {
    batch = (size_t(1) << 30) / (fc.n_slots * 8);  // the scratch stays below ~1 GiB
    batch = std::min(std::max<size_t>(256, batch & ~size_t(255)), n);
    scratch = DBuf<u64>(ctx, batch * fc.n_slots);
  }
  ctx.h2d(d_code.p, fc.code.data(), fc.code.size() * 4);
  ctx.h2d(d_outs.p, fc.outs.data(), fc.outs.size() * 4);
  if (!fc.consts.empty()) ctx.h2d(d_consts.p, fc.consts.data(), fc.consts.size() * 8);
  ingest_wait_for_producer(ctx, producer_stream);
  try {
    DBuf<u64> inp, bad;
    if (h_in) {
      inp = DBuf<u64>(ctx, h_in * fc.n_inputs);
      bad = DBuf<u64>(ctx, 1);
      HIP_CHECK(hipMemsetAsync(bad.p, 0xFF, 8, ctx.stream));
      ingest_goldilocks(ctx, view, inp.p, bad.p);
      u64 bad_h = ~u64(0);
      ctx.d2h(&bad_h, bad.p, 8);  // the one host wait: nothing has been written yet, and the caller's matrix has been read
      if (bad_h != ~u64(0))
        fail("non-canonical input value: row " + std::to_string(bad_h / fc.n_inputs) + ", column " + std::to_string(bad_h % fc.n_inputs));
    }
    FlParams p;
    p.trace = wit.traces[ci].p;
    p.pre = c.pre_width ? c.d_preprocessed.p : nullptr;
    p.inp = inp.p;
    p.n = n, p.h_in = h_in;
    p.main_w = (uint32_t)c.main_width, p.pre_w = (uint32_t)c.pre_width, p.n_in = (uint32_t)fc.n_inputs;
    p.code = d_code.p, p.consts = d_consts.p, p.outs = d_outs.p;
    p.n_instr = (uint32_t)fc.n_instr, p.n_outs = (uint32_t)(fc.outs.size() / 2);
    p.row0 = 0, p.rows = n, p.scratch = nullptr;
    if (lanes) {
      hipLaunchKernelGGL(fill_k<true>, dim3((unsigned)((n + lanes - 1) / lanes)), dim3(lanes), fc.n_slots * lanes * 8, ctx.stream, p);
    } else {
      p.scratch = scratch.p;
      for (size_t r0 = 0; r0 < n; r0 += batch) {
        p.row0 = r0;
        p.rows = std::min(batch, n - r0);
        hipLaunchKernelGGL(fill_k<false>, dim3((unsigned)((p.rows + 255) / 256)), dim3(256), 0, ctx.stream, p);
      }
    }
    HIP_CHECK(hipGetLastError());
    // SystemWitness::from_stage_1 again for the values the witness holds (checked above: the sweep fits)
    if (held && !lookup_values_device(ctx, c.prefix_prog, wit.traces[ci].p, c.pre_width ? c.d_preprocessed.p : nullptr, n, c.main_width, c.pre_width,
                                      c.args_width, lk.mult.p, lk.args.p))
      fail("internal error (the lookup prefix was found to fit and does not)");
  } catch (...) {
    (void)hipStreamSynchronize(ctx.stream);  // what has been queued may still be reading the caller's matrix
    abandon_pending();
    throw;
  }
}

}  // namespace msamd
