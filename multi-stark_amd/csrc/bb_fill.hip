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
// ONE host wait for that word], the groups in order. Every refusal comes before bb_fill_k is launched.
//
// SCAN steps (a program of the second format, "\0MFILB02"): trace[0][dst] = init, trace[r+1][dst] = A(r) * trace[r][dst] + B(r).
// The groups of the program run in order on the stream: an ordinary group is one bb_fill_k launch as above; a scan group is its
// COEFFICIENT PASS - bb_fill_k over the roots A, B with the call's temporary as its output: column-major with leading dimension
// n, Montgomery words, A in tmp[r], B in tmp[n + r] (B alone in tmp[r] when A is the constant 1: the ADDITIVE form, no
// multiplications) - and then the scan of the affine maps x -> a x + b over Montgomery pairs. (a, b) then (a', b') is
// (a' a, a' b + b') with bb_mul on the words as they lie: a Montgomery product of two Montgomery words is the Montgomery word of
// the product, so nothing is converted inside the scan, the composition is associative and exact, and the parallel result equals
// the sequential loop bit for bit. Row r carries the map (A(r-1), B(r-1)), row 0 the map (1, init), rows from n on the
// identity, and the value before row 0 is 0. A tile is BSC_TILE = 256 threads x 4 consecutive rows:
//   (a) bb_scan_reduce_k   one workgroup per tile composes its rows into one aggregate: a thread composes its 4 rows, a wave scans
//                          the 64 thread aggregates with __shfl_up, the 4 wave aggregates are joined through LDS
//   (b) bb_scan_starts_k   ONE workgroup turns the tile aggregates into the value in front of each tile, BSC_THREADS = 256
//                          aggregates per round with the value behind the round carried into the next
//   (c) bb_scan_apply_k    one workgroup per tile scans its rows again from that value and stores the dst cells, each once
// and a circuit of at most one tile takes launch (c) alone. No workgroup waits for another inside a kernel: the three phases are
// ordered by the launches. A thread's rows r0 .. r0 + 3 need the coefficients of rows r0 - 1 .. r0 + 2: it loads those of its
// own rows r0 .. r0 + 3, ONE 16-byte load per coefficient column where that address is 16-byte aligned and all four rows lie
// below n (4-byte loads guarded by n otherwise: the temporary is aligned and r0 a multiple of 4, so that is the tail alone), and
// takes row r0 - 1 from the lane before it (lane 0 of a wave loads it itself). The dst column of a column-major trace is
// contiguous: the four cells are one 16-byte store under the same two conditions - with ld below 4 (heights 1 and 2) or a dst
// column that starts off a 16-byte boundary, 4-byte stores. Bytes per row and scan: 8 written by the coefficient pass, 8 read
// by (a), 8 read and 4 written by (c) - 28 (additive: 4 + 4 + 4 + 4 = 16), next to what the pass itself reads; (a) and (b) move
// 12 / 1024 bytes per row more. Temporaries of the call: 8 bytes x n (4 when every scan is additive), shared by its scans, and
// 12 bytes per tile.
#include <algorithm>

#include "bb_host.h"
#include "fill_program.h"
#include "ingest.h"

namespace msbb {

namespace {

using namespace msamd;  // the node kinds of program.h and fill_program.h, FillCode, the ingest helpers

constexpr const char* FL_CALL = "msbb_witness_fill";

struct BflParams {
  const u32* trace;      // main_w columns of leading dimension ld, Montgomery: read
  u32* out;              // written, column-major with leading dimension out_ld: the trace (out_ld = ld), or the temporary of a coefficient pass (n)
  size_t out_ld;
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
  for (u32 o = 0; o < p.n_outs; o++) p.out[p.outs[2 * o] * p.out_ld + r] = bb_to_monty(slots[p.outs[2 * o + 1] * stride]);
}

// ---- scan steps: the affine map x -> a x + b over Montgomery words (ADD: a = 1 throughout and is not carried)
constexpr u32 BSC_THREADS = 256, BSC_ROWS = 4, BSC_TILE = BSC_THREADS * BSC_ROWS, BSC_WAVES = BSC_THREADS / 64;
static_assert(BSC_ROWS % 4 == 0, "a thread's rows are whole 16-byte groups");

struct BAff {
  u32 a, b;
};

struct BscParams {
  u32* dst;        // the dst column of the trace: n contiguous Montgomery words
  const u32* tmp;  // the coefficient pass's output: A in tmp[r], B in tmp[n + r]; ADD: B in tmp[r]
  u32* aggs;       // per tile: a in aggs[t], b in aggs[n_tiles + t]; ADD: b in aggs[t]
  u32* starts;     // per tile: the value in front of its first row (nullptr: one tile, 0)
  size_t n;
  u32 init;  // Montgomery
  u32 n_tiles;
};

template <bool ADD>
__device__ __forceinline__ BAff bsc_then(BAff f, BAff g) {  // f first, then g
  if (ADD) return BAff{BB_R1, bb_add(f.b, g.b)};
  return BAff{bb_mul(g.a, f.a), bb_add(bb_mul(g.a, f.b), g.b)};
}
template <bool ADD>
__device__ __forceinline__ u32 bsc_at(BAff f, u32 x) {
  return ADD ? bb_add(x, f.b) : bb_add(bb_mul(f.a, x), f.b);
}
__device__ __forceinline__ u32 bsc_up(u32 v, u32 d) { return (u32)__shfl_up((unsigned)v, d, 64); }

// One coefficient column (n words) for the rows r0 .. r0 + BSC_ROWS - 1 of a thread, r0 a multiple of 4: out[j] = col[r0 + j - 1],
// the coefficient that row r0 + j follows. The thread loads col[r0 ..] - 16 bytes at a time where the address is aligned and
// the four rows lie below n, else word by word under the guard - and col[r0 - 1] is the last word of the lane before it; lane 0
// of a wave loads it itself. A word from n on, or in front of row 0, is never used (those rows carry the identity, or init).
// Every thread of the workgroup takes part in the shuffle.
__device__ __forceinline__ void bsc_load(const u32* col, size_t n, size_t r0, u32 out[BSC_ROWS]) {
  u32 v[BSC_ROWS];
  for (u32 q = 0; q < BSC_ROWS; q += 4) {
    const u32* a = col + r0 + q;
    if (r0 + q + 4 <= n && (reinterpret_cast<uintptr_t>(a) & 15) == 0) {
      const uint4 w = *reinterpret_cast<const uint4*>(a);
      v[q] = w.x, v[q + 1] = w.y, v[q + 2] = w.z, v[q + 3] = w.w;
    } else {
      for (u32 j = 0; j < 4; j++) v[q + j] = r0 + q + j < n ? a[j] : 0;
    }
  }
  u32 prev = bsc_up(v[BSC_ROWS - 1], 1);
  if ((threadIdx.x & 63) == 0) prev = r0 > 0 && r0 - 1 < n ? col[r0 - 1] : 0;
  out[0] = prev;
  for (u32 j = 1; j < BSC_ROWS; j++) out[j] = v[j - 1];
}

// the maps of the thread's rows: (1, init) at row 0, (A(r-1), B(r-1)) behind it, the identity from row n on
template <bool ADD>
__device__ __forceinline__ void bsc_rows(const BscParams& p, size_t r0, BAff row[BSC_ROWS]) {
  u32 a[BSC_ROWS], b[BSC_ROWS];
  if (!ADD) bsc_load(p.tmp, p.n, r0, a);
  bsc_load(ADD ? p.tmp : p.tmp + p.n, p.n, r0, b);
  for (u32 j = 0; j < BSC_ROWS; j++) {
    const size_t r = r0 + j;
    row[j] = r >= p.n ? BAff{BB_R1, 0} : r == 0 ? BAff{BB_R1, p.init} : BAff{ADD ? BB_R1 : a[j], b[j]};
  }
}

// Every thread of the workgroup brings the map of its rows (threads in row order): excl = the maps of all earlier threads
// composed, total = those of the whole workgroup. sm: BSC_WAVES entries; free again on return.
template <bool ADD>
__device__ __forceinline__ void bsc_block_scan(BAff mine, BAff& excl, BAff& total, BAff* sm) {
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  BAff inc = mine;
  for (u32 d = 1; d < 64; d <<= 1) {
    BAff prev{ADD ? BB_R1 : bsc_up(inc.a, d), bsc_up(inc.b, d)};  // (every lane takes part in the shuffle)
    if (lane >= d) inc = bsc_then<ADD>(prev, inc);
  }
  if (lane == 63) sm[wave] = inc;
  BAff pre{ADD ? BB_R1 : bsc_up(inc.a, 1), bsc_up(inc.b, 1)};
  if (lane == 0) pre = BAff{BB_R1, 0};
  __syncthreads();
  BAff before{BB_R1, 0};
  total = BAff{BB_R1, 0};
  for (u32 k = 0; k < BSC_WAVES; k++) {
    const BAff w = sm[k];
    if (k < wave) before = bsc_then<ADD>(before, w);
    total = bsc_then<ADD>(total, w);
  }
  excl = bsc_then<ADD>(before, pre);
  __syncthreads();
}

template <bool ADD>
__global__ __launch_bounds__(BSC_THREADS) void bb_scan_reduce_k(BscParams p) {
  __shared__ BAff sm[BSC_WAVES];
  const size_t r0 = blockIdx.x * size_t(BSC_TILE) + threadIdx.x * BSC_ROWS;
  BAff row[BSC_ROWS];
  bsc_rows<ADD>(p, r0, row);
  BAff mine = row[0];
  for (u32 j = 1; j < BSC_ROWS; j++) mine = bsc_then<ADD>(mine, row[j]);
  BAff excl, total;
  bsc_block_scan<ADD>(mine, excl, total, sm);
  if (threadIdx.x == 0) {
    if (ADD) {
      p.aggs[blockIdx.x] = total.b;
    } else {
      p.aggs[blockIdx.x] = total.a;
      p.aggs[size_t(p.n_tiles) + blockIdx.x] = total.b;
    }
  }
}

template <bool ADD>
__global__ __launch_bounds__(BSC_THREADS) void bb_scan_starts_k(BscParams p) {  // one workgroup
  __shared__ BAff sm[BSC_WAVES];
  u32 carry = 0;  // the value in front of the round's first tile
  for (u32 t0 = 0; t0 < p.n_tiles; t0 += BSC_THREADS) {
    const u32 t = t0 + threadIdx.x;
    BAff mine{BB_R1, 0};
    if (t < p.n_tiles) mine = ADD ? BAff{BB_R1, p.aggs[t]} : BAff{p.aggs[t], p.aggs[size_t(p.n_tiles) + t]};
    BAff excl, total;
    bsc_block_scan<ADD>(mine, excl, total, sm);
    if (t < p.n_tiles) p.starts[t] = bsc_at<ADD>(excl, carry);
    carry = bsc_at<ADD>(total, carry);
  }
}

template <bool ADD>
__global__ __launch_bounds__(BSC_THREADS) void bb_scan_apply_k(BscParams p) {
  __shared__ BAff sm[BSC_WAVES];
  const size_t r0 = blockIdx.x * size_t(BSC_TILE) + threadIdx.x * BSC_ROWS;
  BAff row[BSC_ROWS];
  bsc_rows<ADD>(p, r0, row);
  BAff mine = row[0];
  for (u32 j = 1; j < BSC_ROWS; j++) mine = bsc_then<ADD>(mine, row[j]);
  BAff excl, total;
  bsc_block_scan<ADD>(mine, excl, total, sm);
  u32 x = bsc_at<ADD>(excl, p.starts ? p.starts[blockIdx.x] : 0);
  u32 cell[BSC_ROWS];
  for (u32 j = 0; j < BSC_ROWS; j++) cell[j] = x = bsc_at<ADD>(row[j], x);
  for (u32 q = 0; q < BSC_ROWS; q += 4) {
    u32* d = p.dst + r0 + q;
    if (r0 + q + 4 <= p.n && (reinterpret_cast<uintptr_t>(d) & 15) == 0) {
      *reinterpret_cast<uint4*>(d) = make_uint4(cell[q], cell[q + 1], cell[q + 2], cell[q + 3]);
    } else {
      for (u32 j = 0; j < 4; j++)
        if (r0 + q + j < p.n) d[j] = cell[q + j];
    }
  }
}

template <bool ADD>
void bsc_launch(Ctx& ctx, const BscParams& p) {
  if (p.n_tiles > 1) {
    hipLaunchKernelGGL(bb_scan_reduce_k<ADD>, dim3(p.n_tiles), dim3(BSC_THREADS), 0, ctx.stream, p);
    hipLaunchKernelGGL(bb_scan_starts_k<ADD>, dim3(1), dim3(BSC_THREADS), 0, ctx.stream, p);
  }
  hipLaunchKernelGGL(bb_scan_apply_k<ADD>, dim3(p.n_tiles), dim3(BSC_THREADS), 0, ctx.stream, p);
}

unsigned bfl_min_lanes(const FillCode& fc) {
  unsigned lanes = 256;
  for (const FillGroup& g : fc.groups) lanes = std::min(lanes, slot_lds_lanes(g.pass.n_slots, 4, 0));
  return lanes;
}

}  // namespace

void fill_program_info(const uint8_t* program, size_t program_len, u64 out4[4]) {
  const FillCode fc = fill_compile(program, program_len, "msbb_fill_program_info", FILL_BABYBEAR);
  out4[0] = fc.n_instr, out4[1] = fc.n_slots, out4[2] = bfl_min_lanes(fc), out4[3] = fc.n_assigned;
}

void fill_scan_info(const uint8_t* program, size_t program_len, u64 out4[4]) {
  const FillCode fc = fill_compile(program, program_len, "msbb_fill_scan_info", FILL_BABYBEAR);
  size_t launches = 0;
  for (const FillGroup& g : fc.groups) launches += !g.pass.outs.empty();
  out4[0] = fc.n_scans, out4[1] = launches, out4[2] = fc.n_additive, out4[3] = BSC_TILE;
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
  summary[0] = n, summary[1] = fc.n_steps, summary[2] = fc.n_instr, summary[3] = bfl_min_lanes(fc);

  // the passes of all groups in one code, one constant and one output table; where each pass starts, and its row batch
  struct Run {
    const FillGroup* g;
    size_t code0, consts0, outs0, batch;
    unsigned lanes;
  };
  std::vector<Run> runs;
  std::vector<uint32_t> code, outs;
  std::vector<u32> consts;  // (each below p: fill_compile)
  size_t scratch_words = 0;
  bool any_scan = false, all_additive = true;
  for (const FillGroup& g : fc.groups) {
    if (g.pass.outs.empty()) continue;  // no step: nothing to write
    Run r{&g, code.size(), consts.size(), outs.size(), n, slot_lds_lanes(g.pass.n_slots, 4, 0)};
    if (!r.lanes) {
      r.batch = slot_scratch_rows(g.pass.n_slots, 4, n);
      scratch_words = std::max(scratch_words, r.batch * g.pass.n_slots);
    }
    code.insert(code.end(), g.pass.code.begin(), g.pass.code.end());  // (whole instructions: every pass starts 16-byte aligned)
    consts.insert(consts.end(), g.pass.consts.begin(), g.pass.consts.end());
    outs.insert(outs.end(), g.pass.outs.begin(), g.pass.outs.end());
    any_scan |= g.scan;
    all_additive &= !g.scan || g.additive;
    runs.push_back(r);
  }
  if (runs.empty()) return;
  const size_t n_tiles = (n + BSC_TILE - 1) / BSC_TILE;  // (heights are at most 2^27: 2^17 tiles)

  // every buffer of the call before the first launch that writes: a later group reads what an earlier one wrote
  DBuf<uint32_t> d_code(ctx, code.size()), d_outs(ctx, outs.size());
  DBuf<u32> d_consts(ctx, std::max<size_t>(consts.size(), 1)), scratch, tmp, aggs, starts;
  if (scratch_words) scratch = DBuf<u32>(ctx, scratch_words);
  if (any_scan) {
    tmp = DBuf<u32>(ctx, n * (all_additive ? 1 : 2));
    if (n_tiles > 1) aggs = DBuf<u32>(ctx, 2 * n_tiles), starts = DBuf<u32>(ctx, n_tiles);
  }
  ctx.h2d(d_code.p, code.data(), code.size() * 4);
  ctx.h2d(d_outs.p, outs.data(), outs.size() * 4);
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
    for (const Run& r : runs) {  // the groups in order; a scan group: its coefficient pass into tmp, then the scan
      const FillPass& pass = r.g->pass;
      p.out = r.g->scan ? tmp.p : tr.buf.p;
      p.out_ld = r.g->scan ? n : tr.ld;
      p.code = d_code.p + r.code0, p.consts = d_consts.p + r.consts0, p.outs = d_outs.p + r.outs0;
      p.n_instr = (uint32_t)pass.n_instr, p.n_outs = (uint32_t)(pass.outs.size() / 2);
      p.row0 = 0, p.rows = n, p.scratch = nullptr;
      if (r.lanes) {
        hipLaunchKernelGGL(bb_fill_k<true>, dim3((unsigned)((n + r.lanes - 1) / r.lanes)), dim3(r.lanes), pass.n_slots * r.lanes * 4, ctx.stream, p);
      } else {
        p.scratch = scratch.p;
        for (size_t r0 = 0; r0 < n; r0 += r.batch) {
          p.row0 = r0;
          p.rows = std::min(r.batch, n - r0);
          hipLaunchKernelGGL(bb_fill_k<false>, dim3((unsigned)((p.rows + 255) / 256)), dim3(256), 0, ctx.stream, p);
        }
      }
      HIP_CHECK(hipGetLastError());
      if (!r.g->scan) continue;
      BscParams sp;
      sp.dst = tr.buf.p + size_t(r.g->dst) * tr.ld, sp.tmp = tmp.p, sp.aggs = aggs.p, sp.starts = n_tiles > 1 ? starts.p : nullptr;
      sp.n = n, sp.init = bb_to_monty((u32)r.g->init), sp.n_tiles = (u32)n_tiles;  // (init < p: fill_compile)
      if (r.g->additive)
        bsc_launch<true>(ctx, sp);
      else
        bsc_launch<false>(ctx, sp);
      HIP_CHECK(hipGetLastError());
    }
  } catch (...) {
    (void)hipStreamSynchronize(ctx.stream);  // what has been queued may still be reading the caller's matrix
    abandon_pending();
    throw;
  }
}

}  // namespace msbb
