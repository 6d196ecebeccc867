// Trace columns filled on the device from a program, the part that is the same text in both fields (ms_witness_fill in fill.hip,
// msbb_witness_fill in bb_fill.hip; the definition is in include/mstark.h, what differs for BabyBear in include/mstark_bb.h):
// the row interpreter, the scan kernels with their launches, and the driver. Include it from a .hip file only; everything lives
// in an unnamed namespace, so each translation unit compiles the kernels it launches for itself. The caller authors, in the
// front end, how each dependent column of one circuit follows from inputs and other columns - an ordered list of steps (dst
// column, expression) over the constraint algebra plus the witness-only nodes row / bits / inv0 / lt / xor / and - and the
// device evaluates it for every row of the witness's trace. A field describes itself by a plain traits struct F:
//   using Word, BITS, P         slot word (8 or 4 bytes, a CANONICAL value), its width for OP_BITS, the modulus for the OP_XOR fold
//   add / sub / mul / neg / inv0, row(r)   on slot words; inv0 maps 0 to 0
//   load(w) / stored(v)         a word of memory as a slot word, and back
//   struct View                 where a row's data lies: main(row, col), pre(row, col), inp(row, col) are the CELLS, by reference
//                               and as they lie in memory (so an indexed read, which chooses its source at run time, chooses
//                               among addresses and has ONE load and one F::load behind the choice), the heights
//                               n and h_in, store(row, col, v) into the trace or, after to_tmp(tmp, cols), into the temporary of
//                               a coefficient pass; inputs(p, h, w) names the ingested inputs; d_pre, the preprocessed trace
//   PEERS                       whether source 4 + k exists: then View::peer(k, row, col) reads another circuit's trace
//   one(), sc_mul, Column, rows / store / agg_get / agg_put   the scan (below): 1 and the product as the scan computes, a dst
//                               column (View::column(dst)), a thread's four maps, its four cells, a tile's aggregate
//   call, magic, accept, resolve_peers, held_before, after, ingest, init, too_high   the host side (fl_witness_fill, below)
//
// Host side (fill_compile in fill_program.h, no device needed): the blob is checked in full, then linearised into hash-consed
// instances with slots allocated by liveness, with the field's parameters (F::magic: magics, modulus, width of a value).
//
// Device side: fill_k, one thread per row. The slot file is [slot][lane] - in LDS at 256 / 128 / 64 lanes per workgroup (lane l
// touches the words slot * lanes + l: consecutive lanes, consecutive words, no bank conflict), or, when it does not fit 64 KB
// at 64 lanes, in a global scratch walked in row batches (tiers 1 and 4 of check_dev.h, by the placement rules of msamd.h).
// Rows are independent: offset-1 reads of the main trace, and reads of it at a computed row (OP_AT, "INDEXED READS"), are
// refused for every column the program assigns, so no thread reads what another one writes. An indexed read is one scattered
// load of trace, preprocessed trace or inputs, guarded by the source's height: a row from the height on loads nothing.
//
// Order on the context's stream: program upload, [wait for the producer's stream, ingest of the inputs into a temporary with
// the offender word, ONE host wait for that word], the groups in order, F::after. Every refusal comes before fill_k is launched.
//
// SCAN steps (a program of the second format): trace[0][dst] = init, trace[r+1][dst] = A(r) * trace[r][dst] + B(r). The groups
// of the program run in order on the stream: an ordinary group is one fill_k launch as above; a scan group is its COEFFICIENT
// PASS - fill_k over the roots A, B with the call's temporary as its output (A and B of every row; B alone when A is the
// constant 1: the ADDITIVE form, no multiplications) - and then the scan of the affine maps x -> a x + b, whose composition is
// associative and exact, so the parallel result equals the sequential loop bit for bit. The temporary holds the words the scan
// computes on (F::View::store writes them, F::one() is their 1) and nothing is converted inside the scan. Row r carries the
// map (A(r-1), B(r-1)), row 0 the map (1, init), rows from n on the identity, and the value before row 0 is 0. A tile is
// SC_TILE = 256 threads x 4 consecutive rows:
//   (a) scan_reduce_k   one workgroup per tile composes its rows into one aggregate: a thread composes its 4 rows, a wave scans
//                       the 64 thread aggregates with shuffles, the 4 wave aggregates are joined through LDS
//   (b) scan_starts_k   ONE workgroup turns the tile aggregates into the value in front of each tile, 256 aggregates per round
//                       with the value behind the round carried into the next
//   (c) scan_apply_k    one workgroup per tile scans its rows again from that value and stores the dst cells, each once
// and a circuit of at most one tile takes launch (c) alone. No workgroup waits for another inside a kernel: the three phases are
// ordered by the launches. What a field decides is the memory access alone: F::rows loads the maps of a thread's four rows,
// F::store writes its four cells, F::agg_get / agg_put place a tile's aggregate. With W = sizeof(Word), bytes per row and scan:
// 2 W written by the coefficient pass, 2 W read by (a), 2 W read and W written by (c) - 7 W (additive: 4 W), next to what the
// pass itself reads; (a) and (b) move 3 W / 1024 bytes per row more. Temporaries of the call: 2 W x n (W when every scan is
// additive), shared by its scans, and 3 W per tile.
#pragma once
#include <algorithm>
#include <string>

#include "fill_program.h"
#include "ingest.h"

namespace msamd {
namespace {

template <class F>
struct FlParams {
  const uint32_t* code;
  const typename F::Word* consts;
  const uint32_t* outs;
  uint32_t n_instr, n_outs;
  size_t row0, rows;
  typename F::Word* scratch;
  typename F::View v;  // (last: a peer table at its end lies 96 bytes or more into the arguments, so entry src - 4 is reached with
                       // the immediate offsets of the scalar loads, which cannot be negative)
};

template <class F, bool LDS>
__global__ __launch_bounds__(256) void fill_k(FlParams<F> p) {
  using Word = typename F::Word;
  extern __shared__ __attribute__((aligned(16))) u64 sm[];
  const u32 tid = threadIdx.x;
  const size_t t = blockIdx.x * size_t(blockDim.x) + tid;
  if (t >= p.rows) return;  // (no barrier below: every lane owns its column of the slot file)
  const size_t r = p.row0 + t, rn = r + 1 == p.v.n ? 0 : r + 1;
  Word* slots = LDS ? (reinterpret_cast<Word*>(sm) + tid) : (p.scratch + t);
  const size_t stride = LDS ? blockDim.x : p.rows;
  for (u32 pc = 0; pc < p.n_instr; pc++) {
    const uint4 ins = reinterpret_cast<const uint4*>(p.code)[pc];
    Word v;
    switch (ins.x) {
      case OP_CONST: v = p.consts[ins.z]; break;
      case OP_VAR: {
        const u32 src = ins.z & 0xff;
        const size_t row = (ins.z >> 8) ? rn : r;
        if (src == FL_SRC_MAIN)
          v = F::load(p.v.main(row, ins.w));
        else if (src == FL_SRC_PRE)
          v = F::load(p.v.pre(row, ins.w));
        else if (!F::PEERS || src == FL_SRC_INPUT)
          v = row < p.v.h_in ? F::load(p.v.inp(row, ins.w)) : 0;
        else if constexpr (F::PEERS)  // a peer, by THIS circuit's row: a row from the peer's height on loads nothing
          v = F::load(p.v.peer(src - FL_SRC_PEER, row, ins.w));
        break;
      }
      case OP_AT: {  // [row slot, source | column << 8]: the bound check is the definition, a row from the height on loads nothing
        const u64 i = slots[ins.z * stride];
        const u32 src = ins.w & 0xff, col = ins.w >> 8;
        v = 0;
        if constexpr (F::PEERS) {
          if (src >= FL_SRC_PEER) {
            v = F::load(p.v.peer(src - FL_SRC_PEER, i, col));
            break;
          }
        }
        if (i < (u64)(src == FL_SRC_INPUT ? p.v.h_in : p.v.n)) {
          const size_t row = (size_t)i;
          v = F::load(src == FL_SRC_MAIN ? p.v.main(row, col) : src == FL_SRC_PRE ? p.v.pre(row, col) : p.v.inp(row, col));  // (one load)
        }
        break;
      }
      case OP_ROW: v = F::row(r); break;
      case OP_ADD: v = F::add(slots[ins.z * stride], slots[ins.w * stride]); break;
      case OP_SUB: v = F::sub(slots[ins.z * stride], slots[ins.w * stride]); break;
      case OP_MUL: v = F::mul(slots[ins.z * stride], slots[ins.w * stride]); break;
      case OP_NEG: v = F::neg(slots[ins.z * stride]); break;
      case OP_BITS: {
        const u32 length = ins.w >> 8;
        v = (slots[ins.z * stride] >> (ins.w & 0xff)) & (length == F::BITS ? ~Word(0) : (Word(1) << length) - 1);  // <= the operand: canonical
        break;
      }
      case OP_INV0: v = F::inv0(slots[ins.z * stride]); break;
      case OP_LT: v = slots[ins.z * stride] < slots[ins.w * stride] ? 1 : 0; break;
      case OP_XOR: {
        v = slots[ins.z * stride] ^ slots[ins.w * stride];  // < 2^BITS < 2 p
        if (v >= F::P) v -= F::P;
        break;
      }
      default: v = slots[ins.z * stride] & slots[ins.w * stride]; break;  // OP_AND: <= either operand
    }
    slots[ins.y * stride] = v;
  }
  for (u32 o = 0; o < p.n_outs; o++) p.v.store(r, p.outs[2 * o], F::stored(slots[p.outs[2 * o + 1] * stride]));
}

// ---- scan steps: the affine map x -> a x + b (ADD: a = 1 throughout and is not carried)
constexpr u32 SC_THREADS = 256, SC_ROWS = 4, SC_TILE = SC_THREADS * SC_ROWS, SC_WAVES = SC_THREADS / 64;

template <class F>
struct Aff {
  typename F::Word a, b;
};

template <class F>
struct ScParams {
  typename F::Column dst;         // where the dst cells go (F::store)
  const typename F::Word* tmp;    // the coefficient pass's output (F::rows)
  typename F::Word* aggs;         // per tile: (a, b), ADD: b in aggs[t]
  typename F::Word* starts;       // per tile: the value in front of its first row (nullptr: one tile, 0)
  size_t n;
  typename F::Word init;          // as the scan computes (F::init)
  uint32_t n_tiles;
};

template <class F, bool ADD>
__device__ __forceinline__ Aff<F> sc_then(Aff<F> f, Aff<F> g) {  // f first, then g
  if (ADD) return Aff<F>{F::one(), F::add(f.b, g.b)};
  return Aff<F>{F::sc_mul(g.a, f.a), F::add(F::sc_mul(g.a, f.b), g.b)};
}
template <class F, bool ADD>
__device__ __forceinline__ typename F::Word sc_at(Aff<F> f, typename F::Word x) {
  return ADD ? F::add(x, f.b) : F::add(F::sc_mul(f.a, x), f.b);
}
__device__ __forceinline__ u64 sc_up(u64 v, u32 d) { return (u64)__shfl_up((unsigned long long)v, d, 64); }
__device__ __forceinline__ u32 sc_up(u32 v, u32 d) { return (u32)__shfl_up((unsigned)v, d, 64); }

// Every thread of the workgroup brings the map of its rows (threads in row order): excl = the maps of all earlier threads
// composed, total = those of the whole workgroup. sm: SC_WAVES entries; free again on return.
template <class F, bool ADD>
__device__ __forceinline__ void sc_block_scan(Aff<F> mine, Aff<F>& excl, Aff<F>& total, Aff<F>* sm) {
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  Aff<F> inc = mine;
  for (u32 d = 1; d < 64; d <<= 1) {
    Aff<F> prev{ADD ? F::one() : sc_up(inc.a, d), sc_up(inc.b, d)};  // (every lane takes part in the shuffle)
    if (lane >= d) inc = sc_then<F, ADD>(prev, inc);
  }
  if (lane == 63) sm[wave] = inc;
  Aff<F> pre{ADD ? F::one() : sc_up(inc.a, 1), sc_up(inc.b, 1)};
  if (lane == 0) pre = Aff<F>{F::one(), 0};
  __syncthreads();
  Aff<F> before{F::one(), 0};
  total = Aff<F>{F::one(), 0};
  for (u32 k = 0; k < SC_WAVES; k++) {
    const Aff<F> w = sm[k];
    if (k < wave) before = sc_then<F, ADD>(before, w);
    total = sc_then<F, ADD>(total, w);
  }
  excl = sc_then<F, ADD>(before, pre);
  __syncthreads();
}

template <class F, bool ADD>
__global__ __launch_bounds__(SC_THREADS) void scan_reduce_k(ScParams<F> p) {
  __shared__ Aff<F> sm[SC_WAVES];
  const size_t r0 = blockIdx.x * size_t(SC_TILE) + threadIdx.x * SC_ROWS;
  Aff<F> row[SC_ROWS];
  F::template rows<ADD>(p, r0, row);
  Aff<F> mine = row[0];
  for (u32 j = 1; j < SC_ROWS; j++) mine = sc_then<F, ADD>(mine, row[j]);
  Aff<F> excl, total;
  sc_block_scan<F, ADD>(mine, excl, total, sm);
  if (threadIdx.x == 0) {
    if (ADD)
      p.aggs[blockIdx.x] = total.b;
    else
      F::agg_put(p, blockIdx.x, total);
  }
}

template <class F, bool ADD>
__global__ __launch_bounds__(SC_THREADS) void scan_starts_k(ScParams<F> p) {  // one workgroup
  __shared__ Aff<F> sm[SC_WAVES];
  typename F::Word carry = 0;  // the value in front of the round's first tile
  for (u32 t0 = 0; t0 < p.n_tiles; t0 += SC_THREADS) {
    const u32 t = t0 + threadIdx.x;
    Aff<F> mine{F::one(), 0};
    if (t < p.n_tiles) mine = ADD ? Aff<F>{F::one(), p.aggs[t]} : F::agg_get(p, t);
    Aff<F> excl, total;
    sc_block_scan<F, ADD>(mine, excl, total, sm);
    if (t < p.n_tiles) p.starts[t] = sc_at<F, ADD>(excl, carry);
    carry = sc_at<F, ADD>(total, carry);
  }
}

template <class F, bool ADD>
__global__ __launch_bounds__(SC_THREADS) void scan_apply_k(ScParams<F> p) {
  __shared__ Aff<F> sm[SC_WAVES];
  const size_t r0 = blockIdx.x * size_t(SC_TILE) + threadIdx.x * SC_ROWS;
  Aff<F> row[SC_ROWS];
  F::template rows<ADD>(p, r0, row);
  Aff<F> mine = row[0];
  for (u32 j = 1; j < SC_ROWS; j++) mine = sc_then<F, ADD>(mine, row[j]);
  Aff<F> excl, total;
  sc_block_scan<F, ADD>(mine, excl, total, sm);
  typename F::Word x = sc_at<F, ADD>(excl, p.starts ? p.starts[blockIdx.x] : 0);
  typename F::Word cell[SC_ROWS];
  for (u32 j = 0; j < SC_ROWS; j++) cell[j] = x = sc_at<F, ADD>(row[j], x);
  F::store(p, r0, cell);
}

template <class F, bool ADD>
void scan_launch(Ctx& ctx, const ScParams<F>& p) {
  if (p.n_tiles > 1) {
    hipLaunchKernelGGL((scan_reduce_k<F, ADD>), dim3(p.n_tiles), dim3(SC_THREADS), 0, ctx.stream, p);
    hipLaunchKernelGGL((scan_starts_k<F, ADD>), dim3(1), dim3(SC_THREADS), 0, ctx.stream, p);
  }
  hipLaunchKernelGGL((scan_apply_k<F, ADD>), dim3(p.n_tiles), dim3(SC_THREADS), 0, ctx.stream, p);
}

// ---- the host side
template <class F>
unsigned fl_min_lanes(const FillCode& fc) {
  unsigned lanes = 256;
  for (const FillGroup& g : fc.groups) lanes = std::min(lanes, slot_lds_lanes(g.pass.n_slots, sizeof(typename F::Word), 0));
  return lanes;
}

template <class F>
void fl_program_info(const uint8_t* program, size_t program_len, const char* call, u64 out4[4]) {
  const FillCode fc = fill_compile(program, program_len, call, F::magic);
  out4[0] = fc.n_instr, out4[1] = fc.n_slots, out4[2] = fl_min_lanes<F>(fc), out4[3] = fc.n_assigned;
}

template <class F>
void fl_scan_info(const uint8_t* program, size_t program_len, const char* call, u64 out4[4]) {
  const FillCode fc = fill_compile(program, program_len, call, F::magic);
  size_t launches = 0;
  for (const FillGroup& g : fc.groups) launches += !g.pass.outs.empty();
  out4[0] = fc.n_scans, out4[1] = launches, out4[2] = fc.n_additive, out4[3] = SC_TILE;
}

template <class F>
[[noreturn]] void fl_fail(const std::string& what) {
  throw std::runtime_error(std::string(F::call) + ": " + what);
}

// The whole call. What the field brings (Sys / Wit: its system and witness):
//   accept(sys, wit, ci) -> View   its checks of the witness and the circuit's trace; the View of the trace, with d_pre = nullptr
//                                  when the circuit has a preprocessed trace that is not on the device at this height
//   resolve_peers(sys, wit, ci, fc, view)   the program's peer records against the system and the witness, into the View
//   held_before(sys, wit, ci), after(sys, wit, ci)   what the witness holds beside the trace: refused up front, recomputed behind
//   ingest(ctx, in, out, bad)      the inputs into the layout View::inp reads
//   init(u64)                      a scan's initial value as the scan computes; too_high(n_tiles): more tiles than a launch takes
template <class F, class Sys, class Wit>
void fl_witness_fill(Sys& sys, Wit& wit, size_t ci, const uint8_t* program, size_t program_len, const ms_dev_matrix* inputs, void* producer_stream,
                     u64 summary[4]) {
  using Word = typename F::Word;
  Ctx& ctx = *sys.ctx;
  const std::string name(F::call);
  auto fail = [&](const std::string& what) -> void { fl_fail<F>(what); };
  typename F::View view = F::accept(sys, wit, ci);
  const size_t n = view.n;
  const auto& c = sys.circuits[ci];
  const FillCode fc = fill_compile(program, program_len, name, F::magic);
  if (fc.main_w != c.main_width || fc.pre_w != c.pre_width)
    fail("the program is for main_width " + std::to_string(fc.main_w) + " and preprocessed width " + std::to_string(fc.pre_w) + ", circuit " +
         std::to_string(ci) + " has " + std::to_string(c.main_width) + " and " + std::to_string(c.pre_width));
  if (c.pre_width && !view.d_pre) fail("main trace height must equal preprocessed trace height");
  F::resolve_peers(sys, wit, ci, fc, view);
  F::held_before(sys, wit, ci);
  IngestView in;
  size_t h_in = 0;
  if (fc.n_inputs) {
    if (!inputs) fail("the program reads " + std::to_string(fc.n_inputs) + " input columns and no input matrix was given");
    if (inputs->height > n) fail("input height " + std::to_string(inputs->height) + " is above the circuit's height " + std::to_string(n));
    h_in = (size_t)inputs->height;
    if (h_in) {
      try {
        in = ingest_check(ctx, *inputs, ci, fc.n_inputs, sizeof(Word));
      } catch (const std::exception& e) {
        fail(std::string("input matrix: ") + e.what());
      }
    }
  }
  summary[0] = n, summary[1] = fc.n_steps, summary[2] = fc.n_instr, summary[3] = fl_min_lanes<F>(fc);

  // the passes of all groups in one code, one constant and one output table; where each pass starts, and its row batch
  struct Run {
    const FillGroup* g;
    size_t code0, consts0, outs0, batch;
    unsigned lanes;
  };
  std::vector<Run> runs;
  std::vector<uint32_t> code, outs;
  std::vector<Word> consts;  // (each below p: fill_compile)
  size_t scratch_words = 0;
  bool any_scan = false, all_additive = true;
  for (const FillGroup& g : fc.groups) {
    if (g.pass.outs.empty()) continue;  // no step: nothing to write
    Run r{&g, code.size(), consts.size(), outs.size(), n, slot_lds_lanes(g.pass.n_slots, sizeof(Word), 0)};
    if (!r.lanes) {
      r.batch = slot_scratch_rows(g.pass.n_slots, sizeof(Word), n);
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
  const size_t n_tiles = (n + SC_TILE - 1) / SC_TILE;
  if (any_scan && F::too_high(n_tiles)) fail("the circuit is too high for a scan step");

  // every buffer of the call before the first launch that writes: a later group reads what an earlier one wrote
  DBuf<uint32_t> d_code(ctx, code.size()), d_outs(ctx, outs.size());
  DBuf<Word> d_consts(ctx, std::max<size_t>(consts.size(), 1)), scratch, tmp, aggs, starts;
  if (scratch_words) scratch = DBuf<Word>(ctx, scratch_words);
  if (any_scan) {
    tmp = DBuf<Word>(ctx, n * (all_additive ? 1 : 2));
    if (n_tiles > 1) aggs = DBuf<Word>(ctx, 2 * n_tiles), starts = DBuf<Word>(ctx, n_tiles);
  }
  ctx.h2d(d_code.p, code.data(), code.size() * 4);
  ctx.h2d(d_outs.p, outs.data(), outs.size() * 4);
  if (!consts.empty()) ctx.h2d(d_consts.p, consts.data(), consts.size() * sizeof(Word));
  ingest_wait_for_producer(ctx, producer_stream);
  try {
    DBuf<Word> inp;
    DBuf<u64> bad;
    if (h_in) {
      inp = DBuf<Word>(ctx, h_in * fc.n_inputs);
      bad = DBuf<u64>(ctx, 1);
      HIP_CHECK(hipMemsetAsync(bad.p, 0xFF, 8, ctx.stream));
      F::ingest(ctx, in, inp.p, bad.p);
      u64 bad_h = ~u64(0);
      ctx.d2h(&bad_h, bad.p, 8);  // the one host wait: nothing has been written yet, and the caller's matrix has been read
      if (bad_h != ~u64(0))
        fail("non-canonical input value: row " + std::to_string(bad_h / fc.n_inputs) + ", column " + std::to_string(bad_h % fc.n_inputs));
    }
    view.inputs(inp.p, h_in, fc.n_inputs);
    FlParams<F> p;
    for (const Run& r : runs) {  // the groups in order; a scan group: its coefficient pass into tmp, then the scan
      const FillPass& pass = r.g->pass;
      p.v = view;
      if (r.g->scan) p.v.to_tmp(tmp.p, r.g->additive ? 1 : 2);
      p.code = d_code.p + r.code0, p.consts = d_consts.p + r.consts0, p.outs = d_outs.p + r.outs0;
      p.n_instr = (uint32_t)pass.n_instr, p.n_outs = (uint32_t)(pass.outs.size() / 2);
      p.row0 = 0, p.rows = n, p.scratch = nullptr;
      if (r.lanes) {
        hipLaunchKernelGGL((fill_k<F, true>), dim3((unsigned)((n + r.lanes - 1) / r.lanes)), dim3(r.lanes), pass.n_slots * r.lanes * sizeof(Word),
                           ctx.stream, p);
      } else {
        p.scratch = scratch.p;
        for (size_t r0 = 0; r0 < n; r0 += r.batch) {
          p.row0 = r0;
          p.rows = std::min(r.batch, n - r0);
          hipLaunchKernelGGL((fill_k<F, false>), dim3((unsigned)((p.rows + 255) / 256)), dim3(256), 0, ctx.stream, p);
        }
      }
      HIP_CHECK(hipGetLastError());
      if (!r.g->scan) continue;
      ScParams<F> sp;
      sp.dst = view.column(r.g->dst), sp.tmp = tmp.p, sp.aggs = aggs.p, sp.starts = n_tiles > 1 ? starts.p : nullptr;
      sp.n = n, sp.init = F::init(r.g->init), sp.n_tiles = (uint32_t)n_tiles;
      if (r.g->additive)
        scan_launch<F, true>(ctx, sp);
      else
        scan_launch<F, false>(ctx, sp);
      HIP_CHECK(hipGetLastError());
    }
    F::after(sys, wit, ci);
  } catch (...) {
    (void)hipStreamSynchronize(ctx.stream);  // what has been queued may still be reading the caller's matrix
    abandon_pending();
    throw;
  }
}

}  // namespace
}  // namespace msamd
