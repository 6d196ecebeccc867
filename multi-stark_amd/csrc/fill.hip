// Trace columns filled on the device from a program (ms_witness_fill; the definition is in include/mstark.h): the caller
// authors, in the front end, how each dependent column of one circuit follows from inputs and other columns - an ordered list
// of steps (dst column, expression) over the constraint algebra plus the witness-only nodes row / bits / inv0 / lt / xor / and -
// and the device evaluates it for every row of the witness's row-major trace.
//
// Host side (fill_compile, no device needed): the blob is checked in full, then LINEARISED. The steps are walked in order and
// each root's nodes become INSTANCES, hash-consed on (op, operand instances, immediate). A read of a main column at offset 0 that
// an earlier step assigned resolves to that step's root instance, so no thread re-reads its own store and the value a node has
// may differ from step to step; a node that reads no main column at offset 0 keeps one instance for the whole program, the
// others are resolved again in every step that reaches them (their instances are found again by the hash-consing unless a
// column they read was assigned in between). Instances are created operands first, so their order is the instruction order;
// what no final assignment needs is dropped, and slots are allocated by liveness as build_program does for DProgram. The final
// instance of every assigned column stays live to the end, where each assigned cell is stored once.
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
#include <array>
#include <cstring>
#include <map>

#include "host.h"
#include "ingest.h"

namespace msamd {

namespace {

constexpr const char* FL_CALL = "ms_witness_fill";
constexpr u64 FL_MAGIC = 0x31304C4C49464D00ull;
constexpr uint32_t FL_NONE = ~0u;
constexpr uint32_t FL_SRC_PRE = 0, FL_SRC_MAIN = 1, FL_SRC_INPUT = 3;
constexpr size_t FL_MAX_WIDTH = size_t(1) << 20, FL_MAX_NODES = size_t(1) << 24;
enum : uint32_t { OP_ROW = 16, OP_BITS, OP_INV0, OP_LT, OP_XOR, OP_AND };  // behind the kinds of program.h

struct FillCode {  // a compiled program, on the host
  size_t main_w = 0, pre_w = 0, n_inputs = 0, n_steps = 0, n_instr = 0, n_slots = 0, n_assigned = 0;
  std::vector<uint32_t> code;  // [op, dst slot, a, b] per instruction
  std::vector<u64> consts;
  std::vector<uint32_t> outs;  // (column, slot) per assigned column
};

bool fl_unary(uint32_t k) { return k == OP_NEG || k == OP_INV0 || k == OP_BITS; }
bool fl_binary(uint32_t k) { return k == OP_ADD || k == OP_SUB || k == OP_MUL || k == OP_LT || k == OP_XOR || k == OP_AND; }

FillCode fill_compile(const uint8_t* blob, size_t len, const std::string& name) {
  auto fail = [&](const std::string& what) -> void { throw std::runtime_error(name + ": " + what); };
  if (!blob) fail("null program");
  if (len % 8 || len < 48) fail("truncated program blob (" + std::to_string(len) + " bytes)");
  const size_t nw = len / 8;
  auto rd = [&](size_t i) {
    u64 v;
    memcpy(&v, blob + 8 * i, 8);
    return v;
  };
  if (rd(0) != FL_MAGIC) fail("not a fill program (wrong magic)");
  const u64 main_w = rd(1), pre_w = rd(2), n_in = rd(3), nn = rd(4), ns = rd(5);
  if (main_w > FL_MAX_WIDTH || pre_w > FL_MAX_WIDTH || n_in > FL_MAX_WIDTH) fail("widths out of range");
  if (nn > nw / 3 || ns > nw / 2 || 6 + 3 * nn + 2 * ns != nw)
    fail("truncated program blob: " + std::to_string(nw) + " words for " + std::to_string(nn) + " nodes and " + std::to_string(ns) + " steps");
  if (nn > FL_MAX_NODES) fail("more than 2^24 nodes");
  std::vector<PNode> nodes(nn);
  for (size_t i = 0; i < nn; i++) {
    const u64 head = rd(6 + 3 * i);
    if (head >> 24) fail("node " + std::to_string(i) + ": malformed head word");
    nodes[i].kind = (uint32_t)(head & 0xff), nodes[i].source = (uint32_t)((head >> 8) & 0xff), nodes[i].offset = (uint32_t)(head >> 16);
    nodes[i].a = rd(7 + 3 * i), nodes[i].b = rd(8 + 3 * i);
  }
  std::vector<std::pair<uint32_t, uint32_t>> steps(ns);
  std::vector<char> assigned(main_w, 0);
  const size_t s0 = 6 + 3 * nn;
  for (size_t k = 0; k < ns; k++) {
    const u64 dst = rd(s0 + 2 * k), root = rd(s0 + 2 * k + 1);
    if (dst >= main_w) fail("step " + std::to_string(k) + ": dst " + std::to_string(dst) + " is out of range (main_width " + std::to_string(main_w) + ")");
    if (root >= nn) fail("step " + std::to_string(k) + ": root " + std::to_string(root) + " is out of range");
    steps[k] = {(uint32_t)dst, (uint32_t)root};
    assigned[dst] = 1;
  }
  std::vector<char> deps(nn, 0);  // reads, directly or through operands, a main column at offset 0
  for (size_t i = 0; i < nn; i++) {
    const PNode& n = nodes[i];
    const std::string at = "node " + std::to_string(i) + ": ";
    if (n.kind == OP_CONST) {
      if (n.a >= GL_P) fail(at + "non-canonical constant");
    } else if (n.kind == OP_VAR) {
      if (n.source == 2) fail(at + "stage-2 variables are not allowed in a fill program");
      if (n.source != FL_SRC_PRE && n.source != FL_SRC_MAIN && n.source != FL_SRC_INPUT) fail(at + "unknown variable source");
      const u64 width = n.source == FL_SRC_PRE ? pre_w : n.source == FL_SRC_MAIN ? main_w : n_in;
      if (n.offset > 1) fail(at + "row offset out of range");
      if (n.a >= width) fail(at + "variable " + std::to_string(n.a) + " of source " + std::to_string(n.source) + " is out of range (width " + std::to_string(width) + ")");
      if (n.source == FL_SRC_MAIN && n.offset == 1 && assigned[n.a])
        fail(at + "offset-1 read of main column " + std::to_string(n.a) + ", which the program assigns (the next row may be read only of columns no step assigns)");
      deps[i] = n.source == FL_SRC_MAIN && n.offset == 0;
    } else if (n.kind == OP_PUBLIC) {
      fail(at + "publics are not allowed in a fill program");
    } else if (n.kind == OP_IS_FIRST || n.kind == OP_IS_LAST || n.kind == OP_IS_TRANS) {
      fail(at + "selector nodes are not allowed in a fill program (they are polynomials, not flags: use row, lt and inv0)");
    } else if (n.kind == OP_ROW) {
    } else if (fl_unary(n.kind)) {
      if (n.a >= i) fail(at + "forward operand");
      if (n.kind == OP_BITS) {
        const u64 lo = n.b & 0xff, length = n.b >> 8;
        if ((n.b >> 16) || length < 1 || lo + length > 64) fail(at + "bad bits fields (need 1 <= length and lo + length <= 64)");
      }
      deps[i] = deps[n.a];
    } else if (fl_binary(n.kind)) {
      if (n.a >= i || n.b >= i) fail(at + "forward operand");
      deps[i] = deps[n.a] | deps[n.b];
    } else {
      fail(at + "unknown node kind " + std::to_string(n.kind));
    }
  }

  // ---- linearise: the steps in order, nodes -> hash-consed instances
  struct Inst {
    uint32_t op, a, b;
    u64 imm;
  };
  std::vector<Inst> insts;
  std::map<std::array<u64, 3>, uint32_t> known;
  auto intern = [&](uint32_t op, uint32_t a, uint32_t b, u64 imm) {
    const std::array<u64, 3> key{(u64)op | ((u64)a << 32), (u64)b, imm};
    auto it = known.find(key);
    if (it != known.end()) return it->second;
    if (insts.size() >= FL_MAX_NODES) fail("the linearised program exceeds 2^24 instructions");
    const uint32_t id = (uint32_t)insts.size();
    insts.push_back(Inst{op, a, b, imm});
    known.emplace(key, id);
    return id;
  };
  std::vector<uint32_t> inst_of(nn, FL_NONE), stamp(nn, FL_NONE), binding(main_w, FL_NONE), stack;
  for (size_t k = 0; k < ns; k++) {
    auto ready = [&](u64 x) { return inst_of[x] != FL_NONE && (!deps[x] || stamp[x] == (uint32_t)k); };
    stack.assign(1, steps[k].second);
    while (!stack.empty()) {
      const uint32_t i = stack.back();
      if (ready(i)) {
        stack.pop_back();
        continue;
      }
      const PNode& n = nodes[i];
      const bool un = fl_unary(n.kind), bin = fl_binary(n.kind);
      if ((un || bin) && !ready(n.a)) {
        stack.push_back((uint32_t)n.a);
        continue;
      }
      if (bin && !ready(n.b)) {
        stack.push_back((uint32_t)n.b);
        continue;
      }
      uint32_t id;
      if (n.kind == OP_CONST)
        id = intern(OP_CONST, 0, 0, n.a);
      else if (n.kind == OP_VAR)
        id = deps[i] && binding[n.a] != FL_NONE ? binding[n.a] : intern(OP_VAR, n.source | (n.offset << 8), (uint32_t)n.a, 0);
      else if (n.kind == OP_ROW)
        id = intern(OP_ROW, 0, 0, 0);
      else if (un)
        id = intern(n.kind, inst_of[n.a], n.kind == OP_BITS ? (uint32_t)n.b : 0, 0);
      else
        id = intern(n.kind, inst_of[n.a], inst_of[n.b], 0);
      inst_of[i] = id;
      stamp[i] = (uint32_t)k;
      stack.pop_back();
    }
    binding[steps[k].first] = inst_of[steps[k].second];
  }

  // ---- what the final assignments need, last uses, slots by liveness (build_program's scheme)
  const size_t NI = insts.size();
  const uint32_t INF = 0xFFFFFFFFu;
  std::vector<uint8_t> needed(NI, 0);
  std::vector<uint32_t> last_use(NI, 0), slot_of(NI, INF), free_slots;
  FillCode out;
  out.main_w = main_w, out.pre_w = pre_w, out.n_inputs = n_in, out.n_steps = ns;
  for (size_t m = 0; m < main_w; m++)
    if (binding[m] != FL_NONE) {
      needed[binding[m]] = 1;
      last_use[binding[m]] = INF;
      out.n_assigned++;
    }
  auto has_a = [](uint32_t op) { return fl_unary(op) || fl_binary(op); };
  for (size_t i = NI; i-- > 0;) {
    if (!needed[i]) continue;
    auto use = [&](uint32_t c) {
      needed[c] = 1;
      if (last_use[c] != INF && last_use[c] < i) last_use[c] = (uint32_t)i;
    };
    if (has_a(insts[i].op)) use(insts[i].a);
    if (fl_binary(insts[i].op)) use(insts[i].b);
  }
  uint32_t n_slots = 0;
  for (size_t i = 0; i < NI; i++) {
    if (!needed[i]) continue;
    const Inst& n = insts[i];
    uint32_t a = n.a, b = n.b;
    if (n.op == OP_CONST) {
      a = (uint32_t)out.consts.size();
      out.consts.push_back(n.imm);
    }
    if (has_a(n.op)) a = slot_of[n.a];
    if (fl_binary(n.op)) b = slot_of[n.b];
    // operands whose last use is this instruction free their slots (the destination may reuse them: reads precede the write)
    auto maybe_free = [&](uint32_t c) {
      if (last_use[c] == i && slot_of[c] != INF) {
        free_slots.push_back(slot_of[c]);
        slot_of[c] = INF;
      }
    };
    if (has_a(n.op)) maybe_free(n.a);
    if (fl_binary(n.op) && n.b != n.a) maybe_free(n.b);
    uint32_t dst;
    if (!free_slots.empty()) {
      dst = free_slots.back();
      free_slots.pop_back();
    } else {
      dst = n_slots++;
    }
    slot_of[i] = dst;
    out.code.insert(out.code.end(), {n.op, dst, a, b});
  }
  for (size_t m = 0; m < main_w; m++)
    if (binding[m] != FL_NONE) out.outs.insert(out.outs.end(), {(uint32_t)m, slot_of[binding[m]]});
  out.n_instr = out.code.size() / 4;
  out.n_slots = std::max<uint32_t>(n_slots, 1);
  return out;
}

// lanes per workgroup with the slot file in LDS (0: it does not fit 64 KB at 64 lanes)
unsigned fill_lds_lanes(size_t n_slots) {
  for (unsigned th = 256; th >= 64; th >>= 1)
    if (n_slots * th * 8 <= 64 * 1024) return th;
  return 0;
}

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
  const FillCode fc = fill_compile(program, program_len, "ms_fill_program_info");
  out4[0] = fc.n_instr, out4[1] = fc.n_slots, out4[2] = fill_lds_lanes(fc.n_slots), out4[3] = fc.n_assigned;
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
  const FillCode fc = fill_compile(program, program_len, name);
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
  const unsigned lanes = fill_lds_lanes(fc.n_slots);
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
