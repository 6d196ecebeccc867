// The host compiler of fill programs (ms_witness_fill / msbb_witness_fill; the definition is in include/mstark.h): the blob is
// checked in full, then LINEARISED. Host code over the blob alone, so both configurations run this one function; what a field
// decides - the magic word, the modulus a constant must stay below, the width of a value that bits may address - comes in
// through FillField. fill.hip (Goldilocks) and bb_fill.hip (BabyBear) hold the kernels that run a FillCode.
//
// The steps are walked in order and each root's nodes become INSTANCES, hash-consed on (op, operand instances, immediate). A read
// of a main column at offset 0 that an earlier step assigned resolves to that step's root instance, so no thread re-reads its own
// store and the value a node has may differ from step to step; a node that reads no main column at offset 0 keeps one instance for
// the whole program, the others are resolved again in every step that reaches them (their instances are found again by the
// hash-consing unless a column they read was assigned in between). Instances are created operands first, so their order is the
// instruction order; what no final assignment needs is dropped, and slots are allocated by liveness as build_program does for
// DProgram. The final instance of every assigned column stays live to the end, where each assigned cell is stored once.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "program.h"

namespace msamd {

struct FillField {
  uint64_t magic;       // the blob's first word: a program is authored over one field (its constants are folded modulo it)
  uint64_t modulus;     // constants are canonical: below this
  unsigned value_bits;  // bits(x, lo, length) needs lo + length <= value_bits
};
constexpr FillField FILL_GOLDILOCKS{0x31304C4C49464D00ull, 0xFFFFFFFF00000001ull, 64};  // "\0MFILL01"
constexpr FillField FILL_BABYBEAR{0x3130424C49464D00ull, 0x78000001ull, 32};            // "\0MFILB01"

constexpr uint32_t FL_NONE = ~0u;
constexpr uint32_t FL_SRC_PRE = 0, FL_SRC_MAIN = 1, FL_SRC_INPUT = 3;
constexpr size_t FL_MAX_WIDTH = size_t(1) << 20, FL_MAX_NODES = size_t(1) << 24;
enum : uint32_t { OP_ROW = 16, OP_BITS, OP_INV0, OP_LT, OP_XOR, OP_AND };  // behind the kinds of program.h

struct FillCode {  // a compiled program, on the host
  size_t main_w = 0, pre_w = 0, n_inputs = 0, n_steps = 0, n_instr = 0, n_slots = 0, n_assigned = 0;
  std::vector<uint32_t> code;  // [op, dst slot, a, b] per instruction
  std::vector<uint64_t> consts;
  std::vector<uint32_t> outs;  // (column, slot) per assigned column
};

inline bool fl_unary(uint32_t k) { return k == OP_NEG || k == OP_INV0 || k == OP_BITS; }
inline bool fl_binary(uint32_t k) { return k == OP_ADD || k == OP_SUB || k == OP_MUL || k == OP_LT || k == OP_XOR || k == OP_AND; }

inline FillCode fill_compile(const uint8_t* blob, size_t len, const std::string& name, const FillField& field) {
  typedef uint64_t u64;
  auto fail = [&](const std::string& what) -> void { throw std::runtime_error(name + ": " + what); };
  if (!blob) fail("null program");
  if (len % 8 || len < 48) fail("truncated program blob (" + std::to_string(len) + " bytes)");
  const size_t nw = len / 8;
  auto rd = [&](size_t i) {
    u64 v;
    memcpy(&v, blob + 8 * i, 8);
    return v;
  };
  if (rd(0) != field.magic) fail("not a fill program (wrong magic)");
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
      if (n.a >= field.modulus) fail(at + "non-canonical constant");
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
        if ((n.b >> 16) || length < 1 || lo + length > field.value_bits)
          fail(at + "bad bits fields (need 1 <= length and lo + length <= " + std::to_string(field.value_bits) + ")");
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

// lanes per workgroup with the slot file in LDS (0: it does not fit 64 KB at 64 lanes); slot_bytes 8 / 4
inline unsigned fill_lds_lanes(size_t n_slots, size_t slot_bytes) {
  for (unsigned th = 256; th >= 64; th >>= 1)
    if (n_slots * th * slot_bytes <= 64 * 1024) return th;
  return 0;
}

}  // namespace msamd
