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
//
// A program with SCAN steps (the second format, magic "\0MFILL02" / "\0MFILB02") is cut into GROUPS: every scan step is one, every maximal run
// of ordinary steps between scans is one. The part above (fill_linearise) runs once per ordinary group and, for a scan, once as a
// COEFFICIENT PASS over its two roots (mul, add), or over the add root alone when the mul root is the constant 1: a pseudo-group
// whose outputs 0 / 1 go to a temporary instead of the trace and bind no column. A read of a column that an earlier group
// assigned is an ordinary load of the trace, which that group has finished by then.
//
// An INDEXED READ (kind 22, `at`: column c of a source at the row that another node computes) is an instance with ONE operand,
// the row, and an immediate, source | column << 8; it is hash-consed on both, so equal reads are issued once. It never resolves
// to an assignment of its group - the group rule refuses an `at` of a main column that the same or a later group assigns - and
// so it follows the group's assignments (`deps`) through its row operand alone. Its instruction word is
// [OP_AT, dst slot, row slot, source | column << 8]: a column is below 2^20, so the immediate takes 28 bits.
//
// PEER READS (the third format, magic "\0MFILL03"; Goldilocks alone so far): an eighth header word, n_peers, and behind the scan
// records n_peers records [circuit, trace, width]. Source byte 4 + k of a variable or an `at` names record k, whose width bounds
// the column. The call never writes a peer, so such a node has deps = 0, keeps one instance per pass and falls under no group
// rule; the source travels in the immediates as it stands. Apart from that the format is the second: groups, 0 scans allowed.
//
// CLAIM PROGRAMS (ms_witness_claims_fill, msbb_witness_claims_fill; magic "\0MCLAIM1", over BabyBear "\0MCLAIB1", a format of its own): W element roots and an optional keep root over
// the same nodes, no steps. claims_compile reads and checks the nodes with the functions fill_compile uses (fill_read_nodes,
// fill_check_nodes: one text and one order of refusals), without the rules of assigned columns - nothing is assigned, so every
// main column may be read at the next row or at a computed row - and with peer sources refused; it linearises ONE pass with
// bind = false, as a scan's coefficient pass is: outputs 0 .. W - 1 are the elements, output W the keep flag.
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
  uint64_t scan_magic;  // the first word of a program with scan steps; 0: this configuration has none
  uint64_t peer_magic;  // the first word of a program with peer reads (the third format); 0: this configuration has none
  uint64_t claim_magic; // the first word of a claim program (claims_compile); 0: this configuration has none
};
constexpr FillField FILL_GOLDILOCKS{0x31304C4C49464D00ull, 0xFFFFFFFF00000001ull, 64, 0x32304C4C49464D00ull, 0x33304C4C49464D00ull,
                                    0x314D49414C434D00ull};                                                 // "\0MFILL01", "\0MFILL02", "\0MFILL03", "\0MCLAIM1"
constexpr FillField FILL_BABYBEAR{0x3130424C49464D00ull, 0x78000001ull, 32, 0x3230424C49464D00ull, 0,
                                  0x314249414C434D00ull};                                                   // "\0MFILB01", "\0MFILB02", "\0MCLAIB1"

constexpr uint32_t FL_NONE = ~0u;
constexpr uint32_t FL_SRC_PRE = 0, FL_SRC_MAIN = 1, FL_SRC_INPUT = 3, FL_SRC_PEER = 4;  // source 4 + k: peer k of the program
constexpr size_t FL_MAX_PEERS = 8;
constexpr size_t FL_MAX_WIDTH = size_t(1) << 20, FL_MAX_NODES = size_t(1) << 24;
enum : uint32_t { OP_ROW = 16, OP_BITS, OP_INV0, OP_LT, OP_XOR, OP_AND, OP_AT };  // behind the kinds of program.h

struct FillPeer {  // a record of the third format: the main (trace = 1) or preprocessed (0) trace of another circuit of the witness
  uint64_t circuit, trace, width;
};
struct FillPass {  // what one launch of the fill kernel runs
  size_t n_instr = 0, n_slots = 0;
  std::vector<uint32_t> code;  // [op, dst slot, a, b] per instruction
  std::vector<uint64_t> consts;
  std::vector<uint32_t> outs;  // (column, slot) per assigned column; a coefficient pass: columns 0 (mul) and 1 (add), or 0 (add) alone
};
struct FillGroup {
  FillPass pass;                        // the ordinary steps of the group / the coefficient pass of the scan
  bool scan = false, additive = false;  // additive: the mul root is the constant 1, the temporary holds the add root alone
  uint32_t dst = 0;                     // scan: its column and first value
  uint64_t init = 0;
};
// A compiled program, on the host. n_instr is summed and n_slots the largest over the passes. `groups` holds the passes in the
// order they run; without scan steps (the first format) there is one group, and code / consts / outs are that group's too.
struct FillCode : FillPass {
  size_t main_w = 0, pre_w = 0, n_inputs = 0, n_steps = 0, n_assigned = 0, n_scans = 0, n_additive = 0;
  std::vector<FillGroup> groups;
  std::vector<FillPeer> peers;  // source 4 + k reads peers[k]; the driver resolves them against the system and the witness
};

inline bool fl_unary(uint32_t k) { return k == OP_NEG || k == OP_INV0 || k == OP_BITS; }
inline bool fl_binary(uint32_t k) { return k == OP_ADD || k == OP_SUB || k == OP_MUL || k == OP_LT || k == OP_XOR || k == OP_AND; }

// One group: `steps` (dst, root) in order -> instructions, slots, outputs. `deps`: the node reads, directly or through operands,
// a main column at offset 0. bind: a read of main column m at offset 0 sees the latest earlier step of the group that assigned
// m (an ordinary group, out_w = main_width); without it the dsts are output numbers below out_w and no read sees them (a
// coefficient pass).
template <class Fail>
inline FillPass fill_linearise(const std::vector<PNode>& nodes, const std::vector<char>& deps, const std::vector<std::pair<uint32_t, uint32_t>>& steps,
                               size_t out_w, bool bind, const Fail& fail) {
  typedef uint64_t u64;
  const size_t nn = nodes.size(), ns = steps.size();
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
  std::vector<uint32_t> inst_of(nn, FL_NONE), stamp(nn, FL_NONE), binding(out_w, FL_NONE), stack;
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
      if ((bin || n.kind == OP_AT) && !ready(n.b)) {  // (the row operand of an indexed read is its b)
        stack.push_back((uint32_t)n.b);
        continue;
      }
      uint32_t id;
      if (n.kind == OP_CONST)
        id = intern(OP_CONST, 0, 0, n.a);
      else if (n.kind == OP_VAR)
        id = bind && deps[i] && binding[n.a] != FL_NONE ? binding[n.a] : intern(OP_VAR, n.source | (n.offset << 8), (uint32_t)n.a, 0);
      else if (n.kind == OP_ROW)
        id = intern(OP_ROW, 0, 0, 0);
      else if (n.kind == OP_AT)
        id = intern(OP_AT, inst_of[n.b], n.source | ((uint32_t)n.a << 8), 0);
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
  FillPass out;
  for (size_t m = 0; m < out_w; m++)
    if (binding[m] != FL_NONE) {
      needed[binding[m]] = 1;
      last_use[binding[m]] = INF;
    }
  auto has_a = [](uint32_t op) { return fl_unary(op) || fl_binary(op) || op == OP_AT; };  // (OP_AT: a is the row instance, b the immediate)
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
  for (size_t m = 0; m < out_w; m++)
    if (binding[m] != FL_NONE) out.outs.insert(out.outs.end(), {(uint32_t)m, slot_of[binding[m]]});
  out.n_instr = out.code.size() / 4;
  out.n_slots = std::max<uint32_t>(n_slots, 1);
  return out;
}

// The n_nodes nodes of a blob, three words each from word `first` on (rd(i): word i; the caller has checked the length).
template <class Rd, class Fail>
inline std::vector<PNode> fill_read_nodes(const Rd& rd, size_t first, size_t nn, const Fail& fail) {
  std::vector<PNode> nodes(nn);
  for (size_t i = 0; i < nn; i++) {
    const uint64_t head = rd(first + 3 * i);
    if (head >> 24) fail("node " + std::to_string(i) + ": malformed head word");
    nodes[i].kind = (uint32_t)(head & 0xff), nodes[i].source = (uint32_t)((head >> 8) & 0xff), nodes[i].offset = (uint32_t)(head >> 16);
    nodes[i].a = rd(first + 1 + 3 * i), nodes[i].b = rd(first + 2 + 3 * i);
  }
  return nodes;
}

inline std::string fill_peer_name(const std::vector<FillPeer>& peers, size_t k) {
  return "peer " + std::to_string(k) + " (circuit " + std::to_string(peers[k].circuit) + ", " + (peers[k].trace ? "main" : "preprocessed") + " trace)";
}

// Every node against the widths, the field and the peer records, in node order -> deps: the node reads, directly or through
// operands, a main column at offset 0. assigned (nullable): the columns a program of ONE group assigns, which may be read
// neither at the next row nor at a computed row (the first format; the second and third apply the rule by groups, behind this).
// claims: a claim program - its name in the texts, peer sources refused, nothing assigned.
template <class Fail>
inline std::vector<char> fill_check_nodes(const std::vector<PNode>& nodes, const FillField& field, uint64_t main_w, uint64_t pre_w, uint64_t n_in,
                                          const std::vector<FillPeer>& peers, const std::vector<char>* assigned, bool claims, const Fail& fail) {
  typedef uint64_t u64;
  const size_t nn = nodes.size(), npeer = peers.size();
  const std::string program = claims ? "claim" : "fill";
  auto peer_name = [&](size_t k) { return fill_peer_name(peers, k); };
  auto known_source = [&](uint32_t s) { return s == FL_SRC_PRE || s == FL_SRC_MAIN || s == FL_SRC_INPUT || (s >= FL_SRC_PEER && s - FL_SRC_PEER < npeer); };
  auto claims_peer = [&](uint32_t s) { return claims && s >= FL_SRC_PEER && s - FL_SRC_PEER < FL_MAX_PEERS; };
  std::vector<char> deps(nn, 0);  // reads, directly or through operands, a main column at offset 0
  for (size_t i = 0; i < nn; i++) {
    const PNode& n = nodes[i];
    const std::string at = "node " + std::to_string(i) + ": ";
    if (n.kind == OP_CONST) {
      if (n.a >= field.modulus) fail(at + "non-canonical constant");
    } else if (n.kind == OP_VAR) {
      if (n.source == 2) fail(at + "stage-2 variables are not allowed in a " + program + " program");
      if (claims_peer(n.source)) fail(at + "peer reads are not allowed in a claim program (source " + std::to_string(n.source) + ")");
      if (!known_source(n.source)) fail(at + "unknown variable source");
      if (n.offset > 1) fail(at + "row offset out of range");
      if (n.source >= FL_SRC_PEER) {
        const size_t k = n.source - FL_SRC_PEER;
        if (n.a >= peers[k].width) fail(at + "variable " + std::to_string(n.a) + " of " + peer_name(k) + " is out of range (width " + std::to_string(peers[k].width) + ")");
        continue;  // (deps = 0: the call writes no peer)
      }
      const u64 width = n.source == FL_SRC_PRE ? pre_w : n.source == FL_SRC_MAIN ? main_w : n_in;
      if (n.a >= width) fail(at + "variable " + std::to_string(n.a) + " of source " + std::to_string(n.source) + " is out of range (width " + std::to_string(width) + ")");
      if (assigned && n.source == FL_SRC_MAIN && n.offset == 1 && (*assigned)[n.a])  // (the second format: by groups, in fill_compile)
        fail(at + "offset-1 read of main column " + std::to_string(n.a) + ", which the program assigns (the next row may be read only of columns no step assigns)");
      deps[i] = n.source == FL_SRC_MAIN && n.offset == 0;
    } else if (n.kind == OP_AT) {
      if (n.source == 2) fail(at + "stage-2 columns are not allowed in a " + program + " program");
      if (claims_peer(n.source)) fail(at + "peer reads are not allowed in a claim program (source " + std::to_string(n.source) + ")");
      if (!known_source(n.source)) fail(at + "unknown source of an indexed read");
      const bool peer = n.source >= FL_SRC_PEER;
      const u64 width = peer ? peers[n.source - FL_SRC_PEER].width : n.source == FL_SRC_PRE ? pre_w : n.source == FL_SRC_MAIN ? main_w : n_in;
      if (n.offset) fail(at + "the offset field of an indexed read must be 0");
      if (peer && n.a >= width)
        fail(at + "indexed read of column " + std::to_string(n.a) + " of " + peer_name(n.source - FL_SRC_PEER) + ", which is out of range (width " + std::to_string(width) + ")");
      if (n.a >= width)
        fail(at + "indexed read of column " + std::to_string(n.a) + " of source " + std::to_string(n.source) + ", which is out of range (width " + std::to_string(width) + ")");
      if (n.b >= i) fail(at + "forward row operand");
      if (assigned && n.source == FL_SRC_MAIN && (*assigned)[n.a])  // (one group; the second format: by groups, in fill_compile)
        fail(at + "indexed read of main column " + std::to_string(n.a) +
             " by step group 0, which step group 0 assigns (a computed row may be read only of columns that no step of the same or a later group assigns)");
      deps[i] = deps[n.b];
    } else if (n.kind == OP_PUBLIC) {
      fail(at + "publics are not allowed in a " + program + " program");
    } else if (n.kind == OP_IS_FIRST || n.kind == OP_IS_LAST || n.kind == OP_IS_TRANS) {
      fail(at + "selector nodes are not allowed in a " + program + " program (they are polynomials, not flags: use row, lt and inv0)");
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
  return deps;
}

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
  const bool v3 = field.peer_magic && rd(0) == field.peer_magic;  // the third format: an eighth header word, peer records behind the scans
  const bool v2 = v3 || (field.scan_magic && rd(0) == field.scan_magic);  // the second format: a seventh header word, scan records at the end
  if (rd(0) != field.magic && !v2) fail("not a fill program (wrong magic)");
  const size_t hw = v3 ? 8 : v2 ? 7 : 6;
  if (nw < hw) fail("truncated program blob (" + std::to_string(len) + " bytes)");
  const u64 main_w = rd(1), pre_w = rd(2), n_in = rd(3), nn = rd(4), ns = rd(5), nsc = v2 ? rd(6) : 0, npeer = v3 ? rd(7) : 0;
  if (main_w > FL_MAX_WIDTH || pre_w > FL_MAX_WIDTH || n_in > FL_MAX_WIDTH) fail("widths out of range");
  if (v3 && (npeer < 1 || npeer > FL_MAX_PEERS)) fail("a program of the third format declares 1 to " + std::to_string(FL_MAX_PEERS) + " peers, this one " + std::to_string(npeer));
  if (nn > nw / 3 || ns > nw / 2 || nsc > nw / 3 || hw + 3 * nn + 2 * ns + 3 * nsc + 3 * npeer != nw)
    fail("truncated program blob: " + std::to_string(nw) + " words for " + std::to_string(nn) + " nodes and " + std::to_string(ns) + " steps" +
         (v2 ? " and " + std::to_string(nsc) + " scans" : std::string()) + (v3 ? " and " + std::to_string(npeer) + " peers" : std::string()));
  if (nn > FL_MAX_NODES) fail("more than 2^24 nodes");
  const std::vector<PNode> nodes = fill_read_nodes(rd, hw, nn, fail);
  std::vector<std::pair<uint32_t, uint32_t>> steps(ns);
  std::vector<char> assigned(main_w, 0);
  const size_t s0 = hw + 3 * nn;
  for (size_t k = 0; k < ns; k++) {
    const u64 dst = rd(s0 + 2 * k), root = rd(s0 + 2 * k + 1);
    if (dst >= main_w) fail("step " + std::to_string(k) + ": dst " + std::to_string(dst) + " is out of range (main_width " + std::to_string(main_w) + ")");
    if (root >= nn) fail("step " + std::to_string(k) + ": root " + std::to_string(root) + " is out of range");
    steps[k] = {(uint32_t)dst, (uint32_t)root};
    assigned[dst] = 1;
  }
  // scan records [step index, mul root, init], step indices strictly ascending
  struct Scan {
    size_t step;
    uint32_t mul;
    u64 init;
  };
  std::vector<Scan> scans(nsc);
  const size_t c0 = s0 + 2 * ns;
  for (size_t j = 0; j < nsc; j++) {
    const u64 step = rd(c0 + 3 * j), mul = rd(c0 + 3 * j + 1), init = rd(c0 + 3 * j + 2);
    const std::string at = "scan " + std::to_string(j) + ": ";
    if (step >= ns) fail(at + "step index " + std::to_string(step) + " is out of range (" + std::to_string(ns) + " steps)");
    if (j && step <= scans[j - 1].step) fail(at + "step index " + std::to_string(step) + " is not above the one before (the records are in ascending order of steps)");
    if (mul >= nn) fail(at + "mul root " + std::to_string(mul) + " is out of range");
    if (init >= field.modulus) fail(at + "non-canonical init");
    scans[j] = Scan{(size_t)step, (uint32_t)mul, init};
  }
  // peer records [circuit, trace, width], no (circuit, trace) twice
  std::vector<FillPeer> peers(npeer);
  const size_t p0 = c0 + 3 * nsc;
  auto peer_name = [&](size_t k) { return fill_peer_name(peers, k); };
  for (size_t k = 0; k < npeer; k++) {
    peers[k] = FillPeer{rd(p0 + 3 * k), rd(p0 + 3 * k + 1), rd(p0 + 3 * k + 2)};
    const std::string at = "peer " + std::to_string(k) + ": ";
    if (peers[k].trace > 1) fail(at + "trace " + std::to_string(peers[k].trace) + " (0: preprocessed, 1: main)");
    if (peers[k].width > FL_MAX_WIDTH) fail(at + "width " + std::to_string(peers[k].width) + " is out of range");
    if (peers[k].circuit >> 32) fail(at + "circuit " + std::to_string(peers[k].circuit) + " is out of range");
    for (size_t j = 0; j < k; j++)
      if (peers[j].circuit == peers[k].circuit && peers[j].trace == peers[k].trace) fail(at + "the same circuit and trace as peer " + std::to_string(j) + " (" + peer_name(j) + ")");
  }
  const std::vector<char> deps = fill_check_nodes(nodes, field, main_w, pre_w, n_in, peers, v2 ? nullptr : &assigned, false, fail);

  FillCode out;
  out.main_w = main_w, out.pre_w = pre_w, out.n_inputs = n_in, out.n_steps = ns, out.n_scans = nsc;
  out.peers = peers;
  for (size_t m = 0; m < main_w; m++) out.n_assigned += assigned[m];
  typedef std::vector<std::pair<uint32_t, uint32_t>> Steps;
  if (!v2) {
    out.groups.resize(1);
    out.groups[0].pass = fill_linearise(nodes, deps, steps, main_w, true, fail);
    static_cast<FillPass&>(out) = out.groups[0].pass;
    return out;
  }

  // ---- the second and the third format: groups in order, [first step, last step) with the scan record of a scan group
  struct Range {
    size_t lo, hi;
    const Scan* scan;
  };
  std::vector<Range> ranges;
  size_t at_step = 0;
  for (const Scan& sc : scans) {
    if (sc.step > at_step) ranges.push_back(Range{at_step, sc.step, nullptr});
    ranges.push_back(Range{sc.step, sc.step + 1, &sc});
    at_step = sc.step + 1;
  }
  if (ns > at_step) ranges.push_back(Range{at_step, (size_t)ns, nullptr});
  // the offset-1 rule: group g may read the next row of main column m, or m at a computed row, only if no step of group g or of
  // a later group assigns m
  const uint32_t NG = (uint32_t)ranges.size();
  std::vector<uint32_t> last_group(main_w, FL_NONE);  // the last group that assigns the column
  for (uint32_t g = 0; g < NG; g++)
    for (size_t k = ranges[g].lo; k < ranges[g].hi; k++) last_group[steps[k].first] = g;
  std::vector<uint32_t> seen(nn, FL_NONE), stack;
  for (uint32_t g = 0; g < NG; g++) {
    const Range& rg = ranges[g];
    for (size_t k = rg.lo; k < rg.hi; k++) stack.push_back(steps[k].second);
    if (rg.scan) stack.push_back(rg.scan->mul);
    while (!stack.empty()) {
      const uint32_t i = stack.back();
      stack.pop_back();
      if (seen[i] == g) continue;
      seen[i] = g;
      const PNode& n = nodes[i];
      if (fl_unary(n.kind) || fl_binary(n.kind)) stack.push_back((uint32_t)n.a);
      if (fl_binary(n.kind) || n.kind == OP_AT) stack.push_back((uint32_t)n.b);
      if (n.kind == OP_AT && n.source == FL_SRC_MAIN && last_group[n.a] != FL_NONE && last_group[n.a] >= g)  // (a scan's own dst is such a column)
        fail("node " + std::to_string(i) + ": indexed read of main column " + std::to_string(n.a) + " by step group " + std::to_string(g) +
             ", which step group " + std::to_string(last_group[n.a]) + " assigns (a computed row may be read only of columns that no step of the same or a later group assigns)");
      if (n.kind != OP_VAR || n.source != FL_SRC_MAIN) continue;
      if (rg.scan && n.a == steps[rg.lo].first)
        fail("step " + std::to_string(rg.lo) + ": the coefficients of a scan step read its own dst, main column " + std::to_string(n.a) + " at offset " +
             std::to_string(n.offset) + " (node " + std::to_string(i) + "; the previous row's value enters through the recurrence alone)");
      if (n.offset == 1 && last_group[n.a] != FL_NONE && last_group[n.a] >= g)
        fail("node " + std::to_string(i) + ": offset-1 read of main column " + std::to_string(n.a) + " by step group " + std::to_string(g) +
             ", which step group " + std::to_string(last_group[n.a]) + " assigns (the next row may be read only of columns that no step of the same or a later group assigns)");
    }
  }
  for (const Range& rg : ranges) {
    FillGroup gr;
    if (!rg.scan) {
      gr.pass = fill_linearise(nodes, deps, Steps(steps.begin() + rg.lo, steps.begin() + rg.hi), main_w, true, fail);
    } else {
      const uint32_t mul = rg.scan->mul, add = steps[rg.lo].second;
      gr.scan = true, gr.dst = steps[rg.lo].first, gr.init = rg.scan->init;
      gr.additive = nodes[mul].kind == OP_CONST && nodes[mul].a == 1;
      gr.pass = gr.additive ? fill_linearise(nodes, deps, Steps{{0, add}}, 1, false, fail) : fill_linearise(nodes, deps, Steps{{0, mul}, {1, add}}, 2, false, fail);
      out.n_additive += gr.additive;
    }
    out.n_instr += gr.pass.n_instr;
    out.n_slots = std::max(out.n_slots, gr.pass.n_slots);
    out.groups.push_back(std::move(gr));
  }
  out.n_slots = std::max<size_t>(out.n_slots, 1);
  return out;
}

// ---- claim programs
constexpr size_t CL_MAX_WIDTH = size_t(1) << 16;  // elements of one claim
struct ClaimCode {
  FillPass pass;  // outs: (e, slot) for the elements e = 0 .. W - 1 and, with a keep root, (W, slot of the keep flag)
  size_t main_w = 0, pre_w = 0, n_inputs = 0, width = 0;
  bool has_keep = false;
};

// [magic, main_width, pre_width, n_inputs, n_nodes, W, keep root (all ones: none)], the nodes, the W element roots.
inline ClaimCode claims_compile(const uint8_t* blob, size_t len, const std::string& name, const FillField& field) {
  typedef uint64_t u64;
  auto fail = [&](const std::string& what) -> void { throw std::runtime_error(name + ": " + what); };
  if (!field.claim_magic) fail("this configuration has no claim programs");
  if (!blob) fail("null program");
  const size_t hw = 7;
  if (len % 8 || len < 8 * hw) fail("truncated program blob (" + std::to_string(len) + " bytes)");
  const size_t nw = len / 8;
  auto rd = [&](size_t i) {
    u64 v;
    memcpy(&v, blob + 8 * i, 8);
    return v;
  };
  if (rd(0) == field.magic || (field.scan_magic && rd(0) == field.scan_magic) || (field.peer_magic && rd(0) == field.peer_magic))
    fail("a fill program, not a claim program (a claim program assigns nothing, has no scan steps and reads no peer; its magic is another)");
  if (rd(0) != field.claim_magic) fail("not a claim program (wrong magic)");
  const u64 main_w = rd(1), pre_w = rd(2), n_in = rd(3), nn = rd(4), W = rd(5), keep = rd(6);
  if (main_w > FL_MAX_WIDTH || pre_w > FL_MAX_WIDTH || n_in > FL_MAX_WIDTH) fail("widths out of range");
  if (W < 1 || W > CL_MAX_WIDTH) fail("a claim has 1 to 2^16 elements, this program " + std::to_string(W));
  if (nn > nw / 3 || hw + 3 * nn + W != nw)
    fail("truncated program blob: " + std::to_string(nw) + " words for " + std::to_string(nn) + " nodes and " + std::to_string(W) + " elements");
  if (nn > FL_MAX_NODES) fail("more than 2^24 nodes");
  const std::vector<PNode> nodes = fill_read_nodes(rd, hw, nn, fail);
  std::vector<std::pair<uint32_t, uint32_t>> outs(W);
  const size_t e0 = hw + 3 * nn;
  for (size_t e = 0; e < W; e++) {
    const u64 root = rd(e0 + e);
    if (root >= nn) fail("element " + std::to_string(e) + ": root " + std::to_string(root) + " is out of range");
    outs[e] = {(uint32_t)e, (uint32_t)root};
  }
  const bool has_keep = keep != ~u64(0);
  if (has_keep) {
    if (keep >= nn) fail("keep: root " + std::to_string(keep) + " is out of range");
    outs.push_back({(uint32_t)W, (uint32_t)keep});
  }
  fill_check_nodes(nodes, field, main_w, pre_w, n_in, std::vector<FillPeer>(), nullptr, true, fail);
  ClaimCode out;
  out.main_w = main_w, out.pre_w = pre_w, out.n_inputs = n_in, out.width = W, out.has_keep = has_keep;
  // nothing is assigned, so no node's value changes from output to output: deps = 0 throughout, each node is one instance
  out.pass = fill_linearise(nodes, std::vector<char>(nn, 0), outs, W + has_keep, false, fail);
  return out;
}

}  // namespace msamd
