// The witness check, the part that is the same text in both fields (ms_witness_check in check.hip, msbb_witness_check in
// bb_check.hip): the row interpreters, their reduction, the choice of the slot-file form with its launches, and the decoding of
// the report. Include it from a .hip file only; everything lives in an unnamed namespace, so each translation unit compiles
// the kernels it launches for itself. A field describes itself by a plain traits struct F:
//   using Word / Ext            slot word (8 or 4 bytes, in the form the field computes in); the accumulator's extension element
//   add / sub / mul / neg       on slot words
//   struct View                 how a row sees its data: main(row, col), pre(row, col), s2_row(r) and s2(s2_row(r), col), and
//                               x(r) = w^r for the selectors
//   call, acc_words             the C entry point's name (for the error text); report words of the accumulator
//   report(word), acc_is_zero   a device counter word as the report states it; whether the lookups balance
//
// Every user constraint root of every active circuit is evaluated on the TRACE domain, row by row, and the outcome reduced to
// a report - which circuit, which row, which constraint. A row r of a circuit of height n sees main and preprocessed columns
// at row r and (r + 1) mod n, the stage-2 evaluation under the checker's (beta, gamma), the publics [beta, gamma, acc_in,
// acc_out], and the selector POLYNOMIALS of the quotient kernels at x = w^r with their limits: is_first = n at row 0 (else 0),
// is_last = n w at row n - 1 (else 0), is_transition = w^r - w^-1. (They are not the 0 / 1 flags of lookup_values_k.)
//
// The node program is a DProgram, in the slot-file forms of quotient_eval (the report's tier):
//   1  a thread per row, slots in LDS as [slot][lane] at the largest of 256 / 128 / 64 lanes whose slot file fits 64 KB behind
//      the 192-byte header;
//   2  a wave per row over the level-scheduled program (DProgram::wave_code), for short circuits (at most 16384 rows) with
//      large programs;
//   3  a thread per row at 32 lanes per workgroup with up to 160 KB of LDS (short circuits, thousands of live slots), when at
//      most 256 workgroups result;
//   4  a thread per row, slots in a global scratch, in row batches below 1 GiB.
// Reductions: a workgroup counts its failing rows per wave (ballot) and through LDS; a clean workgroup leaves there - no global
// atomic is issued for a clean trace. A failing workgroup reduces per wave (ballot), then through LDS, and issues ONE 64-bit
// atomic per touched counter: failing rows, the packed (row << 32 | constraint) minimum, and per root its count and its first
// row. The value of the first failing root is written by a second, one-row launch that reads the packed minimum from device
// memory ("pick" mode): no value ever depends on the order in which workgroups arrive.
#pragma once
#include <algorithm>
#include <cstring>
#include <string>

#include "../../include/mstark.h"
#include "msamd.h"
#include "program.h"

namespace msamd {
namespace {

constexpr u32 CK_CHUNK = 16;    // roots reduced through LDS per round of a failing workgroup
constexpr u32 CK_FIRST = 16;    // u64 index of the workgroup's packed minimum (behind 16 + 16 u32 of counts / lanes)
constexpr u32 CK_RED = 24;      // u64 words of LDS in front of the slot file (192 bytes: the slots stay 16-byte aligned)
constexpr u64 CK_NONE = ~u64(0);
constexpr u32 CK_WORDS = 8;     // device counters per circuit: failing rows, packed minimum, value, accumulator, spare

template <class F>
struct CkParams {
  typename F::View v;
  size_t n;
  const uint32_t* code;
  const typename F::Word* consts;
  const uint32_t* zero_slots;   // slot (thread per row) or position (wave per row) of each root
  uint32_t n_instr, n_zeros;
  const typename F::Word* publics;  // [beta, gamma, acc_in, acc_out], device
  typename F::Word w_inv, sel_first, sel_last;  // w^-1, n, n w
  size_t row0, rows;
  typename F::Word* scratch;
  u64* circ;                    // [0] failing rows, [1] min (row << 32 | root), [2] that root's value
  u64 *root_cnt, *root_first;   // this circuit's slices
  const u64* pick;              // non-null: evaluate row *pick >> 32 only and write root (*pick & 0xffffffff) to circ[2]
};

template <class F>
struct RowCtx {
  size_t r, rn, r_s2, rn_s2;
  typename F::Word is_first, is_last, is_trans;
};
template <class F>
__device__ __forceinline__ RowCtx<F> row_ctx(const CkParams<F>& p, size_t r) {
  RowCtx<F> c;
  c.r = r;
  c.rn = r + 1 == p.n ? 0 : r + 1;
  c.r_s2 = p.v.s2_row(c.r);
  c.rn_s2 = p.v.s2_row(c.rn);
  c.is_first = r == 0 ? p.sel_first : 0;
  c.is_last = r + 1 == p.n ? p.sel_last : 0;
  c.is_trans = F::sub(p.v.x(r), p.w_inv);
  return c;
}
template <class F>
__device__ __forceinline__ typename F::Word leaf_value(const CkParams<F>& p, const RowCtx<F>& c, const uint4 ins) {
  switch (ins.x) {
    case OP_CONST: return p.consts[ins.z];
    case OP_VAR: {
      const u32 src = ins.z & 0xff, off = ins.z >> 8;
      if (src == 1) return p.v.main(off ? c.rn : c.r, ins.w);
      if (src == 0) return p.v.pre(off ? c.rn : c.r, ins.w);
      return p.v.s2(off ? c.rn_s2 : c.r_s2, ins.w);
    }
    case OP_PUBLIC: return p.publics[ins.z];
    case OP_IS_FIRST: return c.is_first;
    case OP_IS_LAST: return c.is_last;
    case OP_IS_TRANS: return c.is_trans;
    default: return 0;
  }
}

// ---- a thread per row (tiers 1, 3, 4)
template <class F, bool LDS>
__global__ __launch_bounds__(256) void check_k(CkParams<F> p) {
  using Word = typename F::Word;
  extern __shared__ __attribute__((aligned(16))) u64 sm[];
  const u32 tid = threadIdx.x, lane = tid & 63;
  const size_t lt = blockIdx.x * size_t(blockDim.x) + tid;
  const u64 pk = p.pick ? *p.pick : 0;
  if (p.pick && pk == CK_NONE) return;  // nothing failed (the same in every lane)
  const bool active = p.pick ? lt == 0 : lt < p.rows;
  const size_t r = p.pick ? size_t(pk >> 32) : p.row0 + lt;
  Word* slots = LDS ? (reinterpret_cast<Word*>(sm + CK_RED) + tid) : (p.scratch + lt);
  const size_t stride = LDS ? blockDim.x : p.rows;

  u32 kfirst = ~0u;
  if (active) {
    const RowCtx<F> c = row_ctx(p, r);
    for (u32 pc = 0; pc < p.n_instr; pc++) {
      const uint4 ins = reinterpret_cast<const uint4*>(p.code)[pc];
      Word v;
      switch (ins.x) {
        case OP_ADD: v = F::add(slots[ins.z * stride], slots[ins.w * stride]); break;
        case OP_SUB: v = F::sub(slots[ins.z * stride], slots[ins.w * stride]); break;
        case OP_MUL: v = F::mul(slots[ins.z * stride], slots[ins.w * stride]); break;
        case OP_NEG: v = F::neg(slots[ins.z * stride]); break;
        default: v = leaf_value(p, c, ins); break;
      }
      slots[ins.y * stride] = v;
    }
    if (p.pick) {
      p.circ[2] = slots[p.zero_slots[(u32)pk] * stride];
      return;
    }
    for (u32 z = 0; z < p.n_zeros; z++)
      if (slots[p.zero_slots[z] * stride] != 0) {
        kfirst = z;
        break;
      }
  }
  if (p.pick) return;
  // failing rows of the workgroup and its packed minimum: per wave by ballot, then one LDS atomic per wave (everything in the
  // dynamic region: a static block in front of it would eat into the 64 KB the slot files are sized for)
  const bool fail = kfirst != ~0u;
  u32* cnt = reinterpret_cast<u32*>(sm);
  u32* minl = cnt + CK_CHUNK;
  unsigned long long* wg_first = reinterpret_cast<unsigned long long*>(sm + CK_FIRST);
  u32* wg_fail = reinterpret_cast<u32*>(sm + CK_FIRST + 1);
  if (tid == 0) {
    *wg_first = CK_NONE;
    *wg_fail = 0;
  }
  __syncthreads();
  {
    const unsigned long long m = __ballot(fail);
    if (m && lane == (u32)__ffsll(m) - 1) {  // the wave's smallest failing row
      atomicMin(wg_first, ((unsigned long long)r << 32) | kfirst);
      atomicAdd(wg_fail, (u32)__popcll(m));
    }
  }
  __syncthreads();
  const u32 nfail = *wg_fail;
  if (nfail == 0) return;  // a clean workgroup: no global atomic
  const size_t row_base = p.row0 + blockIdx.x * size_t(blockDim.x);
  for (u32 z0 = 0; z0 < p.n_zeros; z0 += CK_CHUNK) {
    if (tid < 2 * CK_CHUNK) cnt[tid] = tid < CK_CHUNK ? 0u : ~0u;
    __syncthreads();
    const u32 zn = min(CK_CHUNK, p.n_zeros - z0);
    for (u32 j = 0; j < zn; j++) {
      const bool nz = active && slots[p.zero_slots[z0 + j] * stride] != 0;
      const unsigned long long m = __ballot(nz);
      if (m && lane == 0) {
        atomicAdd(&cnt[j], (u32)__popcll(m));
        atomicMin(&minl[j], (tid & ~63u) + (u32)__ffsll(m) - 1);
      }
    }
    __syncthreads();
    if (tid < zn && cnt[tid]) {
      atomicAdd(reinterpret_cast<unsigned long long*>(p.root_cnt + z0 + tid), (unsigned long long)cnt[tid]);
      atomicMin(reinterpret_cast<unsigned long long*>(p.root_first + z0 + tid), (unsigned long long)(row_base + minl[tid]));
    }
    __syncthreads();
  }
  if (tid == 0) {
    atomicAdd(reinterpret_cast<unsigned long long*>(p.circ), (unsigned long long)nfail);
    atomicMin(reinterpret_cast<unsigned long long*>(p.circ + 1), *wg_first);
  }
}

// ---- a wave per row (tier 2): the walk of quotient_wave_k over DProgram::wave_code, slot = position (slot words from the
// start of the dynamic region: this form has no header)
template <class F>
__global__ __launch_bounds__(64) void check_wave_k(CkParams<F> p, const uint4* code, uint32_t n_steps, uint32_t n_leaf_steps) {
  using Word = typename F::Word;
  extern __shared__ __attribute__((aligned(16))) u64 sm[];
  Word* smw = reinterpret_cast<Word*>(sm);
  const u32 lane = threadIdx.x;
  const u64 pk = p.pick ? *p.pick : 0;
  if (p.pick && pk == CK_NONE) return;
  const size_t r = p.pick ? size_t(pk >> 32) : p.row0 + blockIdx.x;
  const RowCtx<F> c = row_ctx(p, r);
  u32 s = 0;
  for (; s < n_leaf_steps; s++) smw[s * 64 + lane] = leaf_value(p, c, code[s * 64 + lane]);
  __syncthreads();
  for (; s < n_steps; s++) {
    const uint4 ins = code[s * 64 + lane];
    Word v = 0;
    switch (ins.x) {
      case OP_ADD: v = F::add(smw[ins.z], smw[ins.w]); break;
      case OP_SUB: v = F::sub(smw[ins.z], smw[ins.w]); break;
      case OP_MUL: v = F::mul(smw[ins.z], smw[ins.w]); break;
      case OP_NEG: v = F::neg(smw[ins.z]); break;
      case 15: break;  // padding of a level
      default: v = leaf_value(p, c, ins); break;
    }
    smw[s * 64 + lane] = v;
    if (ins.y) __syncthreads();  // the last step of a level (the flag is the same in all 64 lanes)
  }
  __syncthreads();
  if (p.pick) {
    if (lane == 0) p.circ[2] = smw[p.zero_slots[(u32)pk]];
    return;
  }
  // the workgroup IS the row: each failing root costs one atomic pair per row, the row itself one
  u32 kfirst = ~0u;
  for (u32 z = lane; z < p.n_zeros; z += 64)
    if (smw[p.zero_slots[z]] != 0) {
      if (kfirst == ~0u) kfirst = z;
      atomicAdd(reinterpret_cast<unsigned long long*>(p.root_cnt + z), 1ull);
      atomicMin(reinterpret_cast<unsigned long long*>(p.root_first + z), (unsigned long long)r);
    }
  for (int off = 32; off; off >>= 1) kfirst = min(kfirst, (u32)__shfl_xor((int)kfirst, off));
  if (lane == 0 && kfirst != ~0u) {
    atomicAdd(reinterpret_cast<unsigned long long*>(p.circ), 1ull);
    atomicMin(reinterpret_cast<unsigned long long*>(p.circ + 1), ((unsigned long long)r << 32) | kfirst);
  }
}

// counters of the whole call: zeros, except the minima (all-ones); `acc` (nullable) starts at zero as well
template <class Ext>
__global__ void check_init_k(u64* circ, size_t n_circ_words, u64* root_cnt, u64* root_first, size_t n_roots, Ext* acc) {
  const size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x;
  if (i < sizeof(Ext) / 8 && acc) reinterpret_cast<u64*>(acc)[i] = 0;  // (a word per thread, as the counters are written)
  if (i < n_circ_words) circ[i] = (i % CK_WORDS == 1) ? CK_NONE : 0;
  if (i < n_roots) {
    root_cnt[i] = 0;
    root_first[i] = CK_NONE;
  }
}

size_t big_lds(const void* kernel) {  // dynamic LDS above 64 KB is opted into per kernel and device (see quotient.hip)
  const size_t want = 160 * 1024;
  if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want) == hipSuccess) return want;
  (void)hipGetLastError();
  return size_t(64) * 1024;
}

// ---- the host side
// the device counters of one call, [C x 8 per circuit | R counts | R first rows], where circuit ci owns the roots
// [root_off[ci], root_off[ci + 1]); initialised in the stream
struct CkCounters {
  std::vector<size_t> root_off;
  std::vector<u64> tiers;  // per circuit: tier | lanes << 8 (0: nothing was evaluated)
  DBuf<u64> rep;
  size_t C() const { return tiers.size(); }
  size_t R() const { return root_off.back(); }
  u64* circ(size_t ci) const { return rep.p + ci * CK_WORDS; }
  u64* cnt(size_t ci) const { return rep.p + C() * CK_WORDS + root_off[ci]; }
  u64* first(size_t ci) const { return cnt(ci) + std::max<size_t>(R(), 1); }
  template <class Ext>
  CkCounters(Ctx& ctx, std::vector<size_t> offsets, Ext* acc)
      : root_off(std::move(offsets)), tiers(root_off.size() - 1, 0), rep(ctx, C() * CK_WORDS + 2 * std::max<size_t>(R(), 1)) {
    const size_t items = std::max<size_t>(std::max(C() * CK_WORDS, R()), 1);
    hipLaunchKernelGGL(check_init_k<Ext>, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, ctx.stream, circ(0), C() * CK_WORDS, cnt(0),
                       first(0), R(), acc);
  }
};

// one circuit of height p.n: the sweep in the form its slot file allows and the one-row launch behind it; returns tier | lanes << 8.
// `p` arrives with what the field knows (view, constants, publics, selectors, counters); the program and the rows are set here.
template <class F>
u64 check_launch(Ctx& ctx, const DProgram& prog, CkParams<F> p) {
  using Word = typename F::Word;
  const size_t n = p.n, header = CK_RED * 8;
  p.code = prog.code.p;
  p.zero_slots = prog.zero_slots.p;
  p.n_instr = (uint32_t)prog.n_instr;
  p.n_zeros = (uint32_t)prog.n_zeros;
  p.row0 = 0;
  p.rows = n;
  p.scratch = nullptr;
  p.pick = nullptr;
  CkParams<F> pick = p;  // the one-row launch behind the sweep
  pick.pick = p.circ + 1;
  pick.rows = 1;
  auto lds_bytes = [&](size_t lanes) { return prog.n_slots * lanes * sizeof(Word) + header; };

  const unsigned lanes = slot_lds_lanes(prog.n_slots, sizeof(Word), header);
  if (lanes) {
    const size_t lds = lds_bytes(lanes);
    hipLaunchKernelGGL((check_k<F, true>), dim3((unsigned)((n + lanes - 1) / lanes)), dim3(lanes), lds, ctx.stream, p);
    hipLaunchKernelGGL((check_k<F, true>), dim3(1), dim3(lanes), lds, ctx.stream, pick);
    return 1 | (u64(lanes) << 8);
  }
  if (prog.wave_steps && n <= 16384 && prog.wave_steps * 64 * sizeof(Word) <= big_lds(reinterpret_cast<const void*>(&check_wave_k<F>))) {
    const uint4* code = reinterpret_cast<const uint4*>(prog.wave_code.p);
    p.zero_slots = pick.zero_slots = prog.wave_zero_pos.p;
    const size_t lds = prog.wave_steps * 64 * sizeof(Word);
    hipLaunchKernelGGL(check_wave_k<F>, dim3((unsigned)n), dim3(64), lds, ctx.stream, p, code, (uint32_t)prog.wave_steps, (uint32_t)prog.wave_leaf_steps);
    hipLaunchKernelGGL(check_wave_k<F>, dim3(1), dim3(64), lds, ctx.stream, pick, code, (uint32_t)prog.wave_steps, (uint32_t)prog.wave_leaf_steps);
    return 2 | (u64(64) << 8);
  }
  if ((n + 31) / 32 <= 256 && lds_bytes(32) <= big_lds(reinterpret_cast<const void*>(&check_k<F, true>))) {
    // one round of small workgroups over the CUs, each with its 32 lanes' slot files in up to 160 KB of LDS
    const size_t lds = lds_bytes(32);
    hipLaunchKernelGGL((check_k<F, true>), dim3((unsigned)((n + 31) / 32)), dim3(32), lds, ctx.stream, p);
    hipLaunchKernelGGL((check_k<F, true>), dim3(1), dim3(32), lds, ctx.stream, pick);
    return 3 | (u64(32) << 8);
  }
  const size_t batch = slot_scratch_rows(prog.n_slots, sizeof(Word), n);
  DBuf<Word> scratch(ctx, batch * prog.n_slots);
  p.scratch = pick.scratch = scratch.p;
  for (size_t r0 = 0; r0 < n; r0 += batch) {
    p.row0 = r0;
    p.rows = std::min(batch, n - r0);
    hipLaunchKernelGGL((check_k<F, false>), dim3((unsigned)((p.rows + 255) / 256)), dim3(256), header, ctx.stream, p);
  }
  hipLaunchKernelGGL((check_k<F, false>), dim3(1), dim3(64), header, ctx.stream, pick);
  return 4 | (u64(256) << 8);
}

// one host wait: the whole report. circuits: C x (8 + F::acc_words) words; `acc` is the running accumulator behind the last circuit
template <class F>
void check_report(Ctx& ctx, const CkCounters& k, const std::vector<size_t>& heights, const typename F::Ext* acc, uint32_t* verdict,
                  u64* circuits, u64* root_counts, u64* root_first) {
  const size_t C = k.C(), R = k.R(), A = F::acc_words;
  std::vector<u64> h(k.rep.n);
  typename F::Ext last;
  ctx.d2h_queue(h.data(), k.rep.p, h.size() * 8);
  ctx.d2h(&last, acc, sizeof(last));
  uint32_t v = 0;
  for (size_t ci = 0; ci < C; ci++) {
    const u64* d = h.data() + ci * CK_WORDS;
    u64* o = circuits + ci * (8 + A);
    const bool activec = heights[ci] != 0;
    o[0] = heights[ci];
    o[1] = d[0];
    o[2] = d[1] == CK_NONE ? CK_NONE : d[1] >> 32;
    o[3] = d[1] == CK_NONE ? CK_NONE : (d[1] & 0xffffffffu);
    o[4] = F::report(d[2]);
    for (size_t a = 0; a < A; a++) o[5 + a] = activec ? F::report(d[3 + a]) : 0;
    o[5 + A] = k.root_off[ci + 1] - k.root_off[ci];
    o[6 + A] = k.tiers[ci];
    o[7 + A] = k.root_off[ci];
    if (d[0]) v |= MS_CHECK_CONSTRAINT;
    if (d[0] && d[2] == 0) throw std::runtime_error(std::string(F::call) + ": internal error (the first failing root evaluates to zero)");
  }
  if (!F::acc_is_zero(last)) v |= MS_CHECK_LOOKUPS;
  if (root_counts) memcpy(root_counts, h.data() + C * CK_WORDS, R * 8);
  if (root_first) memcpy(root_first, h.data() + C * CK_WORDS + std::max<size_t>(R, 1), R * 8);
  *verdict = v;
}

}  // namespace
}  // namespace msamd
