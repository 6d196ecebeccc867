// Witness check of the BabyBear / Poseidon2 configuration (msbb_witness_check): check.hip read over BabyBear. Every user
// constraint root of every active circuit evaluated on the TRACE domain, row by row, and the outcome reduced to a report -
// which circuit, which row, which constraint.
//
// A row r of a circuit of height n sees what quotient_k (bb_kernels.hip) sees at x = w^r, w = bb_two_adic_generator(log n): main
// and preprocessed columns at row r and (r + 1) mod n, the stage-2 evaluation bb_stage2 builds under the checker's (beta,
// gamma) - four base coordinates per lookup, natural row order - the 16 public coordinates [beta, gamma, acc_in, acc_out], and
// the selector POLYNOMIALS at x = w^r with their limits: is_first = n at row 0 (else 0), is_last = n w at row n - 1 (else 0),
// is_transition = w^r - w^-1.
//
// The program is NOT the prover's BProgram (one slot per node in a global scratch) but the node vector lowered by
// msamd::build_program over the user roots alone: slot-allocated code, the wave schedule, constants as a Montgomery table. It is
// built on the first check of a circuit (BCheckProgram). Every matrix here is COLUMN-major (bb.h): adjacent lanes read adjacent
// rows of a column, so main, preprocessed and stage-2 reads are coalesced as they stand and nothing is staged through LDS.
// Slots are 4-byte Montgomery words; the four slot-file regimes of check.hip, re-derived for them (header: 192 bytes):
//   1  a thread per row, slots in LDS as [slot][lane]: 256 lanes up to 63 slots, 128 up to 127, 64 up to 255;
//   2  a wave per row over DProgram::wave_code (programs with a wave schedule, at most 16384 rows);
//   3  a thread per row at 32 lanes per workgroup with up to 160 KB of LDS (up to 1278 slots; 510 where only 64 KB can be had),
//      when at most 256 workgroups result;
//   4  a thread per row, slots in a global scratch, in row batches below 1 GiB.
// Reductions are those of check.hip: a workgroup counts its failing rows per wave (ballot) and through LDS; a clean workgroup
// leaves there - no global atomic. A failing workgroup issues ONE 64-bit atomic per touched counter: failing rows, the packed
// (row << 32 | root) minimum, and per root its count and its first row. The value of the first failing root is written by a
// second, one-row launch that reads the packed minimum from device memory ("pick"): nothing depends on arrival order.
#include <algorithm>
#include <cstring>

#include "../../include/mstark_bb.h"
#include "bb_host.h"

namespace msbb {

namespace {

using msamd::OP_ADD;
using msamd::OP_CONST;
using msamd::OP_IS_FIRST;
using msamd::OP_IS_LAST;
using msamd::OP_IS_TRANS;
using msamd::OP_MUL;
using msamd::OP_NEG;
using msamd::OP_PUBLIC;
using msamd::OP_SUB;
using msamd::OP_VAR;

constexpr u32 CK_CHUNK = 16;  // roots reduced through LDS per round of a failing workgroup
constexpr u32 CK_FIRST = 16;  // u64 index of the workgroup's packed minimum (behind 16 + 16 u32 of counts / lanes)
constexpr u32 CK_RED = 24;    // u64 words of LDS in front of the slot file (192 bytes)
constexpr u64 CK_NONE = ~u64(0);
constexpr u32 CK_WORDS = 8;   // device counters per circuit: failing rows, packed minimum, value, accumulator (4), spare

struct CkParams {
  const u32 *trace, *pre, *s2;  // column-major, Montgomery, natural row order
  size_t trace_ld, pre_ld, s2_ld;
  size_t n;
  const uint32_t* code;
  const u32* consts;
  const uint32_t* zero_slots;  // slot (thread per row) or position (wave per row) of each root
  uint32_t n_instr, n_zeros;
  const u32* publics;               // 16 words, device
  u32 w, w_inv, sel_first, sel_last;  // generator of the trace domain, w^-1, n, n w
  size_t row0, rows;
  u32* scratch;
  u64* circ;                   // [0] failing rows, [1] min (row << 32 | root), [2] that root's value (Montgomery word)
  u64 *root_cnt, *root_first;  // this circuit's slices
  const u64* pick;             // non-null: evaluate row *pick >> 32 only and write root (*pick & 0xffffffff) to circ[2]
};

struct RowCtx {
  size_t r, rn;
  u32 is_first, is_last, is_trans;
};
__device__ __forceinline__ RowCtx row_ctx(const CkParams& p, size_t r) {
  RowCtx c;
  c.r = r;
  c.rn = r + 1 == p.n ? 0 : r + 1;
  c.is_first = r == 0 ? p.sel_first : 0;
  c.is_last = r + 1 == p.n ? p.sel_last : 0;
  c.is_trans = bb_sub(bb_pow(p.w, r), p.w_inv);  // (the sweep is bound by memory and LDS, not by these ~2 log n products)
  return c;
}
__device__ __forceinline__ u32 leaf_value(const CkParams& p, const RowCtx& c, const uint4 ins) {
  switch (ins.x) {
    case OP_CONST: return p.consts[ins.z];
    case OP_VAR: {
      const u32 src = ins.z & 0xff, off = ins.z >> 8;
      const size_t row = off ? c.rn : c.r;
      if (src == 1) return p.trace[size_t(ins.w) * p.trace_ld + row];
      if (src == 0) return p.pre[size_t(ins.w) * p.pre_ld + row];
      return p.s2[size_t(ins.w) * p.s2_ld + row];
    }
    case OP_PUBLIC: return p.publics[ins.z];
    case OP_IS_FIRST: return c.is_first;
    case OP_IS_LAST: return c.is_last;
    case OP_IS_TRANS: return c.is_trans;
    default: return 0;
  }
}

// ---- a thread per row (forms 1, 3, 4)
template <bool LDS>
__global__ __launch_bounds__(256) void bb_check_k(CkParams p) {
  extern __shared__ __attribute__((aligned(16))) u64 sm[];
  const u32 tid = threadIdx.x, lane = tid & 63;
  const size_t lt = blockIdx.x * size_t(blockDim.x) + tid;
  const u64 pk = p.pick ? *p.pick : 0;
  if (p.pick && pk == CK_NONE) return;  // nothing failed (the same in every lane)
  const bool active = p.pick ? lt == 0 : lt < p.rows;
  const size_t r = p.pick ? size_t(pk >> 32) : p.row0 + lt;
  u32* slots = LDS ? (reinterpret_cast<u32*>(sm + CK_RED) + tid) : (p.scratch + lt);
  const size_t stride = LDS ? blockDim.x : p.rows;

  u32 kfirst = ~0u;
  if (active) {
    const RowCtx c = row_ctx(p, r);
    for (u32 pc = 0; pc < p.n_instr; pc++) {
      const uint4 ins = reinterpret_cast<const uint4*>(p.code)[pc];
      u32 v;
      switch (ins.x) {
        case OP_ADD: v = bb_add(slots[ins.z * stride], slots[ins.w * stride]); break;
        case OP_SUB: v = bb_sub(slots[ins.z * stride], slots[ins.w * stride]); break;
        case OP_MUL: v = bb_mul(slots[ins.z * stride], slots[ins.w * stride]); break;
        case OP_NEG: v = bb_neg(slots[ins.z * stride]); break;
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

// ---- a wave per row (form 2): DProgram::wave_code, slot = position, 4 bytes each
__global__ __launch_bounds__(64) void bb_check_wave_k(CkParams p, const uint4* code, uint32_t n_steps, uint32_t n_leaf_steps) {
  extern __shared__ __attribute__((aligned(16))) u32 smw[];
  const u32 lane = threadIdx.x;
  const u64 pk = p.pick ? *p.pick : 0;
  if (p.pick && pk == CK_NONE) return;
  const size_t r = p.pick ? size_t(pk >> 32) : p.row0 + blockIdx.x;
  const RowCtx c = row_ctx(p, r);
  u32 s = 0;
  for (; s < n_leaf_steps; s++) smw[s * 64 + lane] = leaf_value(p, c, code[s * 64 + lane]);
  __syncthreads();
  for (; s < n_steps; s++) {
    const uint4 ins = code[s * 64 + lane];
    u32 v = 0;
    switch (ins.x) {
      case OP_ADD: v = bb_add(smw[ins.z], smw[ins.w]); break;
      case OP_SUB: v = bb_sub(smw[ins.z], smw[ins.w]); break;
      case OP_MUL: v = bb_mul(smw[ins.z], smw[ins.w]); break;
      case OP_NEG: v = bb_neg(smw[ins.z]); break;
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

// counters of the whole call: zeros, except the minima (all-ones)
__global__ void bb_check_init_k(u64* circ, size_t n_circ_words, u64* root_cnt, u64* root_first, size_t n_roots) {
  const size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x;
  if (i < n_circ_words) circ[i] = (i % CK_WORDS == 1) ? CK_NONE : 0;
  if (i < n_roots) {
    root_cnt[i] = 0;
    root_first[i] = CK_NONE;
  }
}
// the accumulator chain of msbb_stage2_build, kept on the device: publics of this circuit, accumulator behind it
__global__ void bb_check_chain_k(E4 beta, E4 gamma, E4* acc, const E4* total, u32* publics, u64* circ) {
  const E4 in = *acc, out = e4_add(in, *total);
  for (int k = 0; k < 4; k++) {
    publics[k] = beta.c[k], publics[4 + k] = gamma.c[k], publics[8 + k] = in.c[k], publics[12 + k] = out.c[k];
    circ[3 + k] = out.c[k];
  }
  *acc = out;
}

size_t big_lds(const void* kernel) {  // dynamic LDS above 64 KB is opted into per kernel and device
  const size_t want = 160 * 1024;
  if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want) == hipSuccess) return want;
  (void)hipGetLastError();
  return size_t(64) * 1024;
}
size_t lds_bytes(size_t n_slots, size_t lanes) { return n_slots * lanes * 4 + CK_RED * 8; }

}  // namespace

size_t check_roots(const BCircuit& c) {
  const size_t lookups = 4 * std::max<size_t>(c.num_lookups, 1);
  if (c.constraint_count < lookups || c.zeros.size() != c.constraint_count - lookups)
    throw std::runtime_error("msbb_witness_check: constraint count and constraint roots disagree");
  return c.zeros.size();
}

unsigned check_lds_lanes(size_t n_slots) {
  for (unsigned th = 256; th >= 64; th >>= 1)
    if (lds_bytes(n_slots, th) <= 64 * 1024) return th;
  return 0;
}

const BCheckProgram& check_program(BSystem& sys, size_t ci) {
  BCircuit& c = sys.circuits[ci];
  if (c.check.built) return c.check;
  Ctx& ctx = *sys.ctx;
  check_roots(c);
  BCheckProgram cp;
  msamd::build_program(ctx, c.nodes, c.zeros, {} /* no lookups */, cp.prog);
  // build_program leaves the constants on the device as the canonical 64-bit words of the node vector, in the order its two
  // programs number them: the same table as Montgomery words
  const size_t nc = cp.prog.consts.n;
  std::vector<u64> wide(nc);
  std::vector<u32> monty(nc);
  ctx.d2h(wide.data(), cp.prog.consts.p, nc * 8);
  for (size_t i = 0; i < nc; i++) monty[i] = bb_to_monty((u32)(wide[i] % BB_P));
  cp.consts = DBuf<u32>(ctx, nc);
  ctx.h2d(cp.consts.p, monty.data(), nc * 4);
  ctx.sync();  // (the vectors above go out of scope)
  cp.built = true;
  c.check = std::move(cp);
  return c.check;
}

void witness_check(BSystem& sys, BWitness& wit, E4 beta, E4 gamma, uint32_t* verdict, u64* circuits, u64* root_counts, u64* root_first) {
  Ctx& ctx = *sys.ctx;
  const size_t C = sys.circuits.size();
  if (wit.sys != &sys || wit.heights.size() != C) throw std::runtime_error("witness does not belong to this system");
  if (wit.host_resident)
    throw std::runtime_error("msbb_witness_check takes a device-resident witness (msbb_witness_create, msbb_witness_create_device)");
  std::vector<size_t> root_off(C + 1, 0);
  for (size_t ci = 0; ci < C; ci++) {
    const BCircuit& c = sys.circuits[ci];
    root_off[ci + 1] = root_off[ci] + check_roots(c);
    const size_t n = wit.heights[ci];
    if (!n) continue;
    if ((n & (n - 1)) || log2_strict(n) > BB_TWO_ADICITY) throw std::runtime_error("msbb_witness_check: trace height out of range");
    const BMat& t = wit.traces[ci];
    if (!t.buf.p || t.h != n || t.w != c.main_width) throw std::runtime_error("msbb_witness_check: an active circuit has no trace on this device");
    if (c.pre_width && (n != c.pre_height || !c.pre.buf.p)) throw std::runtime_error("main trace height must equal preprocessed trace height");
  }
  for (size_t ci = 0; ci < C; ci++)
    if (wit.heights[ci]) check_program(sys, ci);  // (a first check builds here, with host waits of its own)
  const size_t R = root_off[C];
  // [C x 8 counters | R counts | R first rows], the running accumulator and one circuit's total, the publics of each circuit
  DBuf<u64> rep(ctx, C * CK_WORDS + 2 * std::max<size_t>(R, 1));
  DBuf<u32> publics(ctx, std::max<size_t>(C, 1) * 16);
  DBuf<E4> acc(ctx, 2);
  u64 *d_circ = rep.p, *d_cnt = rep.p + C * CK_WORDS, *d_first = d_cnt + std::max<size_t>(R, 1);
  {
    const size_t items = std::max<size_t>(std::max(C * CK_WORDS, R), 1);
    hipLaunchKernelGGL(bb_check_init_k, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, ctx.stream, d_circ, C * CK_WORDS, d_cnt, d_first, R);
  }
  bb_claims_accumulator_async(ctx, wit.d_claim_data.p, wit.d_claim_offs.p, wit.claims.size(), beta, gamma, acc.p);
  std::vector<u64> tiers(C, 0);
  for (size_t ci = 0; ci < C; ci++) {
    const size_t n = wit.heights[ci];
    if (!n) continue;
    const BCircuit& c = sys.circuits[ci];
    const BCheckProgram& cp = c.check;
    const msamd::DProgram& prog = cp.prog;
    const unsigned log_n = log2_strict(n);
    BMat s2;
    bb_stage2_async(ctx, c.prog, c.lookup_prefix_len, c.lk, wit.traces[ci], c.pre_width ? &c.pre : nullptr, beta, gamma, s2, acc.p + 1);
    u64* circ = d_circ + ci * CK_WORDS;
    hipLaunchKernelGGL(bb_check_chain_k, dim3(1), dim3(1), 0, ctx.stream, beta, gamma, acc.p, acc.p + 1, publics.p + ci * 16, circ);
    if (prog.n_zeros == 0) continue;  // lookups only: nothing to evaluate

    CkParams p;
    p.trace = wit.traces[ci].buf.p, p.trace_ld = wit.traces[ci].ld;
    p.pre = c.pre_width ? c.pre.buf.p : nullptr, p.pre_ld = c.pre_width ? c.pre.ld : 0;
    p.s2 = s2.buf.p, p.s2_ld = s2.ld;
    p.n = n;
    p.code = prog.code.p;
    p.consts = cp.consts.p;
    p.zero_slots = prog.zero_slots.p;
    p.n_instr = (uint32_t)prog.n_instr;
    p.n_zeros = (uint32_t)prog.n_zeros;
    p.publics = publics.p + ci * 16;
    p.w = bb_two_adic_generator(log_n);
    p.w_inv = bb_inv(p.w);
    p.sel_first = bb_to_monty((u32)(n % BB_P));
    p.sel_last = bb_mul(p.sel_first, p.w);
    p.row0 = 0;
    p.rows = n;
    p.scratch = nullptr;
    p.circ = circ;
    p.root_cnt = d_cnt + root_off[ci];
    p.root_first = d_first + root_off[ci];
    p.pick = nullptr;
    CkParams pick = p;  // the one-row launch behind the sweep
    pick.pick = circ + 1;
    pick.rows = 1;

    const unsigned lanes = check_lds_lanes(prog.n_slots);
    ProfScope prof(ctx, msamd::K_WITNESS_CHECK, double(n) * 4.0 * double(c.main_width + c.pre_width));
    if (lanes) {
      const size_t lds = lds_bytes(prog.n_slots, lanes);
      hipLaunchKernelGGL(bb_check_k<true>, dim3((unsigned)((n + lanes - 1) / lanes)), dim3(lanes), lds, ctx.stream, p);
      hipLaunchKernelGGL(bb_check_k<true>, dim3(1), dim3(lanes), lds, ctx.stream, pick);
      tiers[ci] = 1 | (u64(lanes) << 8);
    } else if (prog.wave_steps && n <= 16384 && prog.wave_steps * 64 * 4 <= big_lds(reinterpret_cast<const void*>(&bb_check_wave_k))) {
      const uint4* code = reinterpret_cast<const uint4*>(prog.wave_code.p);
      p.zero_slots = pick.zero_slots = prog.wave_zero_pos.p;
      const size_t lds = prog.wave_steps * 64 * 4;
      hipLaunchKernelGGL(bb_check_wave_k, dim3((unsigned)n), dim3(64), lds, ctx.stream, p, code, (uint32_t)prog.wave_steps, (uint32_t)prog.wave_leaf_steps);
      hipLaunchKernelGGL(bb_check_wave_k, dim3(1), dim3(64), lds, ctx.stream, pick, code, (uint32_t)prog.wave_steps, (uint32_t)prog.wave_leaf_steps);
      tiers[ci] = 2 | (u64(64) << 8);
    } else if ((n + 31) / 32 <= 256 && lds_bytes(prog.n_slots, 32) <= big_lds(reinterpret_cast<const void*>(&bb_check_k<true>))) {
      // one round of small workgroups over the CUs, each with its 32 lanes' slot files in up to 160 KB of LDS
      const size_t lds = lds_bytes(prog.n_slots, 32);
      hipLaunchKernelGGL(bb_check_k<true>, dim3((unsigned)((n + 31) / 32)), dim3(32), lds, ctx.stream, p);
      hipLaunchKernelGGL(bb_check_k<true>, dim3(1), dim3(32), lds, ctx.stream, pick);
      tiers[ci] = 3 | (u64(32) << 8);
    } else {
      size_t batch = (size_t(1) << 30) / (prog.n_slots * 4);  // the scratch stays below ~1 GiB
      batch = std::max<size_t>(256, batch & ~size_t(255));
      batch = std::min(batch, n);
      DBuf<u32> scratch(ctx, batch * prog.n_slots);
      p.scratch = pick.scratch = scratch.p;
      for (size_t r0 = 0; r0 < n; r0 += batch) {
        p.row0 = r0;
        p.rows = std::min(batch, n - r0);
        hipLaunchKernelGGL(bb_check_k<false>, dim3((unsigned)((p.rows + 255) / 256)), dim3(256), CK_RED * 8, ctx.stream, p);
      }
      hipLaunchKernelGGL(bb_check_k<false>, dim3(1), dim3(64), CK_RED * 8, ctx.stream, pick);
      tiers[ci] = 4 | (u64(256) << 8);
    }
    HIP_CHECK(hipGetLastError());
  }
  // one host wait: the whole report
  const size_t rep_words = C * CK_WORDS + 2 * std::max<size_t>(R, 1);
  std::vector<u64> h(rep_words);
  E4 last;
  ctx.d2h_queue(h.data(), rep.p, rep_words * 8);
  ctx.d2h(&last, acc.p, sizeof(E4));
  uint32_t v = 0;
  for (size_t ci = 0; ci < C; ci++) {
    const u64* d = h.data() + ci * CK_WORDS;
    u64* o = circuits + ci * MSBB_CHECK_CIRCUIT_WORDS;
    const bool activec = wit.heights[ci] != 0;
    o[0] = wit.heights[ci];
    o[1] = d[0];
    o[2] = d[1] == CK_NONE ? CK_NONE : d[1] >> 32;
    o[3] = d[1] == CK_NONE ? CK_NONE : (d[1] & 0xffffffffu);
    o[4] = bb_from_monty((u32)d[2]);
    for (int k = 0; k < 4; k++) o[5 + k] = activec ? bb_from_monty((u32)d[3 + k]) : 0;
    o[9] = root_off[ci + 1] - root_off[ci];
    o[10] = tiers[ci];
    o[11] = root_off[ci];
    if (d[0]) v |= MS_CHECK_CONSTRAINT;
    if (d[0] && d[2] == 0) throw std::runtime_error("msbb_witness_check: internal error (the first failing root evaluates to zero)");
  }
  if (!e4_eq(last, e4_zero())) v |= MS_CHECK_LOOKUPS;
  if (root_counts) memcpy(root_counts, h.data() + C * CK_WORDS, R * 8);
  if (root_first) memcpy(root_first, h.data() + C * CK_WORDS + std::max<size_t>(R, 1), R * 8);
  *verdict = v;
}

}  // namespace msbb
