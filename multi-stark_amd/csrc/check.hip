// Witness check on the device (ms_witness_check): every user constraint root of every active circuit evaluated on the TRACE
// domain, row by row, and the outcome reduced to a report - which circuit, which row, which constraint.
//
// A row r of a circuit of height n sees what the quotient kernels see at x = w^r, w = gl_two_adic_generator(log n): main and
// preprocessed columns at row r and (r + 1) mod n, the stage-2 evaluation the prover would build under the checker's
// (beta, gamma), the publics [beta, gamma, acc_in, acc_out], and the selector POLYNOMIALS of quotient.hip at x = w^r with their
// limits: is_first = n at row 0 (else 0), is_last = n w at row n - 1 (else 0), is_transition = w^r - w^-1. (They are not the
// 0 / 1 flags of lookup_values_k.)
//
// The node program is the circuit's DProgram, walked again here (quotient.hip stays byte for byte what it was) over the
// witness's ROW-MAJOR traces, in the three slot-file regimes of quotient_eval:
//   1  a thread per row, slots in LDS as [slot][lane] at 256 / 128 / 64 lanes;
//   2  a wave per row over the level-scheduled program (DProgram::wave_code), for short circuits with large programs;
//   3  a thread per row at 32 lanes per workgroup with up to 160 KB of LDS (short circuits, thousands of live slots);
//   4  a thread per row, slots in a global scratch, in row batches.
// Reductions: a workgroup counts its failing rows per wave (ballot) and through LDS; a clean workgroup leaves there - no global
// atomic is issued for a clean trace. A failing workgroup reduces per wave (ballot), then through LDS, and issues ONE 64-bit atomic per touched
// counter: failing rows, the packed (row << 32 | constraint) minimum, and per root its count and its first row.
// The value of the first failing root is written by a second, one-row launch that reads the packed minimum from device memory
// ("pick" mode): no value ever depends on the order in which workgroups arrive.
#include <algorithm>

#include "host.h"

namespace msamd {

namespace {

constexpr u32 CK_CHUNK = 16;    // roots reduced through LDS per round of a failing workgroup
constexpr u32 CK_FIRST = 16;    // u64 index of the workgroup's packed minimum (behind 16 + 16 u32 of counts / lanes)
constexpr u32 CK_RED = 24;      // u64 words of LDS in front of the slot file (192 bytes: the slots stay 16-byte aligned)
constexpr u64 CK_NONE = ~u64(0);

struct CkParams {
  const u64 *trace, *pre, *s2;  // n x main_w and n x pre_w ROW-major; n x s2_w column-major with bit-reversed rows
  size_t n;
  unsigned log_n;
  uint32_t main_w, pre_w;
  const uint32_t* code;
  const u64* consts;
  const uint32_t* zero_slots;   // slot (thread per row) or position (wave per row) of each root
  uint32_t n_instr, n_zeros;
  const u64* publics;           // 8 words, device
  const u64 *t0, *t1;           // twiddle tables of the context (W^e = t1[e >> 14] * t0[e & 16383])
  u64 g_inv, sel_first, sel_last;  // w^-1, n, n w
  size_t row0, rows;
  u64* scratch;
  u64* circ;                    // [0] failing rows, [1] min (row << 32 | root), [2] that root's value
  u64 *root_cnt, *root_first;   // this circuit's slices
  const u64* pick;              // non-null: evaluate row *pick >> 32 only and write root (*pick & 0xffffffff) to circ[2]
};

struct RowCtx {
  size_t r, rn, r_s2, rn_s2;
  u64 is_first, is_last, is_trans;
};
__device__ __forceinline__ RowCtx row_ctx(const CkParams& p, size_t r) {
  RowCtx c;
  c.r = r;
  c.rn = r + 1 == p.n ? 0 : r + 1;
  c.r_s2 = bitrev32((u32)c.r, p.log_n);
  c.rn_s2 = bitrev32((u32)c.rn, p.log_n);
  const u32 e = (u32)r << (TW_LOG - p.log_n);
  const u64 x = gl_mul(p.t1[e >> TW_HALF], p.t0[e & ((1u << TW_HALF) - 1)]);
  c.is_first = r == 0 ? p.sel_first : 0;
  c.is_last = r + 1 == p.n ? p.sel_last : 0;
  c.is_trans = gl_sub(x, p.g_inv);
  return c;
}
__device__ __forceinline__ u64 leaf_value(const CkParams& p, const RowCtx& c, const uint4 ins) {
  switch (ins.x) {
    case OP_CONST: return p.consts[ins.z];
    case OP_VAR: {
      const u32 src = ins.z & 0xff, off = ins.z >> 8;
      if (src == 1) return p.trace[(off ? c.rn : c.r) * p.main_w + ins.w];
      if (src == 0) return p.pre[(off ? c.rn : c.r) * p.pre_w + ins.w];
      return p.s2[size_t(ins.w) * p.n + (off ? c.rn_s2 : c.r_s2)];
    }
    case OP_PUBLIC: return p.publics[ins.z];
    case OP_IS_FIRST: return c.is_first;
    case OP_IS_LAST: return c.is_last;
    case OP_IS_TRANS: return c.is_trans;
    default: return 0;
  }
}

// ---- a thread per row (tiers 1, 3, 4)
template <bool LDS>
__global__ __launch_bounds__(256) void check_k(CkParams p) {
  extern __shared__ __attribute__((aligned(16))) u64 sm[];
  const u32 tid = threadIdx.x, lane = tid & 63;
  const size_t lt = blockIdx.x * size_t(blockDim.x) + tid;
  const u64 pk = p.pick ? *p.pick : 0;
  if (p.pick && pk == CK_NONE) return;  // nothing failed (the same in every lane)
  const bool active = p.pick ? lt == 0 : lt < p.rows;
  const size_t r = p.pick ? size_t(pk >> 32) : p.row0 + lt;
  u64* slots = LDS ? (sm + CK_RED + tid) : (p.scratch + lt);
  const size_t stride = LDS ? blockDim.x : p.rows;

  u32 kfirst = ~0u;
  if (active) {
    const RowCtx c = row_ctx(p, r);
    for (u32 pc = 0; pc < p.n_instr; pc++) {
      const uint4 ins = reinterpret_cast<const uint4*>(p.code)[pc];
      u64 v;
      switch (ins.x) {
        case OP_ADD: v = gl_add(slots[ins.z * stride], slots[ins.w * stride]); break;
        case OP_SUB: v = gl_sub(slots[ins.z * stride], slots[ins.w * stride]); break;
        case OP_MUL: v = gl_mul(slots[ins.z * stride], slots[ins.w * stride]); break;
        case OP_NEG: v = gl_neg(slots[ins.z * stride]); break;
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

// ---- a wave per row (tier 2): the walk of quotient_wave_k over DProgram::wave_code, slot = position
__global__ __launch_bounds__(64) void check_wave_k(CkParams p, const uint4* code, uint32_t n_steps, uint32_t n_leaf_steps) {
  extern __shared__ __attribute__((aligned(16))) u64 sm[];
  const u32 lane = threadIdx.x;
  const u64 pk = p.pick ? *p.pick : 0;
  if (p.pick && pk == CK_NONE) return;
  const size_t r = p.pick ? size_t(pk >> 32) : p.row0 + blockIdx.x;
  const RowCtx c = row_ctx(p, r);
  u32 s = 0;
  for (; s < n_leaf_steps; s++) sm[s * 64 + lane] = leaf_value(p, c, code[s * 64 + lane]);
  __syncthreads();
  for (; s < n_steps; s++) {
    const uint4 ins = code[s * 64 + lane];
    u64 v = 0;
    switch (ins.x) {
      case OP_ADD: v = gl_add(sm[ins.z], sm[ins.w]); break;
      case OP_SUB: v = gl_sub(sm[ins.z], sm[ins.w]); break;
      case OP_MUL: v = gl_mul(sm[ins.z], sm[ins.w]); break;
      case OP_NEG: v = gl_neg(sm[ins.z]); break;
      case 15: break;  // padding of a level
      default: v = leaf_value(p, c, ins); break;
    }
    sm[s * 64 + lane] = v;
    if (ins.y) __syncthreads();  // the last step of a level (the flag is the same in all 64 lanes)
  }
  __syncthreads();
  if (p.pick) {
    if (lane == 0) p.circ[2] = sm[p.zero_slots[(u32)pk]];
    return;
  }
  // the workgroup IS the row: each failing root costs one atomic pair per row, the row itself one
  u32 kfirst = ~0u;
  for (u32 z = lane; z < p.n_zeros; z += 64)
    if (sm[p.zero_slots[z]] != 0) {
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
__global__ void check_init_k(u64* circ, size_t n_circ_words, u64* root_cnt, u64* root_first, size_t n_roots, E2* acc) {
  const size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x;
  if (i < n_circ_words) circ[i] = (i % 8 == 1) ? CK_NONE : 0;
  if (i < n_roots) {
    root_cnt[i] = 0;
    root_first[i] = CK_NONE;
  }
  if (i == 0 && acc) *acc = e2(0);
}
// the accumulator chain of ms_stage2_build, kept on the device: publics of this circuit, accumulator behind it
__global__ void check_chain_k(E2 beta, E2 gamma, E2* acc, const E2* total, u64* publics, u64* circ) {
  const E2 in = *acc, out = e2_add(in, *total);
  publics[0] = beta.c0, publics[1] = beta.c1, publics[2] = gamma.c0, publics[3] = gamma.c1;
  publics[4] = in.c0, publics[5] = in.c1, publics[6] = out.c0, publics[7] = out.c1;
  circ[3] = out.c0, circ[4] = out.c1;
  *acc = out;
}

size_t big_lds(const void* kernel) {  // dynamic LDS above 64 KB is opted into per kernel and device (see quotient.hip)
  const size_t want = 160 * 1024;
  if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want) == hipSuccess) return want;
  (void)hipGetLastError();
  return size_t(64) * 1024;
}

}  // namespace

size_t check_roots(const HCircuit& c) {
  const size_t want = c.constraint_count - 2 * std::max<size_t>(c.num_lookups, 1);
  if (c.zeros.size() != want) throw std::runtime_error("ms_witness_check: constraint count and constraint roots disagree");
  return want;
}

// lanes of tier 1 for a slot file (0: it does not fit 64 KB at 64 lanes)
unsigned check_lds_lanes(size_t n_slots) {
  for (unsigned th = 256; th >= 64; th >>= 1)
    if ((n_slots * th + CK_RED) * 8 <= 64 * 1024) return th;
  return 0;
}

void witness_check(HSystem& sys, HWitness& wit, E2 beta, E2 gamma, uint32_t* verdict, u64* circuits, u64* root_counts, u64* root_first) {
  Ctx& ctx = *sys.ctx;
  const size_t C = sys.circuits.size();
  if (wit.sys != &sys || wit.heights.size() != C) throw std::runtime_error("witness does not belong to this system");
  if (wit.host_resident)
    throw std::runtime_error("ms_witness_check takes a device-resident witness (ms_witness_create, ms_witness_create_device, the generators)");
  if (wit.has_remote) throw std::runtime_error("ms_witness_check: this witness lacks traces that another rank computes");
  std::vector<size_t> root_off(C + 1, 0);
  for (size_t ci = 0; ci < C; ci++) {
    const HCircuit& c = sys.circuits[ci];
    root_off[ci + 1] = root_off[ci] + check_roots(c);
    const size_t n = wit.heights[ci];
    if (!n) continue;
    if ((n & (n - 1)) || log2_strict(n) > NTT_MAX_LOG) throw std::runtime_error("ms_witness_check: trace height out of range");
    if (!wit.traces[ci].p) throw std::runtime_error("ms_witness_check: an active circuit has no trace on this device");
    if (c.pre_width && (n != c.pre_height || !c.d_preprocessed.p)) throw std::runtime_error("main trace height must equal preprocessed trace height");
  }
  const size_t R = root_off[C];
  // [C x 8 counters | R counts | R first rows], the running accumulator and one circuit's total, the publics of each circuit
  DBuf<u64> rep(ctx, C * 8 + 2 * std::max<size_t>(R, 1)), publics(ctx, std::max<size_t>(C, 1) * 8);
  DBuf<E2> acc(ctx, 2);
  u64 *d_circ = rep.p, *d_cnt = rep.p + C * 8, *d_first = d_cnt + std::max<size_t>(R, 1);
  {
    const size_t items = std::max<size_t>(std::max(C * 8, R), 1);
    hipLaunchKernelGGL(check_init_k, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, ctx.stream, d_circ, C * 8, d_cnt, d_first, R, acc.p);
  }
  const size_t n_claims = wit.claim_offsets.size() - 1;
  if (n_claims) claims_accumulator_async(ctx, wit.d_claim_data.p, wit.d_claim_offsets.p, n_claims, beta, gamma, acc.p);
  std::vector<u64> tiers(C, 0);
  for (size_t ci = 0; ci < C; ci++) {
    const size_t n = wit.heights[ci];
    if (!n) continue;
    const HCircuit& c = sys.circuits[ci];
    const DProgram& prog = c.prog;
    const unsigned log_n = log2_strict(n);
    DBuf<u64> s2(ctx, n * c.stage2_width);
    stage2_circuit_async(ctx, sys, wit, ci, beta, gamma, s2.p, acc.p + 1);
    u64* circ = d_circ + ci * 8;
    hipLaunchKernelGGL(check_chain_k, dim3(1), dim3(1), 0, ctx.stream, beta, gamma, acc.p, acc.p + 1, publics.p + ci * 8, circ);
    if (prog.n_zeros == 0) continue;  // lookups only: nothing to evaluate

    CkParams p;
    p.trace = wit.traces[ci].p;
    p.pre = c.pre_width ? c.d_preprocessed.p : nullptr;
    p.s2 = s2.p;
    p.n = n;
    p.log_n = log_n;
    p.main_w = (uint32_t)c.main_width;
    p.pre_w = (uint32_t)c.pre_width;
    p.code = prog.code.p;
    p.consts = prog.consts.p;
    p.zero_slots = prog.zero_slots.p;
    p.n_instr = (uint32_t)prog.n_instr;
    p.n_zeros = (uint32_t)prog.n_zeros;
    p.publics = publics.p + ci * 8;
    p.t0 = ctx.tw0;
    p.t1 = ctx.tw1;
    const u64 w = gl_two_adic_generator(log_n);
    p.g_inv = gl_inv(w);
    p.sel_first = (u64)n % GL_P;
    p.sel_last = gl_mul(p.sel_first, w);
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

    const double bytes = double(n) * 8.0 * double(c.main_width + c.pre_width);
    const unsigned lanes = check_lds_lanes(prog.n_slots);
    hipEvent_t ev = ctx.prof_begin(K_WITNESS_CHECK);
    if (lanes) {
      const size_t lds = (prog.n_slots * lanes + CK_RED) * 8;
      hipLaunchKernelGGL(check_k<true>, dim3((unsigned)((n + lanes - 1) / lanes)), dim3(lanes), lds, ctx.stream, p);
      hipLaunchKernelGGL(check_k<true>, dim3(1), dim3(lanes), lds, ctx.stream, pick);
      tiers[ci] = 1 | (u64(lanes) << 8);
    } else if (prog.wave_steps && n <= 16384 && prog.wave_steps * 64 * 8 <= big_lds(reinterpret_cast<const void*>(&check_wave_k))) {
      const uint4* code = reinterpret_cast<const uint4*>(prog.wave_code.p);
      p.zero_slots = pick.zero_slots = prog.wave_zero_pos.p;
      const size_t lds = prog.wave_steps * 64 * 8;
      hipLaunchKernelGGL(check_wave_k, dim3((unsigned)n), dim3(64), lds, ctx.stream, p, code, (uint32_t)prog.wave_steps, (uint32_t)prog.wave_leaf_steps);
      hipLaunchKernelGGL(check_wave_k, dim3(1), dim3(64), lds, ctx.stream, pick, code, (uint32_t)prog.wave_steps, (uint32_t)prog.wave_leaf_steps);
      tiers[ci] = 2 | (u64(64) << 8);
    } else if ((n + 31) / 32 <= 256 && (prog.n_slots * 32 + CK_RED) * 8 <= big_lds(reinterpret_cast<const void*>(&check_k<true>))) {
      // one round of small workgroups over the CUs, each with its 32 lanes' slot files in up to 160 KB of LDS
      const size_t lds = (prog.n_slots * 32 + CK_RED) * 8;
      hipLaunchKernelGGL(check_k<true>, dim3((unsigned)((n + 31) / 32)), dim3(32), lds, ctx.stream, p);
      hipLaunchKernelGGL(check_k<true>, dim3(1), dim3(32), lds, ctx.stream, pick);
      tiers[ci] = 3 | (u64(32) << 8);
    } else {
      size_t batch = (size_t(1) << 30) / (prog.n_slots * 8);  // the scratch stays below ~1 GiB
      batch = std::max<size_t>(256, batch & ~size_t(255));
      batch = std::min(batch, n);
      DBuf<u64> scratch(ctx, batch * prog.n_slots);
      p.scratch = pick.scratch = scratch.p;
      for (size_t r0 = 0; r0 < n; r0 += batch) {
        p.row0 = r0;
        p.rows = std::min(batch, n - r0);
        hipLaunchKernelGGL(check_k<false>, dim3((unsigned)((p.rows + 255) / 256)), dim3(256), CK_RED * 8, ctx.stream, p);
      }
      hipLaunchKernelGGL(check_k<false>, dim3(1), dim3(64), CK_RED * 8, ctx.stream, pick);
      tiers[ci] = 4 | (u64(256) << 8);
    }
    ctx.prof_end(K_WITNESS_CHECK, ev, bytes);
    HIP_CHECK(hipGetLastError());
  }
  // one host wait: the whole report
  std::vector<u64> h(C * 8 + 2 * std::max<size_t>(R, 1) + 2);
  ctx.d2h_queue(h.data(), rep.p, (h.size() - 2) * 8);
  ctx.d2h(h.data() + h.size() - 2, acc.p, sizeof(E2));
  uint32_t v = 0;
  E2 last = e2(h[h.size() - 2], h[h.size() - 1]);
  for (size_t ci = 0; ci < C; ci++) {
    const u64* d = h.data() + ci * 8;
    u64* o = circuits + ci * MS_CHECK_CIRCUIT_WORDS;
    const bool activec = wit.heights[ci] != 0;
    o[0] = wit.heights[ci];
    o[1] = d[0];
    o[2] = d[1] == CK_NONE ? CK_NONE : d[1] >> 32;
    o[3] = d[1] == CK_NONE ? CK_NONE : (d[1] & 0xffffffffu);
    o[4] = d[2];
    o[5] = activec ? d[3] : 0;
    o[6] = activec ? d[4] : 0;
    o[7] = root_off[ci + 1] - root_off[ci];
    o[8] = tiers[ci];
    o[9] = root_off[ci];
    if (d[0]) v |= MS_CHECK_CONSTRAINT;
    if (d[0] && d[2] == 0) throw std::runtime_error("ms_witness_check: internal error (the first failing root evaluates to zero)");
  }
  if (!e2_is_zero(last)) v |= MS_CHECK_LOOKUPS;
  if (root_counts) memcpy(root_counts, h.data() + C * 8, R * 8);
  if (root_first) memcpy(root_first, h.data() + C * 8 + std::max<size_t>(R, 1), R * 8);
  *verdict = v;
}

}  // namespace msamd
