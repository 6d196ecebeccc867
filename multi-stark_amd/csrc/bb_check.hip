// Witness check of the BabyBear / Poseidon2 configuration (msbb_witness_check): what the shared kernels and driver of
// check_dev.h need to know of BabyBear.
//
// A row r of a circuit of height n sees what quotient_k (bb_kernels.hip) sees at x = w^r, w = bb_two_adic_generator(log n): main
// and preprocessed columns, the stage-2 evaluation bb_stage2 builds under the checker's (beta, gamma) - four base coordinates
// per lookup, natural row order - and the 16 public coordinates [beta, gamma, acc_in, acc_out].
//
// The program is NOT the prover's BProgram (one slot per node in a global scratch) but the node vector lowered by
// msamd::build_program over the user roots alone: slot-allocated code, the wave schedule, constants as a Montgomery table. It is
// built on the first check of a circuit (BCheckProgram). Every matrix here is COLUMN-major (bb.h): adjacent lanes read adjacent
// rows of a column, so main, preprocessed and stage-2 reads are coalesced as they stand and nothing is staged through LDS.
// Slots are 4-byte Montgomery words: 256 lanes up to 63 slots, 128 up to 127, 64 up to 255; 32 lanes up to 1278 (510 where
// only 64 KB can be had).
#include "../../include/mstark_bb.h"
#include "bb_host.h"
#include "check_dev.h"

namespace msbb {

namespace {

struct BbCheck {
  using Word = u32;
  using Ext = E4;
  static constexpr const char* call = "msbb_witness_check";
  static constexpr size_t acc_words = 4;
  static __device__ __forceinline__ u32 add(u32 a, u32 b) { return bb_add(a, b); }
  static __device__ __forceinline__ u32 sub(u32 a, u32 b) { return bb_sub(a, b); }
  static __device__ __forceinline__ u32 mul(u32 a, u32 b) { return bb_mul(a, b); }
  static __device__ __forceinline__ u32 neg(u32 a) { return bb_neg(a); }
  static u64 report(u64 word) { return bb_from_monty((u32)word); }
  static bool acc_is_zero(E4 a) { return e4_eq(a, e4_zero()); }
  struct View {
    const u32 *d_main, *d_pre, *d_s2;  // column-major, Montgomery, natural row order
    size_t main_ld, pre_ld, s2_ld;
    u32 w;  // generator of the trace domain
    __device__ __forceinline__ u32 main(size_t row, u32 col) const { return d_main[size_t(col) * main_ld + row]; }
    __device__ __forceinline__ u32 pre(size_t row, u32 col) const { return d_pre[size_t(col) * pre_ld + row]; }
    __device__ __forceinline__ size_t s2_row(size_t r) const { return r; }
    __device__ __forceinline__ u32 s2(size_t row, u32 col) const { return d_s2[size_t(col) * s2_ld + row]; }
    // (the sweep is bound by memory and LDS, not by these ~2 log n products)
    __device__ __forceinline__ u32 x(size_t r) const { return bb_pow(w, r); }
  };
};
static_assert(8 + BbCheck::acc_words == MSBB_CHECK_CIRCUIT_WORDS, "report layout");

// the accumulator chain of msbb_stage2_build, kept on the device: publics of this circuit, accumulator behind it
__global__ void bb_check_chain_k(E4 beta, E4 gamma, E4* acc, const E4* total, u32* publics, u64* circ) {
  const E4 in = *acc, out = e4_add(in, *total);
  for (int k = 0; k < 4; k++) {
    publics[k] = beta.c[k], publics[4 + k] = gamma.c[k], publics[8 + k] = in.c[k], publics[12 + k] = out.c[k];
    circ[3 + k] = out.c[k];
  }
  *acc = out;
}

}  // namespace

size_t check_roots(const BCircuit& c) {
  const size_t lookups = 4 * std::max<size_t>(c.num_lookups, 1);
  if (c.constraint_count < lookups || c.zeros.size() != c.constraint_count - lookups)
    throw std::runtime_error("msbb_witness_check: constraint count and constraint roots disagree");
  return c.zeros.size();
}

unsigned check_lds_lanes(size_t n_slots) { return msamd::slot_lds_lanes(n_slots, 4, msamd::CK_RED * 8); }

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
  // the running accumulator and one circuit's total (the claims' sum starts it), the publics of each circuit
  DBuf<u32> publics(ctx, std::max<size_t>(C, 1) * 16);
  DBuf<E4> acc(ctx, 2);
  msamd::CkCounters k(ctx, std::move(root_off), (E4*)nullptr);
  bb_claims_accumulator_async(ctx, wit.d_claim_data.p, wit.d_claim_offs.p, wit.claims.size(), beta, gamma, acc.p);
  for (size_t ci = 0; ci < C; ci++) {
    const size_t n = wit.heights[ci];
    if (!n) continue;
    const BCircuit& c = sys.circuits[ci];
    const BCheckProgram& cp = c.check;
    BMat s2;
    bb_stage2_async(ctx, c.prog, c.lookup_prefix_len, c.lk, wit.traces[ci], c.pre_width ? &c.pre : nullptr, beta, gamma, s2, acc.p + 1);
    hipLaunchKernelGGL(bb_check_chain_k, dim3(1), dim3(1), 0, ctx.stream, beta, gamma, acc.p, acc.p + 1, publics.p + ci * 16, k.circ(ci));
    if (cp.prog.n_zeros == 0) continue;  // lookups only: nothing to evaluate

    msamd::CkParams<BbCheck> p;
    p.v.d_main = wit.traces[ci].buf.p, p.v.main_ld = wit.traces[ci].ld;
    p.v.d_pre = c.pre_width ? c.pre.buf.p : nullptr, p.v.pre_ld = c.pre_width ? c.pre.ld : 0;
    p.v.d_s2 = s2.buf.p, p.v.s2_ld = s2.ld;
    p.v.w = bb_two_adic_generator(log2_strict(n));
    p.n = n;
    p.consts = cp.consts.p;
    p.publics = publics.p + ci * 16;
    p.w_inv = bb_inv(p.v.w);
    p.sel_first = bb_to_monty((u32)(n % BB_P));
    p.sel_last = bb_mul(p.sel_first, p.v.w);
    p.circ = k.circ(ci);
    p.root_cnt = k.cnt(ci);
    p.root_first = k.first(ci);

    ProfScope prof(ctx, msamd::K_WITNESS_CHECK, double(n) * 4.0 * double(c.main_width + c.pre_width));
    k.tiers[ci] = msamd::check_launch(ctx, cp.prog, p);
    HIP_CHECK(hipGetLastError());
  }
  msamd::check_report<BbCheck>(ctx, k, wit.heights, acc.p, verdict, circuits, root_counts, root_first);
}

}  // namespace msbb
