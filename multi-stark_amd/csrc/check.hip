// Witness check on the device (ms_witness_check): what the shared kernels and driver of check_dev.h need to know of Goldilocks.
//
// A row r of a circuit of height n sees what the quotient kernels see at x = w^r, w = gl_two_adic_generator(log n): the
// witness's ROW-MAJOR main and preprocessed traces, the stage-2 evaluation the prover would build under the checker's (beta,
// gamma) - column-major at bit-reversed rows - and the 8 public words [beta, gamma, acc_in, acc_out]. The node program is the
// circuit's DProgram, walked again in check_dev.h (quotient.hip stays byte for byte what it was). Slots are canonical 8-byte
// words: 256 lanes up to 31 slots, 128 up to 63, 64 up to 127; 32 lanes up to 639 (255 where only 64 KB can be had).
#include "check_dev.h"
#include "host.h"

namespace msamd {

namespace {

struct GlCheck {
  using Word = u64;
  using Ext = E2;
  static constexpr const char* call = "ms_witness_check";
  static constexpr size_t acc_words = 2;
  static __device__ __forceinline__ u64 add(u64 a, u64 b) { return gl_add(a, b); }
  static __device__ __forceinline__ u64 sub(u64 a, u64 b) { return gl_sub(a, b); }
  static __device__ __forceinline__ u64 mul(u64 a, u64 b) { return gl_mul(a, b); }
  static __device__ __forceinline__ u64 neg(u64 a) { return gl_neg(a); }
  static u64 report(u64 word) { return word; }
  static bool acc_is_zero(E2 a) { return e2_is_zero(a); }
  struct View {
    const u64 *d_main, *d_pre, *d_s2;  // n x main_w and n x pre_w ROW-major; n x s2_w column-major with bit-reversed rows
    size_t n;
    unsigned log_n;
    uint32_t main_w, pre_w;
    const u64 *t0, *t1;  // twiddle tables of the context (W^e = t1[e >> 14] * t0[e & 16383])
    __device__ __forceinline__ u64 main(size_t row, u32 col) const { return d_main[row * main_w + col]; }
    __device__ __forceinline__ u64 pre(size_t row, u32 col) const { return d_pre[row * pre_w + col]; }
    __device__ __forceinline__ size_t s2_row(size_t r) const { return bitrev32((u32)r, log_n); }
    __device__ __forceinline__ u64 s2(size_t row, u32 col) const { return d_s2[size_t(col) * n + row]; }
    __device__ __forceinline__ u64 x(size_t r) const {
      const u32 e = (u32)r << (TW_LOG - log_n);
      return gl_mul(t1[e >> TW_HALF], t0[e & ((1u << TW_HALF) - 1)]);
    }
  };
};
static_assert(8 + GlCheck::acc_words == MS_CHECK_CIRCUIT_WORDS, "report layout");

// the accumulator chain of ms_stage2_build, kept on the device: publics of this circuit, accumulator behind it
__global__ void check_chain_k(E2 beta, E2 gamma, E2* acc, const E2* total, u64* publics, u64* circ) {
  const E2 in = *acc, out = e2_add(in, *total);
  publics[0] = beta.c0, publics[1] = beta.c1, publics[2] = gamma.c0, publics[3] = gamma.c1;
  publics[4] = in.c0, publics[5] = in.c1, publics[6] = out.c0, publics[7] = out.c1;
  circ[3] = out.c0, circ[4] = out.c1;
  *acc = out;
}

}  // namespace

size_t check_roots(const HCircuit& c) {
  const size_t want = c.constraint_count - 2 * std::max<size_t>(c.num_lookups, 1);
  if (c.zeros.size() != want) throw std::runtime_error("ms_witness_check: constraint count and constraint roots disagree");
  return want;
}

unsigned check_lds_lanes(size_t n_slots) { return slot_lds_lanes(n_slots, 8, CK_RED * 8); }

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
  // the running accumulator and one circuit's total, the publics of each circuit
  DBuf<u64> publics(ctx, std::max<size_t>(C, 1) * 8);
  DBuf<E2> acc(ctx, 2);
  CkCounters k(ctx, std::move(root_off), acc.p);
  const size_t n_claims = wit.claim_offsets.size() - 1;
  if (n_claims) claims_accumulator_async(ctx, wit.d_claim_data.p, wit.d_claim_offsets.p, n_claims, beta, gamma, acc.p);
  for (size_t ci = 0; ci < C; ci++) {
    const size_t n = wit.heights[ci];
    if (!n) continue;
    const HCircuit& c = sys.circuits[ci];
    const unsigned log_n = log2_strict(n);
    DBuf<u64> s2(ctx, n * c.stage2_width);
    stage2_circuit_async(ctx, sys, wit, ci, beta, gamma, s2.p, acc.p + 1);
    hipLaunchKernelGGL(check_chain_k, dim3(1), dim3(1), 0, ctx.stream, beta, gamma, acc.p, acc.p + 1, publics.p + ci * 8, k.circ(ci));
    if (c.prog.n_zeros == 0) continue;  // lookups only: nothing to evaluate

    CkParams<GlCheck> p;
    p.v.d_main = wit.traces[ci].p;
    p.v.d_pre = c.pre_width ? c.d_preprocessed.p : nullptr;
    p.v.d_s2 = s2.p;
    p.v.n = n;
    p.v.log_n = log_n;
    p.v.main_w = (uint32_t)c.main_width;
    p.v.pre_w = (uint32_t)c.pre_width;
    p.v.t0 = ctx.tw0;
    p.v.t1 = ctx.tw1;
    p.n = n;
    p.consts = c.prog.consts.p;
    p.publics = publics.p + ci * 8;
    const u64 w = gl_two_adic_generator(log_n);
    p.w_inv = gl_inv(w);
    p.sel_first = (u64)n % GL_P;
    p.sel_last = gl_mul(p.sel_first, w);
    p.circ = k.circ(ci);
    p.root_cnt = k.cnt(ci);
    p.root_first = k.first(ci);

    const double bytes = double(n) * 8.0 * double(c.main_width + c.pre_width);
    hipEvent_t ev = ctx.prof_begin(K_WITNESS_CHECK);
    k.tiers[ci] = check_launch(ctx, c.prog, p);
    ctx.prof_end(K_WITNESS_CHECK, ev, bytes);
    HIP_CHECK(hipGetLastError());
  }
  check_report<GlCheck>(ctx, k, wit.heights, acc.p, verdict, circuits, root_counts, root_first);
}

}  // namespace msamd
