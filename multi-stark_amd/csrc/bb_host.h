// Host-side types of the BabyBear / Poseidon2 path that the prover (bb_prover.hip), the verifier (bb_verifier.hip) and the
// C ABI (include/mstark_bb.h, at the end of bb_prover.hip) share: the DuplexChallenger transcript and the System / witness
// mirrors. The counterpart of host.h.
#pragma once
#include <stdexcept>
#include <vector>

#include "../../include/mstark.h"
#include "bb.h"

namespace msbb {

using msamd::PNode;

static unsigned log2_strict(size_t n) {
  unsigned l = 0;
  while ((size_t(1) << l) < n) l++;
  return l;
}
static size_t bitrev_host(size_t x, unsigned bits) {
  size_t r = 0;
  for (unsigned i = 0; i < bits; i++) r |= ((x >> i) & 1) << (bits - 1 - i);
  return r;
}

// DuplexChallenger<BabyBear, Poseidon2BabyBear<16>, 16, 8> (baby_bear_config.rs:37), values in Montgomery form
struct Challenger {
  const Poseidon2* perm;
  u32 state[16];
  std::vector<u32> input, output;
  explicit Challenger(const Poseidon2* p) : perm(p) {
    for (auto& x : state) x = 0;
  }
  void duplexing() {
    for (size_t i = 0; i < input.size(); i++) state[i] = input[i];
    input.clear();
    bb_poseidon2(*perm, state);
    output.assign(state, state + 8);
  }
  void observe(u32 m) {
    output.clear();
    input.push_back(m);
    if (input.size() == 8) duplexing();
  }
  void observe_usize(u64 x) { observe(bb_to_monty((u32)(x % BB_P))); }  // Val::from_usize
  void observe_ext(E4 e) {
    for (int k = 0; k < 4; k++) observe(e.c[k]);
  }
  void observe_cap(const std::vector<Digest8>& cap) {
    for (auto& d : cap)
      for (int k = 0; k < 8; k++) observe(d.w[k]);
  }
  u32 sample() {
    if (!input.empty() || output.empty()) duplexing();
    u32 v = output.back();
    output.pop_back();
    return v;
  }
  E4 sample_ext() {
    E4 e;
    for (int k = 0; k < 4; k++) e.c[k] = sample();
    return e;
  }
  size_t sample_bits(unsigned bits) { return (size_t)(bb_from_monty(sample()) & ((1u << bits) - 1)); }
  bool check_witness(unsigned bits, u32 monty_witness) {
    if (bits == 0) return true;
    observe(monty_witness);
    return sample_bits(bits) == 0;
  }
  // smallest witness (canonical value); ZERO at 0 bits - the deterministic rule of src/types.rs:72-81
  u32 grind(unsigned bits) {
    if (bits == 0) return 0;
    for (u32 w = 0; w < BB_P; w++) {
      Challenger c = *this;
      c.observe(bb_to_monty(w));
      if (c.sample_bits(bits) == 0) {
        observe(bb_to_monty(w));
        sample_bits(bits);
        return w;
      }
    }
    throw std::runtime_error("grind: no witness");
  }
};

struct Params {
  u64 log_blowup = 1, cap_height = 0, log_final_poly_len = 0, max_log_arity = 1, num_queries = 1, commit_pow_bits = 0, query_pow_bits = 0;
};
// the witness check's program of one circuit (bb_check.hip): the node vector lowered by msamd::build_program over the user
// constraint roots alone - slot-allocated code, wave schedule - with the constants as Montgomery words in build_program's order.
// Built on the first msbb_witness_check / msbb_system_check_info of the circuit; system creation and the prover never touch it.
struct BCheckProgram {
  bool built = false;
  msamd::DProgram prog;
  DBuf<u32> consts;
};
struct BCircuit {
  std::vector<PNode> nodes;
  std::vector<uint32_t> degrees, zeros;
  std::vector<std::pair<uint32_t, std::vector<uint32_t>>> lookups;
  size_t main_width = 0, pre_width = 0, pre_height = 0, num_lookups = 0, stage2_width = 0, constraint_count = 0, max_constraint_degree = 0,
         args_width = 0, lookup_prefix_len = 0;
  BProgram prog;
  msamd::JitKernel quotient_jit;  // this circuit's quotient kernel, compiled at system creation (quotient_jit.hip); may be empty
  BLookupsDev lk;
  DBuf<u32> d_zeros;
  BMat pre;  // preprocessed trace (column-major, Montgomery), for witness preparation
  BCheckProgram check;
  size_t quotient_degree() const {
    size_t d = (max_constraint_degree > 2 ? max_constraint_degree : 2) - 1, q = 1;
    while (q < d) q <<= 1;
    return q;
  }
};
struct BSystem {
  Ctx* ctx = nullptr;
  Params params;
  Poseidon2 perm;
  DBuf<Poseidon2> d_perm;
  std::vector<BCircuit> circuits;
  bool has_pre = false;
  std::vector<Digest8> pre_commit;
  std::vector<int> pre_indices;
  BPcsData pre_data;
  std::vector<u32> seed;  // Montgomery form
};
struct BWitness {
  BSystem* sys = nullptr;
  std::vector<size_t> heights;
  std::vector<BMat> traces;
  std::vector<std::vector<u32>> claims;  // canonical (the transcript absorbs them on the host)
  DBuf<u32> d_claim_data;                // Montgomery form, concatenated
  DBuf<u64> d_claim_offs;
  // host-resident form (msbb_witness_create_host): nothing lives in HBM between proofs; every prove() uploads the caller's
  // (page-locked) trace buffers and the claims, and gives the device copies back when it is done
  bool host_resident = false;
  bool pinned = true;  // every trace buffer could be page-locked (otherwise the uploads go through the context's bounce buffer)
  std::vector<const u32*> h_traces;
  std::vector<void*> registered;
  std::vector<u32> h_claims_monty;
  std::vector<u64> h_claim_offs;
  ~BWitness() {
    if (!registered.empty() && sys && sys->ctx) {  // nothing may still be reading the caller's ranges when they lose their page lock
      (void)hipSetDevice(sys->ctx->device);
      (void)hipStreamSynchronize(sys->ctx->main_stream);
    }
    for (void* p : registered) msamd::host_range_unpin(p);
  }
};

// the system blob (frontend.system_blob): little-endian 64-bit words
struct Reader {
  const uint8_t* p;
  size_t n, off = 0;
  u64 word() {
    if (off + 8 > n) throw std::runtime_error("system blob truncated");
    u64 v = 0;
    for (int k = 0; k < 8; k++) v |= (u64)p[off + k] << (8 * k);
    off += 8;
    return v;
  }
};
static const u64 BLOB_MAGIC = 0x31304259534D0000ULL;  // "\0\0MSYB01"

static void set_internal_diag(Poseidon2& k) {
  auto m = [](u32 canonical) { return bb_to_monty(canonical); };
  u32 half = bb_inv(m(2)), i8 = bb_inv(m(256)), i27 = bb_inv(m(1u << 27));
  u32 t[16] = {bb_neg(m(2)), m(1), m(2), half, m(3), m(4), bb_neg(half), bb_neg(m(3)), bb_neg(m(4)), i8, bb_inv(m(4)), bb_inv(m(8)), i27,
               bb_neg(i8), bb_neg(bb_inv(m(16))), bb_neg(i27)};
  for (int i = 0; i < 16; i++) k.diag[i] = t[i];
}

typedef std::vector<std::vector<std::vector<E4>>> OpenedRound;  // matrix -> point -> column

// System::verify_multiple_claims (bb_verifier.hip): 0 = accepted, otherwise the VerificationError code of include/mstark.h
int verify(BSystem& sys, size_t n_claims, const u64* claim_offsets, const u32* claim_data, const uint8_t* proof_bytes, size_t proof_len);
// the same for n_proofs proofs of one system with the per-query arithmetic and every Merkle path on the device (bb_verifier.hip,
// bb_verify_dev.hip): verdicts[i] is what verify() returns for proof i
void verify_batch(BSystem& sys, size_t n_proofs, const u64* n_claims, const u64* const* claim_offsets, const u32* const* claim_data,
                  const uint8_t* const* proofs, const u64* proof_lens, int32_t* verdicts);
// msbb_witness_check (bb_check.hip): the user constraint roots of every active circuit on the trace domain + the lookup balance
// under (beta, gamma); circuits: n_circuits x MSBB_CHECK_CIRCUIT_WORDS; root_counts / root_first nullable
void witness_check(BSystem& sys, BWitness& wit, E4 beta, E4 gamma, uint32_t* verdict, u64* circuits, u64* root_counts, u64* root_first);
size_t check_roots(const BCircuit& c);                        // user constraint roots (throws if `zeros` disagrees)
const BCheckProgram& check_program(BSystem& sys, size_t ci);  // built on first use
unsigned check_lds_lanes(size_t n_slots);                     // lanes of the thread-per-row LDS form (0: the slot file does not fit)
// msbb_witness_lookup_balance (bb_balance.hip): every message grouped by its tuple, exactly; entries: entries_cap x
// MS_LB_ENTRY_WORDS, args_out: canonical words; slot_counts nullable, lookup_balance_slots(sys) + 1 words
size_t lookup_balance_slots(const BSystem& sys);
void witness_lookup_balance(BSystem& sys, BWitness& wit, u64 summary[4], u64* entries, size_t entries_cap, u32* args_out, size_t args_cap,
                            u64* slot_counts);
// msbb_witness_derive_multiplicities (bb_multiplicity.hip): the derived columns of the target slots written from the demand of
// all other messages; entries / args_out as for the balance. One host wait, a second one for the entries when demand is unserved
void witness_derive_multiplicities(BSystem& sys, BWitness& wit, const ms_mult_target* targets, size_t n_targets, u64 summary[MS_DM_SUMMARY_WORDS],
                                   u64* entries, size_t entries_cap, u32* args_out, size_t args_cap);
void multiplicity_slot(const BCircuit& c, size_t slot, u64 out3[3]);  // msbb_system_multiplicity_slot: [eligibility, column, pull]
// msbb_witness_fill (bb_fill.hip): the columns of one circuit that a fill program assigns, evaluated for every row of the
// column-major Montgomery trace; inputs nullable when the program reads none. One host wait when inputs are read, none otherwise
void witness_fill(BSystem& sys, BWitness& wit, size_t circuit, const uint8_t* program, size_t program_len, const ms_dev_matrix* inputs,
                  void* producer_stream, u64 summary[4]);
void fill_program_info(const uint8_t* program, size_t program_len, u64 out4[4]);  // host only: [instructions, slots, LDS lanes, assigned columns]
// msbb_fill_scan_info: host only - [scan steps, launches of the fill kernel, scans in the additive form, rows per scan tile]
void fill_scan_info(const uint8_t* program, size_t program_len, u64 out4[4]);
// msbb_witness_claims_fill (bb_fill.hip): the claims a claim program emits for the first `rows` rows of circuit `ci`, in place of the
// witness's claims or behind them; the traces are not written. At most two host waits; any error leaves the witness as it was
void witness_claims_fill(BSystem& sys, BWitness& wit, size_t ci, const uint8_t* program, size_t program_len, size_t rows, const ms_dev_matrix* inputs,
                         void* producer_stream, uint32_t mode, u64 summary[4]);
// msbb_claims_program_info: host only - [instructions, live slots, lanes of the LDS form (0: global scratch), W | has_keep << 32]
void claims_program_info(const uint8_t* program, size_t program_len, u64 out4[4]);
// msbb_witness_argsort (bb_argsort.hip): the stable sorting permutation of circuit `ci`'s rows under the key columns, cells compared
// as canonical values (or its inverse, what = 1), written into main column dst as Montgomery words. One host wait: the digit histograms
void witness_argsort(BSystem& sys, BWitness& wit, size_t ci, const uint32_t* key_columns, size_t n_keys, uint32_t dst, uint32_t what,
                     u64 summary[4]);
void sort_info(u64 out4[4]);  // host only: [rows per tile, bits per digit, per-tile counts per round of the offsets step, largest n_keys]
// MerkleTreeMmcs::verify_batch for many openings of one commitment, one device thread per opening; everything canonical
void mmcs_verify_batch_device(Ctx& ctx, const Poseidon2* d_perm, const std::vector<size_t>& heights, const std::vector<size_t>& widths,
                              const u32* cap, unsigned cap_height, size_t n_openings, const u64* indices, const u32* vals, const u32* siblings,
                              uint8_t* ok_out);

}  // namespace msbb
