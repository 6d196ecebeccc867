// Host side of the prover: Fiat-Shamir challenger, System / ProverKey / SystemWitness mirrors and prove().
// Mirrors the reference's host orchestration (src/prover.rs:290-603, src/system.rs, src/types.rs) in C++ because
// no Rust toolchain exists in this environment; all heavy steps are launches into the kernels of msamd.h.
#pragma once
#include <memory>
#include <vector>

#include "../../include/mstark.h"
#include "b3_dev.h"
#include "msamd.h"
#include "program.h"

namespace msamd {

// ---- BLAKE3 on the host (challenger, grinding)
void blake3_host(const uint8_t* in, size_t len, uint8_t out[32]);
std::string last_error_text();  // the calling thread's ms_last_error() text (capi.hip)

// DeterministicPow<SerializingChallenger64<Goldilocks, HashChallenger<u8, Blake3, 32>>>, src/types.rs:28-81
struct Challenger {
  std::vector<uint8_t> input, output;
  explicit Challenger(const std::vector<uint8_t>& seed) : input(seed) {}
  void observe_bytes(const uint8_t* p, size_t n) {
    output.clear();
    input.insert(input.end(), p, p + n);
  }
  void observe(u64 v) {
    uint8_t b[8];
    for (int k = 0; k < 8; k++) b[k] = (uint8_t)(v >> (8 * k));
    observe_bytes(b, 8);
  }
  void observe_ext(E2 e) {
    observe(e.c0);
    observe(e.c1);
  }
  void observe_cap(const std::vector<Digest>& cap) {
    for (auto& d : cap) observe_bytes(d.b, 32);
  }
  // replace "hash(input_buffer)" by a digest computed elsewhere (device) for the pending flush
  void flush_with(const Digest& d) {
    input.assign(d.b, d.b + 32);
    output.assign(d.b, d.b + 32);
  }
  uint8_t sample_byte();
  u64 sample_u64();
  u64 sample_base();
  E2 sample_ext();
  size_t sample_bits(unsigned bits);
  u64 grind(unsigned bits);
  bool check_witness(unsigned bits, u64 w) {
    if (bits == 0) return true;  // DeterministicPow: nothing is observed at zero bits (src/types.rs:75-80)
    if (w >= GL_P) return false;
    observe(w);
    return sample_bits(bits) == 0;
  }
};

struct Params {
  u64 log_blowup = 1, cap_height = 0, log_final_poly_len = 0, max_log_arity = 1, num_queries = 1, commit_pow_bits = 0,
      query_pow_bits = 0;
};

struct HCircuit {
  std::vector<PNode> nodes;
  std::vector<uint32_t> degrees, zeros;
  std::vector<std::pair<uint32_t, std::vector<uint32_t>>> lookups;
  size_t main_width = 0, pre_width = 0, pre_height = 0, num_lookups = 0, stage2_width = 0, constraint_count = 0,
         max_constraint_degree = 0, args_width = 0, lookup_prefix_len = 0;
  std::vector<u64> preprocessed;  // row-major
  DBuf<u64> d_preprocessed;       // same, on the device (witness preparation)
  DProgram prog;
  DProgram prefix_prog;           // lookup-expression prefix only (SystemWitness::from_stage_1)
  JitKernel stage2_jit;           // stage-2 terms kernel specialised to this circuit's lookups (quotient_jit.hip)
  JitKernel stage2_trace_jit;     // the same fed by the trace: lookup expressions evaluated in the kernel (host-resident witnesses)
  bool prefix_on_device = false;
  size_t quotient_degree() const {
    size_t d = (max_constraint_degree > 2 ? max_constraint_degree : 2) - 1, q = 1;
    while (q < d) q <<= 1;
    return q;
  }
};

// ProverData of one commitment: bit-reversed LDEs (column-major) + Merkle tree
struct PcsData {
  std::vector<DMat> ldes;
  DTree tree;
};

struct HSystem {
  Ctx* ctx = nullptr;
  Params params;
  std::vector<HCircuit> circuits;
  bool has_pre = false;
  std::vector<Digest> pre_commit;
  std::vector<int> pre_indices;
  PcsData pre_data;
  std::vector<uint8_t> seed;
};
std::unique_ptr<HSystem> system_from_blob(Ctx& ctx, const uint8_t* blob, size_t len);

struct HWitness {
  HSystem* sys = nullptr;
  std::vector<size_t> heights;
  std::vector<DBuf<u64>> traces;  // row-major on device, as uploaded (empty for circuits another rank computes)
  bool has_remote = false;        // some active circuit has no trace here: only prove_sharded accepts the witness
  std::vector<DLookups> lookups;
  // claims: host copy (transcript for small inputs) and device copy
  std::vector<u64> claim_offsets, claim_data;
  // A rank of a joint proof may hold only the part of the claims' data it reads (ms_witness_create_host_sliced): claim_data
  // then holds elements [claim_elem0, claim_elem0 + claim_data.size()) of claim_elems_total, claim_head the first 130 (chunk 0
  // of the claims transcript is hashed by every rank); the offsets are always complete.
  size_t claim_elem0 = 0, claim_elems_total = 0;
  std::vector<u64> claim_head;
  bool claims_partial = false;
  DBuf<u64> d_claim_offsets, d_claim_data;
  // host-resident witness (ms_witness_create_host): between proofs nothing of it lives in HBM. prove() uploads the
  // traces and the claims on the context's copy stream and runs from_stage_1 on the device, every time.
  bool host_resident = false;
  std::vector<const u64*> h_traces;                 // the caller's row-major buffers (pinned by hipHostRegister)
  std::vector<std::vector<u64>> h_mult, h_args;     // only for circuits whose lookup prefix needs the host sweep
  std::vector<void*> registered;                    // ranges this witness pinned; unpinned by the destructor
  // Narrow upload. STARK traces are mostly bytes, bits and small limbs held in 64-bit words, and the upload is the largest
  // single item of a host-resident proof (117 MB at 57 GB/s: 2.1 ms of 8.5). When every value of a trace fits 1 / 2 / 4
  // bytes (found by the validation pass at creation), prove() narrows the trace on host threads - chunk by chunk, range-
  // checked again, each chunk uploaded as soon as it is complete - and widens it on the device. A value that no longer
  // fits (the caller may rewrite its buffers between proofs) sends that proof down the plain path.
  std::vector<unsigned> pack_bytes;                 // per circuit: 0 = upload the 64-bit words as they are
  std::vector<uint8_t*> h_packed;                   // pinned staging for the narrowed rows (h * width * pack_bytes)
  // One upload of the witness: the device buffers and the events that mark their arrival. `next` is filled while a proof
  // runs when prefetching is on (ms_witness_prefetch): the following proof then finds its inputs already in HBM.
  struct Staged {
    bool valid = false, has_host_lookups = false;
    std::vector<DBuf<u64>> traces, mult, args;
    DBuf<u64> claim_offsets, claim_data;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};  // traces, host lookup values, claims
    void clear() {
      valid = false;
      traces.clear();
      mult.clear();
      args.clear();
      claim_offsets.reset();
      claim_data.reset();
    }
  };
  Staged stage[2];
  int cur = 0;             // stage[cur] feeds the running proof, stage[cur ^ 1] is the prefetched one
  bool prefetch = false;
  bool pinned = true;                               // every uploaded range is page-locked
  void pin(const void* p, size_t bytes);
  HWitness() {}
  HWitness(const HWitness&) = delete;
  HWitness& operator=(const HWitness&) = delete;
  ~HWitness();
};
// data_first / data_count: claim_data holds the elements [data_first, data_first + data_count) only (a joint proof's rank:
// claims_slice_range) and head the first min(total, 130) elements; data_count = ~0: claim_data is complete
std::unique_ptr<HWitness> witness_create_host(HSystem& sys, const u64* const* traces, const u64* heights, size_t n_claims,
                                              const u64* claim_offsets, const u64* claim_data, size_t data_first = 0,
                                              size_t data_count = ~size_t(0), const u64* head = nullptr, size_t n_head = 0);
void claims_slice_range(const HSystem& sys, const size_t* heights, size_t n_claims, const u64* offsets, size_t rank, size_t world, size_t& first,
                        size_t& count);
std::unique_ptr<HWitness> witness_create(HSystem& sys, const u64* const* traces, const u64* heights, const u64* const* mult,
                                         const u64* const* args, size_t n_claims, const u64* claim_offsets,
                                         const u64* claim_data);

// traces / claims already resident in HBM (from_stage_1 on the device); and the bench workload generated there.
// ready (optional, one entry per circuit): LookupValues the generator already holds in HBM (mult: h x num_lookups, args:
// h x args_width, as host_lookup_values lays them out); a circuit with an entry takes it as it is, the others run from_stage_1
struct ReadyLookups {
  DBuf<u64> mult, args;
};
std::unique_ptr<HWitness> witness_from_device(HSystem& sys, std::vector<DBuf<u64>>&& traces, const std::vector<size_t>& heights,
                                              DBuf<u64>&& d_claim_offsets, DBuf<u64>&& d_claim_data, size_t n_claims, size_t claim_elems,
                                              std::vector<ReadyLookups>* ready = nullptr);
// ms_witness_create_device: the caller's traces (strided views of 1 / 2 / 4 / 8-byte elements) and, optionally, its claims lie in
// device memory; they are checked and copied by the ingest kernels (ingest.hip) and handed to witness_from_device
std::unique_ptr<HWitness> witness_create_device(HSystem& sys, const ms_dev_matrix* traces, size_t n_claims, const u64* claim_offsets,
                                                const u64* claim_data, bool claims_on_device, void* producer_stream);
std::unique_ptr<HWitness> witness_u32_add_bench(HSystem& sys, size_t num_adds, u32 a0, u32 b0);
// Blake3CompressionClaims::witness for the nine-circuit BLAKE3 system (witness_gen.hip); states_out nullable
std::unique_ptr<HWitness> witness_blake3_compressions(HSystem& sys, size_t n, const u32* states_in, u32* states_out);
// every compression of BLAKE3(data) as 32-word rows (host code); returns the number of rows, of which min(n, cap_rows) are written
size_t blake3_compression_states(const uint8_t* data, size_t len, u32* states_in, size_t cap_rows, uint8_t* digest32);

struct StageMs {
  double v[6] = {0, 0, 0, 0, 0, 0};
};
std::vector<uint8_t> prove(HSystem& sys, HWitness& w, StageMs* times);
typedef ms_comm ms_comm_t;
// the same proof computed by `comm->world` ranks (prover_sharded.inc)
std::vector<uint8_t> prove_sharded(HSystem& sys, HWitness& w, const ms_comm_t* comm, const int32_t* owners, StageMs* times);

// System::verify_multiple_claims (verifier.hip): 0 = accepted, otherwise the VerificationError code of include/mstark.h
int verify(HSystem& sys, size_t n_claims, const u64* claim_offsets, const u64* claim_data, const uint8_t* proof, size_t proof_len);

// the same for n_proofs proofs of one system with the per-query arithmetic and every Merkle path on the device (verifier.hip,
// verify_dev.hip): verdicts[i] is what verify() returns for proof i
void verify_batch(HSystem& sys, size_t n_proofs, const u64* n_claims, const u64* const* claim_offsets, const u64* const* claim_data,
                  const uint8_t* const* proofs, const u64* proof_lens, int32_t* verdicts);
// MerkleTreeMmcs::verify_batch for many openings of one commitment, one device thread per opening
void mmcs_verify_batch_device(Ctx& ctx, const std::vector<size_t>& heights, const std::vector<size_t>& widths, const uint8_t* cap,
                              unsigned cap_height, size_t n_openings, const u64* indices, const u64* vals, const uint8_t* siblings,
                              uint8_t* ok_out);

// Pcs::open / Pcs::verify on their own (prover.hip, verifier.hip)
void pcs_open_standalone(Ctx& ctx, const Params& prm, const std::vector<PcsData*>& data, const std::vector<std::vector<std::vector<E2>>>& points,
                         Challenger& ch, std::vector<E2>& opened_flat, std::vector<uint8_t>& fri_bytes);
bool pcs_verify_standalone(const Params& prm, const std::vector<std::vector<Digest>>& commits, const std::vector<std::vector<unsigned>>& log_n,
                           const std::vector<std::vector<size_t>>& widths, const std::vector<std::vector<std::vector<E2>>>& points,
                           const std::vector<E2>& opened_flat, const uint8_t* fri, size_t fri_len, Challenger& ch);

void commit_matrices(Ctx& ctx, std::vector<DMat>&& ldes, unsigned cap_height, PcsData& out);
// LookupValues::stage_2_traces of one circuit (src/lookup.rs:472-555): from the witness's lookup values, or - when the witness
// holds none for this circuit - straight from its trace with the circuit's fused kernel. Launches only; the circuit's
// total is left in *total_dev.
void stage2_circuit_async(Ctx& ctx, const HSystem& sys, const HWitness& wit, size_t ci, E2 beta, E2 gamma, u64* out_colmajor_bitrev,
                          E2* total_dev);
// the claims part of the transcript (src/prover.rs:369-373) for a device-resident witness: long lists are hashed on the device
void observe_claims(Ctx& ctx, Challenger& ch, HWitness& wit);
// ms_witness_check (check.hip): the user constraint roots of every active circuit on the trace domain + the lookup balance under
// (beta, gamma). circuits: C x MS_CHECK_CIRCUIT_WORDS; root_counts / root_first (nullable): one entry per root, circuit after circuit
void witness_check(HSystem& sys, HWitness& wit, E2 beta, E2 gamma, uint32_t* verdict, u64* circuits, u64* root_counts, u64* root_first);
size_t check_roots(const HCircuit& c);          // constraint_count - 2 max(num_lookups, 1), checked against HCircuit::zeros
unsigned check_lds_lanes(size_t n_slots);       // lanes per workgroup of the check's LDS tier (0: the slot file does not fit)
// ms_witness_lookup_balance (balance.hip): the witness's messages grouped by tuple, exactly; slot_counts (nullable) has
// lookup_balance_slots(sys) + 1 words. One host wait, a second one for the entries when some group is unbalanced
void witness_lookup_balance(HSystem& sys, HWitness& wit, u64 summary[4], u64* entries, size_t entries_cap, u64* args_out, size_t args_cap,
                            u64* slot_counts);
size_t lookup_balance_slots(const HSystem& sys);  // sum of num_lookups over every circuit of the system
// ms_witness_derive_multiplicities (multiplicity.hip): the derived columns of the target slots written from the demand of all
// other messages; entries / args_out as for the balance. One host wait, a second one for the entries when demand is unserved
void witness_derive_multiplicities(HSystem& sys, HWitness& wit, const ms_mult_target* targets, size_t n_targets, u64 summary[MS_DM_SUMMARY_WORDS],
                                   u64* entries, size_t entries_cap, u64* args_out, size_t args_cap);
void multiplicity_slot(const HCircuit& c, size_t slot, u64 out3[3]);  // ms_system_multiplicity_slot: [eligibility, column, pull]
// ms_witness_fill (fill.hip): the columns a fill program assigns, evaluated for every row of circuit `ci` on the device; held
// lookup values of the circuit follow. One host wait when the program reads inputs (their offender word), none otherwise
void witness_fill(HSystem& sys, HWitness& wit, size_t ci, const uint8_t* program, size_t program_len, const ms_dev_matrix* inputs,
                  void* producer_stream, u64 summary[4]);
// ms_fill_program_info: host only - [instructions, live slots, lanes of the LDS form (0: global scratch), assigned columns]
void fill_program_info(const uint8_t* program, size_t program_len, u64 out4[4]);
// ms_fill_scan_info: host only - [scan steps, launches of the fill kernel, scans in the additive form, rows per scan tile]
void fill_scan_info(const uint8_t* program, size_t program_len, u64 out4[4]);
// ms_fill_peer_info: host only - the peer records [circuit, trace, width] into out (written when they fit cap) -> their number
size_t fill_peer_info(const uint8_t* program, size_t program_len, u64* out, size_t cap);
// ms_witness_claims_fill (fill.hip): the claims a claim program emits for the first `rows` rows of circuit `ci`, in place of the
// witness's claims or behind them. At most two host waits: the inputs' offender word with the kept total, and the host copy
void witness_claims_fill(HSystem& sys, HWitness& wit, size_t ci, const uint8_t* program, size_t program_len, size_t rows, const ms_dev_matrix* inputs,
                         void* producer_stream, uint32_t mode, u64 summary[4]);
// ms_claims_program_info: host only - [instructions, live slots, lanes of the LDS form (0: global scratch), W | has_keep << 32]
void claims_program_info(const uint8_t* program, size_t program_len, u64 out4[4]);
// ms_witness_argsort (argsort.hip): the stable sorting permutation of circuit `ci`'s rows under the key columns (or its inverse,
// what = 1) written into main column dst; held lookup values of the circuit follow. One host wait: the digit histograms
void witness_argsort(HSystem& sys, HWitness& wit, size_t ci, const uint32_t* key_columns, size_t n_keys, uint32_t dst, uint32_t what,
                     u64 summary[4]);
// ms_sort_info: host only - [rows per tile, bits per digit, per-tile counts per round of the offsets step, largest n_keys]
void sort_info(u64 out4[4]);
void field_op(Ctx& ctx, int op, const u64* a, const u64* b, size_t n, u64* out);

}  // namespace msamd
