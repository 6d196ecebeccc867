/* mstark.h — C ABI of the MI355X (gfx950) prover for multi-stark's GoldilocksBlake3Config hot path.
 *
 * Every entry point is `extern "C"`, takes plain pointers and sizes, returns an int32 status (0 = ok, <0 = error,
 * text via ms_last_error()) and never unwinds across the boundary: the reference's panics/asserts
 * (src/prover.rs:323-326,522-525,637-641; src/system.rs:149,171-178,249-264) become error codes.
 *
 * Data conventions: Goldilocks elements are canonical u64 (little-endian on the wire); an Ext2
 * value is two consecutive u64 (c0, c1) — the layout `flatten_to_base` produces (src/prover.rs:417,495);
 * matrices cross the ABI row-major (what `RowMajorMatrix.values` holds); digests are 32 raw bytes.
 * The caller owns every host buffer for the duration of a call; the library owns device memory behind the
 * opaque handles below. A ms_ctx is bound to one HIP device and is not thread-safe. Handles may be destroyed in any
 * order: a system keeps its context alive, a witness its system, an mmcs its context (the memory is released when the
 * last dependent handle is destroyed).
 *
 * Threads: one ms_ctx (with its systems and witnesses) is driven by one thread at a time. Several contexts, of one device or of
 * several, each driven by its own host thread, are independent of each other - in this configuration and in the BabyBear /
 * Poseidon2 one (mstark_bb.h) alike; ms_last_error() is per thread. Contexts of one device share, behind locks of the
 * library's own: the BabyBear twiddle tables (per device and size; a table is published only once it has been filled), the
 * hiprtc code objects of the generated circuit kernels and their disk cache (per process), the pool of host threads that
 * narrows host-resident traces (per device, one job at a time), the page-lock counts of caller memory handed to
 * ms_witness_create_host / msbb_witness_create_host (per range: two contexts may be given the same buffers), and the per-device
 * Poseidon2 permutation of the BabyBear PCS-level calls. The last one is the exception to the independence:
 * msbb_set_poseidon2 must not be called while another context of that device is inside a PCS-level msbb_* call.
 *
 * What each group replaces in /root/reference:
 *   ms_system_*    System::new + ProverKey                      src/system.rs:115-203 (preprocessed commit :190-195)
 *   ms_witness_*   SystemWitness / from_stage_1                 src/system.rs:225-328 (host-resident: the witness argument
 *                                                               of prove(), src/prover.rs:290-295)
 *   ms_prove       System::prove_multiple_claims                src/prover.rs:290-603
 *   ms_verify      System::verify_multiple_claims               src/verifier.rs:208-532
 *   ms_prove_sharded   the same proof computed by several GPUs  src/prover.rs:290-603 (commit/open calls :350,419,526,580)
 *   ms_comm_rccl_*     its transport on RCCL (the reference has no collectives: Cargo.toml has no MPI / NCCL crate)
 *   ms_comm_local_*    its transport between threads of one process (peer copies; the reference's own process model)
 *   ms_dft_batch   Radix2DitParallel::dft_batch                 src/prover.rs:650,716 (type fixed at :440)
 *   ms_coset_lde_batch  the LDE inside Pcs::commit              src/prover.rs:350,419; layout pinned by :975-999
 *   ms_quotient_lde     shifted_quotient_slices + lde_from_shifted_coefficients   src/prover.rs:631-717
 *   ms_mmcs_*      MerkleTreeMmcs commit / open_batch           src/types.rs:82-83,202-207; Pcs::commit_ldes src/prover.rs:526
 *   ms_stage2_trace     LookupValues::stage_2_traces            src/lookup.rs:472-555
 *   ms_claims_accumulator   the claims loop                     src/prover.rs:382-387
 *   ms_quotient_values      quotient_values(+_inner)            src/prover.rs:756-962 (sweep: src/eval.rs:67-106;
 *                                                               logUp: src/lookup.rs:152-256)
 *   ms_pcs_commit / ms_pcs_open / ms_pcs_verify / ms_challenger_*   Pcs::commit / open / verify with the transcript as a handle
 *                                                               src/prover.rs:350,419,580; examples/pcs_example.rs:64-121
 *   ms_blake3      Blake3 as used by the challenger             src/types.rs:28-29 (HashChallenger<u8,Blake3,32>)
 */
#ifndef MSTARK_H
#define MSTARK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ms_ctx ms_ctx;         /* one HIP device + stream + twiddle tables + memory pool */
typedef struct ms_system ms_system;   /* System<GoldilocksBlake3Config> + ProverKey (device-resident preprocessed LDE/tree) */
typedef struct ms_witness ms_witness; /* SystemWitness + claims, resident in HBM */
typedef struct ms_mmcs ms_mmcs;       /* ProverData of one commitment */

enum {
  MS_OK = 0,
  MS_ERR = -1,            /* generic failure, see ms_last_error() */
  MS_ERR_NO_DEVICE = -2,  /* no HIP device / HIP runtime failure at context creation */
  MS_ERR_BUFFER = -3      /* caller-provided capacity too small; the needed size is reported */
};

const char* ms_last_error(void);

/* ---- context */
/* HIP devices visible to this process (0 when there is none or no driver); never an error. A host that spreads one proof
 * over N devices (ms_prove_sharded with ms_comm_local_*) checks this first instead of running on fewer. */
int32_t ms_device_count(void);
int32_t ms_ctx_create(int32_t device, ms_ctx** out);
void ms_ctx_destroy(ms_ctx* ctx);
int32_t ms_ctx_sync(ms_ctx* ctx);
/* Diagnostics: how often the host has waited for the context's stream since the context was created (every read-back that a
 * proof needs on the host before it can go on, ms_ctx_sync itself included). A proof's count is the difference around it:
 * two for ms_prove at the bench size (opened values, FRI), and the joint prover is held to that plus two. */
int32_t ms_ctx_sync_count(ms_ctx* ctx, uint64_t* out);
/* release pooled device memory back to the driver */
int32_t ms_ctx_trim(ms_ctx* ctx);
/* Per-kernel-class timing with HIP events on the library's stream. mask bit i enables class i. */
int32_t ms_ctx_set_profile_mask(ms_ctx* ctx, uint32_t mask);
int32_t ms_ctx_kernel_stats(ms_ctx* ctx, int32_t kernel_id, uint64_t* launches, double* ms, double* alg_bytes);
/* work items other than bytes recorded for a class (Poseidon2 permutations of the hash classes on the BabyBear path) */
int32_t ms_ctx_kernel_units(ms_ctx* ctx, int32_t kernel_id, double* units);
int32_t ms_ctx_reset_stats(ms_ctx* ctx);
/* Diagnostics: the nth device allocation from now fails (0 = off). Lets a test check that an error in the middle of a
 * proof leaves the library usable (queued read-backs dropped, pool intact). It serves the calls that make, fill, sort, check
 * and verify as well: each of them says below what an allocation failure leaves behind - the witness as it was before the
 * call, or no witness - and the same call may be made again. */
int32_t ms_ctx_debug_fail_alloc(ms_ctx* ctx, int32_t nth);
int32_t ms_kernel_count(void);
const char* ms_kernel_name(int32_t kernel_id);

/* ---- System::new (src/system.rs:115-203). `blob` is the front-end's system blob: params, then per circuit the
 * compiled node program (graph::ConstraintGraph fields, src/graph.rs:62-76), lookups and preprocessed trace.
 * FriParameters::max_log_arity (src/types.rs:189-190,215) may be 1 .. 6: a commit-phase round folds 2^a values per row, a as
 * large as max_log_arity allows without stepping over the next input's height or below the final height; a row of 2^a
 * extension values is one leaf (at most one BLAKE3 chunk, hence 6). Every config, example and bench of the reference
 * sets 1 (benches/multi_stark.rs:252, examples/simple_proof.rs:54, pcs_example.rs:39, ...), which is the path the
 * device-side transcript and the fused round kernels serve; wider rounds are driven from the host (one synchronisation
 * per round). ms_system_create, ms_pcs_open and ms_pcs_verify (and their msbb_ counterparts) refuse other values with
 * an error code. */
int32_t ms_system_create(ms_ctx* ctx, const uint8_t* blob, size_t len, ms_system** out);
void ms_system_destroy(ms_system* sys);
/* preprocessed commitment (System.preprocessed_commit): writes n_digests * 32 bytes; n_digests = 0 if none */
int32_t ms_system_preprocessed_commit(const ms_system* sys, uint8_t* out, size_t cap, size_t* n_digests);
/* [main_width, pre_width, pre_height, num_lookups, stage2_width, constraint_count, max_constraint_degree,
 *  quotient_degree, args_width] */
int32_t ms_system_circuit_info(const ms_system* sys, size_t circuit, uint64_t out9[9]);
/* Diagnostics: which of the circuit's kernels were generated and compiled at ms_system_create (hiprtc; a circuit without
 * one runs the generic interpreter kernels and produces the same bytes). *flags = a mask of MS_KERNEL_*; 0 when nothing was
 * compiled (no hiprtc, MSAMD_NO_JIT=1, a program over the size limits). The group count G of a grouped stage-2 terms
 * kernel (one wave per 16 lookups) is (*flags >> MS_KERNEL_STAGE2_GROUPS_SHIFT) & MS_KERNEL_STAGE2_GROUPS_MASK. */
#define MS_KERNEL_QUOTIENT 0x1u         /* quotient kernel compiled */
#define MS_KERNEL_QUOTIENT_INLINE 0x2u  /* ... and it reads the Z_H tables from the argument block */
#define MS_KERNEL_STAGE2 0x4u           /* stage-2 terms kernel (fed by lookup values) compiled */
#define MS_KERNEL_STAGE2_GROUPED 0x8u   /* ... in grouped form: G waves per 64 rows */
#define MS_KERNEL_STAGE2_TRACE 0x10u    /* stage-2 terms kernel fed by the trace (host-resident witnesses) compiled */
#define MS_KERNEL_STAGE2_GROUPS_SHIFT 8
#define MS_KERNEL_STAGE2_GROUPS_MASK 0x1fu
int32_t ms_system_circuit_kernels(const ms_system* sys, size_t circuit, uint32_t* flags);

/* ---- SystemWitness (src/system.rs:225-233) + claims. traces[i]: heights[i] x main_width_i row-major (height 0 =
 * inactive circuit). mult[i] / args[i]: the flat LookupValues storage (src/lookup.rs:392-405); pass mult = NULL
 * to have the library run SystemWitness::from_stage_1 (src/system.rs:244-328) on the host. Claims are given as
 * offsets (n_claims + 1) into claim_data. Everything is uploaded once; ms_prove does not consume it. After an allocation
 * failure (MS_ERR) of this or any other call that makes a witness - ms_witness_create_device, ms_witness_u32_add_bench,
 * ms_witness_blake3_compressions - there is no witness, *out is not written, the caller's buffers are as they were and no
 * longer read, the context and the system stay usable, and the call may be made again. */
int32_t ms_witness_create(ms_system* sys, const uint64_t* const* traces, const uint64_t* heights,
                          const uint64_t* const* mult, const uint64_t* const* args, size_t n_claims,
                          const uint64_t* claim_offsets, const uint64_t* claim_data, ms_witness** out);
/* A SystemWitness that STAYS in host memory, which is what the reference's prove() is handed (src/prover.rs:290-295;
 * criterion builds it in the setup closure, benches/multi_stark.rs:292-296). Nothing is uploaded here: the values are
 * validated and the caller's trace buffers are page-locked (hipHostRegister; *pinned = 1 when every range could be, else
 * the uploads of this witness go through a page-locked bounce buffer of the context - no asynchronous copy ever reads
 * pageable caller memory). The locks are counted per range process-wide: several witnesses may be made from the same
 * buffers, the range stays locked until the last of them is destroyed; a range the application has registered itself is
 * left alone. The trace buffers must stay valid and unchanged until ms_witness_destroy, which waits for the context's
 * streams before it gives the locks up. Every
 * ms_prove on such a witness moves traces and claims to HBM on a copy stream (claims travel while stage 1 is computed),
 * runs SystemWitness::from_stage_1 (src/system.rs:244-328) on the device and frees the device copies again, so its
 * wall time is the reference's timed region: witness in host memory at the start, proof bytes in host memory at the end.
 * Narrow upload: a trace of at least 4 MB whose values all fit 1 / 2 / 4 bytes (seen by the validation pass here) is not
 * sent as 64-bit words: every ms_prove narrows it on a pool of host threads (16 by default), checking the range again, uploads the narrowed chunks as they complete and widens them on the device - at the
 * bench size 15 MB instead of 117 MB cross PCIe, in 0.5 ms instead of 2.1. A value that no longer fits sends that proof
 * down the plain path. Environment: MSAMD_NO_PACK=1 (read here) never narrows; MSAMD_PACK_THREADS=n (0: off),
 * MSAMD_PACK_MIN_BYTES, MSAMD_PACK_CHUNKS tune it. */
int32_t ms_witness_create_host(ms_system* sys, const uint64_t* const* traces, const uint64_t* heights, size_t n_claims,
                               const uint64_t* claim_offsets, const uint64_t* claim_data, int32_t* pinned /* nullable */,
                               ms_witness** out);
/* Proving in a stream (a prover service proves one witness after another): with on = 1 every ms_prove of this host-resident
 * witness also queues the upload for the NEXT ms_prove of it, into a second set of device buffers, behind its own; that
 * upload travels over PCIe while the current proof is computed, and the next ms_prove starts with its inputs in HBM. The
 * first proof after switching on still uploads by itself; the last prefetch is unused; on = 0 drops a pending one. (The
 * host buffers are fixed for the life of the witness anyway, see ms_witness_create_host.) bench.py reports this mode as
 * config.pipelined_ms_per_proof, never as the primary figure (whose every step starts with the witness in host memory). */
int32_t ms_witness_prefetch(ms_witness* w, int32_t on);
/* A SystemWitness whose stage-1 traces the CALLER holds in DEVICE memory - written there by its own kernels, by tensor
 * operations or by another library. Nothing crosses PCIe: one launch per circuit reads the caller's matrix through its strides,
 * checks every element against the field modulus and writes the witness's own copy; SystemWitness::from_stage_1 runs on the
 * device. traces: one ms_dev_matrix per circuit; the width is the circuit's main_width; element (r, c) lies at
 * ptr + (r * row_stride + c * col_stride) * elem_bytes and is an unsigned little-endian integer of elem_bytes bytes (row-major:
 * strides (width, 1); column-major: (1, height); a column slice or padded rows: row_stride > width; every k-th row: row_stride =
 * k * width). Only elements of the view are read or judged, never the padding between them.
 *   Copy, not adoption: when the call returns - with any status - the library has finished reading the caller's buffers (traces
 * and claims); they may be freed or overwritten. The result is an ordinary device-resident ms_witness: ms_prove,
 * ms_witness_trace and the Level-2 calls (ms_witness_commit_stage1, ms_challenger_observe_claims, ms_stage2_build, ...) accept
 * it. Circuits held by other ranks (ms_prove_sharded) cannot be expressed: a NULL pointer with height > 0 is MS_ERR.
 *   Two limits. from_stage_1 must be able to run on the device: a circuit with lookups that has neither a generated stage-2
 * kernel fed by the trace (MS_KERNEL_STAGE2_TRACE) nor a lookup prefix small enough for the device sweep is MS_ERR ("lookup
 * prefix does not fit the device sweep"; ms_witness_create runs such a prefix on the host). And the memory must be an
 * allocation the runtime can bound (hipMalloc and what tensor libraries carve out of it): a pointer for which
 * hipMemGetAddressRange reports no base and size - virtual-memory mappings or stream-ordered pools on some runtimes - is
 * refused rather than read unchecked.
 *   Stream ordering: with producer_stream != NULL (a hipStream_t) the library records an event on that stream and makes its own
 * stream wait for it before the first read, so the caller need not synchronise after queuing the work that fills the buffers.
 * With NULL the caller has already made the data visible (or filled them on the null stream, which the library's stream
 * follows).
 *   Host waits: one per call on the traces' path, for the offender words, plus those of from_stage_1 and of the claims.
 *   Refused on the host before anything is launched (MS_ERR, text via ms_last_error()): a pointer that hipPointerGetAttributes
 * does not report as device memory of the context's device (host addresses, other devices), or whose view reaches beyond the
 * allocation hipMemGetAddressRange reports around it; a pointer not aligned to elem_bytes; elem_bytes outside {1, 2, 4, 8}; a stride <= 0; height, width and strides
 * whose product overflows; a height that is not a power of two or above the supported maximum; a height other than the
 * circuit's preprocessed height; a NULL pointer with height > 0.
 *   A value >= p (only 8-byte elements can be): MS_ERR naming the first offender in row-major order, e.g.
 * "non-canonical trace value: circuit 1, row 5, column 3". The context stays usable.
 *   Claims: with claims_on_device = 0 host arrays exactly as for ms_witness_create; with 1 both are device pointers to u64
 * (same device, 8-byte aligned), read behind producer_stream as well. Either way offsets start at 0 and do not decrease and
 * the data are canonical, else MS_ERR. */
typedef struct ms_dev_matrix {      /* one trace in device memory of the system's context's device */
  const void* ptr;                  /* NULL only with height 0 (inactive circuit) */
  uint64_t height;                  /* rows; width is the circuit's main_width */
  uint32_t elem_bytes;              /* 1, 2, 4, 8: unsigned little-endian */
  int64_t row_stride, col_stride;   /* in elements; both > 0 */
} ms_dev_matrix;
int32_t ms_witness_create_device(ms_system* sys, const ms_dev_matrix* traces /* one per circuit */, size_t n_claims,
                                 const uint64_t* claim_offsets, const uint64_t* claim_data, int32_t claims_on_device,
                                 void* producer_stream /* hipStream_t, nullable */, ms_witness** out);
/* The bench workload's witness and claims generated in HBM for the system [ByteTable, U32Add]: build_witness +
 * build_claims of benches/multi_stark.rs:171-238 (two xorshift32 streams from a0, b0; the reference uses 0xdeadbeef,
 * 0xcafebabe) followed by from_stage_1 on the device. Nothing crosses PCIe. */
int32_t ms_witness_u32_add_bench(ms_system* sys, size_t num_adds, uint32_t a0, uint32_t b0, ms_witness** out);
/* Blake3CompressionClaims::witness (src/test_circuits/blake3.rs:1511-2213) on the device, for n claims of the compression
 * circuit. states_in: n x 32 words [cv 8 | 4 words | counter lo, hi | block_len | flags | message 16] (any values: the circuit
 * does not constrain words 8..11). The nine stage-1 traces, the claims [9, state_in 32, state_out 16] and from_stage_1 are
 * produced in HBM; only the n x 32 input words cross PCIe. states_out (nullable): n x 16 output words. The system must be
 * the nine-circuit BLAKE3 system (checked by shape); n = 0, or an n whose tallest trace exceeds the supported height: MS_ERR. */
int32_t ms_witness_blake3_compressions(ms_system* sys, size_t n, const uint32_t* states_in, uint32_t* states_out, ms_witness** out);
/* Host code, no device: every compression of BLAKE3(data) in the order of blake3_new_update_finalize (:32-352), as states_in
 * rows for the call above. MS_ERR_BUFFER with *n = needed rows if cap_rows is too small. digest32 nullable. */
int32_t ms_blake3_compressions(const uint8_t* data, size_t len, uint32_t* states_in, size_t cap_rows, size_t* n, uint8_t* digest32);
/* Diagnostics: read back one stage-1 trace (height x main_width, row-major) of a device-resident witness.
 * MS_ERR_BUFFER with *n_words = needed size. Host-resident witnesses: MS_ERR. */
int32_t ms_witness_trace(ms_witness* w, size_t circuit, uint64_t* out, size_t cap_words, size_t* n_words);
void ms_witness_destroy(ms_witness* w);

/* ---- Witness check (what Plonky3 users know as check_constraints), on the device: does this witness satisfy the system, and
 * if not, WHERE not - for the price of one pass over the traces and one stage-2 build instead of a proof (no LDE, no tree, no
 * FRI). Goldilocks / BLAKE3 configuration; the BabyBear counterpart is msbb_witness_check (include/mstark_bb.h).
 *   Definition. For every active circuit (height n > 0) and every row r in [0, n) the circuit's user constraint roots (the
 * `zeros` of its compiled node program, in that order, index k) are evaluated on exactly the values the quotient kernels see on
 * the trace domain at x = w^r, w = the generator of the subgroup of order n: main and preprocessed variables at row r and, for
 * offset 1, at row (r + 1) mod n; the selector POLYNOMIALS at x = w^r with their limits - is_first = n at row 0 (else 0),
 * is_last = n w at row n - 1 (else 0), is_transition = w^r - w^-1 (not 0 / 1 flags); stage-2 columns and publics (read by roots
 * that came from extension constraints) as the prover would build them under the caller's (beta, gamma): running sums that
 * start at zero, publics [beta, gamma, acc_in, acc_out] with the accumulator chained as ms_stage2_build chains it - the claims'
 * accumulator first, then each active circuit's total. A row fails when some root is non-zero there. The logUp constraints hold
 * by construction of stage 2 and are not evaluated; what is checked of the lookups is the verifier's balance: the accumulator
 * behind the last active circuit must be zero. That check is probabilistic in (beta, gamma) in the same sense as the proof is,
 * and a row whose fingerprint makes beta + fingerprint = 0 makes it meaningless (the inverse does not exist): pick other
 * challenges then. Not checked: anything a proof would add beyond this (the constraint degree bound, the claims' shape).
 *   Report. *verdict: a mask of MS_CHECK_CONSTRAINT (some root is non-zero somewhere) and MS_CHECK_LOOKUPS (the accumulator
 * does not return to zero); 0 = the witness satisfies the system. A failed check is MS_OK with a non-zero verdict; MS_ERR is for
 * misuse. circuits: MS_CHECK_CIRCUIT_WORDS words for every circuit of the system, inactive ones included:
 *   [0] height  [1] failing rows  [2] smallest failing row  [3] smallest failing root index at that row  [4] its value
 *   [5] [6] the accumulator behind the circuit (zeros for an inactive circuit)  [7] number of roots  [8] diagnostics: which
 *   kernel form ran (low byte: 1 thread per row / slots in LDS, 2 wave per row, 3 few lanes with large LDS, 4 global scratch,
 *   0 none) and its lanes per workgroup << 8  [9] where this circuit's roots start in root_counts / root_first.
 * [2], [3] are all-ones when no row fails. root_counts / root_first (each nullable, roots_cap entries): per root, circuit after
 * circuit in system order, the number of rows where it is non-zero and the first such row (all-ones when none); MS_ERR_BUFFER
 * when roots_cap is below the system's total (the sum of out4[0] of ms_system_check_info over the circuits). Every figure is deterministic.
 *   Limits and misuse (MS_ERR, text via ms_last_error(), the context stays usable): a host-resident witness
 * (ms_witness_create_host*: its traces are not in HBM between proofs); a witness with circuits held by another rank; beta or
 * gamma with a coordinate >= p. Accepted: every device-resident witness - ms_witness_create, ms_witness_create_device,
 * ms_witness_u32_add_bench, ms_witness_blake3_compressions. The witness is not changed: ms_prove behind a check writes the bytes
 * it writes without one. After an allocation failure (MS_ERR) it is unchanged too, and the next check gives the full report.
 *   Host waits: one, for the report (plus those of the claims' upload paths it shares with ms_stage2_build). */
#define MS_CHECK_CONSTRAINT 0x1u
#define MS_CHECK_LOOKUPS 0x2u
#define MS_CHECK_CIRCUIT_WORDS 10
int32_t ms_witness_check(ms_witness* w, const uint64_t beta[2], const uint64_t gamma[2], uint32_t* verdict,
                         uint64_t* circuits /* n_circuits x MS_CHECK_CIRCUIT_WORDS */, uint64_t* root_counts /* nullable */,
                         uint64_t* root_first /* nullable */, size_t roots_cap);
/* What the check adds to the nine words of ms_system_circuit_info: out4 = [number of user constraint roots =
 * constraint_count - 2 max(num_lookups, 1), live slots of the circuit's node program, steps of its wave-per-row schedule
 * (0: none), lanes per workgroup of the check's thread-per-row form with slots in LDS (0: the slot file does not fit)] */
int32_t ms_system_check_info(const ms_system* sys, size_t circuit, uint64_t out4[4]);

/* ---- Lookup balance, exact, on the device: WHICH messages do not cancel. ms_witness_check says of the lookups one bit
 * (MS_CHECK_LOOKUPS); this call groups every message of the witness by its tuple and names the groups whose multiplicities do
 * not sum to zero, with where they came from. It takes no challenges. Goldilocks / BLAKE3 configuration.
 *   Definition. A message is (a) a claim i: tuple claim_data[off[i] .. off[i + 1]), multiplicity 1 (src/prover.rs:382-387), or
 * (b) a triple (active circuit c, row r, lookup slot j) with the multiplicity and arguments of SystemWitness::from_stage_1
 * (src/system.rs:244-328, src/lookup.rs:392-405). A message of multiplicity 0 (padding rows) does not exist for this check. Two
 * messages belong to the same GROUP when their tuples are equal after trailing zeros are stripped: the fingerprint is a Horner
 * evaluation (src/lookup.rs:373-384,410-414), so (a, b, 0) and (a, b) are one message to the protocol, and so are the empty
 * tuple and (0, 0). A group's NET is the sum of its multiplicities modulo p; a group is UNBALANCED when its net is not 0.
 * Messages are ordered by ORIGIN: claims first, by index; then the circuits in system order, row-major, slot last. A group's
 * FIRST ORIGIN is the smallest origin among its members. The witness is balanced exactly when no group is unbalanced. Balance
 * implies that ms_witness_check reports no MS_CHECK_LOOKUPS under every (beta, gamma) whose messages are invertible; imbalance
 * implies the bit, except with the probability the proof system itself accepts.
 *   Report. summary: [0] messages of non-zero multiplicity  [1] groups  [2] unbalanced groups  [3] entries written =
 * min([2], entries_cap). entries (entries_cap x MS_LB_ENTRY_WORDS words; nullable with entries_cap 0): the unbalanced groups with
 * the smallest first origins, in ascending order of first origin, whatever their total number:
 *   [0] circuit of the first origin (MS_LB_CLAIMS: a claim)  [1] its row (the claim's index)  [2] its lookup slot (0 for a claim)
 *   [3] net, canonical, non-zero  [4] members  [5] length of the stripped tuple  [6] where the tuple starts in args_out; the
 *   tuples are packed in entry order, and [6] is all-ones for a tuple that would end behind args_cap  [7] reserved, 0.
 * args_out (args_cap words; nullable with args_cap 0): the stripped tuples. slot_counts (nullable, slots_cap words): one word per
 * lookup slot of every circuit of the system in system order (inactive circuits: zeros), then one word for the claims - the
 * number of messages from that source that belong to an unbalanced group; MS_ERR_BUFFER when slots_cap is below
 * sum(num_lookups) + 1. Every figure is deterministic: nothing depends on the order in which threads ran, nor on the hash.
 *   An unbalanced witness is MS_OK. MS_ERR (text via ms_last_error(), the context stays usable) is for misuse: a host-resident
 * witness; a witness with circuits (or claims) held by another rank; a null w or summary; a null buffer with a non-zero capacity.
 * A system without lookups and without claims: MS_OK, zeros. The witness is not changed: ms_prove behind the call writes the bytes
 * it writes without it. A circuit whose lookup values the witness does not hold (ms_witness_create_device: its stage 2 reads the
 * trace) has them computed into temporaries of the call; a lookup prefix that does not fit the device sweep is MS_ERR.
 *   Memory: the grouping table takes 40 bytes x cap, cap = the power of two >= max(64, 2 x M), M = claims + sum over the active
 * circuits of height x num_lookups (1.34 GB at 2^20 additions, M = 14 x 2^20), plus M / 8 bytes of marks; an allocation failure
 * is MS_ERR naming the bytes, leaves the witness unchanged, as the call does, and the call may be made again. MSAMD_LB_HASH_BITS=k (diagnostics, read per call) keeps only the low k bits of the hash: with 0
 * every probe sequence starts at slot 0 - the report is the same, by a longer way.
 *   Host waits: one when the witness is balanced; one more, to fetch entries and tuples, when it is not and entries_cap > 0. */
#define MS_LB_ENTRY_WORDS 8
#define MS_LB_CLAIMS (~(uint64_t)0)
int32_t ms_witness_lookup_balance(ms_witness* w, uint64_t summary[4], uint64_t* entries, size_t entries_cap /* nullable with cap 0 */,
                                  uint64_t* args_out, size_t args_cap /* nullable with cap 0 */, uint64_t* slot_counts /* nullable */,
                                  size_t slots_cap);

/* ---- Table multiplicity columns derived on the device. Every lookup system has table circuits with a main-trace column that
 * counts how often each table row is pulled (ByteTable column 0, the four ByteCS columns, RangeTable column 0); witness builders
 * fill it on the host with a histogram of the consumers' messages. For a witness whose traces were produced in HBM
 * (ms_witness_create_device) this call computes those columns there, from all other messages of the witness: the grouping of
 * ms_witness_lookup_balance followed by a write instead of a report. Goldilocks / BLAKE3 configuration.
 *   Definition. Messages, stripped tuples, origin order and first origin are those of ms_witness_lookup_balance above.
 *   A TARGET is a lookup slot (c, j) named by the caller. It is ELIGIBLE when (1) its compiled multiplicity node is OP_VAR on the
 * main trace at offset 0, column m (a PUSH, sign s = +1), or OP_NEG of such a node (a PULL, s = -1), and (2) column m of circuit c
 * is read by no other lookup expression of that circuit: no argument of any slot (the target's own included) and no other slot's
 * multiplicity, at either row offset, following the node program (not the authoring form). Column m is then a DERIVED column.
 * User constraints may read it; that is the caller's business, and ms_witness_check will tell. ms_system_multiplicity_slot
 * classifies a slot. Misuse (MS_ERR): two targets that share a derived column (the same target named twice is that); a derived
 * column that another target's expressions read (which (2) already excludes); an ineligible or out-of-range target.
 *   DEMAND is every message of the witness that does not come from a target slot: the claims, and every non-target slot of
 * every active circuit; multiplicity 0 does not exist. D(t) is the sum modulo p of the demand multiplicities with stripped
 * tuple t. For a tuple t its PROVIDER is the target row (c, r, j) of smallest origin whose stripped tuple is t (a target row's
 * tuple depends only on its arguments, never on the derived column). The call writes, for every target row,
 *   at the provider: column m of row r = v with s v + D(t) = 0 (mod p), canonical - v = D(t) for a pull, p - D(t) for a push,
 *     0 when D(t) = 0;
 *   at every other target row (a later row with the same tuple - a DUPLICATE - or one whose tuple has no demand): 0.
 * What the derived columns held before is ignored and overwritten. A group with D(t) != 0 and no target row is UNSERVED.
 * Postcondition: the witness is balanced, in the sense of ms_witness_lookup_balance, exactly when nothing is unserved.
 *   Held lookup values. Where the witness holds lookup values for circuit c - made by from_stage_1 or supplied by the caller at
 * ms_witness_create - the multiplicity of slot j is updated to s v in the same call, so that ms_prove, ms_stage2_build,
 * ms_witness_check and ms_witness_lookup_balance behind the call see one consistent witness. Arguments are untouched. Nothing
 * else in the witness changes: other columns, other traces and the claims stay byte-identical.
 *   Report. summary: [0] demand messages  [1] demand groups  [2] served groups with D != 0  [3] unserved groups  [4] duplicate
 * target rows: target rows that are not the provider although an earlier target row has their tuple, demanded or not
 * [5] entries written = min([3], entries_cap). entries / args_out (each nullable with capacity 0): the unserved groups with the
 * smallest first origins among their demand members, ascending, in the MS_LB_ENTRY_WORDS layout of ms_witness_lookup_balance:
 * circuit (or MS_LB_CLAIMS), row, slot, net = D(t), demand members, tuple length, tuple start in args_out (all-ones: it would end
 * behind args_cap), 0. Every written value and every figure is deterministic: nothing depends on thread order or on the hash.
 *   Unserved demand is MS_OK. n_targets == 0 is MS_OK: a pure demand count with no writes. A target circuit that is inactive
 * (height 0) is not an error: it has no rows, so its demand is unserved. MS_ERR (text via ms_last_error(), the context stays
 * usable; each of these is refused before anything is written): a host-resident witness; a witness with circuits or claims held by another rank; a null w or
 * summary; null targets with n_targets > 0; a null buffer with a non-zero capacity; misuse of targets as above; a circuit whose
 * lookup values the witness does not hold and whose lookup prefix does not fit the device sweep.
 *   Memory: the grouping table takes 48 bytes x cap, cap = the power of two >= max(64, 2 x M), M = claims + sum over the active
 * circuits of height x num_lookups (target slots included), plus 8 bytes per target row and M / 8 bytes of marks; lookup values
 * the witness does not hold are computed into temporaries of the call; the entries and tuples take entries_cap x
 * MS_LB_ENTRY_WORDS and min(args_cap, entries_cap x the longest tuple) words, unless entries_cap = 0. An allocation failure is
 * MS_ERR naming the bytes. Every buffer of the call is allocated before the first write: after an allocation failure the traces,
 * the claims and the held lookup values are as they were before the call, and the same call may be made again.
 * MSAMD_LB_HASH_BITS as for ms_witness_lookup_balance.
 *   Host waits: one, for the summary; one more, to fetch entries and tuples, when something is unserved and entries_cap > 0. */
/* out3 = [eligibility: 0 eligible, 1 multiplicity is not one main column at offset 0 (optionally negated),
 *         2 that column is read by another lookup expression of the circuit; column m; sign: 0 push, 1 pull]
 * (column and sign are 0 with eligibility 1) */
int32_t ms_system_multiplicity_slot(const ms_system* sys, size_t circuit, size_t slot, uint64_t out3[3]);

typedef struct ms_mult_target { uint32_t circuit, slot; } ms_mult_target;
#define MS_DM_SUMMARY_WORDS 6
int32_t ms_witness_derive_multiplicities(ms_witness* w, const ms_mult_target* targets, size_t n_targets,
                                         uint64_t summary[MS_DM_SUMMARY_WORDS], uint64_t* entries, size_t entries_cap /* nullable with cap 0 */,
                                         uint64_t* args_out, size_t args_cap /* nullable with cap 0 */);

/* ---- Trace columns filled on the device from a program. ms_witness_derive_multiplicities produces the tables' multiplicity
 * columns; this call produces the others - byte decompositions, carries, inverses, flags, padding - for one circuit of a
 * witness whose traces are in HBM, from a FILL PROGRAM the caller authors in the front end (frontend.compile_fill) and,
 * optionally, a matrix of inputs in device memory. Goldilocks / BLAKE3 configuration.
 *   Program. A little-endian u64-word blob: a magic word (0x31304C4C49464D00), main_width, pre_width, n_inputs, n_nodes,
 * n_steps; the nodes as [kind | source << 8 | offset << 16, a, b]; the steps as [dst, root]. Node kinds 0 (constant a), 1
 * (variable a of source 0 preprocessed / 1 main / 3 input, at row offset 0 or 1), 6 add, 7 sub, 8 mul, 9 neg are those of the
 * system blob; the witness-only kinds follow from 16: 16 row, 17 bits (b = lo | length << 8), 18 inv0, 19 lt, 20 xor, 21 and.
 * Operands a, b of an operator are indices of EARLIER nodes. Stage-2 variables (source 2), publics (kind 2) and the three
 * selector nodes (kinds 3-5) are refused: the selectors are polynomials here, not flags; flags come from row, lt and inv0.
 *   Values at row r of a circuit of height n, operands taken as the canonical integers in [0, p):
 *     input i at offset 0 / 1   column i of the input matrix at row r / row (r + 1) mod n; rows at or beyond its height read 0
 *     preprocessed i            the circuit's preprocessed column at row r / row (r + 1) mod n
 *     row                       r
 *     add, sub, mul, neg        the field operations
 *     bits(x, lo, length)       (x >> lo) & (2^length - 1), 1 <= length, lo + length <= 64
 *     inv0(x)                   the inverse of x modulo p, and 0 for x = 0
 *     lt(x, y)                  1 if x < y as integers, else 0
 *     xor(x, y), and(x, y)      (x ^ y) mod p, x & y
 *   Definition. The steps run in order for every row r: trace[r][dst_k] = the value of root_k at row r. A read of main column m
 * at offset 0 sees the value of the latest EARLIER step of this call that assigned m, and what the trace held before the call
 * if there is none. A read of main column m at offset 1 sees what row (r + 1) mod n held before the call and is allowed only if
 * NO step of the program assigns m - that is what makes the row-parallel execution equal to this sequential definition. The
 * same dst may appear in several steps; the last one wins. Every written value is canonical.
 *   Held lookup values. Where the witness holds lookup values for the circuit they are recomputed by from_stage_1 on the device
 * inside the same call, so that ms_prove, ms_stage2_build, ms_witness_check, ms_witness_lookup_balance and
 * ms_witness_derive_multiplicities behind it see one consistent witness. Nothing else in the witness changes: other columns,
 * other traces and the claims stay byte-identical.
 *   inputs (nullable when the program has n_inputs = 0): one ms_dev_matrix as for ms_witness_create_device, of width n_inputs and
 * a height in [0, n]; it is copied and checked by the same launch, and the library has finished reading it when the call
 * returns, with any status. producer_stream orders that read behind the caller's stream exactly as there.
 *   summary: [0] rows  [1] steps  [2] instructions executed per row (the linearised program: shared subexpressions once,
 * nothing a later assignment overwrites unread)  [3] kernel form: lanes per workgroup with the slot file in LDS, 0 = slots in
 * a global scratch walked in row batches.
 *   MS_ERR (text via ms_last_error(); each refusal comes before anything is written, the context stays usable): a
 * host-resident witness; a witness with circuits held by another rank; a circuit out of range or inactive; a blob with a wrong
 * magic, a length that does not match its counts, widths other than the circuit's, a dst or a variable out of range, a forward
 * operand, bad bits fields, a non-canonical constant or a refused node kind; an offset-1 read of an assigned column; an input
 * matrix that fails the checks of ms_witness_create_device; an input height above n; n_inputs > 0 with inputs = NULL; an
 * 8-byte input element >= p, naming the first offender in row-major order ("non-canonical input value: row 5, column 1"); a
 * witness that holds lookup values for the circuit whose lookup prefix does not fit the device sweep. An allocation failure is
 * MS_ERR as well and comes before the first write too - every buffer of the call, for scans and indexed reads included, is
 * allocated before the first group is launched: the traces, the claims and the held lookup values are as they were before the
 * call, and the same call may be made again (which matters for a program that reads a column it overwrites).
 *   Host waits: one when the program reads inputs of height > 0 (the offender word, before the first write); none otherwise -
 * the call then only queues work on the context's stream.
 *
 *   SCAN STEPS: columns that follow the previous row (running sums and products, counters, Horner accumulators). A step is
 * ORDINARY, (dst, root) as above, or a SCAN (dst, mul root A, add root B, init). The definition is column at a time: step k
 * computes its whole column before step k + 1 starts - for ordinary steps that equals the definition above. A scan step writes
 *     trace[0][dst]     = init
 *     trace[r + 1][dst] = A(r) * trace[r][dst] + B(r)  (mod p),  r = 0 .. n - 2
 * where A(r), B(r) are the values the roots would have at row r if an ordinary step stood at that position. A(n - 1) and
 * B(n - 1) are not used: there is no wrap-around, as under is_transition; at n = 1 only init is written. Every written value
 * is canonical. The affine maps x -> A x + B compose associatively and exactly, so the device's parallel scan is bit-identical
 * to this loop.
 *   Groups. Each scan step is a group of its own; each maximal run of ordinary steps between scans is a group. Inside a group
 * the rules above hold (an offset-0 read of an assigned column sees the latest earlier step of the group, shared subexpressions
 * are computed once, each cell is stored once per group); a read of a column that an earlier group assigned comes from the
 * trace. A read of main column m at offset 1 by a step of group g is allowed exactly when no step of group g or of any later
 * group assigns m - with one group this is the rule above - so a later step may read the next row of a finished scan column
 * (diff = s_next - s; at row n - 1 that is row 0). The coefficients of a scan step may not read its own dst at either offset.
 *   Blob. A program without a scan step is the blob above. With scans: the magic word 0x32304C4C49464D00 ("\0MFILL02"), then
 * main_width, pre_width, n_inputs, n_nodes, n_steps, n_scans (seven header words with the magic); the nodes; the steps as
 * [dst, root], root of a scan step being its add root B; n_scans records [step index, mul root, init] with strictly ascending
 * step indices. Nodes that no step reaches are not subject to the offset-1 rule in this format.
 *   Execution: the groups in order on the context's stream - an ordinary group as above, a scan group as a coefficient pass
 * (the same kernel, writing A and B into a temporary) and a three-launch scan over tiles of T rows (ms_fill_scan_info tells T);
 * a mul root that is the constant 1 takes the additive form (B alone, no multiplications). Temporaries: 16 bytes x n for the
 * call (8 when every scan is additive), shared by its scans, plus 24 bytes per tile. Held lookup values are recomputed once, at
 * the end. Host waits are unchanged. summary for such a program: [1] all steps, [2] instructions per row summed over every
 * launch of the fill kernel, coefficient passes included, [3] the smallest lanes figure over those launches (0 if any of
 * them uses the global scratch).
 *   MS_ERR in addition, before anything is written: a length that does not match the three counts; a scan record whose step
 * index is out of range or not above the one before, whose mul root is out of range or whose init is >= p; a scan step whose
 * coefficients read its own dst; an offset-1 read that the group rule refuses. msbb_witness_fill refuses the blob by its magic.
 *
 *   INDEXED READS: a column of a source at a COMPUTED row - the input row of the item a row belongs to (several rows per item),
 * a sorted or permuted copy of a column (sorted[r] = log[perm[r]]), the table row a lookup points at, a finished running sum at
 * a segment boundary. Node kind 22, `at`: the head word is 22 | source << 8 and its offset field must be 0; a is the column; b
 * is the index of an EARLIER node, the row operand. Sources: 0 preprocessed, 1 main, 3 input; stage 2 (source 2) is refused as
 * for variables.
 *   Value at row r. Let i be the value of node b at row r, taken as the canonical integer in [0, p), and h the height of the
 * source: n for the main and the preprocessed trace, the input matrix's own height for inputs. If i < h the node is the
 * source's column a at row i; if i >= h it is 0. There is no reduction modulo n and no truncation of the index: an index of
 * 2^32 + 1 reads 0, not row 1. The bound check is the definition: no index a program can compute addresses memory outside the
 * three matrices, and a row >= h performs no load.
 *   Main column m. If an earlier group assigned m, `at` sees that group's values, from the trace; if no step assigns m it sees
 * what the trace held before the call; if a step of the same group or of a later group assigns m the program is refused. This
 * is the offset-1 rule applied to `at`, in the first format (one group) and in the second, and as there it is what makes the
 * row-parallel execution equal to the column-at-a-time definition. It follows that the coefficients of a scan step cannot
 * index their own dst, while a later group may index a finished scan column. In the first format the rule holds for every
 * node, in the second for the nodes a group reaches, like the offset-1 rule.
 *   Unchanged: the magic words - a program without an `at` node keeps its blob byte for byte, and a library that predates the
 * node refuses a program with one as "unknown node kind 22" - the host waits, the summary words (an `at` is one instruction,
 * equal reads are issued once per launch), the held-lookup recomputation and every refusal above.
 *   MS_ERR in addition, before anything is written: an `at` node with a forward row operand, a column out of range for its
 * source's width, a non-zero offset field, a stage-2 or unknown source; an `at` of a main column that the group rule refuses,
 * naming node, column, reading group and assigning group.
 *
 *   PEER READS: the main or the preprocessed trace of OTHER circuits of the same witness, at the thread's row, the next row or a
 * computed row - a memory circuit that is the CPU circuit's access log in address order, a consumer that points at the rows of a
 * table circuit, a chip whose rows are those of the dispatcher that asked for it - without the finished columns leaving HBM.
 *   Peers. A program declares 1 .. 8 peers (FL_MAX_PEERS = 8). Peer k is a triple (circuit, trace: 0 preprocessed / 1 main,
 * width). Its height h_k is, for a main peer, the circuit's height in THIS witness (0, an inactive circuit, is allowed) and, for
 * a preprocessed peer, the system's preprocessed height of that circuit, whether or not the witness activates it.
 *   Nodes. The source byte 4 + k in a variable node (kind 1) or an `at` node (kind 22) names peer k; a is the column, b the row
 * operand of an `at`. The head word keeps its 24 bits; the offset field is 0 or 1 for a variable and 0 for an `at`, as above.
 *   Value at row r of the filled circuit (height n). Variable at offset 0 / 1: let row = r / (r + 1) mod n - n is the FILLED
 * circuit's height, exactly as for inputs; the value is peer column a at `row` if row < h_k, else 0. `at`: with i the row
 * operand's value taken as the canonical integer in [0, p), peer column a at row i if i < h_k, else 0. No reduction, no
 * truncation, and no load for a row at or above h_k: the bound check is the definition, as for the other sources. A peer may be
 * taller than the filled circuit; an `at` reaches all of its rows.
 *   No group rule for peers. A peer is never the circuit being filled, so the call never writes what a peer read sees, and the
 * row-parallel execution equals the column-at-a-time definition without further conditions.
 *   Blob, third format. Magic 0x33304C4C49464D00 ("\0MFILL03"); eight header words: magic, main_width, pre_width, n_inputs,
 * n_nodes, n_steps, n_scans, n_peers; then the nodes, the steps, n_scans scan records (0 is allowed) and n_peers records
 * [circuit, trace, width]. Everything else is the second format's: groups, the offset-1 and `at` rules over the nodes a group
 * reaches, scan semantics. A program without a peer read keeps the first or second format byte for byte; the front end emits
 * records only for the (circuit, trace) pairs its steps reach, in ascending order.
 *   MS_ERR on the blob alone (ms_fill_program_info, ms_fill_scan_info, ms_fill_peer_info, and ms_witness_fill before anything
 * is written): n_peers of 0 or above 8 under the third magic; a length that does not match the four counts; a record with
 * trace > 1, width > 2^20 or circuit >= 2^32; two records with the same (circuit, trace); a source byte >= 4 + n_peers
 * ("unknown variable source" / "unknown source of an indexed read", which is also what a peer source under the first or second
 * magic gets); a peer column at or beyond the record's width.
 *   MS_ERR at the call in addition, before anything is written, the text naming the peer, the context staying usable: a peer
 * circuit out of range for the system; a peer circuit equal to the filled circuit (use source 1 / source 0); a declared width
 * other than the circuit's main_width / pre_width; a preprocessed peer whose trace is not on the device; a main peer of
 * height > 0 without a trace on this device.
 *   Unchanged: the summary words (a peer read is one instruction, equal reads are issued once per launch), the host waits (none
 * without inputs), the held-lookup recomputation - of the FILLED circuit only - and allocation before the first write. The
 * peers' traces, their held lookup values and the claims stay byte-identical. msbb_witness_fill refuses the blob by its magic. */
int32_t ms_witness_fill(ms_witness* w, size_t circuit, const uint8_t* program, size_t program_len,
                        const ms_dev_matrix* inputs /* nullable with n_inputs 0 */, void* producer_stream /* hipStream_t, nullable */,
                        uint64_t summary[4]);
/* Host code, no device: checks a fill program as ms_witness_fill does (everything that needs no witness) and describes how it
 * would run: out4 = [instructions per row, live slots, lanes per workgroup of the LDS form (0: the slot file does not fit 64 KB
 * at 64 lanes - global scratch), distinct assigned columns]. For a program with scan steps: instructions summed over the
 * launches of the fill kernel, the largest slot count and the smallest lanes figure among them, and the dst columns of scan
 * steps count as assigned. */
int32_t ms_fill_program_info(const uint8_t* program, size_t program_len, uint64_t out4[4]);
/* Host code, no device: the same checks, and out4 = [scan steps, launches of the fill kernel (one per group of ordinary steps,
 * one coefficient pass per scan), scans in the additive form, T = rows per scan tile]. Texts start "ms_fill_scan_info: ". */
int32_t ms_fill_scan_info(const uint8_t* program, size_t program_len, uint64_t out4[4]);
/* Host code, no device: the same checks, and the program's peers ("PEER READS"): out receives [circuit, trace, width] per peer,
 * *n_peers their number. MS_ERR_BUFFER with *n_peers set when cap (in records) is too small; nothing is written to out then. A
 * program of the first or second format yields *n_peers = 0. Texts start "ms_fill_peer_info: ". */
int32_t ms_fill_peer_info(const uint8_t* program, size_t program_len, uint64_t* out /* cap x 3, nullable with cap 0 */, size_t cap,
                          size_t* n_peers);

/* ---- CLAIM PROGRAMS: the claims of a witness built on the device from its traces. Claims can otherwise only be given when a
 * witness is created, before any column has been filled; for most systems they are a function of filled columns (the bench
 * workload's [1, x, y, z] per addition). With this call the route pairs -> fill -> claims -> multiplicities -> check -> prove
 * leaves HBM only for the proof bytes. Goldilocks / BLAKE3 configuration (the other's: msbb_witness_claims_fill, mstark_bb.h).
 *   Definition. A claim program has W expressions, the elements of one claim (1 <= W <= 2^16), and optionally a `keep`
 * expression. They are written in the algebra of fill programs: constants, main / preprocessed / input variables at offset 0
 * or 1, row, add, sub, mul, neg, bits, inv0, lt, xor, and, and indexed reads (`at`) of the three sources. A claim program
 * ASSIGNS NOTHING, so neither the offset-1 rule nor the group rule applies: any main column may be read at the next row or at a
 * computed row. Refused, with a text naming the node: peer sources, publics, selector nodes, stage-2 variables; there are no
 * scan steps (the format has no record for them, and a fill program handed to this call is refused by its magic).
 *   ms_witness_claims_fill works on circuit `circuit` of height n, with rows <= n. For each row r in [0, rows), in ascending
 * order, for which keep(r) != 0 - every row when there is no keep - ONE claim [e_0(r), ..., e_{W-1}(r)] is emitted. Reads mean
 * what they mean in ms_witness_fill: the next row of row n - 1 is row 0 (n, not `rows`); an input row from the input matrix's
 * height on reads 0; an index from the source's height on reads 0 and performs no load. Every emitted element is a canonical
 * field value by construction.
 *   mode = MS_CLAIMS_REPLACE: the emitted claims become the witness's claims. mode = MS_CLAIMS_APPEND: they follow the claims
 * the witness already has, whose offsets and elements stay as they are, and the offsets continue. The order of claims is part
 * of the transcript, so the order of calls is the caller's way to order the claims of several circuits.
 *   Afterwards the witness is an ordinary device-resident witness: ms_prove, ms_witness_check, ms_witness_lookup_balance,
 * ms_witness_derive_multiplicities, ms_challenger_observe_claims and ms_witness_claims_accumulator see the new claims. The
 * traces and the held lookup values are not touched.
 *   One width per call. A ragged list (claims of several lengths, as a byte-operations chip's are) is made by several calls
 * with keep masks, one per length and in the order the transcript wants, or on the host as before; one call cannot interleave
 * lengths.
 *   summary: [0] rows considered  [1] claims emitted  [2] instructions executed per row  [3] kernel form: lanes per workgroup
 * with the slot file in LDS, 0 = slots in a global scratch walked in row batches.
 *   Blob (little-endian 64-bit words), a format of its own: magic 0x314D49414C434D00 ("\0MCLAIM1"), main_width, pre_width,
 * n_inputs, n_nodes, W, keep root (all ones: none) - seven header words; the nodes, three words each, exactly as in a fill
 * program; the W element roots, one word each. The length is exactly 7 + 3 n_nodes + W words.
 *   Execution. The evaluation is the kernel of ms_witness_fill over the first `rows` rows. Without keep it writes straight into
 * the new claim data behind the claims that stay (rows x W, row-major): there is no second pass. With keep it writes W + 1
 * words per row into a temporary of the call, and the kept rows are compacted over tiles of 1024 rows: per-tile counts, one
 * workgroup that turns them into tile offsets and the total, and a scatter that recomputes each kept row's rank from wave
 * ballots and copies whole claims with consecutive lanes on consecutive words; rows <= 1024 take the scatter alone. The three
 * launches are ordered by the stream; no position depends on the order in which atomics land. Offsets are written on the
 * device. Bytes per row: 8 (W + 1) written by the pass, the flag read twice, and 8 W read and 8 W written per kept row.
 *   The new offset and data arrays, device and host copies, are built beside the witness's and change places with them as the
 * last step. MS_ERR at any point - a refusal, an allocation failure, a non-canonical input - leaves the witness's claims and
 * traces what they were and the context usable.
 *   Host waits: at most two. One brings the inputs' offender word and the kept total in one read-back (not needed without
 * inputs and without keep); one brings the host copy of the new claims, which the witness keeps for short transcripts (in
 * chunks when the list is longer than the staging buffer).
 *   MS_ERR (texts start "ms_witness_claims_fill: "): a witness of another system; a witness that holds only a slice of its
 * claims; a host-resident witness; a witness with circuits held by another rank; mode neither 0 nor 1; a circuit out of range,
 * inactive or without a trace on this device; a blob that ms_claims_program_info refuses; widths other than the circuit's; a
 * preprocessed trace that is not on the device at this height; rows > n; n_inputs > 0 with inputs = NULL, an input height above
 * n, an input matrix that fails the checks of ms_witness_create_device, an 8-byte input element >= p ("non-canonical input
 * value: row 5, column 1"); a total of 2^60 elements or more. */
#define MS_CLAIMS_REPLACE 0
#define MS_CLAIMS_APPEND 1
int32_t ms_witness_claims_fill(ms_system* sys, ms_witness* w, size_t circuit, const uint8_t* program, size_t program_len, size_t rows,
                               const ms_dev_matrix* inputs /* nullable with n_inputs 0 */, void* producer_stream /* hipStream_t, nullable */,
                               uint32_t mode, uint64_t summary[4]);
/* Host code, no device: checks a claim program as ms_witness_claims_fill does (everything that needs no witness): out4 =
 * [instructions per row, live slots, lanes per workgroup of the LDS form (0: global scratch), W | has_keep << 32]. MS_ERR: a
 * wrong magic (a fill program is named as such); a length other than 7 + 3 n_nodes + W words; W = 0 or W > 2^16; an element
 * root or the keep root out of range; every node refusal of ms_fill_program_info with "claim program" in its text; a peer
 * source. Texts start "ms_claims_program_info: ". */
int32_t ms_claims_program_info(const uint8_t* program, size_t program_len, uint64_t out4[4]);
/* Diagnostic, in the manner of ms_witness_trace: the claims of a device-resident witness read back from the DEVICE copy, which
 * is what the prover hashes for long lists. *n_claims and *n_elems are always set; offsets_out receives *n_claims + 1 words,
 * data_out *n_elems. MS_ERR_BUFFER when cap_offsets < *n_claims + 1 or cap_data < *n_elems; nothing is written then.
 * Host-resident witnesses and witnesses that hold a slice of their claims: MS_ERR. */
int32_t ms_witness_claims(ms_witness* w, uint64_t* offsets_out, size_t cap_offsets, uint64_t* data_out, size_t cap_data, size_t* n_claims,
                          size_t* n_elems);

/* ---- The sorting permutation of a circuit's rows, made on the device. Indexed reads let a fill program write a sorted or
 * permuted copy of a column (sorted[r] = log[perm[r]]); this call produces perm, so that the witness of an offline memory
 * check, of a range check by sorted differences or of a permutation argument never leaves HBM: sort, gather, scan.
 * Goldilocks / BLAKE3 configuration; msbb_witness_argsort (include/mstark_bb.h) is the call of the other one.
 *   Definition. Let n be the circuit's height in the witness and k_0 .. k_{m-1} the key columns, 1 <= m <= 8. Row i comes
 * before row j iff the tuple (trace[i][k_0], ..., trace[i][k_{m-1}], i) is lexicographically smaller, the cells compared as the
 * canonical integers in [0, p) that the trace holds: an unsigned 64-bit comparison. The row index is the last component, so the
 * order is total, the sort is stable and the result is unique. The same column may appear several times among the keys; that
 * changes nothing.
 *     what = MS_SORT_PERM   trace[t][dst_column] = the row at sorted position t
 *     what = MS_SORT_RANK   trace[r][dst_column] = the sorted position of row r (the inverse permutation)
 * Every cell of dst_column is written once. No other cell of the trace changes, and no other circuit is touched.
 *   Held lookup values. Where the witness holds lookup values for the circuit they are recomputed by from_stage_1 on the device
 * inside the same call, as ms_witness_fill does.
 *   A trace column, not a caller's buffer: nothing in this interface writes caller memory, ms_witness_trace reads the column
 * back, and no scratch column is needed - the permutation may land in a column that the next fill program overwrites with the
 * sorted keys. With columns (ADDR, VAL, S_ADDR, S_VAL), in the front end's notation, under the group rule of ms_witness_fill:
 *     w.argsort(c, [ADDR], dst=S_ADDR)
 *     w.fill(c, compile_fill(W, 0, 0, [(S_VAL,  E.main_at(VAL,  E.main(S_ADDR))),
 *                                      (S_ADDR, E.main_at(ADDR, E.main(S_ADDR)))]))
 *   Execution: a least-significant-digit radix sort over (key, row index) pairs with 8-bit digits, the last key column first,
 * row indices as u32. One launch per key column counts its eight digit histograms (the one for the last key column also pulls
 * the column out of the row-major trace), the host reads all of them in one copy and skips every digit in which all n rows
 * share one value: a byte-valued column costs one pass, a constant column none. Each pass that runs is three launches over
 * tiles of T rows: per-tile digit counts, exclusive offsets over the digit-major 256 x tiles array by one workgroup in rounds
 * of R counts, and a scatter that recomputes stable local ranks. No position depends on the order in which atomics land.
 *   summary: [0] rows  [1] key columns  [2] digit passes run  [3] digit passes skipped ([2] + [3] = 8 x key columns).
 *   MS_ERR (text via ms_last_error(), starting "ms_witness_argsort: "; each refusal comes before anything is written, the
 * context stays usable): a witness of another system; a host-resident witness; a witness with circuits held by another rank; a
 * circuit out of range, inactive or without a trace on this device; n_keys 0 or above 8; a key column or dst_column at or
 * beyond main_width; dst_column among the keys; what neither 0 nor 1; a height above 2^31; a witness that holds lookup values
 * for the circuit whose lookup prefix does not fit the device sweep.
 *   Host waits: exactly one, the copy of the histograms; nothing has been written to the trace by then.
 *   Temporaries: 24 bytes x n (two key and two index buffers) and 1 KB per tile, next to 8 KB per key column and histogram
 * workgroup (at most 256 of them). An allocation failure is MS_ERR; all of them are allocated before dst_column is written, so
 * the traces, the claims and the held lookup values are then as they were before the call, and the same call may be made again. */
#define MS_SORT_PERM 0
#define MS_SORT_RANK 1
int32_t ms_witness_argsort(ms_system* sys, ms_witness* w, size_t circuit, const uint32_t* key_columns, size_t n_keys,
                           uint32_t dst_column, uint32_t what, uint64_t summary[4]);
/* Host code, no device: out4 = [T = rows per tile, bits per digit, R = per-tile counts handled per round of the offsets step,
 * largest n_keys]. */
int32_t ms_sort_info(uint64_t out4[4]);

/* ---- System::prove_multiple_claims (src/prover.rs:290-603). Writes Proof::to_bytes (src/prover.rs:241-248).
 * stage_ms (optional, 6 doubles): stage1_commit, lookup_construction, stage2_commit, quotient, fri_open, total —
 * the reference's span names (src/prover.rs:336-538). Returns MS_ERR_BUFFER with *proof_len = needed size if
 * cap is too small. */
int32_t ms_prove(ms_system* sys, ms_witness* w, uint8_t* proof_out, size_t cap, size_t* proof_len, double* stage_ms);

/* ---- System::verify_multiple_claims (src/verifier.rs:208-532; shape checks :536-695) on the bytes ms_prove wrote.
 * Returns MS_OK when the check ran; *verdict = 0 if the proof is accepted, else the reference's VerificationError
 * variant (src/verifier.rs:176-192): 2 InvalidOpeningArgument, 3 InvalidProofShape, 4 InvalidSystem,
 * 5 OodEvaluationMismatch, 6 UnbalancedChannel. Claims as in ms_witness_create. The claims part (transcript hash and
 * initial accumulator) runs on the device, the rest on the host. */
#define MS_VERDICT_ACCEPT 0
#define MS_VERDICT_INVALID_OPENING 2
#define MS_VERDICT_INVALID_SHAPE 3
#define MS_VERDICT_INVALID_SYSTEM 4
#define MS_VERDICT_OOD_MISMATCH 5
#define MS_VERDICT_UNBALANCED 6
int32_t ms_verify(ms_system* sys, size_t n_claims, const uint64_t* claim_offsets, const uint64_t* claim_data,
                  const uint8_t* proof, size_t proof_len, int32_t* verdict);
/* N proofs of ONE ms_system. verdicts[i] is what ms_verify writes for proof i (MS_VERDICT_*), for every input.
 * Claims are given per proof as in ms_verify (claim_offsets[i] / claim_data[i] may be NULL where n_claims[i] = 0).
 * n_proofs = 0 is MS_OK. A null proof pointer or null verdicts is MS_ERR. Nothing in a proof's bytes can make the call fail
 * or fault: a malformed proof is a verdict. Per proof the host parses, checks the shape, replays the transcript, checks both
 * proofs of work, the arity schedule and the constraints at zeta; the per-query arithmetic (reduced openings, FRI fold
 * chain, final polynomial) and every Merkle path of the batch run on the device in two launches, with one host wait per
 * call (per 256 MB of openings) when the claims stay below 8192 transcript words. MS_ERR for a system whose traces of one
 * kind are together wider than 8192 columns (one leaf is hashed inside a thread). An allocation failure is MS_ERR with the
 * verdicts unspecified; the same call made again gives them all. */
int32_t ms_verify_batch(ms_system* sys, size_t n_proofs, const uint64_t* n_claims, const uint64_t* const* claim_offsets,
                        const uint64_t* const* claim_data, const uint8_t* const* proofs, const uint64_t* proof_lens,
                        int32_t* verdicts);

/* ---- One proof over several GPUs (one process per GPU; SURVEY §8e, BASELINE config 3). The reference has no such
 * mode: this is System::prove_multiple_claims (src/prover.rs:290-603) with the Pcs::commit / Pcs::open calls
 * (:350,419,526,580) spread over ranks, producing the same Proof bytes as ms_prove on one device.
 * Every rank creates the SAME system and a witness that holds: the traces of the circuits it computes (its own
 * "sharded" circuit and every replicated one; traces[i] = NULL with heights[i] > 0 marks a circuit computed elsewhere),
 * the heights of all circuits, and all claims. owners[i] = rank that computes circuit i, or -1 = replicated on every
 * rank (small tables). A rank may own any number of circuits (none included) of any shapes: the reference's multi-circuit
 * systems (one wide circuit beside tables of other widths and heights, src/test_circuits/blake3.rs:2215-2613) split as they
 * are. Limits: the number of ranks is a power of two; every committed LDE has at least as many rows as there are ranks
 * (any cap_height: a cap taller than log2(ranks) is gathered from inside the ranks' sub-trees). When there is exactly one sharded circuit per rank, all of one shape, the k-th owned by rank k
 * (BASELINE config 3) the row ranges travel by one symmetric all-to-all per column group; otherwise every sharded matrix is
 * handed out by its owner (ms_comm.scatter_cols_start, which the transport must then offer).
 * The library calls back for the two exchanges it needs; both take DEVICE pointers of this context's device, are
 * called with the context's stream idle, and must have completed when they return (0 = ok):
 *   all_to_all: send/recv hold `world` blocks of bytes_per_peer bytes; block k of send goes to rank k, block k of recv
 *               comes from rank k (row ranges of the LDE matrices before leaf hashing);
 *   all_gather: every rank contributes `bytes`, recv gets world * bytes ordered by rank (sub-tree roots, logUp totals,
 *               opened values, reduced openings, query openings).
 * With torch.distributed these are all_to_all_single / all_gather_into_tensor on RCCL (multi-stark_amd/sharded.py). */
typedef struct ms_comm {
  /* sizeof(ms_comm) as the HOST compiled it. Members are only ever appended: the library reads the first `size` bytes and
   * treats every member beyond them as NULL (not offered), so a host built against an older header stays valid. A size that
   * does not even cover all_gather is refused. */
  uint32_t size;
  int32_t rank, world;
  void* user;
  int32_t (*all_to_all)(void* user, const void* send_dev, void* recv_dev, size_t bytes_per_peer);
  int32_t (*all_gather)(void* user, const void* send_dev, void* recv_dev, size_t bytes);
  /* Optional pair (both NULL = not offered): a non-blocking all_to_all, so that the exchange of one group of LDE columns
   * runs while the next group is being transformed. `start` is called with the context's stream idle and returns at once;
   * chunk k of the exchange is bytes_per_peer bytes at send_dev + k * send_stride (to rank k) and at recv_dev +
   * k * recv_stride (from rank k). Buffers stay untouched until `wait` - which completes every started exchange - returns. */
  int32_t (*all_to_all_start)(void* user, const void* send_dev, size_t send_stride, void* recv_dev, size_t recv_stride,
                              size_t bytes_per_peer);
  int32_t (*all_to_all_wait)(void* user);
  /* Optional (NULL = not offered; needs all_to_all_wait): the same non-blocking exchange read STRAIGHT OUT OF a column-major
   * matrix, so that no send buffer has to be packed first. For every rank k, `ncols` segments of seg_bytes bytes each way:
   * segment c for rank k is read at send_dev + k * send_peer_stride + c * send_col_stride (rows [k h / N, (k + 1) h / N)
   * of column c of this rank's LDE), and segment c coming from rank k is written at recv_dev + k * recv_peer_stride +
   * c * recv_col_stride (block k of this rank's receive buffer, column c). Segments of one peer travel in column order on
   * both sides; the rank's own segments (k = rank) are copied on the device. Completed by all_to_all_wait. */
  int32_t (*all_to_all_cols_start)(void* user, const void* send_dev, size_t send_peer_stride, size_t send_col_stride, void* recv_dev,
                                   size_t recv_peer_stride, size_t recv_col_stride, size_t ncols, size_t seg_bytes);
  /* Optional (NULL = not offered): order the transport with a HIP stream by events instead of by the host. After
   * set_stream_ordered(user, s) every call above (1) first makes the transport's own stream wait for what has been queued on
   * `s` so far - so the caller need not leave `s` idle - and (2) returns without waiting: the blocking calls and
   * all_to_all_wait make `s` wait for the transport's stream instead of the host. A joint proof synchronises with the host some
   * twenty times less often this way. set_stream_ordered(user, NULL) restores the blocking contract; ms_prove_sharded
   * switches the mode on for its own duration when the transport offers it (MSAMD_SHARDED_HOST_SYNC=1: never). */
  int32_t (*set_stream_ordered)(void* user, void* hip_stream);
  /* Optional (NULL = not offered): all_to_all_cols_start with flags. MS_COMM_SKIP_SELF: the rank's own segments (k = rank) are
   * NOT copied - the library hashes and reduces its own rows where they are, inside its LDE, so that block of the receive buffer
   * is never read (at world 1 the exchange then moves nothing at all). Without this member the library calls
   * all_to_all_cols_start; the self-copy is then made and ignored. */
  int32_t (*all_to_all_cols_start2)(void* user, const void* send_dev, size_t send_peer_stride, size_t send_col_stride, void* recv_dev,
                                    size_t recv_peer_stride, size_t recv_col_stride, size_t ncols, size_t seg_bytes, uint32_t flags);
  /* Optional (NULL = not offered; needs all_to_all_wait): ONE rank's matrix handed out by row ranges - what the library uses
   * when the sharded circuits differ in shape or in number per rank. Rank `root` sends, to every OTHER rank k, ncols segments
   * of seg_bytes read at send_dev + k * send_peer_stride + c * send_col_stride; every other rank receives its ncols
   * segments at recv_dev + c * recv_col_stride. Nothing is copied for k = root (its rows stay where they are); send_dev is
   * ignored on the other ranks, recv_dev on root. Non-blocking like all_to_all_start, completed by all_to_all_wait; every
   * rank makes the same sequence of calls. */
  int32_t (*scatter_cols_start)(void* user, int32_t root, const void* send_dev, size_t send_peer_stride, size_t send_col_stride,
                                void* recv_dev, size_t recv_col_stride, size_t ncols, size_t seg_bytes);
  /* Optional (NULL = not offered): this rank cannot go on - a validation that fails on ONE rank, an allocation failure, a
   * failed exchange - while its peers have entered, or are about to enter, the next exchange. ms_prove_sharded calls it on
   * every error path before it returns, so that the peers' pending and future calls FAIL instead of waiting for operations
   * that will never be issued (RCCL: ncclCommAbort; threads: ms_comm_local_group_abort). The transport is unusable
   * afterwards. Without it only the host's watchdog ends a proof one rank has left. Must not fail and must not throw. */
  void (*abort)(void* user, const char* why);
} ms_comm;
#define MS_COMM_SKIP_SELF 1u
int32_t ms_prove_sharded(ms_system* sys, ms_witness* w, const ms_comm* comm, const int32_t* owners, uint8_t* proof_out, size_t cap,
                         size_t* proof_len, double* stage_ms);
/* A rank of a joint proof need not hold ALL claims on the host (8.4 M claims on each of eight ranks at BASELINE config 3): it
 * reads the element range ms_claims_slice_range reports - the claims whose transcript words fall into its range of BLAKE3
 * chunks, cut from the system's shape, the circuits' heights and the n_claims + 1 element offsets (which every rank keeps
 * in full: 8 bytes per claim) - plus the first 130 elements, which every rank needs for the transcript's first chunk.
 * ms_witness_create_host_sliced is ms_witness_create_host with that part of claim_data only: data_slice holds the elements
 * [data_first, data_first + data_count), head the first min(total, 130). A list of at most 8192 transcript words is absorbed
 * whole by every rank (the range is then everything). Only ms_prove_sharded accepts such a witness. */
int32_t ms_claims_slice_range(ms_system* sys, const uint64_t* heights, size_t n_claims, const uint64_t* claim_offsets, int32_t rank,
                              int32_t world, uint64_t* first_elem, uint64_t* n_elems);
int32_t ms_witness_create_host_sliced(ms_system* sys, const uint64_t* const* traces, const uint64_t* heights, size_t n_claims,
                                      const uint64_t* claim_offsets, uint64_t data_first, uint64_t data_count,
                                      const uint64_t* data_slice, const uint64_t* head, size_t n_head, int32_t* pinned,
                                      ms_witness** out);

/* Where a joint proof is: the library records every call it makes into the transport - the prover's phase, the collective,
 * its size, the rank ("stage-2 commit: all_to_all_cols_start (29360128 bytes, part 3) on rank 5 of 8"). `out` receives the
 * text of the LAST call entered through this context, *seq how many have been entered since the context was created and
 * *in_flight whether that call has not returned yet. Callable from any thread while ms_prove_sharded runs on another (it is
 * what a watchdog prints when a peer never joins a collective: which exchange, on which rank). */
int32_t ms_ctx_comm_progress(ms_ctx* ctx, char* out, size_t cap, uint64_t* seq, int32_t* in_flight);

/* ---- Native transport for ms_prove_sharded: RCCL over xGMI (csrc/comm_rccl.hip; librccl is loaded at run time). The host
 * needs no Python: rank 0 draws the 128-byte id (ncclGetUniqueId) and hands it to the other ranks by whatever channel the
 * host already has (a file, MPI, a TCP store); every rank then creates its transport on its own context (collective:
 * ncclCommInitRank) and passes ms_comm_rccl_table() to ms_prove_sharded. all_to_all = one grouped ncclSend / ncclRecv
 * pair per peer, all_gather = ncclAllGather, both on the transport's own stream; world = 1 needs no id and no librccl. */
#define MS_RCCL_UNIQUE_ID_BYTES 128
typedef struct ms_comm_rccl ms_comm_rccl;
int32_t ms_comm_rccl_unique_id(uint8_t out[MS_RCCL_UNIQUE_ID_BYTES]);
int32_t ms_comm_rccl_create(ms_ctx* ctx, const uint8_t unique_id[MS_RCCL_UNIQUE_ID_BYTES], int32_t rank, int32_t world,
                            ms_comm_rccl** out);
const ms_comm* ms_comm_rccl_table(ms_comm_rccl* c);
uint64_t ms_comm_rccl_bytes_moved(ms_comm_rccl* c); /* bytes this rank has put through the two exchanges so far */
void ms_comm_rccl_destroy(ms_comm_rccl* c);

/* ---- In-process transport for ms_prove_sharded (csrc/comm_local.hip): the ranks are THREADS of one process, each with its
 * own ms_ctx (one device each, or several contexts on one device), and the exchanges are device-to-device copies pulled by the
 * receiving rank, ordered between the ranks' streams by HIP events - peer copies over xGMI when the contexts sit on
 * different GPUs. For a host that drives a whole node from one process (the reference's prover is one process with a thread
 * pool, Cargo.toml:45) and for tests: RCCL refuses two ranks on one device, thread ranks do not, so BASELINE config 3 runs at
 * world 8 on a one-GPU box. Create the group once, then one handle per rank (any thread); every rank's thread passes
 * ms_comm_local_table() to ms_prove_sharded. A rank that fails or never arrives does not hang the others: the rendezvous times
 * out (MSAMD_LOCAL_TIMEOUT_S, default 120) and ms_comm_local_group_abort wakes every waiting rank with an error. Handles and
 * group may be destroyed in any order. */
typedef struct ms_comm_local_group ms_comm_local_group;
typedef struct ms_comm_local ms_comm_local;
int32_t ms_comm_local_group_create(int32_t world, ms_comm_local_group** out);
void ms_comm_local_group_abort(ms_comm_local_group* g);
void ms_comm_local_group_destroy(ms_comm_local_group* g);
int32_t ms_comm_local_create(ms_comm_local_group* g, ms_ctx* ctx, int32_t rank, ms_comm_local** out);
const ms_comm* ms_comm_local_table(ms_comm_local* c);
uint64_t ms_comm_local_bytes_moved(ms_comm_local* c);
void ms_comm_local_destroy(ms_comm_local* c);

/* ---- PCS-level entry points (host buffers in, host buffers out) */
/* out[k] = sum_j in[j] w_h^{jk} per column (inverse != 0: the inverse transform incl. 1/h); natural order both sides */
int32_t ms_dft_batch(ms_ctx* ctx, const uint64_t* in, size_t h, size_t w, int32_t inverse, uint64_t* out);
/* coset_lde_batch(evals, log_blowup, GENERATOR).bit_reverse_rows(): (h << log_blowup) x w */
int32_t ms_coset_lde_batch(ms_ctx* ctx, const uint64_t* in, size_t h, size_t w, uint32_t log_blowup, uint64_t* out);
/* quotient evaluations in natural order on the quotient domain ((n q) x D) -> committed LDE ((n B) x (q D)) */
int32_t ms_quotient_lde(ms_ctx* ctx, const uint64_t* in, uint32_t log_n, uint32_t log_q, uint32_t log_blowup, size_t D,
                        uint64_t* out);
/* Merkle commit over matrices of power-of-two heights (mixed heights allowed); cap_out: 32 << cap_height bytes */
int32_t ms_mmcs_commit(ms_ctx* ctx, size_t n, const uint64_t* const* mats, const uint64_t* heights,
                       const uint64_t* widths, uint32_t cap_height, uint8_t* cap_out, ms_mmcs** out);
/* open_batch(index): opened rows concatenated in matrix order; siblings bottom-up; *n_siblings written */
int32_t ms_mmcs_open(ms_mmcs* m, size_t index, uint64_t* vals_out, uint8_t* proof_out, size_t* n_siblings);
void ms_mmcs_destroy(ms_mmcs* m);
/* MerkleTreeMmcs::verify_batch for many openings of one commitment at once, one device thread per opening. The commitment
 * is described by its cap (32 << cap_height bytes, cap_height <= log2 of the tallest height) and the matrices' heights and
 * widths. Opening k is indices[k], the opened rows concatenated in matrix order (sum of widths words each) and its siblings
 * bottom-up ((log2 max height - cap_height) * 32 bytes each): the layout ms_mmcs_open writes. ok_out[k] = 1 / 0; an index
 * beyond the tallest height or a non-canonical value is refused (0). n_openings = 0 is MS_OK. */
int32_t ms_mmcs_verify_batch(ms_ctx* ctx, size_t n_mats, const uint64_t* heights, const uint64_t* widths, const uint8_t* cap,
                             uint32_t cap_height, size_t n_openings, const uint64_t* indices, const uint64_t* vals,
                             const uint8_t* siblings, uint8_t* ok_out);
int32_t ms_blake3(ms_ctx* ctx, const uint8_t* bytes, size_t len, uint8_t out32[32]);

/* ---- Pcs::commit / Pcs::open / Pcs::verify on their own (examples/pcs_example.rs:64-121; the calls of src/prover.rs:350,419,580
 * for a host that keeps its own prover loop). The transcript is a handle: ms_challenger_create(params7) is
 * config.initialise_challenger() (src/types.rs:118-130) for the seven parameter words [log_blowup, cap_height,
 * log_final_poly_len, max_log_arity, num_queries, commit_proof_of_work_bits, query_proof_of_work_bits].
 * ms_pcs_commit: evaluations over the natural domains (row-major, heights[i] x widths[i]) -> coset LDE + Merkle tree, all
 * kept on the device behind ms_mmcs. ms_pcs_open: one ms_mmcs per round; n_points has one entry per matrix (rounds
 * flattened, at most two points per matrix), points holds (c0, c1) per point. Over ALL rounds the matrices of one LDE
 * height may be opened at no more than two distinct points; a pair (z, z g), g the generator of the matrix's trace domain,
 * counts as two. A third point at a height fails with MS_ERR ("more than two opening points at one LDE height") after
 * the opened values have been absorbed: the context stays usable, the challenger has been advanced and must be restarted
 * from a fresh one. (Plonky3 has no such limit, and neither has msbb_pcs_open, which keeps the limit of two points per
 * matrix only.) A matrix may have no point; so may every matrix of a height or of a round. Opened values are written in
 * round -> matrix -> point -> column order (2 words each); fri_out receives the FriProof (the opening_proof field of
 * Proof::to_bytes); MS_ERR_BUFFER with *fri_len = needed size if a capacity is too small (the challenger has then been
 * advanced: restart from a fresh one). ms_pcs_verify: the same rounds described by their caps (32-byte digests), log2 domain
 * sizes and widths; *accepted = 1 / 0. */
typedef struct ms_challenger ms_challenger;
int32_t ms_challenger_create(const uint64_t params7[7], ms_challenger** out);
void ms_challenger_destroy(ms_challenger* ch);
int32_t ms_challenger_observe(ms_challenger* ch, const uint64_t* elems, size_t n);
int32_t ms_challenger_observe_digests(ms_challenger* ch, const uint8_t* digests, size_t n);
int32_t ms_challenger_sample_ext(ms_challenger* ch, uint64_t out2[2]);
int32_t ms_challenger_sample_bits(ms_challenger* ch, uint32_t bits, uint64_t* out);
int32_t ms_pcs_commit(ms_ctx* ctx, uint32_t log_blowup, uint32_t cap_height, size_t n, const uint64_t* const* evals,
                      const uint64_t* heights, const uint64_t* widths, uint8_t* cap_out, ms_mmcs** out);
int32_t ms_pcs_open(ms_ctx* ctx, const uint64_t params7[7], size_t n_rounds, ms_mmcs* const* rounds, const uint64_t* n_points,
                    const uint64_t* points, ms_challenger* ch, uint64_t* opened_out, size_t opened_cap_words, uint8_t* fri_out,
                    size_t fri_cap, size_t* fri_len);
int32_t ms_pcs_verify(const uint64_t params7[7], size_t n_rounds, const uint8_t* const* caps, const uint64_t* cap_sizes,
                      const uint64_t* n_mats, const uint64_t* log_n, const uint64_t* widths, const uint64_t* n_points,
                      const uint64_t* points, const uint64_t* opened, const uint8_t* fri, size_t fri_len, ms_challenger* ch,
                      int32_t* accepted);

/* ---- Level 2: the prover's steps on DEVICE HANDLES, for a host that keeps the reference's own prover loop
 * (src/prover.rs:290-603: "Rust host keeps the multi-circuit / lookup bookkeeping and calls kernels through FFI") and
 * calls the device once per step. Between the calls only commitments, accumulators and challenges cross the boundary;
 * traces, LDEs and trees stay in HBM behind ms_witness / ms_trace / ms_mmcs. Together with ms_challenger_* and ms_pcs_open
 * these are all the device calls of prove_multiple_claims (tests/test_gpu_level2.py drives exactly that loop from Python
 * and obtains the bytes ms_prove writes):
 *   ms_witness_commit_stage1      pcs.commit(stage-1 traces)                             src/prover.rs:338-350
 *   ms_challenger_observe_claims  the claims absorbed by the transcript                  src/prover.rs:369-373
 *   ms_witness_claims_accumulator the initial accumulator                                src/prover.rs:382-387
 *   ms_stage2_build               LookupValues::stage_2_traces -> evaluation handles     src/prover.rs:400, src/lookup.rs:472-555
 *   ms_pcs_commit_traces          pcs.commit(stage-2 traces) on those handles            src/prover.rs:414-419
 *   ms_quotient                   quotient_values + shifted_quotient_slices +            src/prover.rs:459-468,483,511-517
 *                                 lde_from_shifted_coefficients -> LDE handle
 *   ms_pcs_commit_ldes            pcs.commit_ldes                                        src/prover.rs:526
 *   ms_system_preprocessed_mmcs   the ProverKey's preprocessed prover data (a view)      src/system.rs:190-195
 * Matrices of a commitment are indexed by ACTIVE position (circuits with an empty trace are skipped), as the reference's
 * per-stage matrix lists are (src/prover.rs:216-225). A handle consumed by a commit call keeps existing but is empty;
 * destroy it like any other. Host-resident witnesses (ms_witness_create_host) are not accepted here. */
typedef struct ms_trace ms_trace;
void ms_trace_destroy(ms_trace* t);
int32_t ms_trace_info(const ms_trace* t, uint64_t out3[3]); /* height, width, kind (0 evaluations, 1 LDE) */
int32_t ms_system_preprocessed_mmcs(ms_system* sys, ms_mmcs** out); /* *out = NULL when the system has no preprocessed trace */
int32_t ms_witness_commit_stage1(ms_witness* w, uint8_t* cap_out, ms_mmcs** out);
int32_t ms_challenger_observe_claims(ms_challenger* ch, ms_witness* w);
int32_t ms_witness_claims_accumulator(ms_witness* w, const uint64_t beta[2], const uint64_t gamma[2], uint64_t acc_out[2]);
/* accs_out: 2 words per active circuit (the accumulator after each circuit, src/lookup.rs:544-550); traces_out: one handle
 * per active circuit */
int32_t ms_stage2_build(ms_witness* w, const uint64_t beta[2], const uint64_t gamma[2], const uint64_t acc_in[2], uint64_t* accs_out,
                        ms_trace** traces_out);
int32_t ms_pcs_commit_traces(ms_ctx* ctx, uint32_t log_blowup, uint32_t cap_height, size_t n, ms_trace* const* evals, uint8_t* cap_out,
                             ms_mmcs** out);
/* publics8 = [beta, gamma, acc_in, acc_out] as (c0, c1) pairs (src/lookup.rs:78-84); s1 / s2: the stage commitments and
 * the circuit's matrix index inside each */
int32_t ms_quotient(ms_system* sys, size_t circuit, uint32_t log_n, ms_mmcs* s1, size_t s1_idx, ms_mmcs* s2, size_t s2_idx,
                    const uint64_t publics8[8], const uint64_t alpha[2], ms_trace** q_lde_out);
int32_t ms_pcs_commit_ldes(ms_ctx* ctx, uint32_t cap_height, size_t n, ms_trace* const* ldes, uint8_t* cap_out, ms_mmcs** out);

/* ---- in-tree kernels of the reference, host buffers in and out (kernel-level parity tests) */
int32_t ms_stage2_trace(ms_ctx* ctx, size_t height, size_t num_lookups, const uint64_t* mult,
                        const uint64_t* arg_offsets, const uint64_t* args, const uint64_t beta[2],
                        const uint64_t gamma[2], const uint64_t acc_in[2], uint64_t* trace_out, uint64_t acc_out[2]);
int32_t ms_claims_accumulator(ms_ctx* ctx, size_t n_claims, const uint64_t* claim_offsets, const uint64_t* claim_data,
                              const uint64_t beta[2], const uint64_t gamma[2], uint64_t acc_out[2]);
/* traces given as natural-order evaluations on the quotient domain ((n q) rows each, row-major); out: (n q) x 2 */
int32_t ms_quotient_values(ms_system* sys, size_t circuit, const uint64_t publics8[8], uint32_t log_n, uint32_t log_q,
                           const uint64_t* pre_q, const uint64_t* s1_q, const uint64_t* s2_q, const uint64_t alpha[2],
                           uint64_t* out);
/* element-wise field ops on device, for arithmetic known-answer tests: op 0 add, 1 sub, 2 mul, 3 inverse(a),
 * 4 ext2 mul (pairs), 5 ext2 inverse (pairs) */
int32_t ms_field_op(ms_ctx* ctx, int32_t op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* MSTARK_H */
