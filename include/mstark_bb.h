/* mstark_bb.h — C ABI of the MI355X (gfx950) prover for multi-stark's SECOND configuration: BabyBear, degree-4
 * binomial extension, Poseidon2 sponge / compression, DuplexChallenger — the StarkGenericConfig instantiated in
 * /root/reference/src/test_circuits/baby_bear_config.rs:28-127 (BASELINE config 4). Same conventions as mstark.h
 * (which this header builds on: ms_ctx, status codes, ms_last_error), with these differences:
 *   - BabyBear elements cross the ABI as canonical u32; an Ext4 value is four consecutive u32 (c0..c3); a digest is
 *     eight u32 ([BabyBear; 8]);
 *   - the proof bytes carry every field element the way p3-monty-31 serialises it (its Montgomery word, 4 bytes LE);
 *   - the system blob starts with the magic "MSYB01" and carries, after the seven parameters, the 141 round constants
 *     of Poseidon2BabyBear<16> (8 x 16 external, then 13 internal, canonical). The reference draws them from
 *     rand::SmallRng::seed_from_u64(42) (baby_bear_config.rs:54-55); that stream cannot be reproduced without the crate,
 *     so a maintainer passes `perm`'s constants in.
 *
 * What each entry point replaces in /root/reference (SC = BabyBearPoseidon2Config):
 *   msbb_system_*    System::<SC>::new + ProverKey                   src/system.rs:115-203
 *   msbb_witness_*   SystemWitness::from_stage_1                      src/system.rs:225-328
 *   msbb_prove       System::<SC>::prove_multiple_claims              src/prover.rs:290-603
 *   msbb_dft_batch / msbb_coset_lde_batch    Radix2DitParallel<BabyBear>   baby_bear_config.rs:38; src/prover.rs:350,419,650,716
 *   msbb_mmcs_*      MerkleTreeMmcs<.., PaddingFreeSponge<Perm,16,8,8>, TruncatedPermutation<Perm,2,8,16>, 2, 8>   baby_bear_config.rs:30-33
 *   msbb_poseidon2_permute   Poseidon2BabyBear<16>::permute           baby_bear_config.rs:29
 *   msbb_verify      System::<SC>::verify_multiple_claims             src/verifier.rs:208-532
 *   msbb_verify_batch        the same for N proofs, queries and Merkle paths on the device
 */
#ifndef MSTARK_BB_H
#define MSTARK_BB_H

#include "mstark.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct msbb_system msbb_system;   /* System<BabyBearPoseidon2Config> + ProverKey */
typedef struct msbb_witness msbb_witness; /* SystemWitness + claims, resident in HBM */
typedef struct msbb_mmcs msbb_mmcs;       /* ProverData of one commitment */

int32_t msbb_system_create(ms_ctx* ctx, const uint8_t* blob, size_t len, msbb_system** out);
void msbb_system_destroy(msbb_system* sys);
/* preprocessed commitment: n_digests * 8 canonical words */
int32_t msbb_system_preprocessed_commit(const msbb_system* sys, uint32_t* out, size_t cap_words, size_t* n_digests);
/* the nine numbers of ms_system_circuit_info */
int32_t msbb_system_circuit_info(const msbb_system* sys, size_t circuit, uint64_t out9[9]);
/* as ms_system_circuit_kernels; this configuration generates the quotient kernel only: *flags = MS_KERNEL_QUOTIENT or 0 */
int32_t msbb_system_circuit_kernels(const msbb_system* sys, size_t circuit, uint32_t* flags);

/* traces[i]: heights[i] x main_width_i row-major canonical u32 (height 0 = inactive circuit). The lookup values of
 * SystemWitness::from_stage_1 (src/system.rs:244-328) are computed on the device. Claims: offsets (n_claims + 1) into
 * claim_data. */
int32_t msbb_witness_create(msbb_system* sys, const uint32_t* const* traces, const uint64_t* heights, size_t n_claims,
                            const uint64_t* claim_offsets, const uint32_t* claim_data, msbb_witness** out);
/* A SystemWitness that STAYS in host memory - what the reference's prove() is handed (src/prover.rs:290-295; the setup closure
 * of a criterion bench builds it). Values are validated and the caller's trace buffers page-locked here (*pinned = 1 when
 * every range could be; otherwise the uploads go through a page-locked bounce buffer; the locks are counted per range as for
 * ms_witness_create_host); they must stay valid and unchanged until msbb_witness_destroy. Every msbb_prove on such a witness
 * uploads traces and claims, runs from_stage_1 on the device and releases the device copies: its wall time is the reference's
 * timed region (witness in host memory at the start, proof bytes in host memory at the end). */
int32_t msbb_witness_create_host(msbb_system* sys, const uint32_t* const* traces, const uint64_t* heights, size_t n_claims,
                                 const uint64_t* claim_offsets, const uint32_t* claim_data, int32_t* pinned /* nullable */,
                                 msbb_witness** out);
/* ms_witness_create_device for this configuration: the traces lie in device memory as ms_dev_matrix views (include/mstark.h)
 * with elem_bytes 1, 2 or 4; a 4-byte value >= p is refused with its circuit, row and column; the library's copy is the
 * column-major Montgomery matrix msbb_witness_create would have made. Same copy semantics, producer_stream ordering, single
 * host wait on the traces' path and host-side refusals. Claims come from host memory, as for msbb_witness_create. After an
 * allocation failure (MS_ERR) of this call or of msbb_witness_create there is no witness, nothing queued still reads the
 * caller's buffers, which the call never writes, and the call may be made again. */
int32_t msbb_witness_create_device(msbb_system* sys, const ms_dev_matrix* traces /* one per circuit */, size_t n_claims,
                                   const uint64_t* claim_offsets, const uint32_t* claim_data, void* producer_stream /* hipStream_t, nullable */,
                                   msbb_witness** out);
void msbb_witness_destroy(msbb_witness* w);

/* ---- Witness check: ms_witness_check (include/mstark.h, "Witness check") for this configuration - its definition read over
 * BabyBear. Every active circuit, every row r, the circuit's user constraint roots (`zeros`, in that order) on the values the
 * BabyBear quotient kernel would see on the trace domain at x = w^r, w = the two-adic generator of order n (0x1a427a41 squared
 * 27 - log n times): main and preprocessed variables at row r and (r + 1) mod n; is_first = n at row 0 (else 0), is_last = n w
 * at row n - 1 (else 0), is_transition = w^r - w^-1; the stage-2 columns msbb_stage2_build makes under the caller's (beta,
 * gamma) - four base coordinates per lookup - and the 16 public coordinates [beta, gamma, acc_in, acc_out], the accumulator
 * chained as msbb_stage2_build chains it: the claims' accumulator first, then each active circuit's total. logUp constraints are
 * not evaluated; of the lookups the balance is checked: the accumulator behind the last active circuit must be zero in all four
 * coordinates.
 *   Report. *verdict: the mask of MS_CHECK_CONSTRAINT | MS_CHECK_LOOKUPS. circuits: MSBB_CHECK_CIRCUIT_WORDS words per circuit
 * of the system, inactive ones included:
 *   [0] height  [1] failing rows  [2] smallest failing row  [3] smallest failing root at that row  [4] its value (canonical)
 *   [5..8] the accumulator behind the circuit (canonical; zeros for an inactive circuit)  [9] number of roots  [10] which kernel
 *   form ran (low byte: 1 thread per row / slots in LDS, 2 wave per row, 3 few lanes with large LDS, 4 global scratch, 0 none)
 *   and its lanes per workgroup << 8  [11] where this circuit's roots start in root_counts / root_first.
 * [2], [3] are all-ones when no row fails. root_counts / root_first: as for ms_witness_check; MS_ERR_BUFFER when roots_cap is
 * below the system's total. Every figure is deterministic. A failed check is MS_OK with a non-zero verdict.
 *   Misuse (MS_ERR, text via ms_last_error(), the context stays usable): a host-resident witness (msbb_witness_create_host); a
 * coordinate of beta or gamma >= p; a null argument. Accepted: msbb_witness_create, msbb_witness_create_device. The witness is
 * not changed: msbb_prove behind a check writes the bytes it writes without one. Host waits: one per call, for the report
 * (the first check of a circuit also builds its check program). After an allocation failure (MS_ERR) the witness is unchanged
 * and no half-built check program is kept: the next check builds it again and gives the full report. */
#define MSBB_CHECK_CIRCUIT_WORDS 12
int32_t msbb_witness_check(msbb_witness* w, const uint32_t beta[4], const uint32_t gamma[4], uint32_t* verdict,
                           uint64_t* circuits /* n_circuits x MSBB_CHECK_CIRCUIT_WORDS */, uint64_t* root_counts /* nullable */,
                           uint64_t* root_first /* nullable */, size_t roots_cap);
/* out4 = [user constraint roots = constraint_count - 4 max(num_lookups, 1), live slots of the check's program, steps of its
 * wave-per-row schedule (0: none), lanes per workgroup of the thread-per-row form with 4-byte slots in LDS: 256 up to 63 slots,
 * 128 up to 127, 64 up to 255 (0: the slot file does not fit)] */
int32_t msbb_system_check_info(const msbb_system* sys, size_t circuit, uint64_t out4[4]);

/* ---- Lookup balance, exact: ms_witness_lookup_balance (include/mstark.h, "Lookup balance") for this configuration - its
 * definition read over p = 2^31 - 2^27 + 1. Messages are the claims (multiplicity 1) and every (active circuit, row, lookup
 * slot) of non-zero multiplicity, with the multiplicity and arguments msbb_stage2_build evaluates; tuples are compared after
 * trailing zeros are stripped; a group's net is the sum of its multiplicities modulo p; origin order is claims by index, then
 * the circuits in system order, row-major, slot last. It takes no challenges.
 *   Report: the layout of ms_witness_lookup_balance. summary: [0] messages  [1] groups  [2] unbalanced groups  [3] entries
 * written = min([2], entries_cap). entries: MS_LB_ENTRY_WORDS words each, the same eight fields ([0] circuit or MS_LB_CLAIMS,
 * [1] row or claim index, [2] slot, [3] net, canonical and non-zero, [4] members, [5] length of the stripped tuple, [6] where it
 * starts in args_out - all-ones for a tuple that would end behind args_cap - [7] reserved, 0), in ascending order of first
 * origin whatever their total number. args_out: the stripped tuples as canonical 4-byte words, packed in entry order.
 * slot_counts (nullable): sum(num_lookups) + 1 words, per lookup slot in system order and then the claims, the messages that
 * belong to an unbalanced group; MS_ERR_BUFFER when slots_cap is below that. Every figure is deterministic.
 *   An unbalanced witness is MS_OK. MS_ERR (text via ms_last_error(), the context stays usable) is for misuse: a host-resident
 * witness (msbb_witness_create_host); a witness that does not belong to the system; a null w or summary; a null buffer with a
 * non-zero capacity; 2^32 messages or more (each group's multiplicities are summed in one 64-bit word, exact below that). A
 * system without lookups and without claims: MS_OK, zeros. The witness is not changed: msbb_prove behind the call writes the
 * bytes it writes without it.
 *   Memory: the witness keeps no lookup values, so each active circuit's are swept into temporaries of the call -
 * 4 x height x (num_lookups + args_width) bytes, plus 4 x height x lookup prefix length of scratch while its sweep runs; the
 * grouping table takes 32 bytes x cap, cap = the power of two >= max(64, 2 x M), M = claims + sum over the active circuits of
 * height x num_lookups (134 MB for MulAir at 2^20 rows, M = 2^21), plus M / 8 bytes of marks. An allocation failure is MS_ERR
 * naming the bytes; the witness is unchanged by it, as by the call, and the call may be made again. MSAMD_LB_HASH_BITS=k (diagnostics, read per call) keeps only the low k bits of the hash, as for
 * ms_witness_lookup_balance: the report is the same, by a longer way.
 *   Host waits: one when the witness is balanced; one more, to fetch entries and tuples, when it is not and entries_cap > 0. */
int32_t msbb_witness_lookup_balance(msbb_witness* w, uint64_t summary[4], uint64_t* entries, size_t entries_cap /* nullable with cap 0 */,
                                    uint32_t* args_out, size_t args_cap /* nullable with cap 0; canonical values */,
                                    uint64_t* slot_counts /* nullable */, size_t slots_cap);

/* ---- Table multiplicity columns derived on the device: ms_witness_derive_multiplicities (include/mstark.h, "Table multiplicity
 * columns") for this configuration - its definition read over p = 2^31 - 2^27 + 1, with the same notions: target, eligibility,
 * demand D(t), provider (the target row of smallest origin with the tuple), duplicates, unserved groups. Messages, stripped tuples
 * and origin order are those of msbb_witness_lookup_balance above. ms_mult_target, the summary words - [0] demand messages
 * [1] demand groups  [2] served groups with D != 0  [3] unserved groups  [4] duplicate target rows  [5] entries written = min([3],
 * entries_cap) - and the entries' layout and order are those of mstark.h. What differs from the Goldilocks call:
 *   Values cross the ABI as canonical u32: args_out holds the stripped tuples of the unserved groups as 4-byte words.
 *   Storage: the library's copy of a trace is a column-major matrix of Montgomery words. The provider's cell of column m receives
 * v - D(t) for a pull, (p - D(t)) mod p for a push - in that form, every other target row 0; msbb_witness_trace shows the
 * canonical values.
 *   No held lookup values: a witness of this configuration holds none - msbb_prove, msbb_stage2_build, msbb_witness_check and
 * msbb_witness_lookup_balance each compute them from the traces - so there is nothing beside the column to update, and every call
 * behind this one sees the derived column. Other columns, other traces and the claims stay byte-identical.
 *   Message limit: 2^32 messages or more (target rows count) is MS_ERR, as for msbb_witness_lookup_balance: a group's canonical
 * multiplicities are summed in one 64-bit word, exact below that.
 *   Unserved demand, n_targets == 0 (a pure demand count with no writes) and an inactive target circuit are MS_OK. MS_ERR (text
 * via ms_last_error(), the context stays usable; each is refused before anything is written): a host-resident witness; a witness
 * that does not belong to the system; a null w or summary; null targets with n_targets > 0; a null buffer with a non-zero
 * capacity; a target that is out of range, not eligible, or that shares its derived column with an earlier target.
 *   Memory: the grouping table takes 40 bytes x cap, cap = the power of two >= max(64, 2 x M), M = claims + sum over the active
 * circuits of height x num_lookups (target slots included) - the four arrays of the balance and one word per slot for the
 * provider - plus 8 bytes per target row, M / 8 bytes of marks, the sweep temporaries of msbb_witness_lookup_balance and, unless
 * entries_cap = 0, the entries and tuples at the caller's capacities. An allocation failure is MS_ERR naming the bytes; every
 * buffer is allocated before the first write, so the traces and the claims are then as they were before the call, and the same
 * call may be made again. MSAMD_LB_HASH_BITS as for msbb_witness_lookup_balance.
 *   Host waits: one, for the summary; one more, to fetch entries and tuples, when something is unserved and entries_cap > 0. */
/* the three numbers of ms_system_multiplicity_slot: [eligibility, column m, sign: 0 push, 1 pull]; one classifier serves both
 * configurations, as it reads the node program only */
int32_t msbb_system_multiplicity_slot(const msbb_system* sys, size_t circuit, size_t slot, uint64_t out3[3]);
int32_t msbb_witness_derive_multiplicities(msbb_witness* w, const ms_mult_target* targets, size_t n_targets,
                                           uint64_t summary[MS_DM_SUMMARY_WORDS], uint64_t* entries, size_t entries_cap /* nullable with cap 0 */,
                                           uint32_t* args_out, size_t args_cap /* nullable with cap 0; canonical values */);

/* ---- Trace columns filled on the device from a program: ms_witness_fill (include/mstark.h, "Trace columns filled on the device")
 * for this configuration, its definition read over p = 2^31 - 2^27 + 1, with the same notions: fill program, steps, the
 * sequential definition (a read of an assigned column at offset 0 sees the latest earlier step; offset-1 reads only of columns no
 * step assigns; the last assignment of a column wins), inputs and producer_stream. With msbb_witness_derive_multiplicities behind
 * it the pipeline of the other configuration runs here too: fill, derive, check, prove, all in HBM. What differs from the
 * Goldilocks call:
 *   Blob: the same layout - u64 words, a header of six, nodes [kind | source << 8 | offset << 16, a, b], steps [dst, root] - under
 * the magic word 0x3130424C49464D00 ("\0MFILB01"). The blob carries no other mark of its field and its constants were folded
 * modulo the field it was authored over (frontend.compile_fill under frontend.field(BABYBEAR)), so each call refuses the other
 * field's magic as a wrong magic instead of running the program with another meaning.
 *   Values: operands are the canonical integers in [0, p). bits(x, lo, length) needs 1 <= length and lo + length <= 32;
 * xor(x, y) = (x ^ y) mod p, one conditional subtraction as x ^ y < 2^31 < 2 p; and, lt, inv0 (0 -> 0) and row (r: heights are
 * at most 2^27 < p) as there. A constant >= p is refused as non-canonical.
 *   Indexed reads: node kind 22, `at`, is the "INDEXED READS" paragraph of include/mstark.h read over this p: the row operand is
 * the canonical integer in [0, p), compared with the source's height (n, or the input matrix's own height) before anything is
 * addressed, and a row from the height on reads 0. A program of the first format is one group: an `at` of a main column that
 * any step assigns is refused. The same refusals as there.
 *   inputs: an ms_dev_matrix as for msbb_witness_create_device - elem_bytes 1, 2 or 4 - of width n_inputs and a height in
 * [0, n]; rows at or beyond its height read 0. A 4-byte element >= p is refused, naming the first offender in row-major order
 * ("non-canonical input value: row 5, column 1").
 *   Storage: the library's copy of a trace, and of a preprocessed trace, is a column-major matrix of Montgomery words. The call
 * reads and writes that form; every written cell is the Montgomery word of a canonical value, and msbb_witness_trace shows the
 * canonical values.
 *   No held lookup values: a witness of this configuration holds none, so nothing beside the assigned columns changes - other
 * columns, other traces and the claims stay byte-identical - and every call behind this one sees the filled columns.
 *   summary: [0] rows  [1] steps  [2] instructions executed per row  [3] kernel form: lanes per workgroup with the slot file in
 * LDS (4-byte slots: 256 lanes up to 64 live slots, 128 up to 128, 64 up to 256), 0 = slots in a global scratch walked in row
 * batches.
 *   MS_ERR (text via ms_last_error(), starting "msbb_witness_fill: "; each refusal comes before anything is written, the context
 * stays usable): the list of ms_witness_fill without its held-lookup case - a host-resident witness; a witness that does not
 * belong to the system; a circuit out of range or inactive; a blob with a wrong magic, a length that does not match its counts,
 * widths other than the circuit's, a dst or a variable out of range, a forward operand, bad bits fields, a non-canonical
 * constant or a refused node kind; an offset-1 read of an assigned column; an input matrix that fails the checks of
 * msbb_witness_create_device (8-byte elements among them); an input height above n; n_inputs > 0 with inputs = NULL; a
 * non-canonical input element; a null w, program or summary. An allocation failure is MS_ERR as well and comes before the
 * first write too: the witness is as it was before the call, and the same call may be made again.
 *   Host waits: one when the program reads inputs of height > 0 (the offender word, before the first write); none otherwise.
 *
 *   SCAN STEPS: columns that follow the previous row (running sums and products, counters, Horner accumulators) - the paragraph
 * of include/mstark.h read over p = 2^31 - 2^27 + 1. A step is ORDINARY, (dst, root) as above, or a SCAN (dst, mul root A, add
 * root B, init). The definition is column at a time: step k computes its whole column before step k + 1 starts - for ordinary
 * steps that equals the definition above. A scan step writes
 *     trace[0][dst]     = init
 *     trace[r + 1][dst] = A(r) * trace[r][dst] + B(r)  (mod p),  r = 0 .. n - 2
 * where A(r), B(r) are the values the roots would have at row r if an ordinary step stood at that position. A(n - 1) and
 * B(n - 1) are not used: there is no wrap-around, as under is_transition; at n = 1 only init is written. Every written value
 * is canonical - every stored cell is the Montgomery word of a canonical value. The affine maps x -> A x + B compose
 * associatively and exactly, so the device's parallel scan is bit-identical to this loop.
 *   Groups. Each scan step is a group of its own; each maximal run of ordinary steps between scans is a group. Inside a group
 * the rules above hold (an offset-0 read of an assigned column sees the latest earlier step of the group, shared subexpressions
 * are computed once, each cell is stored once per group); a read of a column that an earlier group assigned comes from the
 * trace. A read of main column m at offset 1 by a step of group g is allowed exactly when no step of group g or of any later
 * group assigns m - with one group this is the rule above - so a later step may read the next row of a finished scan column
 * (diff = s_next - s; at row n - 1 that is row 0). The `at` rule applies by groups in the same way: an `at` of main column m is
 * refused when a step of the same or of a later group assigns m, so a later group may read a finished scan column at offset 0,
 * at offset 1 or at a computed row. The coefficients of a scan step may not read their own dst at either offset, nor index it.
 *   Blob. A program without a scan step keeps "\0MFILB01" byte for byte. With scans: the magic word 0x3230424C49464D00
 * ("\0MFILB02") and the layout of "\0MFILL02" - main_width, pre_width, n_inputs, n_nodes, n_steps, n_scans (seven header words
 * with the magic); the nodes; the steps as [dst, root], root of a scan step being its add root B; n_scans records [step index,
 * mul root, init] with strictly ascending step indices and init < p. Nodes that no step reaches are not subject to the
 * offset-1 rule in this format. Each call goes on refusing BOTH magics of the other field as a wrong magic.
 * msbb_witness_fill also refuses the third format of include/mstark.h ("PEER READS", magic "\0MFILL03") by its magic: this
 * configuration has no peer reads yet. A claim program ("\0MCLAIB1", msbb_witness_claims_fill below) is refused as a wrong
 * magic too: it is no fill program.
 *   Not part of this: accumulators over the degree-4 extension (four coupled columns that follow the previous row together,
 * as the running sum of a lookup argument over the challenge field) - a scan step is one base-field column.
 *   Execution: the groups in order on the context's stream - an ordinary group as above, a scan group as a coefficient pass
 * (the same kernel, writing A and B as Montgomery words into a column-major temporary) and a three-launch scan over tiles of T
 * rows (msbb_fill_scan_info tells T): a reduction per tile, ONE workgroup that turns the tile aggregates into the value in
 * front of each tile, R = 256 aggregates per round with a carry between rounds, and the apply launch that stores each dst cell
 * once; a circuit of at most T rows takes the apply launch alone. A mul root that is the constant 1 takes the additive form (B
 * alone, no multiplications). Temporaries of the call: 8 bytes x n (4 when every scan is additive), shared by its scans, plus
 * 12 bytes per tile, next to the program tables, the scratch of the global-scratch form and the ingest temporary; all of them
 * are allocated before the first write to the trace, so after an allocation failure the witness is as it was and the same call
 * may be made again - which matters here, since a later group reads what an earlier group wrote. Host waits are unchanged.
 * summary for such a program: [1] all steps, [2] instructions per row summed over every launch of the fill kernel, coefficient
 * passes included, [3] the smallest lanes figure over those launches (0 if any of them uses the global scratch).
 *   MS_ERR in addition, before anything is written: a length that does not match the three counts; a scan record whose step
 * index is out of range or not above the one before, whose mul root is out of range or whose init is >= p; a scan step whose
 * coefficients read its own dst; an offset-1 read or an `at` that the group rule refuses. */
int32_t msbb_witness_fill(msbb_witness* w, size_t circuit, const uint8_t* program, size_t program_len,
                          const ms_dev_matrix* inputs /* nullable with n_inputs 0 */, void* producer_stream /* hipStream_t, nullable */,
                          uint64_t summary[4]);
/* Host code, no device: checks a fill program as msbb_witness_fill does (everything that needs no witness) and describes how it
 * would run: out4 = [instructions per row, live slots, lanes per workgroup of the LDS form (0: global scratch), distinct assigned
 * columns]. Texts start "msbb_fill_program_info: ". For a program with scan steps: instructions summed over the launches of the
 * fill kernel, the largest slot count and the smallest lanes figure among them, and the dst columns of scan steps count as
 * assigned. */
int32_t msbb_fill_program_info(const uint8_t* program, size_t program_len, uint64_t out4[4]);
/* Host code, no device: the same checks, and out4 = [scan steps, launches of the fill kernel (one per group of ordinary steps,
 * one coefficient pass per scan), scans in the additive form, T = rows per scan tile]. Texts start "msbb_fill_scan_info: ". */
int32_t msbb_fill_scan_info(const uint8_t* program, size_t program_len, uint64_t out4[4]);

/* ---- Claim programs: ms_witness_claims_fill (include/mstark.h, "CLAIM PROGRAMS") for this configuration, its definition read
 * over p = 2^31 - 2^27 + 1, with the same notions: W element expressions (1 <= W <= 2^16) and an optional keep, exactly one claim
 * per kept row r < rows <= n in ascending row order, MS_CLAIMS_REPLACE / MS_CLAIMS_APPEND, the same summary words, the same
 * refused nodes (peer sources, publics, selectors, stage-2 variables), no scan steps, neither the offset-1 rule nor the group
 * rule, the next row of row n - 1 being row 0, an input row from the input height on reading 0 and an index from the source's
 * height on reading 0 without a load. With it the route of the other configuration runs here too and leaves HBM only for the
 * proof bytes: msbb_witness_create_device (zero traces, no claims), msbb_witness_fill, msbb_witness_claims_fill,
 * msbb_witness_derive_multiplicities, msbb_witness_check, msbb_witness_lookup_balance, msbb_prove. What differs from the
 * Goldilocks call:
 *   The system comes from the witness, as for msbb_witness_fill.
 *   Blob: the same layout - seven header words (magic, main_width, pre_width, n_inputs, n_nodes, W, keep root or all ones), the
 * nodes, the W element roots - under a magic of its own, 0x314249414C434D00 ("\0MCLAIB1"): the blob carries no other mark of its
 * field and its constants were folded modulo it (frontend.compile_claims under frontend.field(BABYBEAR)). Each configuration's
 * calls refuse the other's claim magic, and the other's fill magics, as a wrong magic; "\0MFILB01" / "\0MFILB02" are named as "a
 * fill program, not a claim program".
 *   Values: as in msbb_witness_fill - operands are the canonical integers in [0, p), bits needs lo + length <= 32, xor folds
 * once, a constant >= p is refused, row is r.
 *   inputs: elem_bytes 1, 2 or 4 (8-byte elements are refused); a 4-byte element >= p is refused, naming the first offender in
 * row-major order.
 *   Storage: on the device the claim list is row-major Montgomery words (claim k of a call is W consecutive words) with u64
 * offsets, what msbb_prove and the level-2 calls read; on the host the witness keeps the canonical vectors the transcript
 * absorbs. Both are replaced together. msbb_witness_claims shows canonical values. The keep flag is compared as the stored
 * word: a stored cell is the Montgomery word in [0, p) of a canonical value, which is 0 exactly when the value is 0, so the
 * kept rows are those of the definition. In append mode the new elements start wherever the old ones end; nothing assumes more
 * than 4-byte alignment.
 *   No held lookup values, no sliced and no remote witnesses exist in this configuration, so their refusals do not either.
 *   Execution: the kernel of msbb_witness_fill (4-byte slots: 256 lanes up to 64 live slots, 128 up to 128, 64 up to 256, else a
 * global scratch walked in row batches) with a row-major output of rows x (W + keep) words - the traces are column-major, so
 * with W > 1 a wave's stores are W words apart. Without keep it writes straight into the new claim data; with keep into a
 * temporary that the three launches of the Goldilocks call compact over tiles of 1024 rows, on 4-byte words. Bytes per row:
 * 4 (W + 1) written by the pass, the flag read twice, and 4 W read and 4 W written per kept row; 16 bytes per tile.
 *   The guarantee is that of the Goldilocks call: the new offset and data arrays, device and host, are built beside the
 * witness's own and change places with them last, so MS_ERR at any point - a refusal, an allocation failure, a non-canonical
 * input - leaves claims and traces byte-identical and the context usable. Traces are never written.
 *   Host waits: at most two - the inputs' offender word and the kept total in one read-back (not needed without inputs and
 * without keep), then the host copy: one read-back of the new elements, converted to canonical on the host.
 *   MS_ERR (texts start "msbb_witness_claims_fill: "): a null w, program or summary; a host-resident witness; a witness of
 * another system; mode neither 0 nor 1; a circuit out of range, inactive or without a trace on this device; a blob that
 * msbb_claims_program_info refuses; widths other than the circuit's; a preprocessed trace that is not on the device at this
 * height; rows > n; the input refusals of msbb_witness_fill; a total of 2^60 elements or more. */
int32_t msbb_witness_claims_fill(msbb_witness* w, size_t circuit, const uint8_t* program, size_t program_len, size_t rows,
                                 const ms_dev_matrix* inputs /* nullable with n_inputs 0 */, void* producer_stream /* hipStream_t, nullable */,
                                 uint32_t mode, uint64_t summary[4]);
/* Host code, no device: checks a claim program as msbb_witness_claims_fill does (everything that needs no witness): out4 =
 * [instructions per row, live slots, lanes per workgroup of the LDS form (0: global scratch), W | has_keep << 32]; the refusals
 * of ms_claims_program_info over this field's magics, modulus and value width. Texts start "msbb_claims_program_info: ". */
int32_t msbb_claims_program_info(const uint8_t* program, size_t program_len, uint64_t out4[4]);
/* Diagnostic, as ms_witness_claims: the claims read back from the DEVICE copy and shown as canonical values. *n_claims and
 * *n_elems are always set; offsets_out receives *n_claims + 1 words, data_out *n_elems. MS_ERR_BUFFER when a capacity is too
 * small; nothing is written then. A host-resident witness: MS_ERR. */
int32_t msbb_witness_claims(msbb_witness* w, uint64_t* offsets_out, size_t cap_offsets, uint32_t* data_out, size_t cap_data, size_t* n_claims,
                            size_t* n_elems);

/* ---- The sorting permutation of a circuit's rows, made on the device: ms_witness_argsort (include/mstark.h, "The sorting
 * permutation of a circuit's rows") for this configuration, its definition read over p = 2^31 - 2^27 + 1: row i comes before
 * row j iff (trace[i][k_0], ..., trace[i][k_{m-1}], i) is lexicographically smaller, 1 <= m <= 8, a column may repeat among the
 * keys, ties go by row index, MS_SORT_PERM / MS_SORT_RANK as there. With msbb_witness_fill's indexed reads behind it a sorted
 * copy of a column - a memory log in address order, a range check by sorted differences - is made without leaving HBM, and with
 * its scan steps the running columns over that copy too: sort, gather, scan. What differs from the Goldilocks call:
 *   The system comes from the witness, as for msbb_witness_fill.
 *   Order: cells are compared as the CANONICAL integers in [0, p), not as the Montgomery words that lie in memory (whose order
 * is another one).
 *   Storage: the library's copy of a trace is a column-major matrix of Montgomery words. Every cell of dst_column is written
 * once, as the Montgomery word of a row index or a position; heights are at most 2^27 < p, so each is a canonical value and
 * msbb_witness_trace shows it as it is. No other cell, circuit or claim changes.
 *   No held lookup values: a witness of this configuration holds none, so nothing follows the column.
 *   Execution: the radix sort of ms_witness_argsort over canonical 32-bit keys - FOUR 8-bit digits per key column. One launch
 * per key column reads the column (contiguous), converts and counts its four digit histograms; the host reads all of them in one
 * copy and skips every digit in which all n rows share one value; each pass that runs is the same three launches over tiles of
 * T rows, with keys and row indices in separate 4-byte buffers: 20 bytes per row and pass where the other call moves 32.
 *   summary: [0] rows  [1] key columns  [2] digit passes run  [3] digit passes skipped ([2] + [3] = 4 x key columns).
 *   MS_ERR (text via ms_last_error(), starting "msbb_witness_argsort: "; each refusal comes before anything is written, the
 * context stays usable): a null w or summary, or null key_columns with n_keys > 0; a host-resident witness; a witness that does
 * not belong to its system; a circuit out of range, inactive or without a trace on this device; n_keys 0 or above 8; a key
 * column or dst_column at or beyond main_width; dst_column among the keys; what neither 0 nor 1. A height above 2^27 cannot
 * reach the call: msbb_witness_create, msbb_witness_create_host and msbb_witness_create_device each refuse a trace taller than
 * the two-adicity of the field allows ("trace too tall for the two-adicity of BabyBear"); the call keeps the check all the same.
 * An allocation failure is MS_ERR as well; every buffer is allocated before dst_column is written, so the witness is then as it
 * was before the call, and the same call may be made again.
 *   Host waits: exactly one, the copy of the histograms; nothing has been written to the trace by then.
 *   Temporaries: 16 bytes x n (two key and two index buffers) and 1 KB per tile, next to 4 KB per key column and histogram
 * workgroup (at most 256 of them). */
int32_t msbb_witness_argsort(msbb_witness* w, size_t circuit, const uint32_t* key_columns, size_t n_keys, uint32_t dst_column,
                             uint32_t what /* MS_SORT_PERM, MS_SORT_RANK */, uint64_t summary[4]);
/* Host code, no device: out4 = [T = rows per tile, bits per digit, R = per-tile counts handled per round of the offsets step,
 * largest n_keys]. */
int32_t msbb_sort_info(uint64_t out4[4]);

/* Diagnostics, as ms_witness_trace: one stage-1 trace of a device-resident witness read back, height x main_width, row-major,
 * canonical u32. MS_ERR_BUFFER with *n_words = the needed size; an inactive circuit: 0 words, MS_OK. A host-resident witness or
 * an out-of-range circuit: MS_ERR. */
int32_t msbb_witness_trace(msbb_witness* w, size_t circuit, uint32_t* out, size_t cap_words, size_t* n_words);

/* Writes Proof::to_bytes (src/prover.rs:241-248). stage_ms (optional, 6 doubles) as for ms_prove. */
int32_t msbb_prove(msbb_system* sys, msbb_witness* w, uint8_t* proof_out, size_t cap, size_t* proof_len, double* stage_ms);

/* System::<SC>::verify_multiple_claims (src/verifier.rs:208-532, shape checks :536-695) on the bytes msbb_prove wrote;
 * *verdict as for ms_verify (MS_VERDICT_*). Host code. */
int32_t msbb_verify(msbb_system* sys, size_t n_claims, const uint64_t* claim_offsets, const uint32_t* claim_data,
                    const uint8_t* proof, size_t proof_len, int32_t* verdict);

/* msbb_verify for N proofs of ONE system: verdicts[i] is what msbb_verify writes for (claims i, proof i), for every input.
 * Claims: per proof its count, its offset table (n_claims[i] + 1 entries) and its data; claim_offsets[i] / claim_data[i] may
 * be null where n_claims[i] = 0. n_proofs = 0 is MS_OK. A null proof pointer or null verdicts is MS_ERR. Nothing in a proof's
 * bytes can make the call fail or fault: a malformed proof is a verdict. Per proof the host parses, checks the shape, replays
 * the duplex transcript, checks both proofs of work, the arity schedule and the constraints at zeta; the per-query
 * arithmetic (reduced openings, FRI fold chain, final polynomial) and every Merkle path of the batch run on the device in
 * two launches, with one host wait per call (per 256 MB of openings). An allocation failure is MS_ERR with the verdicts
 * unspecified; the same call made again gives them all. */
int32_t msbb_verify_batch(msbb_system* sys, size_t n_proofs, const uint64_t* n_claims, const uint64_t* const* claim_offsets,
                          const uint32_t* const* claim_data, const uint8_t* const* proofs, const uint64_t* proof_lens,
                          int32_t* verdicts);

/* ---- PCS-level entry points (host buffers in and out, canonical u32) */
/* the permutation used by msbb_poseidon2_permute / msbb_mmcs_commit: 141 canonical round constants */
int32_t msbb_set_poseidon2(ms_ctx* ctx, const uint32_t* constants141);
/* n states of 16 words, permuted in place */
int32_t msbb_poseidon2_permute(ms_ctx* ctx, uint32_t* states, size_t n);
int32_t msbb_dft_batch(ms_ctx* ctx, const uint32_t* in, size_t h, size_t w, int32_t inverse, uint32_t* out);
/* coset_lde_batch(evals, log_blowup, GENERATOR = 31).bit_reverse_rows() */
int32_t msbb_coset_lde_batch(ms_ctx* ctx, const uint32_t* in, size_t h, size_t w, uint32_t log_blowup, uint32_t* out);
/* cap_out: (8 << cap_height) words */
int32_t msbb_mmcs_commit(ms_ctx* ctx, size_t n, const uint32_t* const* mats, const uint64_t* heights, const uint64_t* widths,
                         uint32_t cap_height, uint32_t* cap_out, msbb_mmcs** out);
/* opened rows concatenated in matrix order; siblings bottom-up, 8 words each */
int32_t msbb_mmcs_open(msbb_mmcs* m, size_t index, uint32_t* vals_out, uint32_t* proof_out, size_t* n_siblings);
void msbb_mmcs_destroy(msbb_mmcs* m);
/* MerkleTreeMmcs::verify_batch for many openings of one commitment at once, one device thread per opening, with the
 * permutation of msbb_set_poseidon2. The commitment is described by its cap (8 << cap_height words, cap_height <= log2 of
 * the tallest height) and the matrices' heights and widths. Opening k is indices[k], the opened rows concatenated in matrix
 * order (sum of widths words each) and its siblings bottom-up ((log2 max height - cap_height) * 8 words each): the layout
 * msbb_mmcs_open writes. ok_out[k] = 1 / 0; an index beyond the tallest height, or a value or digest word >= p, is refused
 * (0). n_openings = 0 is MS_OK. */
int32_t msbb_mmcs_verify_batch(ms_ctx* ctx, size_t n_mats, const uint64_t* heights, const uint64_t* widths, const uint32_t* cap,
                               uint32_t cap_height, size_t n_openings, const uint64_t* indices, const uint32_t* vals,
                               const uint32_t* siblings, uint8_t* ok_out);
/* op 0 add, 1 sub, 2 mul, 3 inverse(a), 4 ext4 mul (quads), 5 ext4 inverse (quads) */
int32_t msbb_field_op(ms_ctx* ctx, int32_t op, const uint32_t* a, const uint32_t* b, size_t n, uint32_t* out);

/* ---- Level 2: the prover's steps on DEVICE HANDLES for this configuration, the counterpart of include/mstark.h's Level 2 - a
 * host that keeps the reference's own prover loop (src/prover.rs:290-603) calls the device once per step, and only
 * commitments, accumulators and challenges cross the boundary. Field elements are canonical u32, extension elements four
 * of them, digests eight (as everywhere in this header; the proof bytes hold Montgomery words, src/prover.rs:241-248).
 * tests/test_gpu_bb_level2.py drives the loop from Python and obtains the bytes msbb_prove writes.
 *   msbb_challenger_create          config.initialise_challenger()                       baby_bear_config.rs:108-114
 *   msbb_challenger_observe / _observe_digests / _sample_ext / _sample_bits              DuplexChallenger, baby_bear_config.rs:37
 *   msbb_challenger_observe_claims  the claims absorbed by the transcript                src/prover.rs:369-373
 *   msbb_witness_commit_stage1      pcs.commit(stage-1 traces)                           src/prover.rs:338-350
 *   msbb_witness_claims_accumulator the initial accumulator                              src/prover.rs:382-387
 *   msbb_stage2_build               LookupValues::stage_2_traces -> evaluation handles   src/prover.rs:400, src/lookup.rs:472-555
 *   msbb_pcs_commit_traces          pcs.commit(stage-2 traces) on those handles          src/prover.rs:414-419
 *   msbb_quotient                   quotient_values + slices + LDE -> LDE handle         src/prover.rs:459-468,483,511-517
 *   msbb_pcs_commit_ldes            pcs.commit_ldes                                      src/prover.rs:526
 *   msbb_system_preprocessed_mmcs   the ProverKey's preprocessed prover data (a view)    src/system.rs:190-195
 *   msbb_pcs_open                   pcs.open: opened values + the FriProof bytes         src/prover.rs:580
 * Matrices of a commitment are indexed by ACTIVE position. A handle consumed by a commit call keeps existing but is empty.
 * The commitment parameters (log_blowup, cap_height) and the FRI parameters are the system's. Host-resident witnesses are
 * not accepted. msbb_pcs_open: n_points has one entry per matrix (rounds flattened, at most two points per matrix), points
 * four words per point; opened values come back in round -> matrix -> point -> column order, four words each;
 * MS_ERR_BUFFER with *fri_len = the needed size when a capacity is too small (the challenger has then been advanced). */
typedef struct msbb_challenger msbb_challenger;
typedef struct msbb_trace msbb_trace;
int32_t msbb_challenger_create(msbb_system* sys, msbb_challenger** out);
void msbb_challenger_destroy(msbb_challenger* ch);
int32_t msbb_challenger_observe(msbb_challenger* ch, const uint32_t* elems, size_t n);
int32_t msbb_challenger_observe_digests(msbb_challenger* ch, const uint32_t* digests, size_t n);
int32_t msbb_challenger_sample_ext(msbb_challenger* ch, uint32_t out4[4]);
int32_t msbb_challenger_sample_bits(msbb_challenger* ch, uint32_t bits, uint64_t* out);
int32_t msbb_challenger_observe_claims(msbb_challenger* ch, msbb_witness* w);
void msbb_trace_destroy(msbb_trace* t);
int32_t msbb_trace_info(const msbb_trace* t, uint64_t out3[3]); /* height, width, kind (0 evaluations, 1 LDE) */
int32_t msbb_system_preprocessed_mmcs(msbb_system* sys, msbb_mmcs** out); /* *out = NULL when the system has no preprocessed trace */
int32_t msbb_witness_commit_stage1(msbb_witness* w, uint32_t* cap_out, msbb_mmcs** out);
int32_t msbb_witness_claims_accumulator(msbb_witness* w, const uint32_t beta[4], const uint32_t gamma[4], uint32_t acc_out[4]);
/* accs_out: 4 words per active circuit (the accumulator after each circuit); traces_out: one handle per active circuit */
int32_t msbb_stage2_build(msbb_witness* w, const uint32_t beta[4], const uint32_t gamma[4], const uint32_t acc_in[4], uint32_t* accs_out,
                          msbb_trace** traces_out);
int32_t msbb_pcs_commit_traces(msbb_system* sys, size_t n, msbb_trace* const* evals, uint32_t* cap_out, msbb_mmcs** out);
/* publics16 = [beta, gamma, acc_in, acc_out] (src/lookup.rs:78-84) */
int32_t msbb_quotient(msbb_system* sys, size_t circuit, uint32_t log_n, msbb_mmcs* s1, size_t s1_idx, msbb_mmcs* s2, size_t s2_idx,
                      const uint32_t publics16[16], const uint32_t alpha[4], msbb_trace** q_lde_out);
int32_t msbb_pcs_commit_ldes(msbb_system* sys, size_t n, msbb_trace* const* ldes, uint32_t* cap_out, msbb_mmcs** out);
int32_t msbb_pcs_open(msbb_system* sys, size_t n_rounds, msbb_mmcs* const* rounds, const uint64_t* n_points, const uint32_t* points,
                      msbb_challenger* ch, uint32_t* opened_out, size_t opened_cap_words, uint8_t* fri_out, size_t fri_cap, size_t* fri_len);

#ifdef __cplusplus
}
#endif
#endif /* MSTARK_BB_H */
