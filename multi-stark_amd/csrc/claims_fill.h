// The claims of a witness built on the device from its traces, the part that is the same text in both fields
// (ms_witness_claims_fill in fill.hip, msbb_witness_claims_fill in bb_fill.hip; the definition is in include/mstark.h, "CLAIM
// PROGRAMS", what differs for BabyBear in include/mstark_bb.h): the driver, in the shape of fl_witness_fill. Include it from a
// .hip file only; everything lives in an unnamed namespace.
//
// The program's one pass is fill_k<C::Fill, LDS> as the field's fill launches it, over the first `rows` rows and with
// View::to_tmp as its output, rows x (W + keep) words ROW-MAJOR: without a keep root straight into the new claim data behind the
// claims that stay (the rows ARE the claims), with one into a temporary that claims_dev.h compacts. The new offset and data
// arrays are built beside the witness's and change places with them, host copies included, as the last thing the call does:
// until then it writes nothing the witness owns, so every refusal, an allocation failure at any point and the offender word of
// the inputs leave the witness as it was. Host waits: [the offender word and the kept total, one read-back: when there are
// inputs or a keep root], the host copy of the new claims. The new data starts at Word e_base of its array, whatever e_base is:
// every store of the pass, of the scatter and of the copies is one Word, so nothing asks for more alignment than a Word's.
//
// A field describes itself by a plain traits struct C:
//   Fill                        the traits fill_k is instantiated with (fill_dev.h); Fill::View::to_tmp(p, cols) must redirect
//                               the output to rows x cols row-major at p, and Fill::stored(v) != 0 exactly when v != 0 (the
//                               keep flag is compared as the stored word)
//   call                        the name in front of every text
//   accept(sys, wit)            the field's checks of the witness, in front of the mode
//   trace(sys, wit, ci) -> View the checks of the circuit and its trace; the View of the trace, with d_pre = nullptr when the
//                               circuit has a preprocessed trace that is not on the device at this height
//   n_claims(wit), n_elems(wit), d_offs(wit), d_data(wit)   the claims the witness holds, and their device arrays
//   struct Host                 the host copy of the new claims, built beside the witness's: Host(wit, n_base, e_base, kept, W)
//                               allocates it (and may throw), read(ctx, d_offs, d_data) queues and waits for the read-back of
//                               the NEW offsets and elements (the second host wait), publish(wit, offs, data) exchanges host
//                               and device arrays with the witness's and cannot throw
#pragma once
#include "claims_dev.h"
#include "fill_dev.h"

namespace msamd {
namespace {

template <class C>
void cl_program_info(const uint8_t* program, size_t program_len, const char* call, u64 out4[4]) {
  const ClaimCode cc = claims_compile(program, program_len, call, C::Fill::magic);
  out4[0] = cc.pass.n_instr, out4[1] = cc.pass.n_slots, out4[2] = slot_lds_lanes(cc.pass.n_slots, sizeof(typename C::Fill::Word), 0);
  out4[3] = cc.width | (u64(cc.has_keep) << 32);
}

template <class C, class Sys, class Wit>
void cl_witness_claims_fill(Sys& sys, Wit& wit, size_t ci, const uint8_t* program, size_t program_len, size_t rows, const ms_dev_matrix* inputs,
                            void* producer_stream, uint32_t mode, u64 summary[4]) {
  using F = typename C::Fill;
  using Word = typename F::Word;
  constexpr double S = sizeof(Word);
  Ctx& ctx = *sys.ctx;
  const std::string name(C::call);
  auto fail = [&](const std::string& what) -> void { throw std::runtime_error(name + ": " + what); };
  C::accept(sys, wit);
  if (mode != MS_CLAIMS_REPLACE && mode != MS_CLAIMS_APPEND) fail("mode " + std::to_string(mode) + " (MS_CLAIMS_REPLACE = 0, MS_CLAIMS_APPEND = 1)");
  typename F::View view = C::trace(sys, wit, ci);
  const size_t n = view.n;
  const auto& c = sys.circuits[ci];
  const ClaimCode cc = claims_compile(program, program_len, name, F::magic);
  if (cc.main_w != c.main_width || cc.pre_w != c.pre_width)
    fail("the program is for main_width " + std::to_string(cc.main_w) + " and preprocessed width " + std::to_string(cc.pre_w) + ", circuit " +
         std::to_string(ci) + " has " + std::to_string(c.main_width) + " and " + std::to_string(c.pre_width));
  if (c.pre_width && !view.d_pre) fail("main trace height must equal preprocessed trace height");
  if (rows > n) fail("rows " + std::to_string(rows) + " is above the circuit's height " + std::to_string(n));
  IngestView in;
  size_t h_in = 0;
  if (cc.n_inputs) {
    if (!inputs) fail("the program reads " + std::to_string(cc.n_inputs) + " input columns and no input matrix was given");
    if (inputs->height > n) fail("input height " + std::to_string(inputs->height) + " is above the circuit's height " + std::to_string(n));
    h_in = (size_t)inputs->height;
    if (h_in) {
      try {
        in = ingest_check(ctx, *inputs, ci, cc.n_inputs, sizeof(Word));
      } catch (const std::exception& e) {
        fail(std::string("input matrix: ") + e.what());
      }
    }
  }
  const FillPass& pass = cc.pass;
  const bool keep = cc.has_keep;
  const size_t W = cc.width, cols = W + keep;
  const bool append = mode == MS_CLAIMS_APPEND;
  const size_t n_base = append ? C::n_claims(wit) : 0, e_base = append ? C::n_elems(wit) : 0;  // the claims that stay
  if ((e_base + rows * W) >> 60) fail("the last claim offset would be out of range");         // (rows x W < 2^42)
  const unsigned lanes = slot_lds_lanes(pass.n_slots, sizeof(Word), 0);
  const size_t batch = lanes || !rows ? rows : slot_scratch_rows(pass.n_slots, sizeof(Word), rows);
  const size_t n_tiles = (rows + CL_TILE - 1) / CL_TILE;

  // the buffers whose sizes are known now; with a keep root the new arrays follow the kept total
  DBuf<uint32_t> d_code(ctx, pass.code.size()), d_outs(ctx, pass.outs.size());
  DBuf<Word> d_consts(ctx, std::max<size_t>(pass.consts.size(), 1));
  DBuf<u64> fb(ctx, 2), counts, offsets, new_offs;
  DBuf<Word> scratch, tmp, packed, new_data, inp;
  if (!lanes && rows) scratch = DBuf<Word>(ctx, batch * pass.n_slots);
  if (keep && rows) {
    tmp = DBuf<Word>(ctx, rows * cols);
    if (n_tiles > 1)
      counts = DBuf<u64>(ctx, n_tiles), offsets = DBuf<u64>(ctx, n_tiles);
    else
      packed = DBuf<Word>(ctx, rows * W);  // (one tile: launch (c) alone, into a buffer of the call, since the total is not known yet)
  }
  if (!keep) new_offs = DBuf<u64>(ctx, n_base + rows + 1), new_data = DBuf<Word>(ctx, std::max<size_t>(e_base + rows * W, 1));
  if (h_in) inp = DBuf<Word>(ctx, h_in * cc.n_inputs);
  std::vector<Word> consts(pass.consts.begin(), pass.consts.end());  // (each below p: claims_compile)
  ctx.h2d(d_code.p, pass.code.data(), pass.code.size() * 4);
  ctx.h2d(d_outs.p, pass.outs.data(), pass.outs.size() * 4);
  if (!consts.empty()) ctx.h2d(d_consts.p, consts.data(), consts.size() * sizeof(Word));
  ingest_wait_for_producer(ctx, producer_stream);
  try {
    HIP_CHECK(hipMemsetAsync(fb.p, 0xFF, 16, ctx.stream));  // [the inputs' offender word, the kept total]
    if (h_in) F::ingest(ctx, in, inp.p, fb.p);
    if (rows) {
      FlParams<F> p;
      p.v = view;
      p.v.inputs(inp.p, h_in, cc.n_inputs);
      p.v.to_tmp(keep ? tmp.p : new_data.p + e_base, (uint32_t)cols);
      p.code = d_code.p, p.consts = d_consts.p, p.outs = d_outs.p;
      p.n_instr = (uint32_t)pass.n_instr, p.n_outs = (uint32_t)(pass.outs.size() / 2);
      p.row0 = 0, p.rows = rows, p.scratch = nullptr;
      if (lanes) {
        hipLaunchKernelGGL((fill_k<F, true>), dim3((unsigned)((rows + lanes - 1) / lanes)), dim3(lanes), pass.n_slots * lanes * sizeof(Word), ctx.stream, p);
      } else {
        p.scratch = scratch.p;
        for (size_t r0 = 0; r0 < rows; r0 += batch) {
          p.row0 = r0;
          p.rows = std::min(batch, rows - r0);
          hipLaunchKernelGGL((fill_k<F, false>), dim3((unsigned)((p.rows + 255) / 256)), dim3(256), 0, ctx.stream, p);
        }
      }
      HIP_CHECK(hipGetLastError());
    }
    ClParams<Word> cp{tmp.p, packed.p, counts.p, nullptr, fb.p + 1, rows, (u32)W, (u32)n_tiles};
    if (keep && rows) {  // (profiled as K_WITNESS_CLAIMS with the bytes the layout states: the flags here, the kept rows with the scatter)
      hipEvent_t ev = ctx.prof_begin(K_WITNESS_CLAIMS);
      if (n_tiles > 1) {
        cp.offsets = offsets.p;
        hipLaunchKernelGGL((claims_count_k<Word>), dim3((unsigned)n_tiles), dim3(CL_THREADS), 0, ctx.stream, cp);
        hipLaunchKernelGGL((claims_offsets_k<Word>), dim3(1), dim3(CL_THREADS), 0, ctx.stream, cp);
      } else {
        hipLaunchKernelGGL((claims_scatter_k<Word>), dim3(1), dim3(CL_THREADS), 0, ctx.stream, cp);
      }
      HIP_CHECK(hipGetLastError());
      ctx.prof_end(K_WITNESS_CLAIMS, ev, S * double(rows) + 16.0 * double(n_tiles));
    }
    u64 fb_h[2] = {~u64(0), 0};
    if (h_in || (keep && rows)) ctx.d2h(fb_h, fb.p, 16);  // the first host wait: nothing of the witness has been written, and the caller's matrix has been read
    if (h_in && fb_h[0] != ~u64(0))
      fail("non-canonical input value: row " + std::to_string(fb_h[0] / cc.n_inputs) + ", column " + std::to_string(fb_h[0] % cc.n_inputs));
    const size_t kept = !keep ? rows : rows ? (size_t)fb_h[1] : 0;
    if (kept > rows) fail("internal error (more kept rows than rows)");
    if (keep) new_offs = DBuf<u64>(ctx, n_base + kept + 1), new_data = DBuf<Word>(ctx, std::max<size_t>(e_base + kept * W, 1));
    typename C::Host host(wit, n_base, e_base, kept, W);
    if (n_base) HIP_CHECK(hipMemcpyAsync(new_offs.p, C::d_offs(wit), n_base * 8, hipMemcpyDeviceToDevice, ctx.stream));
    if (e_base) HIP_CHECK(hipMemcpyAsync(new_data.p, C::d_data(wit), e_base * sizeof(Word), hipMemcpyDeviceToDevice, ctx.stream));
    if (keep && kept) {
      hipEvent_t ev = ctx.prof_begin(K_WITNESS_CLAIMS);
      if (n_tiles > 1) {
        cp.dst = new_data.p + e_base, cp.total = nullptr;
        hipLaunchKernelGGL((claims_scatter_k<Word>), dim3((unsigned)n_tiles), dim3(CL_THREADS), 0, ctx.stream, cp);
      } else {
        HIP_CHECK(hipMemcpyAsync(new_data.p + e_base, packed.p, kept * W * sizeof(Word), hipMemcpyDeviceToDevice, ctx.stream));
      }
      ctx.prof_end(K_WITNESS_CLAIMS, ev, S * double(rows) + 2.0 * S * double(kept) * double(W));
    }
    hipLaunchKernelGGL(claims_arith_offsets_k, dim3((unsigned)((kept + 1 + 255) / 256)), dim3(256), 0, ctx.stream, new_offs.p + n_base, (u64)e_base, (u64)W,
                       kept + 1);
    HIP_CHECK(hipGetLastError());
    host.read(ctx, new_offs.p + n_base, new_data.p + e_base);  // the second host wait: the host copy (the transcript absorbs it)
    host.publish(wit, std::move(new_offs), std::move(new_data));  // the exchange: cannot throw
    summary[0] = rows, summary[1] = kept, summary[2] = pass.n_instr, summary[3] = lanes;
  } catch (...) {
    (void)hipStreamSynchronize(ctx.stream);  // what has been queued may still be reading the caller's matrix
    abandon_pending();
    throw;
  }
}

}  // namespace
}  // namespace msamd
