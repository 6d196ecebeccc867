// Host-side bookkeeping of the opening that the one-GPU prover (prover.hip: prove, pcs_open) and the joint prover
// (prover_sharded.inc: prove_sharded) share: the outer transcript's steps, the placeholder opening points of the device
// transcript, the unique opening points, the opened values from the raw barycentric sums and the reduced-opening plan per
// LDE height. The proof bytes depend on every order kept here. Each prover keeps its own loops over its own containers
// and its own launches, and hands one matrix at a time to this code.
#pragma once
#include <cstring>
#include <stdexcept>
#include <vector>

#include "host.h"
#include "quotient_params.h"

namespace msamd {

inline bool e2_same(E2 a, E2 b) { return a.c0 == b.c0 && a.c1 == b.c1; }

// ---- the outer transcript's steps on the host challenger (src/prover.rs:382-433, 538)
inline void tx_beta_gamma(Challenger& ch, E2& beta, E2& gamma) {
  beta = ch.sample_ext();
  ch.observe_ext(beta);
  gamma = ch.sample_ext();
  ch.observe_ext(gamma);
}
inline E2 tx_alpha(Challenger& ch, const std::vector<Digest>& s2_cap, const std::vector<E2>& accs) {
  ch.observe_cap(s2_cap);
  for (auto& a : accs) ch.observe_ext(a);
  return ch.sample_ext();
}
inline E2 tx_zeta(Challenger& ch, const std::vector<Digest>& q_cap) {
  ch.observe_cap(q_cap);
  return ch.sample_ext();
}

// ---- the outer transcript on the device (outer.hip): what it leaves in device memory and the queued host copies
struct OuterDev {
  DBuf<Digest> digest;
  DBuf<u32> state;  // 12 words behind gamma, 8 behind alpha (the one-GPU prover: 8 more behind zeta)
  DBuf<E2> accs, alpha, points;
  DBuf<E2> tot;     // joint prover only: the totals summed over ranks
  DBuf<u32> lds;
  DBuf<uint8_t> circuits;
  std::vector<DBuf<uint8_t>> qdyn;  // per active circuit: QDyn, then the reversed alpha powers
  Digest h_digest;
  E2 h_bg[2], h_alpha;
  std::vector<E2> h_points;
  std::vector<unsigned> uniq_ld;  // the distinct trace heights: points[1 + k] = zeta * g(2^uniq_ld[k])
};

// An opening point that only the DEVICE knows while the opening's first kernels are queued is named by a placeholder: c1 is
// not a canonical field element, so it never equals a real point; its value lies at od.points[id].
inline E2 sym_point(size_t id) { return e2((u64)id, ~u64(0)); }
inline bool is_sym_point(E2 z) { return z.c1 == ~u64(0); }
inline void swap_in(std::vector<E2>& pts, const std::vector<E2>& values) {
  for (auto& z : pts)
    if (is_sym_point(z)) z = values[z.c0];
}

// zeta (id 0) and zeta * g per distinct trace height (id 1 + k) sampled on the device behind the quotient commitment d_cap;
// returns their placeholders. d_state_out: see outer_zeta.
inline void zeta_placeholders(Ctx& ctx, OuterDev& od, const std::vector<unsigned>& log_degrees, const Digest* d_cap, size_t ncap, u32* d_state_out,
                              E2& pt_zeta, std::vector<E2>& pt_next) {
  pt_zeta = sym_point(0);
  for (size_t pos = 0; pos < log_degrees.size(); pos++) {
    size_t k = 0;
    while (k < od.uniq_ld.size() && od.uniq_ld[k] != log_degrees[pos]) k++;
    if (k == od.uniq_ld.size()) od.uniq_ld.push_back(log_degrees[pos]);
    pt_next[pos] = sym_point(1 + k);
  }
  const size_t n_ld = od.uniq_ld.size();
  od.lds = DBuf<u32>(ctx, n_ld);
  ctx.h2d(od.lds.p, od.uniq_ld.data(), n_ld * sizeof(u32));
  od.points = DBuf<E2>(ctx, 1 + n_ld);
  od.h_points.assign(1 + n_ld, e2(0));
  outer_zeta(ctx, od.state.p + 12, d_cap, ncap, od.lds.p, n_ld, od.points.p, d_state_out);
  ctx.d2h_queue(od.h_points.data(), od.points.p, (1 + n_ld) * sizeof(E2));
}
// The host has replayed the transcript: its challenges against the device's (arrived by now); returns the placeholders' values.
inline std::vector<E2> replayed_points(const OuterDev& od, E2 beta, E2 gamma, E2 alpha, E2 zeta) {
  bool same = e2_same(beta, od.h_bg[0]) && e2_same(gamma, od.h_bg[1]) && e2_same(alpha, od.h_alpha) && e2_same(zeta, od.h_points[0]);
  std::vector<E2> values(1 + od.uniq_ld.size());
  values[0] = zeta;
  for (size_t k = 0; k < od.uniq_ld.size(); k++) {
    values[1 + k] = e2_mul_base(zeta, gl_two_adic_generator(od.uniq_ld[k]));
    same = same && e2_same(values[1 + k], od.h_points[1 + k]);
  }
  if (!same) throw std::runtime_error("the device transcript's challenges differ from the host challenger's");
  return values;
}

// One circuit's quotient inputs: the LDEs it reads and, under the device transcript, its challenge block qdyn (else null:
// quotient_publics follows)
inline QuotientArgs fill_quotient_args(const HSystem& sys, size_t ci, const DMat& s1, const DMat& s2, unsigned log_n, unsigned log_q, const uint8_t* qdyn) {
  QuotientArgs qa;
  if (sys.has_pre && sys.pre_indices[ci] >= 0) {
    const DMat& pm = sys.pre_data.ldes[sys.pre_indices[ci]];
    qa.pre = pm.d();
    qa.pre_h = pm.h;
  }
  qa.s1 = s1.d();
  qa.s1_h = s1.h;
  qa.s2 = s2.d();
  qa.s2_h = s2.h;
  qa.log_n = log_n;
  qa.log_q = log_q;
  if (qdyn) {
    qa.dyn = reinterpret_cast<const QDyn*>(qdyn);
    qa.alpha_rev = reinterpret_cast<const E2*>(qdyn + sizeof(QDyn));
  }
  return qa;
}
inline void quotient_publics(QuotientArgs& qa, E2 beta, E2 gamma, E2 acc_in, E2 acc_out, E2 alpha) {
  const E2 four[4] = {beta, gamma, acc_in, acc_out};
  for (int k = 0; k < 4; k++) {
    qa.publics[2 * k] = four[k].c0;
    qa.publics[2 * k + 1] = four[k].c1;
  }
  qa.alpha = alpha;
}

// ---- unique opening points and the tallest matrix opened at each. The order of first notes is the launch order of the
// inverse denominators; only note() grows the set - a point looked up later must have been noted, its arrays exist by then.
struct OpenPoints {
  std::vector<E2> upts;
  std::vector<size_t> uh;
  void note(E2 z, size_t height) {
    size_t k = 0;
    while (k < upts.size() && !e2_same(upts[k], z)) k++;
    if (k == upts.size()) {
      upts.push_back(z);
      uh.push_back(0);
    }
    uh[k] = std::max(uh[k], height);
  }
  size_t index(E2 z) const {
    for (size_t i = 0; i < upts.size(); i++)
      if (e2_same(upts[i], z)) return i;
    throw std::runtime_error("pcs_open: an opening point that was not noted before the inverse denominators were allocated");
  }
  void resolve(const std::vector<E2>& values) { swap_in(upts, values); }
};

// the opened values of one matrix from its raw barycentric sums (index c * np + p): one vector per point
inline std::vector<std::vector<E2>> finish_opened(const E2* sums, size_t w, unsigned log_n, const std::vector<E2>& pts) {
  const int np = (int)pts.size();
  std::vector<std::vector<E2>> per_point;
  if (!np) return per_point;
  std::vector<E2> ys(np * w);
  bary_finish(sums, w, log_n, pts.data(), np, ys.data());
  for (int p = 0; p < np; p++) per_point.emplace_back(ys.begin() + p * w, ys.begin() + (p + 1) * w);
  return per_point;
}

inline std::vector<E2> alpha_powers(E2 alpha, size_t gw) {  // alpha^0 .. alpha^gw
  std::vector<E2> apow(gw + 1);
  apow[0] = e2(1);
  for (size_t i = 1; i <= gw; i++) apow[i] = e2_mul(apow[i - 1], alpha);
  return apow;
}

// ---- reduced openings per LDE height: every height's matrix list, its (at most two, locally numbered) opening points and
// the running column count that fixes each coefficient. Matrices are added in the prover's own visit order - that order is
// part of the proof. hpts[lh].den point into `dens`: the plan goes before those buffers are released.
struct DeepPlan {
  static constexpr size_t NEXT_MARK = size_t(1) << 62;
  std::vector<size_t> num_reduced = std::vector<size_t>(33, 0);
  std::vector<std::vector<DeepMat>> lists = std::vector<std::vector<DeepMat>>(33);
  std::vector<DeepPoints> hpts = std::vector<DeepPoints>(33);
  std::vector<std::vector<size_t>> hpt_global = std::vector<std::vector<size_t>>(33);
  std::vector<char> present = std::vector<char>(33, 0);
  const OpenPoints& points;
  const std::vector<DBuf<E2>>& dens;  // per unique point: 1 / (z - x_i), indexed by the full domain's row
  const E2 alpha;
  const std::vector<E2>& apow;
  const unsigned lb;
  DeepPlan(const OpenPoints& op, const std::vector<DBuf<E2>>& d, E2 a, const std::vector<E2>& ap, unsigned log_blowup)
      : points(op), dens(d), alpha(a), apow(ap), lb(log_blowup) {
    for (auto& hp : hpts) memset(&hp, 0, sizeof(hp));
  }
  // One matrix of LDE height 2^lh: d column-major with column stride `stride` (0 = the launch's height), opened at pts with
  // the values ys (per point). next: pts[1] = pts[0] * g, g the generator of the trace domain, and is read through the first
  // point's arrays - 1 / (z g - x_j) = g^-1 / (z - x_sigma(j)) - so it is named by those arrays plus a mark (all matrices of
  // one height share g, so the pair identifies the point at this height).
  void add(unsigned lh, const u64* d, size_t stride, size_t w, const std::vector<E2>& pts, bool next, const std::vector<std::vector<E2>>& ys) {
    present[lh] = 1;
    if (pts.empty()) return;
    DeepMat dm;
    memset(&dm, 0, sizeof(dm));  // the struct crosses to the device as bytes
    dm.d = d;
    dm.stride = stride;
    dm.w = (uint32_t)w;
    dm.npoints = (uint32_t)pts.size();
    for (size_t pi = 0; pi < pts.size(); pi++) {
      const bool nx = pi == 1 && next;
      const size_t gk = points.index(pts[nx ? 0 : pi]) | (nx ? NEXT_MARK : size_t(0));
      size_t local = 0;
      while (local < hpt_global[lh].size() && hpt_global[lh][local] != gk) local++;
      if (local == hpt_global[lh].size()) {
        if (local == 2) throw std::runtime_error("pcs_open: more than two opening points at one LDE height");
        hpt_global[lh].push_back(gk);
        hpts[lh].den[local] = dens[gk & ~NEXT_MARK].p;
        hpts[lh].shift[local] = nx ? (uint32_t(1) << lb) : 0u;  // g = w_H^blowup
        hpts[lh].K[local] = e2(0);
        hpts[lh].n = (uint32_t)(local + 1);
      }
      E2 coeff = e2_pow(alpha, num_reduced[lh]);
      E2 rz = e2(0);
      for (size_t c = 0; c < w; c++) rz = e2_add(rz, e2_mul(apow[c], ys[pi][c]));
      if (nx) coeff = e2_mul_base(coeff, gl_inv(gl_two_adic_generator(lh - lb)));
      dm.pt[pi] = (uint32_t)local;
      dm.coeff[pi] = coeff;
      dm.coeff7[pi] = gl_mul(coeff.c1, GL_EXT_W);
      hpts[lh].K[local] = e2_add(hpts[lh].K[local], e2_mul(coeff, rz));
      num_reduced[lh] += w;
    }
    lists[lh].push_back(dm);
  }
};

}  // namespace msamd
