// Host check of the batched BabyBear verifier: the collection (verify_batch.h's pcs_collect) and both kernel bodies
// (bb_verify_dev.h) run as host code, one "thread" per call, against verify() on oracle-made proofs and their mutations. CPU
// only: it is built and run by tools/bb_verify_host_check.py (address and undefined-behaviour sanitizers on), never loaded
// into Python.
#include "../multi-stark_amd/csrc/bb_verifier.hip"

#include <cstdio>
#include <fstream>
#include <random>

namespace msbb {
namespace {

std::vector<uint8_t> slurp(const std::string& p) {
  std::ifstream f(p, std::ios::binary);
  if (!f) throw std::runtime_error("cannot open " + p);
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

// the host half of system_from_blob; the commitment to the preprocessed traces, which the library computes on the device, is
// the oracle's (canonical words)
std::unique_ptr<BSystem> host_system(const std::vector<uint8_t>& blob, const std::vector<uint8_t>& pre_commit) {
  Reader rd{blob.data(), blob.size()};
  if (rd.word() != BLOB_MAGIC) throw std::runtime_error("magic");
  std::unique_ptr<BSystem> sys(new BSystem());
  Params& p = sys->params;
  p.log_blowup = rd.word(), p.cap_height = rd.word(), p.log_final_poly_len = rd.word(), p.max_log_arity = rd.word();
  p.num_queries = rd.word(), p.commit_pow_bits = rd.word(), p.query_pow_bits = rd.word();
  for (int r = 0; r < 8; r++)
    for (int i = 0; i < 16; i++) sys->perm.external[r][i] = bb_to_monty((u32)rd.word());
  for (int r = 0; r < 13; r++) sys->perm.internal[r] = bb_to_monty((u32)rd.word());
  set_internal_diag(sys->perm);
  const char* tag = "multi-stark/v0";
  for (int i = 0; i < 14; i++) sys->seed.push_back(bb_to_monty((u32)(uint8_t)tag[i]));
  const u64 ps[7] = {p.log_blowup, p.cap_height, p.log_final_poly_len, p.max_log_arity, p.num_queries, p.commit_pow_bits, p.query_pow_bits};
  for (u64 x : ps) sys->seed.push_back(bb_to_monty((u32)(x % BB_P)));
  const size_t D = 4;
  size_t nc = rd.word(), n_pre = 0;
  for (size_t ci = 0; ci < nc; ci++) {
    sys->circuits.emplace_back();
    BCircuit& c = sys->circuits.back();
    c.main_width = rd.word(), c.pre_width = rd.word(), c.pre_height = rd.word();
    size_t nn = rd.word(), nz = rd.word(), nl = rd.word();
    c.num_lookups = nl;
    c.stage2_width = std::max<size_t>(nl, 1) * D;
    c.nodes.resize(nn);
    c.degrees.resize(nn);
    for (size_t i = 0; i < nn; i++) {
      u64 w0 = rd.word();
      PNode& nd = c.nodes[i];
      nd.kind = (uint32_t)(w0 & 0xff), nd.source = (uint32_t)((w0 >> 8) & 0xff), nd.offset = (uint32_t)((w0 >> 16) & 0xff);
      nd.a = rd.word(), nd.b = rd.word();
      uint32_t deg = 0;
      switch (nd.kind) {
        case msamd::OP_VAR:
        case msamd::OP_IS_FIRST:
        case msamd::OP_IS_LAST: deg = 1; break;
        case msamd::OP_ADD:
        case msamd::OP_SUB: deg = std::max(c.degrees[nd.a], c.degrees[nd.b]); break;
        case msamd::OP_MUL: deg = c.degrees[nd.a] + c.degrees[nd.b]; break;
        case msamd::OP_NEG: deg = c.degrees[nd.a]; break;
        default: break;
      }
      c.degrees[i] = deg;
    }
    uint32_t graph_deg = 0;
    for (size_t i = 0; i < nz; i++) {
      u64 z = rd.word();
      c.zeros.push_back((uint32_t)z);
      graph_deg = std::max(graph_deg, c.degrees[z]);
    }
    uint32_t logup_deg = nl ? 0 : 1;
    for (size_t j = 0; j < nl; j++) {
      u64 m = rd.word();
      size_t na = rd.word();
      std::vector<uint32_t> args;
      uint32_t msg = 0;
      for (size_t k = 0; k < na; k++) {
        u64 a = rd.word();
        args.push_back((uint32_t)a);
        msg = std::max(msg, c.degrees[a]);
      }
      logup_deg = std::max(logup_deg, std::max(msg + 1, c.degrees[m]));
      c.lookups.emplace_back((uint32_t)m, std::move(args));
    }
    c.constraint_count = nz + std::max<size_t>(nl, 1) * D;
    c.max_constraint_degree = std::max(graph_deg, logup_deg);
    if (c.pre_width) {
      for (size_t i = 0; i < c.pre_height * c.pre_width; i++) rd.word();  // the table itself: only the prover reads it
      sys->pre_indices.push_back((int)n_pre++);
    } else {
      c.pre_height = 0;
      sys->pre_indices.push_back(-1);
    }
  }
  if (rd.off != blob.size()) throw std::runtime_error("trailing");
  if (n_pre) {
    if (pre_commit.empty() || pre_commit.size() % sizeof(Digest8)) throw std::runtime_error("host check: no preprocessed commitment");
    sys->has_pre = true;
    sys->pre_commit.resize(pre_commit.size() / sizeof(Digest8));
    memcpy(sys->pre_commit.data(), pre_commit.data(), pre_commit.size());
    for (auto& d : sys->pre_commit)
      for (u32& w : d.w) w = bb_to_monty(w);
  }
  return sys;
}

size_t g_queued = 0, g_dev_fail = 0, g_refused = 0, g_host = 0;

typedef msamd::VBatch<BbVerify> BVBatch;

// vbatch_run with the two kernels as host loops over exactly-sized arrays (an out-of-bounds index is an ASan report)
void run_host(const BSystem& sys, BVBatch& B, std::vector<u32>& fail) {
  fail.assign(B.n_flags, 0);
  if (B.items.empty() && B.qmap.empty()) return;
  msamd::vbatch_seal(B);
  std::vector<u32> words(B.words);
  words.resize(B.words.size() + B.fri_words, 0xdeadbeefu);
  std::vector<E4> ro(B.ro_count);
  BVDev d;
  d.items = B.items.data(), d.proofs = B.proofs.data(), d.mats = B.mats.data(), d.heights = B.heights.data();
  d.u32s = B.u32s.data(), d.qmap = B.qmap.data(), d.ext = B.ext.data(), d.digs = B.digs.data();
  d.fail = fail.data(), d.words = words.data(), d.ro = ro.data(), d.perm = &sys.perm;
  for (size_t t = 0; t < B.qmap.size(); t++) bbv_query_body(d, (u32)t);
  for (size_t t = 0; t < B.items.size(); t++) bbv_path_body(d, (u32)t);
}

// verify_batch_run for a batch of `copies` of one proof, with run_host in the place of vbatch_run
int batch_verdict(const BSystem& sys, size_t n_claims, const u64* offs, const u32* data, const std::vector<uint8_t>& proof, int copies) {
  BVBatch B;
  std::vector<std::pair<size_t, int>> waiting;
  std::vector<int> verdicts(copies, -1);
  for (int i = 0; i < copies; i++) {
    Prepared P(sys);
    const int v = verify_prepare(sys, n_claims, offs, data, proof.data(), proof.size(), P);
    if (v != V_OK) {
      verdicts[i] = v;
      continue;
    }
    const Challenger at_pcs = P.ch;
    const int c = msamd::pcs_collect<BbVerify>(sys.params, P.rounds, P.proof, P.ch, B, (u32)waiting.size());
    if (c == msamd::COLLECT_HOST) {
      g_host++;
      Challenger ch = at_pcs;
      verdicts[i] = pcs_verify(sys, P.rounds, P.proof, ch) ? verify_ood(sys, P) : V_INVALID_OPENING;
      continue;
    }
    if (c == msamd::COLLECT_REFUSED) {
      g_refused++;
      verdicts[i] = V_INVALID_OPENING;
      continue;
    }
    g_queued++;
    waiting.push_back({(size_t)i, verify_ood(sys, P)});
  }
  std::vector<u32> fail;
  B.n_flags = waiting.size();
  run_host(sys, B, fail);
  for (size_t k = 0; k < waiting.size(); k++) {
    if (fail[k]) g_dev_fail++;
    verdicts[waiting[k].first] = fail[k] ? V_INVALID_OPENING : waiting[k].second;
  }
  for (int i = 1; i < copies; i++)
    if (verdicts[i] != verdicts[0]) throw std::runtime_error("copies of one proof disagree");
  return verdicts[0];
}

}  // namespace
}  // namespace msbb

int main(int argc, char** argv) {
  using namespace msbb;
  const std::string dir = argc > 1 ? argv[1] : ".";
  const int muts = argc > 2 ? atoi(argv[2]) : 200;
  const char* names[] = {"arity1", "arity2",  "arity3",       "arity6", "caps_final", "evenodd", "evenodd_dead", "evenodd_dead_table",
                         "height1", "squares_mixed"};
  std::mt19937_64 rng(12345);
  size_t total = 0, disagree = 0, rejected = 0;
  {  // the sponge in a thread against hash_words, every length 0 .. 40, under three permutations
    auto sys = host_system(slurp(dir + "/arity1.blob"), {});
    for (u32 n = 0; n <= 40; n++) {
      std::vector<u32> v(n);
      for (auto& x : v) x = (u32)(rng() % BB_P);
      u32 st[16];
      bbv_hash_words(sys->perm, v.data(), n, st);
      const Digest8 want = hash_words(sys->perm, v);
      if (memcmp(st, want.w, 32)) {
        printf("SPONGE MISMATCH at %u words\n", n);
        return 1;
      }
    }
    printf("sponge: 0..40 words agree with hash_words\n");
  }
  for (const char* nm : names) {
    auto sys = host_system(slurp(dir + "/" + nm + ".blob"), slurp(dir + "/" + nm + ".precommit"));
    const auto cl = slurp(dir + "/" + std::string(nm) + ".claims");
    const auto proof = slurp(dir + "/" + std::string(nm) + ".proof");
    u64 n_claims;
    memcpy(&n_claims, cl.data(), 8);
    std::vector<u64> offs(n_claims + 1);
    memcpy(offs.data(), cl.data() + 8, 8 * (n_claims + 1));
    std::vector<u32> data((cl.size() - 8 - 8 * (n_claims + 1)) / 4 + 1);
    memcpy(data.data(), cl.data() + 8 + 8 * (n_claims + 1), cl.size() - 8 - 8 * (n_claims + 1));
    const int a = verify(*sys, n_claims, offs.data(), data.data(), proof.data(), proof.size());
    const int b = batch_verdict(*sys, n_claims, offs.data(), data.data(), proof, 3);
    printf("%-14s valid: verify %d, batch %d\n", nm, a, b);
    if (a != 0 || b != 0) return 1;
    if (std::ifstream(dir + "/" + nm + ".width.proof").good()) {
      // the directed mutation: a matrix opened at no point shows a longer row in the second query only. The collector cannot
      // lay that out (COLLECT_HOST) and the batch must say what verify() says, between untouched copies or alone
      const auto wide = slurp(dir + "/" + std::string(nm) + ".width.proof");
      const size_t host_before = g_host;
      const int wa = verify(*sys, n_claims, offs.data(), data.data(), wide.data(), wide.size());
      const int wb = batch_verdict(*sys, n_claims, offs.data(), data.data(), wide, 3);
      printf("%-14s row width differs between queries: verify %d, batch %d, host path taken %zu times\n", nm, wa, wb, g_host - host_before);
      if (wa != wb || g_host - host_before != 3) return 1;
    }
    size_t rej = 0, dis = 0;
    for (int k = 0; k < muts; k++) {
      std::vector<uint8_t> bad = proof;
      const int kind = k % 8;
      if (kind <= 3) {  // one bit
        bad[rng() % bad.size()] ^= (uint8_t)(1u << (rng() % 8));
      } else if (kind == 4) {  // a field word replaced by a small / large canonical value
        const size_t pos = (rng() % (bad.size() / 4)) * 4 + (proof.size() % 4);
        const u32 vals[4] = {0, 1, BB_P - 1, (u32)(rng() % BB_P)};
        if (pos + 4 <= bad.size()) memcpy(bad.data() + pos, &vals[rng() % 4], 4);
      } else if (kind == 5) {  // a length word
        const size_t pos = rng() % (bad.size() - 8);
        const u64 vals[4] = {0, 1, 0xFFFFFFFFull, 1ull << 40};
        memcpy(bad.data() + pos, &vals[rng() % 4], 8);
      } else if (kind == 6) {
        bad.resize(rng() % bad.size());
      } else {
        for (int j = 0; j < 5; j++) bad.push_back((uint8_t)rng());
      }
      const int va = verify(*sys, n_claims, offs.data(), data.data(), bad.data(), bad.size());
      const int vb = batch_verdict(*sys, n_claims, offs.data(), data.data(), bad, 1);
      total++;
      rej += va != 0;
      if (va != vb) {
        dis++;
        printf("  DISAGREE %s mutation %d kind %d: verify %d batch %d\n", nm, k, kind, va, vb);
      }
    }
    rejected += rej;
    disagree += dis;
    printf("%-14s %d mutations, %zu rejected, %zu disagreements\n", nm, muts, rej, dis);
  }
  printf("total %zu mutations, %zu rejected, %zu disagreements; queued %zu (device flag set %zu), refused on host %zu, host path %zu\n", total,
         rejected, disagree, g_queued, g_dev_fail, g_refused, g_host);
  return disagree ? 1 : 0;
}
