// One proof over several GPUs (SURVEY §8e; BASELINE config 3): included at the end of prover.hip, inside namespace
// msamd, so it shares the single-GPU prover's helpers; the opening's host bookkeeping and the outer transcript's steps
// are the ones prove() and pcs_open use (open_plan.h). Every circuit is either "sharded" - owned by ONE rank, which
// computes its columns: LDE, stage-2 trace, quotient, opened values; a rank may own any number of circuits, of any
// shapes - or "replicated": every rank computes it (small tables). Every commitment is ONE Merkle tree whose leaf i hashes row i of
// ALL matrices (src/types.rs:82-83), so before hashing the ranks exchange row ranges: rank k receives rows
// [k H/N, (k+1) H/N) of every sharded matrix (all-to-all), builds the sub-tree over them (replicated matrices
// inject their own row slice), the N sub-tree roots are all-gathered and every rank hashes the top log2 N levels.
// The reduced openings are computed on the same row ranges and all-gathered; FRI then runs replicated (it is
// latency-bound and a 16th of the data), the transcript is replicated on every host, and the query openings of
// the input commitments are served by the rank that owns the queried row. Field sums are never reduced by a
// collective (there is no mod-p all-reduce): every exchange moves values, the arithmetic stays local and exact.
// The proof bytes equal those of the single-GPU prover on the same system and witness.

namespace {

struct Comm {
  Ctx& ctx;
  const ms_comm_t* c;
  bool ordered = false;  // the transport orders itself with ctx.stream by events (ms_comm.set_stream_ordered): no host waits
  const char* phase = "start";  // the prover's phase, for the progress record
  Comm(Ctx& x, const ms_comm_t* t) : ctx(x), c(t) {
    if (c->set_stream_ordered && !getenv("MSAMD_SHARDED_HOST_SYNC")) {
      if (c->set_stream_ordered(c->user, ctx.main_stream) != 0) throw std::runtime_error("ms_comm.set_stream_ordered failed");
      ordered = true;
    }
  }
  ~Comm() {
    if (ordered) (void)c->set_stream_ordered(c->user, nullptr);
  }
  Comm(const Comm&) = delete;
  Comm& operator=(const Comm&) = delete;
  // every call into the transport is recorded in the context (ms_ctx_comm_progress): a collective that a peer never joins
  // blocks inside the transport, and the record names it
  struct Call {
    Ctx& ctx;
    Call(Comm& cm, const char* what, size_t bytes, size_t detail = 0) : ctx(cm.ctx) {
      char buf[200];
      snprintf(buf, sizeof(buf), "%s: %s (%zu bytes%s%s) on rank %d of %d", cm.phase, what, bytes, detail ? ", part " : "",
               detail ? std::to_string(detail).c_str() : "", cm.rank(), cm.world());
      std::lock_guard<std::mutex> lk(ctx.comm_mu);
      ctx.comm_what = buf;
      ctx.comm_seq++;
      ctx.comm_in_flight = true;
    }
    ~Call() {
      std::lock_guard<std::mutex> lk(ctx.comm_mu);
      ctx.comm_in_flight = false;
    }
  };
  // what went wrong in a callback: the transport's own message (the library's transports leave it in ms_last_error)
  [[noreturn]] void fail(const char* what) {
    std::string why = last_error_text();
    throw std::runtime_error(std::string("ms_comm.") + what + " failed in phase '" + phase + "'" + (why.empty() ? "" : ": " + why));
  }
  // the callbacks' contract: the context's stream is idle when they are called - unless the transport waits for it itself
  void idle() {
    if (!ordered) ctx.sync();
  }
  int rank() const { return c->rank; }
  int world() const { return c->world; }
  void all_to_all(const void* send, void* recv, size_t bytes_per_peer) {
    idle();
    Call rec(*this, "all_to_all", bytes_per_peer);
    if (c->all_to_all(c->user, send, recv, bytes_per_peer) != 0) fail("all_to_all");
  }
  void all_gather(const void* send, void* recv, size_t bytes, const char* what = "all_gather") {
    if (world() == 1 && !getenv("MSAMD_SHARDED_WORLD1_TRANSPORT")) {
      // a single rank gathers from itself: a copy on the prover's own stream, no hop through the transport's stream
      if (bytes) HIP_CHECK(hipMemcpyAsync(recv, send, bytes, hipMemcpyDeviceToDevice, ctx.stream));
      return;
    }
    idle();
    Call rec(*this, what, bytes);
    if (c->all_gather(c->user, send, recv, bytes) != 0) fail("all_gather");
  }
  bool can_overlap() const { return c->all_to_all_start && c->all_to_all_wait && !getenv("MSAMD_SHARDED_NO_OVERLAP"); }
  void all_to_all_start(const void* send, size_t send_stride, void* recv, size_t recv_stride, size_t bytes_per_peer, size_t group = 0) {
    idle();
    Call rec(*this, "all_to_all_start", bytes_per_peer, group + 1);
    if (c->all_to_all_start(c->user, send, send_stride, recv, recv_stride, bytes_per_peer) != 0) fail("all_to_all_start");
  }
  void all_to_all_wait() {
    if (world() == 1 && c->all_to_all_cols_start2 && can_cols() && !getenv("MSAMD_SHARDED_WORLD1_TRANSPORT")) return;
    Call rec(*this, "all_to_all_wait", 0);
    if (c->all_to_all_wait(c->user) != 0) fail("all_to_all_wait");
  }
  // the exchange straight out of the column-major LDE (no packed send buffer)
  bool can_cols() const { return c->all_to_all_cols_start && c->all_to_all_wait && !getenv("MSAMD_SHARDED_PACK"); }
  void all_to_all_cols_start(const void* send, size_t sps, size_t scs, void* recv, size_t rps, size_t rcs, size_t ncols, size_t seg,
                             size_t group = 0) {
    if (world() == 1 && c->all_to_all_cols_start2 && !getenv("MSAMD_SHARDED_WORLD1_TRANSPORT")) return;  // nobody to exchange with; own rows stay in place
    idle();
    Call rec(*this, "all_to_all_cols_start", ncols * seg, group + 1);
    // this rank's own rows are read where they are (ShardMat::slice points into the LDE): a transport that can, skips them
    const int rc = c->all_to_all_cols_start2 ? c->all_to_all_cols_start2(c->user, send, sps, scs, recv, rps, rcs, ncols, seg, MS_COMM_SKIP_SELF)
                                             : c->all_to_all_cols_start(c->user, send, sps, scs, recv, rps, rcs, ncols, seg);
    if (rc != 0) fail("all_to_all_cols_start");
  }
  // one rank's matrix handed out by row ranges (the general ownership pattern)
  bool can_scatter() const { return c->scatter_cols_start && c->all_to_all_wait; }
  void scatter_cols_start(int root, const void* send, size_t sps, size_t scs, void* recv, size_t rcs, size_t ncols, size_t seg, size_t part = 0) {
    idle();
    Call rec(*this, "scatter_cols_start", ncols * seg, part + 1);
    if (c->scatter_cols_start(c->user, root, send, sps, scs, recv, rcs, ncols, seg) != 0) fail("scatter_cols_start");
  }
  // For the duration of the scope the stream-ordered transport is ordered with `s` - another stream of this context (the side
  // stream) - instead of the main stream: an exchange issued from work that runs BESIDE the main stream's (the claims
  // transcript's chaining values beside the stage-1 hashing) then neither waits for the main stream nor holds it up. The
  // transport's own stream is in order, so the exchanges still complete in the order every rank issued them. A transport
  // that is not stream-ordered needs nothing: its calls wait for the context on the host (idle()).
  struct OnStream {
    Comm& cm;
    bool on;
    OnStream(Comm& c, hipStream_t s) : cm(c), on(c.ordered && s != c.ctx.main_stream) {
      if (on && cm.c->set_stream_ordered(cm.c->user, s) != 0) throw std::runtime_error("ms_comm.set_stream_ordered failed");
    }
    ~OnStream() {
      if (on) (void)cm.c->set_stream_ordered(cm.c->user, cm.ctx.main_stream);
    }
  };
  // host convenience: every rank contributes `bytes` host bytes; returns world * bytes ordered by rank
  std::vector<uint8_t> all_gather_host(const void* mine, size_t bytes, const char* what = "all_gather (host values)") {
    DBuf<uint8_t> s(ctx, std::max<size_t>(bytes, 1)), r(ctx, std::max<size_t>(bytes, 1) * world());
    std::vector<uint8_t> out(bytes * world());
    if (bytes == 0) return out;
    ctx.h2d(s.p, mine, bytes);
    all_gather(s.p, r.p, bytes, what);
    ctx.d2h(out.data(), r.p, out.size());
    return out;
  }
};

struct ShardMat {
  size_t h = 0, w = 0;      // global LDE height, width
  int owner = -1;           // rank holding the full matrix; -1 = replicated (every rank holds it)
  DMat full;                // the full column-major LDE where this rank computed it
  const u64* slice = nullptr;  // this rank's rows [rank h / N, (rank + 1) h / N) of the matrix, column stride = slice_stride
  size_t rows = 0;
  size_t slice_stride = 0;     // = rows for a received or copied range; = h where the range is read in place inside `full`
  const u64* foreign = nullptr;  // where another rank's range of this matrix was received
  bool pending = false;          // own matrix: buffer allocated, columns still to be produced (sharded_commit's producer)
};
struct ShardedCommit {
  std::vector<ShardMat> mats;   // batch (active circuit) order
  DBuf<u64> recv;               // uniform pattern: row ranges received from the owners, [source rank][column][row]
  std::vector<DBuf<u64>> recvs; // general pattern: one block per foreign sharded matrix, [column][row]
  DTree subtree;                // Merkle tree over this rank's rows
  std::vector<std::vector<Digest>> top;  // top[0] = the N sub-tree roots, ..., top.back() = { root }
  size_t maxh = 0;
  std::vector<Digest> cap;
  // the same levels where they are hashed - on the device (merkle_tree_top): 2 N - 1 digests, level l behind level l - 1; the
  // host copy h_top is QUEUED by sharded_commit and delivered by the next synchronisation, finish() then fills top and cap
  DBuf<Digest> d_top;
  std::vector<Digest> h_top;
  const Digest* d_cap = nullptr;  // the commitment in device memory: what the device transcript observes (outer.hip)
  size_t ncap = 0;
  unsigned lw = 0, cap_height = 0;
  bool finished = false;
  void finish() {
    if (finished) return;
    const size_t N = size_t(1) << lw;
    top.clear();
    if (cap_height > lw) {  // the cap lies inside the sub-trees: h_top is the cap itself, no level above it is ever opened
      if (h_top.size() != (size_t(1) << cap_height)) throw std::runtime_error("sharded commitment: cap missing");
      cap = h_top;
      finished = true;
      return;
    }
    if (h_top.size() != 2 * N - 1) throw std::runtime_error("sharded commitment: top levels missing");
    size_t off = 0;
    for (size_t len = N; len >= 1; len >>= 1) {
      top.emplace_back(h_top.begin() + off, h_top.begin() + off + len);
      off += len;
    }
    cap = top[lw - cap_height];
    finished = true;
  }
};

unsigned log2_world(int world) {
  if (world < 1 || (world & (world - 1))) throw std::runtime_error("sharded proving needs a power-of-two number of ranks");
  return log2_strict((size_t)world);
}

// mats[i].full is set wherever this rank holds the matrix. Exchanges the row ranges and builds the tree.
// `produce(i, c0, c1)`, when given, computes columns [c0, c1) of matrix i, one of this rank's own sharded matrices whose
// buffer is allocated but not yet filled (ShardMat::pending): the columns are produced in groups, and the exchange of one
// group runs while the next one is transformed.
// Two exchange patterns. UNIFORM - exactly one sharded matrix per rank, all of one shape, the k-th owned by rank k (BASELINE
// config 3: one adder per GPU): one symmetric all-to-all per column group. GENERAL - any number of sharded matrices per rank
// (none included), any shapes (the reference's multi-circuit systems: one wide circuit beside tables of other widths and
// heights, src/test_circuits/blake3.rs:2215-2613): every sharded matrix is handed out by its owner, row range by row range
// (ms_comm.scatter_cols_start), in batch order on every rank.
typedef std::function<void(size_t, size_t, size_t)> ColumnProducer;
// `defer`: the top levels' host copy is only queued (ShardedCommit::finish() after the caller's next synchronisation); the
// commitment is consumed on the device (sc.d_cap) in the meantime.
void sharded_commit(Comm& cm, ShardedCommit& sc, unsigned cap_height, const ColumnProducer* produce = nullptr,
                    const std::function<void()>* beside_hashing = nullptr, bool defer = false) {
  Ctx& ctx = cm.ctx;
  const size_t N = (size_t)cm.world(), me = (size_t)cm.rank();
  const unsigned lw = log2_world(cm.world());
  size_t sw = 0, shh = 0, n_sharded = 0;
  bool uniform = true;
  sc.maxh = 0;
  for (auto& m : sc.mats) {
    sc.maxh = std::max(sc.maxh, m.h);
    if (m.h < N) throw std::runtime_error("sharded proving: a committed matrix has fewer rows than there are ranks");
    m.rows = m.h / N;
    if (m.owner >= (int)N) throw std::runtime_error("sharded proving: owner rank out of range");
    if (m.owner >= 0) {
      if (n_sharded == 0) {
        sw = m.w;
        shh = m.h;
      } else if (m.w != sw || m.h != shh) {
        uniform = false;
      }
      if (m.owner != (int)n_sharded) uniform = false;
      if (m.owner == (int)me && !m.full.d()) throw std::runtime_error("sharded proving: this rank's own matrix is missing");
      n_sharded++;
    } else if (!m.full.d()) {
      throw std::runtime_error("sharded proving: a replicated matrix is missing on this rank");
    }
  }
  if (n_sharded != N) uniform = false;
  if (getenv("MSAMD_SHARDED_GENERAL")) uniform = false;  // (tests: the general pattern on a uniform system)
  sc.recvs.clear();
  if (uniform) {
    // ---- row-range all-to-all of the sharded matrices (block k of the send buffer = my rows for rank k)
    const size_t rows = shh / N, blk = sw * rows;
    sc.recv = DBuf<u64>(ctx, blk * N);
    size_t mine_i = sc.mats.size();
    for (size_t i = 0; i < sc.mats.size(); i++)
      if (sc.mats[i].owner == (int)me) mine_i = i;
    const ShardMat* mine = &sc.mats[mine_i];
    const bool prod = produce && mine->pending;
    if (cm.can_cols()) {
      // Rows [k h / N, (k + 1) h / N) of a column are contiguous in the column-major LDE and so is the place they take in
      // rank k's receive buffer: the transport sends them from where they are, column by column - no send buffer, no
      // packing pass over the LDE in front of every exchange. Column groups still overlap with the transforms.
      // (a single rank has nobody to exchange with: one launch per transform pass, as in the one-GPU prover)
      const size_t groups = prod && sw >= 8 && !getenv("MSAMD_SHARDED_NO_OVERLAP") && (N > 1 || getenv("MSAMD_SHARDED_WORLD1_TRANSPORT")) ? 4 : 1;
      for (size_t g = 0; g < groups; g++) {
        const size_t c0 = sw * g / groups, c1 = sw * (g + 1) / groups;
        if (prod) (*produce)(mine_i, c0, c1);
        cm.all_to_all_cols_start(mine->full.d() + c0 * shh, rows * 8, shh * 8, sc.recv.p + c0 * rows, blk * 8, rows * 8, c1 - c0, rows * 8, g);
      }
      cm.all_to_all_wait();
    } else {
      DBuf<u64> send(ctx, blk * N);
      auto pack = [&](size_t c0, size_t c1) {  // columns [c0, c1) of every peer's block
        for (size_t k = 0; k < N; k++)
          HIP_CHECK(hipMemcpy2DAsync(send.p + k * blk + c0 * rows, rows * 8, mine->full.d() + c0 * shh + k * rows, shh * 8, rows * 8,
                                     c1 - c0, hipMemcpyDeviceToDevice, ctx.stream));
      };
      const size_t groups = prod && cm.can_overlap() && sw >= 8 ? 4 : 1;
      if (groups == 1) {
        if (prod) (*produce)(mine_i, 0, sw);
        pack(0, sw);
        cm.all_to_all(send.p, sc.recv.p, blk * 8);
      } else {
        for (size_t g = 0; g < groups; g++) {
          const size_t c0 = sw * g / groups, c1 = sw * (g + 1) / groups;
          (*produce)(mine_i, c0, c1);
          pack(c0, c1);
          // chunk k of this group: columns [c0, c1) inside peer block k, on both sides
          cm.all_to_all_start(send.p + c0 * rows, blk * 8, sc.recv.p + c0 * rows, blk * 8, (c1 - c0) * rows * 8, g);
        }
        cm.all_to_all_wait();
      }
    }
    for (auto& m : sc.mats)
      if (m.owner >= 0 && m.owner != (int)me) m.foreign = sc.recv.p + (size_t)m.owner * blk;
  } else {
    // ---- every sharded matrix is handed out by its owner: the exchange of matrix i (non-blocking) runs while this rank
    // produces its next own matrix
    if (n_sharded && !cm.can_scatter())
      throw std::runtime_error("sharded proving: circuits of different shapes or counts per rank need ms_comm.scatter_cols_start, which this transport does not offer");
    size_t part = 0;
    for (size_t i = 0; i < sc.mats.size(); i++) {
      ShardMat& m = sc.mats[i];
      if (m.owner < 0) continue;
      if (m.owner == (int)me) {
        if (produce && m.pending) (*produce)(i, 0, m.w);
        cm.scatter_cols_start(m.owner, m.full.d(), m.rows * 8, m.h * 8, nullptr, 0, m.w, m.rows * 8, part++);
      } else {
        sc.recvs.emplace_back(ctx, m.w * m.rows);
        m.foreign = sc.recvs.back().p;
        cm.scatter_cols_start(m.owner, nullptr, 0, 0, sc.recvs.back().p, m.rows * 8, m.w, m.rows * 8, part++);
      }
    }
    if (part) cm.all_to_all_wait();
  }
  for (auto& m : sc.mats) m.pending = false;
  // ---- local views: received ranges, and this rank's range of every replicated matrix
  sc.subtree = DTree();
  sc.subtree.cap_height = 0;
  ctx.side_join();  // replicated short matrices were produced on the side stream
  // A matrix this rank holds in full - its own sharded one, every replicated one - is hashed, reduced and opened where it
  // is: the row range is a window of the LDE (column stride = the LDE's height), no copy. Only other ranks' ranges live
  // in the receive buffer.
  for (auto& m : sc.mats) {
    if (m.owner >= 0 && m.owner != (int)me) {
      m.slice = m.foreign;
      m.slice_stride = m.rows;
    } else {
      m.slice = m.full.d() + me * m.rows;
      m.slice_stride = m.h;
    }
    sc.subtree.mat_d.push_back(m.slice);
    sc.subtree.mat_h.push_back(m.rows);
    sc.subtree.mat_w.push_back(m.w);
    sc.subtree.mat_stride.push_back(m.slice_stride);
  }
  if (beside_hashing) {
    // work that does not depend on this commitment (the claims transcript's chaining values) runs on the side stream beside
    // the leaf hashing and the tree levels - integer-ALU work both, but the hashing leaves room - not beside the transforms
    ctx.side_fork();
    SideScope beside(ctx, true);
    (*beside_hashing)();
  }
  merkle_build(ctx, sc.subtree);
  // ---- sub-tree roots -> top levels, hashed on the device (N - 1 compressions in log2 N dependent steps): the commitment is
  // in device memory for the transcript kernels before the host has seen it
  const size_t root_layer = sc.subtree.layer_len.size() - 1;
  // the commitment is the layer of 2^cap_height digests (the whole leaf layer of a tree that is shorter than that)
  cap_height = std::min(cap_height, log2_strict(sc.maxh));
  sc.lw = lw;
  sc.cap_height = cap_height;
  sc.ncap = size_t(1) << cap_height;
  sc.finished = false;
  if (cap_height > lw) {
    // a cap taller than the ranks' sub-trees are apart: it is made of the sub-trees' layers 2^(cap_height - lw) digests wide,
    // gathered in rank order; nothing above it is hashed or opened
    const unsigned d = cap_height - lw;
    const size_t cnt = size_t(1) << d, layer = root_layer - d;
    if (sc.subtree.layer_len[layer] != cnt) throw std::runtime_error("sharded commitment: sub-tree layer size");
    sc.d_top = DBuf<Digest>(ctx, cnt * N);
    cm.all_gather(sc.subtree.base() + sc.subtree.layer_off[layer], sc.d_top.p, cnt * sizeof(Digest), "all_gather of the cap's digests");
    sc.d_cap = sc.d_top.p;
    sc.h_top.assign(cnt * N, Digest());
    ctx.d2h_queue(sc.h_top.data(), sc.d_top.p, cnt * N * sizeof(Digest));
  } else {
    DBuf<Digest> roots(ctx, N);
    cm.all_gather(sc.subtree.base() + sc.subtree.layer_off[root_layer], roots.p, sizeof(Digest), "all_gather of the sub-tree roots");
    sc.d_top = DBuf<Digest>(ctx, 2 * N - 1);
    merkle_tree_top(ctx, roots.p, N, sc.d_top.p);
    size_t off = 0;
    for (unsigned l = 0; l < lw - cap_height; l++) off += N >> l;
    sc.d_cap = sc.d_top.p + off;
    sc.h_top.assign(2 * N - 1, Digest());
    ctx.d2h_queue(sc.h_top.data(), sc.d_top.p, (2 * N - 1) * sizeof(Digest));
  }
  if (!defer) {
    ctx.sync();
    sc.finish();
  }
}

// number of sibling digests in an opening of this commitment (sub-tree levels + replicated top levels below the cap)
size_t sharded_nsib(const ShardedCommit& sc, unsigned cap_height) {
  const unsigned lmh = log2_strict(sc.maxh);
  return lmh - std::min(cap_height, lmh);
}

}  // namespace

// How a long claims list is split over N ranks (host-resident witnesses): rank r hashes the BLAKE3 chunks [r per, (r + 1) per) of
// the transcript `pl` prefix bytes || claim words, so it needs the claims whose words reach into that range - [sl_lo, sl_hi),
// one claim of margin at the end: the chunk kernel reads one word beyond a shifted block - and it inverts the fingerprints of
// [inv_lo, inv_hi), which partition the claims. `offsets` = the n_claims + 1 element offsets of ALL claims.
void claims_cut(size_t pl, size_t claim_words, size_t n_claims, const u64* offsets, size_t N, size_t r, size_t& sl_lo, size_t& sl_hi, size_t& inv_lo,
                size_t& inv_hi) {
  const size_t total_len = pl + 8 * claim_words;
  const size_t nchunks = blake3_num_chunks(pl, claim_words);
  const size_t per = (nchunks + N - 1) / N;
  auto wstart = [&](size_t i) { return 1 + i + (size_t)offsets[i]; };  // first transcript word of claim i
  // first claim whose words reach into the chunk range of rank q (n_claims when that range is empty)
  auto first_claim = [&](size_t q) -> size_t {
    const size_t b0 = q * per * 1024;
    if (b0 >= total_len) return n_claims;
    const size_t wa = b0 <= pl ? 0 : (b0 - pl) / 8;
    if (wa == 0) return 0;
    size_t lo = 0, hi = n_claims;  // the last claim with wstart <= wa
    while (lo + 1 < hi) {
      const size_t mid = (lo + hi) / 2;
      if (wstart(mid) <= wa)
        lo = mid;
      else
        hi = mid;
    }
    return lo;
  };
  // one claim past the last word the chunk kernel may touch for rank q (it reads one word beyond a shifted block)
  auto end_claim = [&](size_t q) -> size_t {
    const size_t b1 = std::min((q + 1) * per * 1024, total_len);
    if (b1 <= pl) return 0;
    const size_t wb = std::min(claim_words, (b1 - pl + 7) / 8 + 1);
    size_t lo = 0, hi = n_claims;  // the first claim with wstart >= wb
    while (lo < hi) {
      const size_t mid = (lo + hi) / 2;
      if (wstart(mid) >= wb)
        hi = mid;
      else
        lo = mid + 1;
    }
    return lo;
  };
  inv_lo = first_claim(r);
  inv_hi = r + 1 < N ? first_claim(r + 1) : n_claims;
  sl_lo = inv_lo;
  sl_hi = std::max(std::max(end_claim(r), inv_hi), sl_lo);
}
// length of the transcript in front of the claims: follows from the system's shape and the active circuits' heights alone
size_t claims_prefix_len(const HSystem& sys, const size_t* heights) {
  const size_t C = sys.circuits.size();
  size_t n_active = 0, max_lde_log = 0;
  for (size_t i = 0; i < C; i++)
    if (heights[i] > 0) {
      n_active++;
      max_lde_log = std::max<size_t>(max_lde_log, log2_strict(heights[i]) + (size_t)sys.params.log_blowup);
    }
  const size_t cap_digests = size_t(1) << std::min<size_t>((size_t)sys.params.cap_height, max_lde_log);
  return sys.seed.size() + 8 * (1 + 7 * C) + (sys.has_pre ? 32 * sys.pre_commit.size() : 0) + 32 * cap_digests + 8 * n_active;
}
// the element range [first, first + count) of the claims' data that rank `rank` of `world` reads in a joint proof
void claims_slice_range(const HSystem& sys, const size_t* heights, size_t n_claims, const u64* offsets, size_t rank, size_t world, size_t& first,
                        size_t& count) {
  const size_t total = n_claims ? (size_t)offsets[n_claims] : 0;
  const size_t claim_words = 1 + n_claims + total;
  if (claim_words <= 8192 || world <= 1) {  // a short list is absorbed whole by every rank
    first = 0;
    count = total;
    return;
  }
  size_t sl_lo, sl_hi, inv_lo, inv_hi;
  claims_cut(claims_prefix_len(sys, heights), claim_words, n_claims, offsets, world, rank, sl_lo, sl_hi, inv_lo, inv_hi);
  first = (size_t)offsets[sl_lo];
  count = (size_t)offsets[sl_hi] - first;
}

std::vector<uint8_t> prove_sharded(HSystem& sys, HWitness& wit, const ms_comm_t* comm, const int32_t* owners, StageMs* times) {
  Ctx& ctx = *sys.ctx;
  HIP_CHECK(hipSetDevice(ctx.device));
  Comm cm(ctx, comm);
  const Params& prm = sys.params;
  const unsigned lb = (unsigned)prm.log_blowup;
  const size_t C = sys.circuits.size();
  const size_t N = (size_t)cm.world(), me = (size_t)cm.rank();
  const unsigned lw = log2_world(cm.world());
  if (wit.sys != &sys || wit.heights.size() != C) throw std::runtime_error("witness does not belong to this system");
  double t_begin = now_ms(), t0;
  auto lap = [&](int slot) {
    if (times) {
      ctx.sync();
      times->v[slot] = now_ms() - t0;
    }
  };
  PhaseTrace tr(ctx);
  // host-resident witness: this rank's traces start travelling now; the claims follow as per-rank slices further down
  HostUpload up(wit, ctx);
  up.skip_claims = true;
  up.start();
  const size_t n_claims = wit.claim_offsets.size() - 1;
  const size_t claim_elems = wit.claim_elems_total;  // (the witness may hold only this rank's part of them: HWitness::claims_partial)
  const size_t claim_words = 1 + n_claims + claim_elems;
  // Host-resident witness: a rank uploads only the claims it works on - those whose transcript words fall into its range of
  // BLAKE3 chunks - and inverts the fingerprints of a sub-range of them; the ranges partition the claims. The slice is cut
  // and queued NOW, behind the trace on the copy stream, so that it travels while stage 1 is computed; that needs the
  // length of the transcript in front of the claims, which is known from the system's shape alone.
  DBuf<u64> sl_offs, sl_data;   // this rank's slice: offsets of claims [sl_lo, sl_hi] and their elements
  size_t sl_lo = 0, sl_hi = 0, inv_lo = 0, inv_hi = 0;
  const bool sliced = wit.host_resident && claim_words > 8192;
  size_t n_active = 0;
  for (size_t i = 0; i < C; i++) n_active += wit.heights[i] > 0;
  size_t max_lde_log = 0;
  for (size_t i = 0; i < C; i++)
    if (wit.heights[i] > 0) max_lde_log = std::max<size_t>(max_lde_log, log2_strict(wit.heights[i]) + lb);
  const size_t cap_digests = size_t(1) << std::min<size_t>((size_t)prm.cap_height, max_lde_log);  // (the three commitments share their tallest height)
  const size_t pl_expected = sys.seed.size() + 8 * (1 + 7 * C) + (sys.has_pre ? 32 * sys.pre_commit.size() : 0) + 32 * cap_digests + 8 * n_active;
  // The outer transcript on the device (outer.hip), as in the one-GPU prover: with the claims digest computed there, beta /
  // gamma, alpha and zeta are sampled in the stream - the commitments' top levels are hashed on the device too
  // (merkle_tree_top) - so that nothing between the stage-1 exchange and the opened-value sums waits for the host; the host
  // challenger replays the steps when the commitments arrive with the opened values, and is the authority. Needs the
  // transcript in front of the claims inside BLAKE3 chunk 0 (so that everything else of the claims digest is hashed early).
  const bool dev_outer = claim_words > 8192 && outer_fits(cap_digests, n_active) && pl_expected <= 1024 &&
                         blake3_num_chunks(pl_expected, claim_words) >= 2 && !getenv("MSAMD_HOST_TRANSCRIPT");
  OuterDev od;
  LateChunk0 late0;
  if (sliced) {
    claims_cut(pl_expected, claim_words, n_claims, wit.claim_offsets.data(), N, me, sl_lo, sl_hi, inv_lo, inv_hi);
    const size_t cnt = sl_hi - sl_lo, o0 = (size_t)wit.claim_offsets[sl_lo], o1 = (size_t)wit.claim_offsets[sl_hi];
    sl_offs = DBuf<u64>(ctx, cnt + 1);
    sl_data = DBuf<u64>(ctx, std::max<size_t>(o1 - o0, 1));
    // ordered behind the trace on the copy stream, like the claims of the one-GPU prover (and behind whatever kernels of the
    // main stream may still be using the pool blocks just handed out)
    HIP_CHECK(hipEventRecord(ctx.copy_ev[3], ctx.stream));
    HIP_CHECK(hipStreamWaitEvent(ctx.copy_stream, ctx.copy_ev[3], 0));
    ctx.copy_delay();  // (diagnostics: MSAMD_COPY_DELAY_US)
    auto from_caller = [&](void* dst, const void* src, size_t bytes) {  // (as in HostUpload::issue: page-locked ranges, or the bounce buffer)
      if (wit.pinned)
        HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx.copy_stream));
      else
        ctx.bounce_h2d(dst, src, bytes, ctx.copy_stream);
    };
    from_caller(sl_offs.p, wit.claim_offsets.data() + sl_lo, (cnt + 1) * 8);
    if (o0 < wit.claim_elem0 || o1 > wit.claim_elem0 + wit.claim_data.size())
      throw std::runtime_error("sharded proving: this rank's witness does not hold the part of the claims it reads (ms_claims_slice_range)");
    if (o1 > o0) from_caller(sl_data.p, wit.claim_data.data() + (o0 - wit.claim_elem0), (o1 - o0) * 8);
    HIP_CHECK(hipEventRecord(ctx.copy_ev[0], ctx.copy_stream));
  }

  // Only the BLAKE3 chunks that hold transcript bytes in front of the claims (chunk 0, on rank 0) depend on the stage-1
  // commitment: the chaining values of every other chunk of this rank's range are computed beside the hashing of that
  // commitment (sharded_commit's side-stream hook), so that behind the commitment only chunk 0, the gather and the tree over
  // the chunks remain - as in the one-GPU prover.
  DBuf<u64> cl_words;
  DBuf<Digest> cl_part, cl_all;
  size_t cl_nchunks = 0, cl_per = 0, cl_prefix_chunks = 0, cl_w_first = 0;
  bool cl_early_done = false;
  std::function<void()> early_claims = [&]() {
    const size_t pl = pl_expected;
    cl_nchunks = blake3_num_chunks(pl, claim_words);
    cl_per = (cl_nchunks + N - 1) / N;
    cl_prefix_chunks = std::min(cl_nchunks, (pl + 1023) / 1024);
    auto wstart = [&](size_t i) { return 1 + i + (size_t)wit.claim_offsets[i]; };
    if (sliced) {
      const size_t cnt = sl_hi - sl_lo, o0 = (size_t)wit.claim_offsets[sl_lo];
      HIP_CHECK(hipStreamWaitEvent(ctx.stream, ctx.copy_ev[0], 0));  // this rank's slice of the claims has arrived
      cl_w_first = sl_lo == 0 ? 0 : wstart(sl_lo);
      const size_t w_end = sl_hi == n_claims ? claim_words : wstart(sl_hi);
      const size_t span = std::max<size_t>(w_end - cl_w_first, 1) + 2;
      cl_words = DBuf<u64>(ctx, span);
      HIP_CHECK(hipMemsetAsync(cl_words.p, 0, span * 8, ctx.stream));
      if (cnt) claims_transcript_words_slice(ctx, sl_data.p - o0, sl_offs.p, sl_lo, cnt, n_claims, cl_words.p - cl_w_first);
    } else {  // the claims are in HBM in full (device-resident witness): every rank still hashes only its range of chunks
      cl_w_first = 0;
      cl_words = DBuf<u64>(ctx, claim_words + 2);
      claims_transcript_words(ctx, wit.d_claim_data.p, wit.d_claim_offsets.p, n_claims, claim_elems, cl_words.p);
    }
    cl_part = DBuf<Digest>(ctx, cl_per);
    cl_all = DBuf<Digest>(ctx, cl_per * N);
    HIP_CHECK(hipMemsetAsync(cl_part.p, 0, cl_per * sizeof(Digest), ctx.stream));
    const size_t c0 = std::max(me * cl_per, cl_prefix_chunks), c1 = (me + 1) * cl_per;
    if (c1 > c0) blake3_chunk_cvs(ctx, nullptr, pl, cl_words.p - cl_w_first, claim_words, c0, c1, cl_part.p - me * cl_per);
    if (dev_outer) {
      // Chunk 0 alone depends on the commitment (pl <= 1024): every other chaining value is gathered NOW - on whichever stream
      // this runs, the side stream beside the hashing - and the tree above the chunks is hashed with a placeholder in slot 0;
      // behind the commitment one wave finishes the digest and samples beta and gamma (claims_root_k).
      {
        Comm::OnStream os(cm, ctx.stream);
        cm.all_gather(cl_part.p, cl_all.p, cl_per * sizeof(Digest), "all_gather of the claims transcript's chaining values");
      }
      blake3_late_chunk0_prepare(ctx, cl_all.p, cl_nchunks, late0);
    }
    cl_early_done = true;
  };

  Challenger ch(sys.seed);
  ch.observe((u64)C);
  for (auto& c : sys.circuits) {
    ch.observe((u64)c.constraint_count);
    ch.observe((u64)c.max_constraint_degree);
    ch.observe((u64)c.pre_height);
    ch.observe((u64)c.pre_width);
    ch.observe((u64)c.main_width);
    ch.observe((u64)c.stage2_width);
  }
  std::vector<uint8_t> active(C);
  std::vector<size_t> aidx;
  std::vector<int> apos(C, -1);
  for (size_t i = 0; i < C; i++) {
    active[i] = wit.heights[i] > 0;
    ch.observe(active[i] ? 1 : 0);
    if (active[i]) {
      apos[i] = (int)aidx.size();
      aidx.push_back(i);
    }
  }
  if (aidx.empty()) throw std::runtime_error("cannot prove with every circuit deactivated (all traces empty)");
  const size_t NA = aidx.size();
  // which circuits this rank computes: its own sharded one and every replicated one
  std::vector<char> mine(NA, 0);
  for (size_t pos = 0; pos < NA; pos++) {
    const int o = owners[aidx[pos]];
    if (o >= (int)N) throw std::runtime_error("owner rank out of range");
    mine[pos] = o < 0 || o == (int)me;
    if (mine[pos] && !wit.traces[aidx[pos]].p) throw std::runtime_error("sharded proving: this rank lacks the trace of a circuit it computes");
  }
  std::vector<unsigned> log_degrees;
  for (size_t ci : aidx) log_degrees.push_back(log2_strict(wit.heights[ci]));
  // Short replicated circuits beside a long sharded one (the byte table beside 2^20 additions, on EVERY rank): their
  // kernels are a handful of workgroups each and cost launch latency, not work; as in the one-GPU prover they are queued on
  // the context's side stream and run beside the long kernels, joined before each commitment is hashed.
  ctx.side_config();
  std::vector<char> on_side(NA, 0);
  bool use_side = false;
  {
    unsigned own_ld = 0;
    for (size_t pos = 0; pos < NA; pos++)
      if (owners[aidx[pos]] == (int)me) own_ld = log_degrees[pos];
    for (size_t pos = 0; pos < NA; pos++)
      if (ctx.side_enabled && owners[aidx[pos]] < 0 && log_degrees[pos] <= ctx.side_max_log && own_ld > ctx.side_max_log) {
        on_side[pos] = 1;
        use_side = true;
      }
  }
  struct SideSession {  // whatever happens, the streams are joined when the proof is left
    Ctx& c;
    ~SideSession() { c.side_join(); }
  } side_session{ctx};
  auto fork_side = [&]() {
    if (use_side && !ctx.side_forked) ctx.side_fork();
  };

  // ---- stage 1 commit
  t0 = now_ms();
  cm.phase = "stage-1 commit";
  up.wait_traces();
  ShardedCommit s1;
  fork_side();
  for (size_t pos = 0; pos < NA; pos++) {
    const size_t ci = aidx[pos];
    ShardMat m;
    m.h = wit.heights[ci] << lb;
    m.w = sys.circuits[ci].main_width;
    m.owner = owners[ci];
    SideScope sc(ctx, on_side[pos]);
    if (mine[pos] && m.owner < 0) m.full = lde_of_host_matrix(ctx, wit.traces[ci].p, wit.heights[ci], m.w, lb);
    s1.mats.push_back(std::move(m));
  }
  {
    // this rank's own matrices are extended inside sharded_commit, column group by column group, so that the exchange of
    // one group (or of one matrix) runs while the next one is transformed
    std::vector<DBuf<u64>> evs1(NA);
    for (size_t pos = 0; pos < NA; pos++) {
      if (owners[aidx[pos]] != (int)me) continue;
      ShardMat& m = s1.mats[pos];
      const size_t n = wit.heights[aidx[pos]];
      evs1[pos] = DBuf<u64>(ctx, n * m.w);
      transpose_in(ctx, wit.traces[aidx[pos]].p, evs1[pos].p, n, m.w, true);
      m.full.h = m.h;
      m.full.w = m.w;
      m.full.buf = DBuf<u64>(ctx, m.h * m.w);
      m.pending = true;
    }
    ColumnProducer prod = [&](size_t pos, size_t c0, size_t c1) {
      ShardMat& m = s1.mats[pos];
      const size_t n = wit.heights[aidx[pos]];
      coset_lde(ctx, evs1[pos].p + c0 * n, m.full.d() + c0 * m.h, log_degrees[pos], lb, c1 - c0);
      if (c1 == m.w) evs1[pos].reset();
    };
    sharded_commit(cm, s1, (unsigned)prm.cap_height, &prod, (sliced || dev_outer) ? &early_claims : nullptr, dev_outer);
  }
  lap(0);
  tr.mark("stage1_commit");

  cm.phase = "claims";
  if (sys.has_pre) ch.observe_cap(sys.pre_commit);
  const size_t cap_off = ch.input.size();
  if (dev_outer)
    ch.observe_cap(std::vector<Digest>(cap_digests));  // placeholder bytes: the device patches the commitment over them
  else
    ch.observe_cap(s1.cap);
  for (unsigned ld : log_degrees) ch.observe(ld);
  DBuf<ChallengeBG> d_bg;
  // claims: every rank holds all of them (the transcript absorbs them in order) but the work is split: each rank
  // hashes 1/N of the BLAKE3 chunks of the claims transcript and inverts 1/N of the claim fingerprints; chaining
  // values and partial sums are all-gathered (values only - the field additions happen locally, in rank order)
  if (wit.claims_partial && !sliced) throw std::runtime_error("sharded proving: a short claims list must be held in full by every rank");
  if (wit.host_resident && !sliced) {  // a short list: every rank takes all of it
    wit.d_claim_offsets = DBuf<u64>(ctx, n_claims + 1);
    wit.d_claim_data = DBuf<u64>(ctx, std::max<size_t>(claim_elems, 1));
    ctx.h2d(wit.d_claim_offsets.p, wit.claim_offsets.data(), (n_claims + 1) * 8);
    if (claim_elems) ctx.h2d(wit.d_claim_data.p, wit.claim_data.data(), claim_elems * 8);
  }
  if (dev_outer) {
    const size_t pl = ch.input.size();
    if (pl != pl_expected) throw std::runtime_error("sharded proving: transcript prefix length differs from the expected one");
    if (!cl_early_done) early_claims();  // (not reached: the stage-1 commit runs it)
    ctx.side_join();
    // chunk 0: the transcript so far (placeholder bytes where the commitment goes) and the first words of the claims, which
    // every rank has on the host
    DBuf<uint8_t> d_prefix(ctx, pl);
    ctx.h2d(d_prefix.p, ch.input.data(), pl);
    std::vector<u64> w0;
    w0.push_back((u64)n_claims);
    for (size_t i = 0; i < n_claims && w0.size() < 130; i++) {
      const size_t a = wit.claim_offsets[i], b = wit.claim_offsets[i + 1];
      w0.push_back((u64)(b - a));
      for (size_t k = a; k < b && w0.size() < 130; k++) w0.push_back(wit.claims_partial ? wit.claim_head.at(k) : wit.claim_data[k]);
    }
    DBuf<u64> d_w0(ctx, w0.size());
    ctx.h2d(d_w0.p, w0.data(), w0.size() * 8);
    od.digest = DBuf<Digest>(ctx, 1);
    od.state = DBuf<u32>(ctx, 20);
    d_bg = DBuf<ChallengeBG>(ctx, 1);
    blake3_late_chunk0_finish(ctx, d_prefix.p, pl, d_w0.p, claim_words, s1.d_cap, cap_off, cap_digests, late0, cl_nchunks, od.digest.p, d_bg.p,
                              od.state.p);
    ctx.d2h_queue(&od.h_digest, od.digest.p, sizeof(Digest));
    ctx.d2h_queue(od.h_bg, d_bg.p, 2 * sizeof(E2));  // beta, gamma lead the block
    cl_words.reset();
    cl_part.reset();
    cl_all.reset();
    late0.reset();
  } else if (sliced) {
    const size_t pl = ch.input.size();
    if (pl != pl_expected) throw std::runtime_error("sharded proving: transcript prefix length differs from the one the claim slices were cut for");
    if (!cl_early_done) early_claims();  // (not reached: the stage-1 commit runs it)
    ctx.side_join();
    // what is left behind the commitment: the chunks that hold prefix bytes (rank 0's chunk 0), the gather, the tree
    const size_t c0 = me * cl_per, c1 = std::min((me + 1) * cl_per, cl_prefix_chunks);
    if (c1 > c0) {
      DBuf<uint8_t> d_prefix(ctx, pl);
      ctx.h2d(d_prefix.p, ch.input.data(), pl);
      blake3_chunk_cvs(ctx, d_prefix.p, pl, cl_words.p - cl_w_first, claim_words, c0, c1, cl_part.p - me * cl_per);
      cm.all_gather(cl_part.p, cl_all.p, cl_per * sizeof(Digest), "all_gather of the claims transcript's chaining values");
      Digest d = blake3_from_cvs(ctx, cl_all.p, cl_nchunks);
      ch.flush_with(d);
    } else {
      cm.all_gather(cl_part.p, cl_all.p, cl_per * sizeof(Digest), "all_gather of the claims transcript's chaining values");
      Digest d = blake3_from_cvs(ctx, cl_all.p, cl_nchunks);
      ch.flush_with(d);
    }
    cl_words.reset();
    cl_part.reset();
    cl_all.reset();
  } else if (claim_words > 8192) {
    DBuf<uint8_t> d_prefix(ctx, ch.input.size());
    ctx.h2d(d_prefix.p, ch.input.data(), ch.input.size());
    DBuf<u64> d_words(ctx, claim_words);
    claims_transcript_words(ctx, wit.d_claim_data.p, wit.d_claim_offsets.p, n_claims, claim_elems, d_words.p);
    const size_t nchunks = blake3_num_chunks(ch.input.size(), claim_words);
    const size_t per = (nchunks + N - 1) / N;
    DBuf<Digest> part(ctx, per), all(ctx, per * N);
    HIP_CHECK(hipMemsetAsync(part.p, 0, per * sizeof(Digest), ctx.stream));
    blake3_chunk_cvs(ctx, d_prefix.p, ch.input.size(), d_words.p, claim_words, me * per, (me + 1) * per, part.p - me * per);
    cm.all_gather(part.p, all.p, per * sizeof(Digest));
    Digest d = blake3_from_cvs(ctx, all.p, nchunks);
    ch.flush_with(d);
  } else {
    ch.observe((u64)n_claims);
    for (size_t i = 0; i < n_claims; i++) {
      size_t a = wit.claim_offsets[i], b = wit.claim_offsets[i + 1];
      ch.observe((u64)(b - a));
      for (size_t k = a; k < b; k++) ch.observe(wit.claim_data[k]);
    }
  }
  E2 beta = e2(0), gamma = e2(0), alpha = e2(0), zeta = e2(0);
  if (!dev_outer) {
    tx_beta_gamma(ch, beta, gamma);
    d_bg = challenge_bg_upload(ctx, beta, gamma);
  }
  // The claims accumulator (this rank's share of the fingerprints) and every circuit's logUp total stay in device memory:
  // nothing needs them on the host before the stage-2 commitment is observed, so they travel in ONE all_gather behind that
  // commitment (values only - the field additions happen on the host, in rank order) instead of one round trip each.
  DBuf<E2> d_part(ctx, NA + 1);  // [pos] = total of circuit pos where this rank computes it, [NA] = claims share
  HIP_CHECK(hipMemsetAsync(d_part.p, 0, (NA + 1) * sizeof(E2), ctx.stream));
  {
    // nothing reads the claims' share before the totals are gathered in front of the stage-2 commitment: with a side stream it
    // runs there, beside the stage-2 terms (the streams join in front of that gather), as in the one-GPU prover
    const bool beside = ctx.side_enabled && !getenv("MSAMD_CLAIMS_ACC_MAIN");
    if (beside && !ctx.side_forked) ctx.side_fork();
    SideScope sc(ctx, beside);
    const size_t per = (n_claims + N - 1) / N;
    const size_t a = std::min(n_claims, me * per), b = std::min(n_claims, (me + 1) * per);
    if (sliced) {  // this rank's share of the partition that follows the chunk ranges
      if (inv_hi > inv_lo)
        claims_accumulator_dyn(ctx, sl_data.p - (size_t)wit.claim_offsets[sl_lo], sl_offs.p + (inv_lo - sl_lo), inv_hi - inv_lo, d_bg.p,
                               d_part.p + NA);
    } else if (b > a) {
      claims_accumulator_dyn(ctx, wit.d_claim_data.p, wit.d_claim_offsets.p + a, b - a, d_bg.p, d_part.p + NA);
    }
  }
  tr.mark("claims");

  // ---- lookup construction + stage 2 commit; every circuit's total travels by all_gather, never by a field reduction
  t0 = now_ms();
  up.lookup_values();
  std::vector<DBuf<u64>> s2_evals(NA);
  fork_side();  // behind the claims accumulator and the lookup values
  for (size_t pos = 0; pos < NA; pos++) {
    if (!mine[pos]) continue;
    const size_t ci = aidx[pos];
    const HCircuit& c = sys.circuits[ci];
    SideScope sc(ctx, on_side[pos]);
    s2_evals[pos] = DBuf<u64>(ctx, wit.heights[ci] * c.stage2_width);
    stage2_circuit_dyn(ctx, sys, wit, ci, d_bg.p, s2_evals[pos].p, d_part.p + pos);
  }
  lap(1);
  t0 = now_ms();
  cm.phase = "stage-2 commit";
  ShardedCommit s2;
  for (size_t pos = 0; pos < NA; pos++) {
    const size_t ci = aidx[pos];
    const HCircuit& c = sys.circuits[ci];
    ShardMat m;
    m.h = wit.heights[ci] << lb;
    m.w = c.stage2_width;
    m.owner = owners[ci];
    SideScope sc(ctx, on_side[pos]);
    if (mine[pos]) {
      m.full.h = m.h;
      m.full.w = m.w;
      m.full.buf = DBuf<u64>(ctx, m.h * m.w);
      if (m.owner < 0) {
        coset_lde(ctx, s2_evals[pos].p, m.full.d(), log_degrees[pos], lb, m.w);
        s2_evals[pos].reset();
      }
    }
    s2.mats.push_back(std::move(m));
  }
  ctx.side_join();  // the totals of the replicated circuits were written on the side stream
  // every circuit's logUp total and the claims shares are complete once the stage-2 evaluations are (above): their
  // all_gather is queued now and its read-back rides on the synchronisation that fetches the commitment's sub-tree roots
  DBuf<E2> d_all(ctx, (NA + 1) * N);
  std::vector<E2> all_tot((NA + 1) * N);
  cm.all_gather(d_part.p, d_all.p, (NA + 1) * sizeof(E2), "all_gather of the logUp totals");
  ctx.d2h_queue(all_tot.data(), d_all.p, all_tot.size() * sizeof(E2));
  {
    for (size_t pos = 0; pos < NA; pos++)
      if (owners[aidx[pos]] == (int)me) s2.mats[pos].pending = true;
    ColumnProducer prod = [&](size_t pos, size_t c0, size_t c1) {
      ShardMat& m = s2.mats[pos];
      const size_t n = wit.heights[aidx[pos]];
      coset_lde(ctx, s2_evals[pos].p + c0 * n, m.full.d() + c0 * m.h, log_degrees[pos], lb, c1 - c0);
      if (c1 == m.w) s2_evals[pos].reset();
    };
    sharded_commit(cm, s2, (unsigned)prm.cap_height, &prod, nullptr, dev_outer);
  }
  E2 acc_initial = e2(0);
  std::vector<E2> accs;
  auto host_alpha = [&]() {  // src/prover.rs:382-433; all_tot was delivered by a synchronisation since it was queued
    const std::vector<E2>& all = all_tot;
    acc_initial = e2(0);
    accs.clear();
    for (size_t r = 0; r < N; r++) acc_initial = e2_add(acc_initial, all[r * (NA + 1) + NA]);
    E2 acc = acc_initial;
    for (size_t pos = 0; pos < NA; pos++) {
      const int o = owners[aidx[pos]];
      const size_t src = o < 0 ? me : (size_t)o;
      acc = e2_add(acc, all[src * (NA + 1) + pos]);
      accs.push_back(acc);
    }
    alpha = tx_alpha(ch, s2.cap, accs);
  };
  if (dev_outer) {
    // the same sums on the device, then alpha and every circuit's challenge block (outer_alpha_k)
    std::vector<int> src(NA);
    for (size_t pos = 0; pos < NA; pos++) src[pos] = owners[aidx[pos]] < 0 ? (int)me : owners[aidx[pos]];
    od.tot = DBuf<E2>(ctx, NA + 1);
    outer_joint_totals(ctx, d_all.p, N, NA, src, od.tot.p);
    od.accs = DBuf<E2>(ctx, NA + 1);
    od.alpha = DBuf<E2>(ctx, 1);
    od.qdyn.resize(NA);
    std::vector<OuterTarget> targets(NA);
    for (size_t pos = 0; pos < NA; pos++) {
      const size_t k = sys.circuits[aidx[pos]].prog.constraint_count;
      od.qdyn[pos] = DBuf<uint8_t>(ctx, sizeof(QDyn) + std::max<size_t>(k, 1) * sizeof(E2));
      targets[pos].dyn = reinterpret_cast<QDyn*>(od.qdyn[pos].p);
      targets[pos].alpha_rev = reinterpret_cast<E2*>(od.qdyn[pos].p + sizeof(QDyn));
      targets[pos].log_n = log_degrees[pos];
      targets[pos].k = k;
    }
    outer_alpha(ctx, od.state.p, s2.d_cap, cap_digests, od.tot.p, NA, d_bg.p, targets, od.accs.p, od.alpha.p, od.state.p + 12, od.circuits);
    ctx.d2h_queue(&od.h_alpha, od.alpha.p, sizeof(E2));
    lap(2);
    tr.mark("stage2");
  } else {
    lap(2);
    tr.mark("stage2");
    host_alpha();
  }

  // ---- quotient
  t0 = now_ms();
  cm.phase = "quotient commit";
  ShardedCommit qd;
  fork_side();
  for (size_t pos = 0; pos < NA; pos++) {
    const size_t ci = aidx[pos];
    const HCircuit& c = sys.circuits[ci];
    SideScope sc(ctx, on_side[pos]);
    const unsigned log_n = log_degrees[pos], log_q = log2_strict(c.quotient_degree());
    const size_t n = size_t(1) << log_n, nq = n << log_q;
    ShardMat m;
    m.h = n << lb;
    m.w = 2 << log_q;
    m.owner = owners[ci];
    if (mine[pos]) {
      QuotientArgs qa = fill_quotient_args(sys, ci, s1.mats[pos].full, s2.mats[pos].full, log_n, log_q, dev_outer ? od.qdyn[pos].p : nullptr);
      if (!dev_outer) quotient_publics(qa, beta, gamma, pos ? accs[pos - 1] : acc_initial, accs[pos], alpha);
      DBuf<u64> qv(ctx, nq * 2);
      quotient_eval(ctx, c.prog, qa, qv.p);
      m.full.h = m.h;
      m.full.w = m.w;
      m.full.buf = DBuf<u64>(ctx, m.h * m.w);
      quotient_lde(ctx, qv.p, m.full.d(), log_n, log_q, lb, 2);
    }
    qd.mats.push_back(std::move(m));
  }
  sharded_commit(cm, qd, (unsigned)prm.cap_height, nullptr, nullptr, dev_outer);
  // zeta and zeta * g per trace height: values in host mode, placeholders for device values otherwise (swapped for the values
  // when the opened-value sums have arrived and the host has replayed the transcript)
  E2 pt_zeta = e2(0);
  std::vector<E2> pt_next(NA);
  if (dev_outer) zeta_placeholders(ctx, od, log_degrees, qd.d_cap, cap_digests, nullptr, pt_zeta, pt_next);
  lap(3);
  tr.mark("quotient");

  // ---- opening
  t0 = now_ms();
  cm.phase = "opening";
  if (!dev_outer) {
    zeta = tx_zeta(ch, qd.cap);
    pt_zeta = zeta;
    for (size_t pos = 0; pos < NA; pos++) pt_next[pos] = e2_mul_base(zeta, gl_two_adic_generator(log_degrees[pos]));
  }
  ShardedCommit* scs[3] = {&s1, &s2, &qd};
  // points per round / matrix: rounds 0..2 = s1, s2, quotient; round 3 = preprocessed
  std::vector<std::vector<std::vector<E2>>> rpoints(3);
  for (size_t pos = 0; pos < NA; pos++) {
    rpoints[0].push_back({pt_zeta, pt_next[pos]});
    rpoints[1].push_back({pt_zeta, pt_next[pos]});
    rpoints[2].push_back({pt_zeta});
  }
  std::vector<std::vector<E2>> pre_points;
  if (sys.has_pre)
    for (size_t ci = 0; ci < C; ci++) {
      if (sys.pre_indices[ci] < 0) continue;
      if (apos[ci] >= 0)
        pre_points.push_back({pt_zeta, pt_next[apos[ci]]});
      else
        pre_points.push_back({});
    }
  // The second point of a matrix is its first times the generator g of its trace domain: it needs no inverse denominators of
  // its own - 1 / (z g - x_j) = g^-1 / (z - x_sigma(j)), sigma a permutation of the storage order (open.hip::rev_dec) - so
  // barycentric sums and reduced openings read the first point's arrays through sigma (MSAMD_NO_NEXT_SHIFT=1: its own pass).
  // sigma maps the row range of rank k onto the row range of ONE rank (the same one while ranks <= blowup): sigma_range.
  const bool next_shift = !getenv("MSAMD_NO_NEXT_SHIFT") && lb <= 31;
  auto is_next = [&](const std::vector<E2>& pts) { return next_shift && pts.size() == 2; };
  auto sigma_range = [&](size_t k) -> size_t {  // range of a domain cut into N row ranges that sigma maps range k onto
    if (lw <= lb) return k;
    const size_t low = bitrev64(k, lw);  // the low lw bits of the natural index of range k's rows
    return bitrev64((low - (size_t(1) << lb)) & (N - 1), lw);
  };
  // unique opening points and the tallest matrix opened at each
  size_t gmax = 0, gw = 0;
  for (auto* sc : scs)
    for (auto& m : sc->mats) {
      gmax = std::max(gmax, m.h);
      gw = std::max(gw, m.w);
    }
  if (sys.has_pre)
    for (auto& m : sys.pre_data.ldes) {
      gmax = std::max(gmax, m.h);
      gw = std::max(gw, m.w);
    }
  const unsigned log_gmax = log2_strict(gmax);
  OpenPoints op;
  for (int ri = 0; ri < 3; ri++)
    for (size_t mi = 0; mi < NA; mi++)
      for (size_t pi = 0; pi < rpoints[ri][mi].size(); pi++) {
        if (pi == 1 && is_next(rpoints[ri][mi])) continue;  // read through the first point's arrays
        op.note(rpoints[ri][mi][pi], scs[ri]->mats[mi].h);
      }
  if (sys.has_pre)
    for (size_t mi = 0; mi < sys.pre_data.ldes.size(); mi++)
      for (size_t pi = 0; pi < pre_points[mi].size(); pi++) {
        if (pi == 1 && is_next(pre_points[mi])) continue;
        op.note(pre_points[mi][pi], sys.pre_data.ldes[mi].h);
      }
  const std::vector<E2>& upts = op.upts;
  const std::vector<size_t>& uh = op.uh;
  // short matrices beside tall ones: their launches go to the side stream, queued behind the tall ones'
  const size_t short_h = size_t(1) << (ctx.side_max_log + lb);
  const bool open_side = use_side && gmax > short_h;
  std::vector<DBuf<E2>> dens(upts.size()), xdens(upts.size());
  for (int pass = 0; pass < 2; pass++) {
    // the short matrices' sums also read the tall points' weights: fork once those are queued
    if (pass == 1 && open_side) ctx.side_fork();
    for (size_t k = 0; k < upts.size(); k++) {
      if ((int)(open_side && uh[k] <= short_h) != pass) continue;
      SideScope sc(ctx, pass == 1);
      dens[k] = DBuf<E2>(ctx, uh[k]);
      xdens[k] = DBuf<E2>(ctx, uh[k] >> lb);
      // Only the rows somebody reads: the barycentric weights are the trace-domain prefix [0, h / blowup) of the tallest
      // matrix, a sharded height is reduced on this rank's row range alone, a replicated height on all its rows. At eight
      // ranks that is 3/8 of the domain instead of all of it.
      std::vector<std::pair<size_t, size_t>> need;
      need.emplace_back(size_t(0), uh[k] >> lb);
      auto reads = [&](size_t h, bool sharded, const std::vector<E2>& pts) {
        const bool nx = is_next(pts);
        for (size_t pi = 0; pi < pts.size(); pi++) {
          const bool through = pi == 1 && nx;  // the second point reads the FIRST point's arrays, through sigma
          if (!e2_same(pts[through ? 0 : pi], upts[k])) continue;
          if (!sharded) {
            need.emplace_back(size_t(0), h);
          } else {
            const size_t r = through ? sigma_range(me) : me;
            need.emplace_back(r * (h / N), (r + 1) * (h / N));
          }
        }
      };
      for (int ri = 0; ri < 3; ri++)
        for (size_t mi = 0; mi < NA; mi++) {
          bool sh = false;  // a height is reduced on row ranges when ANY matrix of that height is sharded (add_deep below)
          for (int rj = 0; rj < 3 && !sh; rj++)
            for (auto& m2 : scs[rj]->mats) sh = sh || (m2.owner >= 0 && m2.h == scs[ri]->mats[mi].h);
          reads(scs[ri]->mats[mi].h, sh, rpoints[ri][mi]);
        }
      if (sys.has_pre)
        for (size_t mi = 0; mi < sys.pre_data.ldes.size(); mi++) {
          bool sh = false;
          for (int rj = 0; rj < 3 && !sh; rj++)
            for (auto& m2 : scs[rj]->mats) sh = sh || (m2.owner >= 0 && m2.h == sys.pre_data.ldes[mi].h);
          reads(sys.pre_data.ldes[mi].h, sh, pre_points[mi]);
        }
      std::sort(need.begin(), need.end());
      std::vector<std::pair<size_t, size_t>> merged;
      for (auto& iv : need) {
        if (iv.first >= iv.second) continue;
        if (!merged.empty() && iv.first <= merged.back().second)
          merged.back().second = std::max(merged.back().second, iv.second);
        else
          merged.push_back(iv);
      }
      for (auto& iv : merged) {
        if (is_sym_point(upts[k]))  // the device sampled the point (outer_zeta_k): read it where it lies
          inv_denoms_rows_dev(ctx, od.points.p + upts[k].c0, log2_strict(uh[k]), dens[k].p, xdens[k].p, uh[k] >> lb, iv.first, iv.second - iv.first);
        else
          inv_denoms_rows(ctx, upts[k], log2_strict(uh[k]), dens[k].p, xdens[k].p, uh[k] >> lb, iv.first, iv.second - iv.first);
      }
    }
  }
  // opened values: this rank evaluates the matrices it holds in full; the sharded ones travel by all_gather
  struct Ev {
    int ri;
    size_t mi;
    size_t off;
  };
  std::vector<Ev> evs;
  size_t total_vals = 0;
  auto enqueue = [&](int ri, size_t mi, const DMat& m, const std::vector<E2>& pts) {
    if (pts.empty()) return;
    if (pts.size() > 2) throw std::runtime_error("pcs_open: more than two points per matrix");
    evs.push_back(Ev{ri, mi, total_vals});
    total_vals += pts.size() * m.w;
  };
  for (int ri = 0; ri < 3; ri++)
    for (size_t mi = 0; mi < NA; mi++)
      if (mine[mi]) enqueue(ri, mi, scs[ri]->mats[mi].full, rpoints[ri][mi]);
  if (sys.has_pre)
    for (size_t mi = 0; mi < sys.pre_data.ldes.size(); mi++) enqueue(3, mi, sys.pre_data.ldes[mi], pre_points[mi]);
  DBuf<E2> d_sums(ctx, std::max<size_t>(total_vals, 1));
  DBuf<E2> bary_partials[2];
  for (int pass = 0; pass < 2; pass++) {
    std::vector<BarySpec> specs;  // the matrices of one stream share a pair of launches (open.hip::bary_sums_batch)
    for (auto& e : evs) {
      const DMat& m = e.ri < 3 ? scs[e.ri]->mats[e.mi].full : sys.pre_data.ldes[e.mi];
      if ((int)(open_side && m.h <= short_h) != pass) continue;
      const std::vector<E2>& pts = e.ri < 3 ? rpoints[e.ri][e.mi] : pre_points[e.mi];
      const int np = (int)pts.size();
      const bool nx = is_next(pts);
      const E2* d0 = xdens[op.index(pts[0])].p;
      const E2* d1 = np == 2 && !nx ? xdens[op.index(pts[1])].p : d0;
      specs.push_back(BarySpec{m.d(), m.h, m.w, log2_strict(m.h) - lb, d0, d1, np, d_sums.p + e.off, nx});
    }
    if (!specs.empty()) {
      SideScope sc(ctx, pass == 1);
      bary_sums_batch(ctx, specs, bary_partials[pass]);
    }
  }
  ctx.side_join();  // the blob copies and the read-back below see every sum
  // The raw barycentric sums of this rank's own circuits (rounds 0..2, one blob per rank) are all-gathered ON THE DEVICE and
  // come back with the sums of everything else this rank evaluated in ONE read-back; the finishing scale factors are applied
  // on the host for every circuit alike.
  // blob of rank r: for each circuit it owns (in batch order) the sums of rounds 0..2; every rank can size every blob from
  // the system's shape, and the all_gather carries the longest one's length
  auto circuit_len = [&](size_t pos) {
    size_t n = 0;
    for (int ri = 0; ri < 3; ri++) n += rpoints[ri][pos].size() * scs[ri]->mats[pos].w;
    return n;
  };
  std::vector<size_t> blob_of(N, 0);
  for (size_t pos = 0; pos < NA; pos++)
    if (owners[aidx[pos]] >= 0) blob_of[(size_t)owners[aidx[pos]]] += circuit_len(pos);
  size_t blob_len = 0;
  for (size_t r = 0; r < N; r++) blob_len = std::max(blob_len, blob_of[r]);
  DBuf<E2> d_blob(ctx, std::max<size_t>(blob_len, 1)), d_blobs(ctx, std::max<size_t>(blob_len, 1) * N);
  if (blob_len) {
    if (blob_of[me] < blob_len) HIP_CHECK(hipMemsetAsync(d_blob.p, 0, blob_len * sizeof(E2), ctx.stream));
    size_t off = 0;
    for (size_t pos = 0; pos < NA; pos++) {
      if (owners[aidx[pos]] != (int)me) continue;
      for (int ri = 0; ri < 3; ri++)
        for (auto& e : evs)
          if (e.ri == ri && e.mi == pos) {
            const size_t cnt = rpoints[ri][pos].size() * scs[ri]->mats[pos].w;
            HIP_CHECK(hipMemcpyAsync(d_blob.p + off, d_sums.p + e.off, cnt * sizeof(E2), hipMemcpyDeviceToDevice, ctx.stream));
            off += cnt;
          }
    }
    if (off != blob_of[me]) throw std::runtime_error("sharded proving: opened-value blob layout");
  }
  std::vector<E2> h_sums(std::max<size_t>(total_vals, 1)), h_blobs(std::max<size_t>(blob_len, 1) * N);
  if (blob_len) cm.all_gather(d_blob.p, d_blobs.p, blob_len * sizeof(E2), "all_gather of the opened values");
  ctx.d2h_queue(h_sums.data(), d_sums.p, total_vals * sizeof(E2));
  ctx.d2h_queue(h_blobs.data(), d_blobs.p, blob_len * N * sizeof(E2));
  ctx.sync();  // the opened values - and with them everything queued since the stage-1 exchange
  if (dev_outer) {
    // the host learns the commitments, the totals and the challenges now: it replays the transcript on its own challenger
    // (the authority) and fails the proof on any difference, then swaps the placeholder points for their values
    s1.finish();
    s2.finish();
    qd.finish();
    ch.flush_with(od.h_digest);
    tx_beta_gamma(ch, beta, gamma);
    host_alpha();
    zeta = tx_zeta(ch, qd.cap);
    const std::vector<E2> values = replayed_points(od, beta, gamma, alpha, zeta);
    op.resolve(values);
    for (auto& r : rpoints)
      for (auto& pts : r) swap_in(pts, values);
    for (auto& pts : pre_points) swap_in(pts, values);
  }
  std::vector<OpenedRound> opened(sys.has_pre ? 4 : 3);
  for (int ri = 0; ri < 3; ri++) opened[ri].resize(NA);
  if (sys.has_pre) opened[3].resize(sys.pre_data.ldes.size());
  for (auto& e : evs) {
    const DMat& m = e.ri < 3 ? scs[e.ri]->mats[e.mi].full : sys.pre_data.ldes[e.mi];
    const std::vector<E2>& pts = e.ri < 3 ? rpoints[e.ri][e.mi] : pre_points[e.mi];
    opened[e.ri][e.mi] = finish_opened(&h_sums[e.off], m.w, log2_strict(m.h) - lb, pts);
  }
  {
    std::vector<size_t> cursor(N, 0);  // position inside each rank's blob
    for (size_t pos = 0; pos < NA; pos++) {
      const int o = owners[aidx[pos]];
      if (o < 0) continue;
      const size_t at = cursor[(size_t)o];
      cursor[(size_t)o] += circuit_len(pos);
      if (o == (int)me) continue;
      const E2* src = &h_blobs[(size_t)o * blob_len + at];
      size_t off = 0;
      for (int ri = 0; ri < 3; ri++) {
        const ShardMat& m = scs[ri]->mats[pos];
        const std::vector<E2>& pts = rpoints[ri][pos];
        opened[ri][pos] = finish_opened(src + off, m.w, log2_strict(m.h) - lb, pts);
        off += pts.size() * m.w;
      }
    }
  }
  // observe in round -> matrix -> point order; rounds as prove() orders them: s1, s2, quotient, pre
  for (auto& orr : opened)
    for (auto& m : orr)
      for (auto& pt : m)
        for (auto& y : pt) ch.observe_ext(y);
  tr.mark("opened_values");
  const E2 alpha_fri = ch.sample_ext();
  const std::vector<E2> apow = alpha_powers(alpha_fri, gw);
  DBuf<E2> d_apow(ctx, gw + 1);
  ctx.h2d(d_apow.p, apow.data(), (gw + 1) * sizeof(E2));

  // ---- reduced openings per LDE height: heights with sharded matrices on this rank's row range (then all-gathered),
  // the others replicated
  std::vector<char> sharded_h(33, 0);
  for (int ri = 0; ri < 3; ri++)
    for (auto& m : scs[ri]->mats)
      if (m.owner >= 0) sharded_h[log2_strict(m.h)] = 1;
  DeepPlan plan(op, dens, alpha_fri, apow, lb);
  for (int ri = 0; ri < 3; ri++)
    for (size_t mi = 0; mi < NA; mi++) {
      const ShardMat& m = scs[ri]->mats[mi];
      const unsigned lh = log2_strict(m.h);
      // at a sharded height every matrix is read through its local row range (column stride = rows of the range)
      plan.add(lh, sharded_h[lh] ? m.slice : m.full.d(), sharded_h[lh] ? m.slice_stride : 0, m.w, rpoints[ri][mi], is_next(rpoints[ri][mi]), opened[ri][mi]);
    }
  if (sys.has_pre)
    for (size_t mi = 0; mi < sys.pre_data.ldes.size(); mi++) {
      const DMat& m = sys.pre_data.ldes[mi];
      const unsigned lh = log2_strict(m.h);
      // (a preprocessed matrix that shares a sharded height is read through its row range in place)
      plan.add(lh, sharded_h[lh] ? m.d() + me * (m.h / N) : m.d(), sharded_h[lh] ? m.h : 0, m.w, pre_points[mi], is_next(pre_points[mi]), opened[3][mi]);
    }
  const auto& lists = plan.lists;
  const auto& hpts = plan.hpts;
  const auto& present = plan.present;
  // Row-sharded FRI head (SURVEY 8e item 5): when the tallest reduced-opening vector is the (only) sharded one, its first
  // log2 N commit-phase rounds run on the ranks' row ranges - contiguous storage rows are closed under the fold's pairs and
  // form a sub-tree of each round's Merkle tree - with one all-gather of N sub-tree roots per round; only the remainder
  // (1/N of the vector) is all-gathered, instead of the whole vector before round 0. MSAMD_SHARDED_FULL_FRI=1: the old way.
  int lh_top = -1, n_sharded_heights = 0;
  for (int lh = 32; lh >= 0; lh--)
    if (present[lh]) {
      if (lh_top < 0) lh_top = lh;
      if (sharded_h[lh] && !lists[lh].empty()) n_sharded_heights++;
    }
  const size_t fri_stop = (size_t(1) << lb) << prm.log_final_poly_len;
  const size_t H_top = lh_top >= 0 ? size_t(1) << lh_top : 0;
  // (binary rounds only: with max_log_arity > 1 the whole vector is gathered and fri_prove folds it - on the device transcript
  // where that applies, round by round)
  // (and commitments of at most N digests: a taller cap would cut into the rounds' sub-trees - the whole vector is gathered then)
  const bool use_head = N > 1 && prm.max_log_arity == 1 && (unsigned)prm.cap_height <= lw && !getenv("MSAMD_SHARDED_FULL_FRI") && lh_top >= 0 && sharded_h[lh_top] && !lists[lh_top].empty() &&
                        n_sharded_heights == 1 && H_top >= N * N && H_top / N > fri_stop;
  if (getenv("MSAMD_TRACE"))
    fprintf(stderr, "[msamd] fri head: N %zu lh_top %d sharded_top %d lists %zu n_sharded_heights %d H %zu stop %zu -> %d\n", N, lh_top,
            lh_top >= 0 ? (int)sharded_h[lh_top] : -1, lh_top >= 0 ? lists[lh_top].size() : 0, n_sharded_heights, H_top, fri_stop, (int)use_head);
  DBuf<E2> head_part;             // this rank's rows of the tallest vector
  DTree head_tree0, fri_round0;   // leaf layers hashed by the reduction pass: the head's first round / FRI's first round (one rank)
  std::vector<DBuf<E2>> inputs;  // descending height
  if (open_side) ctx.side_fork();  // behind the upload of the alpha powers
  for (int lh = 32; lh >= 0; lh--) {
    if (!present[lh]) continue;
    const size_t h = size_t(1) << lh;
    SideScope sc(ctx, open_side && h <= short_h && !sharded_h[lh]);
    // the tallest vector is FRI's first committed matrix: its leaf layer is hashed by the pass that produces it (as in pcs_open)
    const bool fuse_leaves = inputs.empty() && prm.max_log_arity == 1 && !getenv("MSAMD_NO_DEEP_LEAVES") && !lists[lh].empty();
    if (use_head && lh == lh_top) {
      head_part = DBuf<E2>(ctx, h / N);
      Digest* leaves = nullptr;
      if (fuse_leaves && h / N >= 8192) {
        merkle_alloc(ctx, head_tree0, (h / N) / 2);
        leaves = head_tree0.base();
      }
      deep_reduce(ctx, lists[lh], hpts[lh], h / N, d_apow.p, head_part.p, apow.data(), leaves, nullptr, me * (h / N), h);
      inputs.emplace_back();  // placeholder: filled with the gathered remainder after the head rounds
      continue;
    }
    DBuf<E2> ro(ctx, h);
    if (lists[lh].empty()) {
      HIP_CHECK(hipMemsetAsync(ro.p, 0, h * sizeof(E2), ctx.stream));
    } else if (sharded_h[lh] && N == 1 && !getenv("MSAMD_SHARDED_WORLD1_TRANSPORT")) {
      // a single rank's row range is the whole domain: reduced where FRI reads it, no gather
      Digest* leaves = nullptr;
      if (fuse_leaves && h >= 8192) {
        merkle_alloc(ctx, fri_round0, h / 2);
        leaves = fri_round0.base();
      }
      deep_reduce(ctx, lists[lh], hpts[lh], h, d_apow.p, ro.p, apow.data(), leaves, nullptr, 0, h);
    } else if (sharded_h[lh]) {
      const size_t rows = h / N;
      DBuf<E2> part(ctx, rows);
      deep_reduce(ctx, lists[lh], hpts[lh], rows, d_apow.p, part.p, apow.data(), nullptr, nullptr, me * rows, h);
      cm.all_gather(part.p, ro.p, rows * sizeof(E2), "all_gather of reduced openings");
    } else {
      deep_reduce(ctx, lists[lh], hpts[lh], h, d_apow.p, ro.p, apow.data());
    }
    inputs.push_back(std::move(ro));
  }
  ctx.side_join();  // the short reduced openings read the tall points' denominators, released next
  for (auto& d : dens) d.reset();
  for (auto& d : xdens) d.reset();
  tr.mark("deep_reduce+gather");

  // ---- FRI head on row shards
  FriHead head;
  std::vector<DBuf<E2>> head_layers;                       // this rank's slice of v_r, r < lw
  std::vector<DTree> head_trees;                           // the sub-tree over its leaves
  std::vector<std::vector<std::vector<Digest>>> head_tops; // per round: the N sub-tree roots, ..., the root
  std::vector<DBuf<Digest>> head_top_dev;                  // the same levels where the device hashed them (2 N - 1 digests per round) ...
  std::vector<std::vector<Digest>> head_top_host;          // ... and their queued host copies: head_tops is built from them after FRI's wait
  if (use_head) {
    cm.phase = "FRI head rounds";
    head.n_rounds = lw;
    head.log_max_height = (unsigned)lh_top;
    DBuf<E2> cur = std::move(head_part);
    size_t next_in = 1;
    // The rounds' transcript steps on the DEVICE, under the conditions of fri_prove's own device rounds (a root-only commitment,
    // the challenger's pending input exactly one digest, a short proof-of-work): the N gathered sub-tree roots, the levels above
    // them and the challenger step (observe the root, grind, sample beta) are ONE single-workgroup launch per round
    // (merkle_top_challenge), the fold reads beta where that launch left it, and fri_prove goes on from the same device state -
    // no host synchronisation inside the head (it was two per round: the roots, the proof-of-work search).
    const bool dev_head = prm.cap_height == 0 && ch.input.size() == 32 && prm.commit_pow_bits <= 16 && N <= 1024 && !getenv("MSAMD_HOST_FRI");
    if (dev_head) {
      head.on_device = true;
      head.d_state = DBuf<uint32_t>(ctx, 8);
      ctx.h2d(head.d_state.p, ch.input.data(), 32);
      head.d_recs = DBuf<FriTailRound>(ctx, lw);
    }
    for (unsigned r = 0; r < lw; r++) {
      const size_t m = (H_top >> r) / N;     // my elements of v_r
      const size_t rows_total = H_top >> (r + 1);  // leaves of this round's tree = length of the folded vector
      const bool prehashed = r == 0 && head_tree0.digests.p != nullptr;
      if (prehashed)
        head_trees.push_back(std::move(head_tree0));
      else
        head_trees.emplace_back();
      DTree& t = head_trees.back();
      t.cap_height = 0;
      fri_tree_build(ctx, t, prehashed ? nullptr : cur.p, m / 2);
      const size_t root_layer = t.layer_len.size() - 1;
      if (dev_head) {
        head_top_dev.emplace_back(ctx, 2 * N - 1);
        Digest* top = head_top_dev.back().p;
        cm.all_gather(t.base() + t.layer_off[root_layer], top, sizeof(Digest), "all_gather of a FRI head round's sub-tree roots");
        merkle_top_challenge(ctx, top, N, FriChallenge{head.d_state.p, head.d_recs.p + r, (uint32_t)prm.commit_pow_bits});
        head_top_host.emplace_back(2 * N - 1);
        ctx.d2h_queue(head_top_host.back().data(), top, (2 * N - 1) * sizeof(Digest));
        head.nsib.push_back(log2_strict(rows_total));
        const E2* roll = nullptr;
        if (next_in < inputs.size() && inputs[next_in].n == rows_total) roll = inputs[next_in++].p + me * (rows_total / N);
        DBuf<E2> nxt(ctx, m / 2);
        fri_fold_dev(ctx, cur.p, m / 2, head.d_recs.p + r, roll, nxt.p, nullptr, me * (m / 2), rows_total);
        head_layers.push_back(std::move(cur));
        cur = std::move(nxt);
        continue;
      }
      DBuf<Digest> roots(ctx, N);
      cm.all_gather(t.base() + t.layer_off[root_layer], roots.p, sizeof(Digest), "all_gather of a FRI head round's sub-tree roots");
      std::vector<std::vector<Digest>> top(1, std::vector<Digest>(N));
      ctx.d2h(top[0].data(), roots.p, N * sizeof(Digest));
      while (top.back().size() > 1) {
        const auto& prev = top.back();
        std::vector<Digest> next(prev.size() / 2);
        for (size_t i = 0; i < next.size(); i++) {
          uint8_t buf[64];
          memcpy(buf, prev[2 * i].b, 32);
          memcpy(buf + 32, prev[2 * i + 1].b, 32);
          blake3_host(buf, 64, next[i].b);
        }
        top.push_back(std::move(next));
      }
      const std::vector<Digest>& cap = top[lw - (unsigned)prm.cap_height];
      ch.observe_cap(cap);
      head.commits.push_back(cap);
      head.pow.push_back(grind(ctx, ch, (unsigned)prm.commit_pow_bits));
      const E2 beta_r = ch.sample_ext();
      head.nsib.push_back(log2_strict(rows_total) - (size_t)prm.cap_height);
      const E2* roll = nullptr;
      if (next_in < inputs.size() && inputs[next_in].n == rows_total) roll = inputs[next_in++].p + me * (rows_total / N);
      DBuf<E2> nxt(ctx, m / 2);
      fri_fold(ctx, cur.p, m / 2, beta_r, roll, nxt.p, me * (m / 2), rows_total);
      head_layers.push_back(std::move(cur));
      head_tops.push_back(std::move(top));
      cur = std::move(nxt);
    }
    // the remainder: 1 / N of the original vector, gathered to every rank; inputs rolled in above are done with
    const size_t rem = H_top >> lw;
    DBuf<E2> full(ctx, rem);
    cm.all_gather(cur.p, full.p, (rem / N) * sizeof(E2), "all_gather of the FRI remainder");
    std::vector<DBuf<E2>> rest;
    rest.push_back(std::move(full));
    for (size_t k = next_in; k < inputs.size(); k++) rest.push_back(std::move(inputs[k]));
    inputs = std::move(rest);
    tr.mark("fri_head_rounds");
  }

  // ---- FRI, replicated; the openings of the input rounds are served by the rank that owns the queried row
  cm.phase = "FRI queries";
  InputShape shape;
  for (auto* sc : scs) {
    std::vector<size_t> widths;
    for (auto& m : sc->mats) widths.push_back(m.w);
    shape.widths.push_back(std::move(widths));
    shape.nsib.push_back(sharded_nsib(*sc, (unsigned)prm.cap_height));
  }
  if (sys.has_pre) {
    std::vector<size_t> widths;
    for (auto& m : sys.pre_data.ldes) widths.push_back(m.w);
    shape.widths.push_back(std::move(widths));
    shape.nsib.push_back(sys.pre_data.tree.cap_layer());
  }
  size_t input_qbytes = 0;
  for (size_t ri = 0; ri < shape.widths.size(); ri++) {
    for (size_t w : shape.widths[ri]) input_qbytes += 8 * w;
    input_qbytes += 32 * shape.nsib[ri];
  }
  const size_t head_qbytes = use_head ? head.qbytes() : 0;
  // Every rank serves the queries whose rows it holds: ONE gather kernel over all queries (those of other ranks' row ranges are
  // skipped and stay zero), ONE all_gather of the blocks, one read-back - queued on the device behind the query indices as soon
  // as the device has sampled them, so the openings arrive with the FRI phase's own synchronisation (fri_prove calls `queue`);
  // with host-sampled indices `fetch` uploads them and runs the same sequence. The siblings above the sub-trees come from the
  // replicated top levels, which every host holds.
  const unsigned owner_shift = log_gmax - lw;  // a query belongs to the rank whose row range holds its row: the top lw bits
  auto owner_of = [&](uint64_t index) { return (size_t)(index >> owner_shift); };
  std::vector<GatherSeg> qsegs;  // what this rank reads for ONE query: rows (local range for sharded data), sub-tree siblings
  std::vector<size_t> local_nsib, head_nloc;
  size_t lbytes = 0;
  {
    size_t off = 0;
    for (auto* sc : scs) {
      const unsigned lmh = log2_strict(sc->maxh);
      const unsigned sh0 = log_gmax - lmh;
      for (auto& m : sc->mats) {
        const unsigned sh = sh0 + (lmh - log2_strict(m.h));
        // local view: element (row, c) at slice[c * rows + row - me * rows]; pointer pre-shifted by the range start
        add_gather_seg(qsegs, off, m.slice - me * m.rows, m.slice_stride, (uint32_t)m.w, 0, sh, 0);
      }
      const DTree& t = sc->subtree;
      // levels below the sub-tree root - or below the cap, when that lies inside the sub-tree
      const size_t nloc = std::min(t.layer_len.size() - 1, sharded_nsib(*sc, (unsigned)prm.cap_height));
      for (size_t i = 0; i < nloc; i++)
        add_gather_seg(qsegs, off, t.base() + t.layer_off[i] - me * t.layer_len[i], 0, 1, 1, sh0 + (unsigned)i, 1);
      local_nsib.push_back(nloc);
    }
    if (sys.has_pre) {
      const DTree& t = sys.pre_data.tree;
      const unsigned lmh = log2_strict(t.max_height());
      const unsigned sh0 = log_gmax - lmh;
      for (auto& m : sys.pre_data.ldes) add_gather_seg(qsegs, off, m.d(), m.h, (uint32_t)m.w, 0, sh0 + (lmh - log2_strict(m.h)), 0);
      for (size_t i = 0; i < t.cap_layer(); i++) add_gather_seg(qsegs, off, t.base() + t.layer_off[i], 0, 1, 1, sh0 + (unsigned)i, 1);
      local_nsib.push_back(t.cap_layer());
    }
    // head rounds: the sibling value in my slice of v_r and the siblings inside my sub-tree of round r's tree
    for (unsigned r = 0; r < head.n_rounds; r++) {
      const size_t m = (H_top >> r) / N;
      add_gather_seg(qsegs, off, head_layers[r].p - me * m, 0, 1, 2, r, 1);
      const DTree& t = head_trees[r];
      const size_t nloc = t.layer_len.size() - 1;
      for (size_t i = 0; i < nloc; i++)
        add_gather_seg(qsegs, off, t.base() + t.layer_off[i] - me * t.layer_len[i], 0, 1, 1, (uint32_t)(r + 1 + i), 1);
      head_nloc.push_back(nloc);
    }
    lbytes = off;
  }
  DBuf<uint8_t> q_loc, q_all;
  DBuf<GatherSeg> q_segs_dev;
  std::vector<uint8_t>& q_host = ctx.host_scratch2;
  size_t q_queued = 0;  // queries whose blocks have been queued for the read-back
  InputGather remote;
  remote.queue = [&](const u64* d_indices, size_t nq) {
    if (nq == 0 || lbytes == 0) return;
    q_loc = DBuf<uint8_t>(ctx, nq * lbytes);
    q_all = DBuf<uint8_t>(ctx, nq * lbytes * N);
    q_segs_dev = DBuf<GatherSeg>(ctx, qsegs.size());
    HIP_CHECK(hipMemsetAsync(q_loc.p, 0, nq * lbytes, ctx.stream));
    gather_queries_launch(ctx, qsegs, q_segs_dev.p, d_indices, nq, lbytes, q_loc.p, owner_shift, (uint32_t)me);
    cm.all_gather(q_loc.p, q_all.p, nq * lbytes, "all_gather of the query openings");
    if (q_host.size() < nq * lbytes * N) q_host.resize(nq * lbytes * N);
    ctx.d2h_queue(q_host.data(), q_all.p, nq * lbytes * N);
    q_queued = nq;
  };
  remote.fetch = [&](const std::vector<uint64_t>& indices, size_t qbytes, uint8_t* out) {
    if (qbytes != input_qbytes + head_qbytes) throw std::runtime_error("sharded proving: query block size mismatch");
    const size_t nq = indices.size();
    if (q_queued != nq) {  // the indices were sampled on the host: the same sequence now, behind an upload of the indices
      DBuf<u64> d_idx(ctx, std::max<size_t>(nq, 1));
      ctx.h2d(d_idx.p, indices.data(), nq * 8);
      remote.queue(d_idx.p, nq);
      ctx.sync();
    }
    if (head_tops.empty() && !head_top_host.empty()) {  // the head rounds' top levels, hashed on the device, have arrived by now
      for (auto& flat : head_top_host) {
        std::vector<std::vector<Digest>> top;
        size_t off = 0;
        for (size_t len = N; len >= 1; len >>= 1) {
          top.emplace_back(flat.begin() + off, flat.begin() + off + len);
          off += len;
        }
        head_tops.push_back(std::move(top));
      }
    }
    // global layout per query: rows, local siblings, then the siblings from the replicated top levels
    for (size_t qi = 0; qi < nq; qi++) {
      const size_t o = owner_of(indices[qi]);
      if (o >= N) throw std::runtime_error("sharded proving: query index outside the domain");
      const uint8_t* src = &q_host[(o * nq + qi) * lbytes];
      uint8_t* dst = out + qi * qbytes;
      for (size_t ri = 0; ri < shape.widths.size(); ri++) {
        size_t rb = 0;
        for (size_t w : shape.widths[ri]) rb += 8 * w;
        memcpy(dst, src, rb + 32 * local_nsib[ri]);
        src += rb + 32 * local_nsib[ri];
        dst += rb + 32 * local_nsib[ri];
        if (ri < 3) {
          const ShardedCommit& sc = *scs[ri];
          const unsigned lmh = log2_strict(sc.maxh);
          const uint64_t row = indices[qi] >> (log_gmax - lmh);
          const size_t nloc = local_nsib[ri];
          for (size_t lvl = nloc; lvl < shape.nsib[ri]; lvl++) {
            const size_t node = (size_t)((row >> lvl) ^ 1);
            memcpy(dst, sc.top[lvl - nloc][node].b, 32);
            dst += 32;
          }
        }
      }
      for (unsigned r = 0; r < head.n_rounds; r++) {
        const size_t loc = 16 + 32 * head_nloc[r];
        memcpy(dst, src, loc);
        src += loc;
        dst += loc;
        const uint64_t leaf = indices[qi] >> (r + 1);  // leaf of round r's tree
        for (size_t lvl = head_nloc[r]; lvl < head.nsib[r]; lvl++) {
          const size_t node = (size_t)((leaf >> lvl) ^ 1);
          memcpy(dst, head_tops[r][lvl - head_nloc[r]][node].b, 32);
          dst += 32;
        }
      }
      if ((size_t)(dst - (out + qi * qbytes)) != qbytes) throw std::runtime_error("sharded proving: query block layout");
    }
  };
  PW fri;
  fri_prove(sys, ch, inputs, log_gmax, std::vector<GatherSeg>(), input_qbytes, shape, &remote, fri, tr, use_head ? &head : nullptr,
            fri_round0.digests.p ? &fri_round0 : nullptr);
  lap(4);

  // ---- Proof bytes, field order of src/prover.rs:213-238
  PW w;
  w.u64_(C);
  for (auto a : active) w.u8(a);
  w.cap(s1.cap);
  w.cap(s2.cap);
  w.cap(qd.cap);
  w.u64_(accs.size());
  for (auto& a : accs) w.ext(a);
  w.u64_(log_degrees.size());
  for (unsigned ld : log_degrees) w.u8((uint8_t)ld);
  w.raw(fri.b.data(), fri.b.size());
  write_round(w, opened[2]);
  w.u8(sys.has_pre ? 1 : 0);
  if (sys.has_pre) write_round(w, opened[3]);
  write_round(w, opened[0]);
  write_round(w, opened[1]);
  ctx.prof_collect();
  if (times) times->v[5] = now_ms() - t_begin;
  return std::move(w.b);
}
