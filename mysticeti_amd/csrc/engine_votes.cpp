// mv_votes_* / mv_aggregate_votes / mv_dev_aggregate_votes: the host side of votes.hip. One call =
// the scan, its totals read back (they size the event lists and decide about room), the insert
// rounds of the sharing blocks' references into the store's own table, rows, events, one pass per
// segment (most calls have one), the per-block counts and the store's statistics.
#include <algorithm>
#include <cstring>
#include <vector>

#include "engine_internal.h"

using namespace mvi;

namespace {

using Votes = Device::Votes;
constexpr size_t kSlotBytes = 64;
constexpr uint64_t kMaxRows = 1ull << 31, kMaxCells = 1ull << 40, kMaxEvents = 0xfffffff0ull;
constexpr int kMaxRounds = 1 << 16;

uint64_t slots_for_rows(uint64_t rows) {
  uint64_t s = 16;
  while (s < 4 * rows) s <<= 1;
  return s;
}

mvk::VoteStore view_of(mv_ctx* ctx, const Votes& q, const DevBuf& tab, const DevBuf& rowmap, const DevBuf& row_key,
                       const DevBuf& row_base, const DevBuf& row_n, const DevBuf& row_agg, const DevBuf& cells,
                       uint64_t slots, uint64_t cap_rows, uint64_t cap_cells) {
  mvk::VoteStore v{};
  v.t = mvk::IndexTable{tab.as<unsigned long long>(), slots - 1, ctx->index_secret[0], ctx->index_secret[1], 64};
  v.rowmap = rowmap.as<uint32_t>();
  v.row_key = row_key.as<uint64_t>();
  v.row_base = row_base.as<uint64_t>();
  v.row_n = row_n.as<uint32_t>();
  v.row_agg = row_agg.as<uint32_t>();
  v.cells = cells.as<uint64_t>();
  v.cap_rows = cap_rows, v.cap_cells = cap_cells;
  v.cw = 2 + q.voter_words;
  return v;
}
mvk::VoteStore view_of(mv_ctx* ctx, const Votes& q) {
  return view_of(ctx, q, q.tab, q.rowmap, q.row_key, q.row_base, q.row_n, q.row_agg, q.cells, q.slots, q.cap_rows,
                 q.cap_cells);
}

// the control words on the host (synchronises s); a failed device check is MV_E_HIP
mv_status read_votes_ctl(mv_ctx* ctx, Votes& q, hipStream_t s, const uint64_t** words) {
  HIPCHK(ctx, hipMemcpyAsync(q.h_ctl.p, q.ctl.p, 8 * mvk::VT_CTL_WORDS, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  const uint64_t* w = q.h_ctl.as<uint64_t>();
  *words = w;
  if (w[mvk::VT_CTL_ERR] || w[mvk::IX_CTL_ERR])
    return set_err(ctx, MV_E_HIP,
                   "votes: " + std::to_string(w[mvk::VT_CTL_ERR] + w[mvk::IX_CTL_ERR]) +
                       " device checks failed (a row, cell or event number outside its array); mv_votes_clear resets the store");
  return MV_OK;
}

// A store of cap_rows rows and cap_cells cells; the rows of the one in force that have an
// aggregating cell move into it (the others, and their cells, are dropped). Synchronises s.
mv_status votes_rebuild(mv_ctx* ctx, Votes& q, uint64_t cap_rows, uint64_t cap_cells, hipStream_t s) {
  cap_rows = std::max<uint64_t>(cap_rows, 1), cap_cells = std::max<uint64_t>(cap_cells, 1);
  if (cap_rows > kMaxRows || cap_cells > kMaxCells) return set_err(ctx, MV_E_INVALID_ARG, "votes: store too large");
  const uint64_t slots = slots_for_rows(cap_rows);
  const size_t cw = 2 + (size_t)q.voter_words;
  DevBuf tab, rowmap, row_key, row_base, row_n, row_agg, cells;
  if (tab.ensure(kSlotBytes * slots) != hipSuccess || rowmap.ensure(4 * slots) != hipSuccess ||
      row_key.ensure(48 * cap_rows) != hipSuccess || row_base.ensure(8 * cap_rows) != hipSuccess ||
      row_n.ensure(4 * cap_rows) != hipSuccess || row_agg.ensure(4 * cap_rows) != hipSuccess ||
      cells.ensure(8 * cw * cap_cells) != hipSuccess) {
    (void)hipGetLastError();
    return set_err(ctx, MV_E_ALLOC, "votes: no device memory for " + std::to_string(cap_rows) + " rows and " +
                                        std::to_string(cap_cells) + " cells");
  }
  HIPCHK(ctx, q.ctl.ensure(8 * mvk::VT_CTL_WORDS));
  HIPCHK(ctx, q.h_ctl.ensure(8 * mvk::VT_CTL_WORDS));
  HIPCHK(ctx, hipMemsetAsync(q.ctl.p, 0, 8 * mvk::VT_CTL_WORDS, s));
  HIPCHK(ctx, hipMemsetAsync(tab.p, 0, kSlotBytes * slots, s));
  HIPCHK(ctx, hipMemsetAsync(rowmap.p, 0xff, 4 * slots, s));
  HIPCHK(ctx, hipMemsetAsync(cells.p, 0, 8 * cw * cap_cells, s));
  const mvk::VoteStore fresh = view_of(ctx, q, tab, rowmap, row_key, row_base, row_n, row_agg, cells, slots, cap_rows,
                                       cap_cells);
  if (q.on && q.nrows) HIPCHK(ctx, mvk::launch_votes_move(view_of(ctx, q), q.nrows, fresh, q.ctl.as<uint64_t>(), s));
  const uint64_t* w = nullptr;
  const mv_status st = read_votes_ctl(ctx, q, s, &w);  // the old store is read until here
  if (st != MV_OK) return st;
  std::swap(q.tab, tab), std::swap(q.rowmap, rowmap), std::swap(q.row_key, row_key), std::swap(q.row_base, row_base);
  std::swap(q.row_n, row_n), std::swap(q.row_agg, row_agg), std::swap(q.cells, cells);
  q.slots = slots, q.cap_rows = cap_rows, q.cap_cells = cap_cells;
  q.nrows = w[mvk::VT_CTL_NROWS], q.ncells = w[mvk::VT_CTL_NCELLS];
  q.live_cells = q.ncells;
  q.on = true;
  return MV_OK;
}

// `need` entries where `cap` are: as they are, or a geometric step
uint64_t grown_to(uint64_t cap, uint64_t need) { return need <= cap ? cap : std::max(need, cap + cap / 2); }

// bump allocation out of one scratch buffer
struct Carve {
  uint8_t* p;
  size_t at = 0;
  template <class T>
  T* take(size_t count) {
    T* r = reinterpret_cast<T*>(p + at);
    at += ix_al(sizeof(T) * std::max<size_t>(count, 1));
    return r;
  }
};
template <class Fn>
mv_status carved(mv_ctx* ctx, DevBuf& buf, Fn fn) {
  Carve sizing{nullptr};
  fn(sizing);
  HIPCHK(ctx, buf.ensure(sizing.at));
  Carve real{buf.as<uint8_t>()};
  fn(real);
  return MV_OK;
}

// One call on device arrays, on stream s, which it synchronises.
mv_status votes_run(mv_ctx* ctx, Device& dev, const uint8_t* d_buf, uint64_t buf_bytes, const uint64_t* d_off,
                    const uint64_t* d_len, uint32_t n, uint32_t flags, uint8_t* d_status, uint64_t* d_counts,
                    uint64_t* d_cert, uint64_t cap_cert, uint64_t* n_cert, hipStream_t s) {
  Votes& q = dev.votes;
  const mvh::Committee& com = ctx->committee;
  if (!q.on) return set_err(ctx, MV_E_INVALID_ARG, "votes: no store (mv_votes_reserve makes it)");
  if ((com.size() + 63) / 64 != q.voter_words)
    return set_err(ctx, MV_E_INVALID_ARG, "votes: the store was reserved for a committee of another voter word count");
  *n_cert = 0;
  if (n == 0) return MV_OK;
  uint64_t* ctl = q.ctl.as<uint64_t>();
  mvk::VoteCall c{};
  c.buf = d_buf, c.buf_bytes = buf_bytes, c.off = d_off, c.len = d_len, c.n = n, c.flags = flags;
  c.stakes = dev.tab.stakes.as<uint64_t>(), c.n_auth = com.size(), c.quorum = com.quorum_threshold + 1;
  void* wg_n = nullptr;
  mv_status st = carved(ctx, q.blk, [&](Carve& a) {
    c.status = d_status ? d_status : a.take<uint8_t>(n);
    c.key = a.take<uint64_t>(6 * (size_t)n), c.keyoff = a.take<uint64_t>(n);
    c.author = a.take<uint32_t>(n), c.n_st = a.take<uint32_t>(n), c.nreg = a.take<uint32_t>(n);
    c.nev = a.take<uint32_t>(n), c.bflags = a.take<uint32_t>(n);
    c.unk = a.take<uint64_t>(n), c.evbase = a.take<uint64_t>(n), c.brk = a.take<uint8_t>(n);
    wg_n = a.take<uint8_t>(mvk::wg_scan_bytes(n));
  });
  if (st != MV_OK) return st;
  // the words of one call (the cursors VT_CTL_NROWS / _NCELLS are the store's and stay)
  HIPCHK(ctx, hipMemsetAsync(ctl, 0, 8 * mvk::VT_CTL_NROWS, s));
  HIPCHK(ctx, hipMemsetAsync(ctl + mvk::VT_CTL_ERR, 0, 8 * (mvk::VT_CTL_WORDS - mvk::VT_CTL_ERR), s));
  HIPCHK(ctx, mvk::launch_votes_scan(c, ctl, s));
  HIPCHK(ctx, mvk::launch_votes_scan_u32(c.nev, n, c.evbase, ctl + mvk::VT_CTL_NEV, nullptr, wg_n, s));
  const uint64_t* w = nullptr;
  if ((st = read_votes_ctl(ctx, q, s, &w)) != MV_OK) return st;
  const uint64_t nev = w[mvk::VT_CTL_NEV], nshare = w[mvk::VT_CTL_NSHARE], newcells = w[mvk::VT_CTL_NEWCELLS];
  if (nev > kMaxEvents) return set_err(ctx, MV_E_INVALID_ARG, "votes: too many statements in one call");
  // room: rows without an aggregating cell go, with their cells, before the store would grow and
  // whenever they hold half of what is in use
  const uint64_t dead_cells = q.ncells - q.live_cells, dead_rows = q.nrows - q.pending;
  if (q.nrows + nshare > q.cap_rows || q.ncells + newcells > q.cap_cells || (dead_cells && 2 * dead_cells >= q.ncells) ||
      (dead_rows && 2 * dead_rows >= q.nrows)) {
    st = votes_rebuild(ctx, q, grown_to(q.cap_rows, q.pending + nshare), grown_to(q.cap_cells, q.live_cells + newcells), s);
    if (st != MV_OK) return st;
  }
  c.cap_ev = nev;
  st = carved(ctx, q.evs, [&](Carve& a) {
    c.ev = a.take<uint64_t>(3 * (size_t)nev), c.evc = a.take<uint32_t>(nev), c.evx = a.take<uint32_t>(nev);
  });
  if (st != MV_OK) return st;
  const mvk::VoteStore v = view_of(ctx, q);
  // the sharing blocks' references into the table: index.hip's rounds, the retry counter read back
  HIPCHK(ctx, q.item.ensure(8 * (size_t)n));
  if (nshare) {
    const mvk::IndexKeys ks{reinterpret_cast<const uint8_t*>(c.key), c.keyoff, 0, 0};
    for (int round = 0;; round++) {
      HIPCHK(ctx, hipMemsetAsync(ctl + mvk::IX_CTL_RETRY, 0, 8, s));
      HIPCHK(ctx, mvk::launch_index_round(v.t, ks, n, q.item.as<uint64_t>(), 1, round, ctl, s));
      if ((st = read_votes_ctl(ctx, q, s, &w)) != MV_OK) return st;
      if (w[mvk::IX_CTL_RETRY] == 0) break;
      if (round >= kMaxRounds) return set_err(ctx, MV_E_HIP, "votes: an insert did not settle");
    }
    HIPCHK(ctx, mvk::launch_votes_rows(v, c, q.item.as<uint64_t>(), ctl, s));
  }
  HIPCHK(ctx, mvk::launch_votes_emit(v, c, q.item.as<uint64_t>(), ctl, s));
  if ((st = read_votes_ctl(ctx, q, s, &w)) != MV_OK) return st;
  q.nrows = w[mvk::VT_CTL_NROWS], q.ncells = w[mvk::VT_CTL_NCELLS];
  // segments: one ends ahead of every block that registers into a row that was there before it
  std::vector<uint64_t> cut{0};
  if (w[mvk::VT_CTL_NBRK]) {
    std::vector<uint8_t> brk(n);
    std::vector<uint64_t> evbase(n);
    HIPCHK(ctx, hipMemcpyAsync(brk.data(), c.brk, n, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(evbase.data(), c.evbase, 8 * (size_t)n, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    for (uint32_t i = 0; i < n; i++)
      if (brk[i] && evbase[i] > cut.back() && evbase[i] < nev) cut.push_back(evbase[i]);
  }
  cut.push_back(nev);
  uint64_t longest = 0;
  for (size_t k = 0; k + 1 < cut.size(); k++) longest = std::max(longest, cut[k + 1] - cut[k]);
  mvk::VoteSeg g{};
  const uint64_t nrows = q.nrows;
  st = carved(ctx, q.seg, [&](Carve& a) {
    g.row_cnt = a.take<uint32_t>(nrows), g.row_cur = a.take<uint32_t>(nrows), g.row_lb = a.take<uint64_t>(nrows);
    g.list = a.take<uint32_t>(longest), g.sorted = a.take<uint32_t>(longest), g.certbase = a.take<uint64_t>(longest);
    g.wg = a.take<uint8_t>(mvk::wg_scan_bytes(std::max(nrows, longest)));
  });
  if (st != MV_OK) return st;
  for (size_t k = 0; k + 1 < cut.size(); k++)
    HIPCHK(ctx, mvk::launch_votes_segment(v, c, nrows, cut[k], cut[k + 1], g, d_cert, d_cert ? cap_cert : 0, ctl, s));
  HIPCHK(ctx, mvk::launch_votes_blockout(c, d_counts, s));
  HIPCHK(ctx, mvk::launch_votes_stats(v, nrows, ctl, s));
  if ((st = read_votes_ctl(ctx, q, s, &w)) != MV_OK) return st;
  q.pending = w[mvk::VT_CTL_PENDING], q.agg = w[mvk::VT_CTL_AGG], q.live_cells = w[mvk::VT_CTL_LIVECELLS];
  q.certified += w[mvk::VT_CTL_NCERT];
  *n_cert = w[mvk::VT_CTL_NCERT];
  return MV_OK;
}

bool votes_args_ok(const void* buf, const void* off, const void* len, uint32_t n, uint32_t flags, const void* status,
                   const void* counts, const void* cert, uint64_t cap, const void* n_cert) {
  if ((flags & ~MV_VOTES_REGISTER_ONLY) || !n_cert || (cap && !cert)) return false;
  return n == 0 || (buf && off && len && status && counts);
}

}  // namespace

extern "C" {

mv_status mv_votes_reserve(mv_ctx* ctx, uint64_t blocks, uint64_t cells) {
  if (!ctx) return MV_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!committee_ready(ctx)) return set_err(ctx, MV_E_NO_COMMITTEE, "mv_votes_reserve needs mv_set_committee");
  Device& dev = ctx->devs[0];
  Votes& q = dev.votes;
  HIPCHK(ctx, hipSetDevice(dev.id));
  const uint32_t words = (ctx->committee.size() + 63) / 64;
  if (q.on && q.voter_words != words)
    return set_err(ctx, MV_E_INVALID_ARG, "votes: the store holds voter sets of another word count (mv_votes_clear first)");
  if (q.on && blocks <= q.cap_rows && cells <= q.cap_cells) return MV_OK;
  q.voter_words = words;
  // (growing keeps the rows that are pending; the others could not be told from absent ones)
  return votes_rebuild(ctx, q, std::max(blocks, q.cap_rows), std::max(cells, q.cap_cells), dev.stream);
}

mv_status mv_votes_clear(mv_ctx* ctx) {
  if (!ctx) return MV_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device& dev = ctx->devs[0];
  HIPCHK(ctx, hipSetDevice(dev.id));
  HIPCHK(ctx, hipStreamSynchronize(dev.stream));
  mvr::reset(dev.votes);
  return MV_OK;
}

mv_status mv_votes_stats(mv_ctx* ctx, uint64_t* out) {
  if (!ctx || !out) return set_err(ctx, MV_E_INVALID_ARG, "bad votes stats args");
  std::lock_guard<std::mutex> lk(ctx->mu);
  const Votes& q = ctx->devs[0].votes;
  out[0] = q.pending, out[1] = q.agg, out[2] = q.ncells, out[3] = q.certified;
  return MV_OK;
}

mv_status mv_aggregate_votes(mv_ctx* ctx, const uint8_t* buf, const uint64_t* off, const uint64_t* len, uint32_t n,
                             uint32_t flags, uint8_t* blk_status, uint64_t* blk_counts, uint64_t* certified,
                             uint64_t cap_certified, uint64_t* n_certified) {
  if (!ctx || !votes_args_ok(buf, off, len, n, flags, blk_status, blk_counts, certified, cap_certified, n_certified))
    return set_err(ctx, MV_E_INVALID_ARG, "bad votes args");
  uint64_t lo = ~0ull, hi = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (off[i] + len[i] < off[i]) return set_err(ctx, MV_E_INVALID_ARG, "votes: a block's span overflows");
    lo = std::min(lo, off[i]);
    hi = std::max(hi, off[i] + len[i]);
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!committee_ready(ctx)) return set_err(ctx, MV_E_NO_COMMITTEE, "mv_aggregate_votes needs mv_set_committee");
  Device& dev = ctx->devs[0];
  Votes& q = dev.votes;
  hipStream_t s = dev.stream;
  HIPCHK(ctx, hipSetDevice(dev.id));
  if (n == 0) return votes_run(ctx, dev, nullptr, 0, nullptr, nullptr, 0, flags, nullptr, nullptr, nullptr, 0, n_certified, s);
  const uint64_t span = hi - lo;
  HIPCHK(ctx, q.in.ensure(span + 16));
  HIPCHK(ctx, q.ol.ensure(16 * (size_t)n));
  uint8_t* d_st = nullptr;
  uint64_t *d_counts = nullptr, *d_cert = nullptr;
  mv_status st = carved(ctx, q.out, [&](Carve& a) {
    d_st = a.take<uint8_t>(n), d_counts = a.take<uint64_t>(4 * (size_t)n), d_cert = a.take<uint64_t>(8 * (size_t)cap_certified);
  });
  if (st != MV_OK) return st;
  std::vector<uint64_t> ol(2 * (size_t)n);
  for (uint32_t i = 0; i < n; i++) {
    ol[i] = off[i] - lo;
    ol[(size_t)n + i] = len[i];
  }
  uint8_t* d_in = q.in.as<uint8_t>();
  if (span) HIPCHK(ctx, hipMemcpyAsync(d_in, buf + lo, span, hipMemcpyHostToDevice, s));
  HIPCHK(ctx, hipMemsetAsync(d_in + span, 0, 16, s));
  HIPCHK(ctx, hipMemcpyAsync(q.ol.p, ol.data(), 16 * (size_t)n, hipMemcpyHostToDevice, s));
  HIPCHK(ctx, hipStreamSynchronize(s));  // (pageable sources)
  st = votes_run(ctx, dev, d_in, span, q.ol.as<uint64_t>(), q.ol.as<uint64_t>() + n, n, flags, d_st, d_counts,
                 cap_certified ? d_cert : nullptr, cap_certified, n_certified, s);
  if (st != MV_OK) return st;
  HIPCHK(ctx, hipMemcpyAsync(blk_status, d_st, n, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipMemcpyAsync(blk_counts, d_counts, 32 * (size_t)n, hipMemcpyDeviceToHost, s));
  const uint64_t rows = std::min(*n_certified, cap_certified);
  if (rows) HIPCHK(ctx, hipMemcpyAsync(certified, d_cert, 64 * (size_t)rows, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  return MV_OK;
}

mv_status mv_dev_aggregate_votes(mv_ctx* ctx, int device, const uint8_t* d_buf, uint64_t buf_bytes,
                                 const uint64_t* d_off, const uint64_t* d_len, uint32_t n, uint32_t flags,
                                 uint8_t* d_blk_status, uint64_t* d_blk_counts, uint64_t* d_certified,
                                 uint64_t cap_certified, uint64_t* n_certified, void* stream) {
  if (!ctx || !votes_args_ok(d_buf, d_off, d_len, n, flags, d_blk_status, d_blk_counts, d_certified, cap_certified,
                             n_certified))
    return set_err(ctx, MV_E_INVALID_ARG, "bad votes args");
  if (((uintptr_t)d_buf | (uintptr_t)d_off | (uintptr_t)d_len | (uintptr_t)d_blk_counts | (uintptr_t)d_certified) & 7)
    return set_err(ctx, MV_E_INVALID_ARG, "votes: misaligned device pointer");
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!committee_ready(ctx)) return set_err(ctx, MV_E_NO_COMMITTEE, "mv_dev_aggregate_votes needs mv_set_committee");
  Device* dev = find_dev(ctx, device);
  if (!dev || dev != &ctx->devs[0]) return set_err(ctx, MV_E_NO_DEVICE, "votes run on the context's first device");
  HIPCHK(ctx, hipSetDevice(dev->id));
  hipStream_t s = stream ? (hipStream_t)stream : (hipStream_t)dev->stream;
  return votes_run(ctx, *dev, d_buf, buf_bytes, d_off, d_len, n, flags, d_blk_status, d_blk_counts,
                   cap_certified ? d_certified : nullptr, cap_certified, n_certified, s);
}

}  // extern "C"
