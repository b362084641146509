// The byte walkers of the library under the host sanitizers (tests/test_walk_sanitized.py
// builds and runs this with -fsanitize=address,undefined). It includes the product headers as they
// ship -- bincode_walk.h, ingest_lane.h, votes_walk.h, frame_walk.h, wal_entry.h, block_ref.h -- and
// links block_codec.cpp; it restates no parsing rule. Every input is a separate heap allocation
// of exactly the size the walker's contract grants, so that a read or write outside the contract
// lands in a redzone:
//
//   block_walk      the block at offset d = 0..7 of an 8-aligned allocation of round_up(d + L, 8) + 8
//   ingest_lane     the input 8-aligned and readable 16 bytes past the block (d + L + 16); the stage
//                   exactly [round_up(d, 8), d + L); seen 16 zeroed words; one element per output
//   votes walker    as block_walk
//   frames          exactly the stream's bytes (frame_walk.h loads with memcpy)
//   parse_block     exactly L bytes; pre exactly cap bytes for cap = |P|, |P| - 1, 0
//
//   walk_san blocks   CORPUS COMMITTEE   every record at d = 0..7
//   walk_san prefixes CORPUS COMMITTEE   every prefix of every record at d = 0..7
//   walk_san frames   CORPUS             every record as one stream
//   walk_san frame-prefixes CORPUS       every prefix of every record as one stream
//   walk_san sweep    FILE               lines "w tag pos plen size" (wal_entry.h) and "r len k" (block_ref.h)
//
// A corpus is records of a u32 length and that many bytes; a committee file is u32 n_auth, u64
// epoch, u64 quorum threshold and n_auth u64 stakes. One line per case on stdout, "d=*" when the
// eight alignments gave the same line.
#include <hip/hip_runtime.h>

#include <inttypes.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#define MV_DEV inline
#define MV_VT_DEV inline
#include "../mysticeti_amd/csrc/bincode_walk.h"
#include "../mysticeti_amd/csrc/block_codec.h"
#include "../mysticeti_amd/csrc/block_ref.h"
#include "../mysticeti_amd/csrc/block_verdict.h"
#include "../mysticeti_amd/csrc/frame_walk.h"
#include "../mysticeti_amd/csrc/ingest_lane.h"
#include "../mysticeti_amd/csrc/votes_walk.h"
#include "../mysticeti_amd/csrc/wal_entry.h"

namespace {

#ifndef WALK_SAN_PAD
#define WALK_SAN_PAD 8  // bincode_walk.h: "an 8-byte aligned buffer padded by 8 bytes"
#endif

std::string fmt(const char* f, ...) __attribute__((format(printf, 1, 2)));
std::string fmt(const char* f, ...) {
  char b[256];
  va_list ap;
  va_start(ap, f);
  vsnprintf(b, sizeof b, f, ap);
  va_end(ap);
  return b;
}
std::string hex(const uint8_t* p, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string s(2 * n, '0');
  for (size_t i = 0; i < n; i++) s[2 * i] = d[p[i] >> 4], s[2 * i + 1] = d[p[i] & 15];
  return s;
}

// An allocation of exactly n bytes (malloc: 16-byte aligned, redzones on both sides).
struct Heap {
  uint8_t* p;
  explicit Heap(size_t n, int fill = 0) : p(static_cast<uint8_t*>(malloc(n ? n : 1))) {
    if (!p) abort();
    if (!n) {  // nothing may be touched: one byte was asked for only to get a pointer
      free(p);
      p = static_cast<uint8_t*>(malloc(0));
    }
    if (n) memset(p, fill, n);
  }
  ~Heap() { free(p); }
  Heap(const Heap&) = delete;
  Heap& operator=(const Heap&) = delete;
};

uint64_t round_up8(uint64_t x) { return (x + 7) & ~7ull; }

std::vector<std::vector<uint8_t>> read_corpus(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    perror(path);
    exit(2);
  }
  std::vector<std::vector<uint8_t>> out;
  uint32_t n;
  while (fread(&n, 4, 1, f) == 1) {
    std::vector<uint8_t> b(n);
    if (n && fread(b.data(), 1, n, f) != n) {
      fprintf(stderr, "%s: short record\n", path);
      exit(2);
    }
    out.push_back(std::move(b));
  }
  fclose(f);
  return out;
}

struct CommitteeFile {
  mvh::Committee host;
  std::vector<uint64_t> stakes;
  mv::CommitteeView view;
};
void read_committee(const char* path, CommitteeFile& c) {
  FILE* f = fopen(path, "rb");
  uint32_t n = 0;
  uint64_t epoch = 0, thr = 0;
  if (!f || fread(&n, 4, 1, f) != 1 || fread(&epoch, 8, 1, f) != 1 || fread(&thr, 8, 1, f) != 1) {
    fprintf(stderr, "%s: no committee\n", path);
    exit(2);
  }
  c.stakes.resize(n);
  if (n && fread(c.stakes.data(), 8, n, f) != n) exit(2);
  fclose(f);
  c.host.stakes = c.stakes;
  c.host.pks.assign(32 * (size_t)n, 0);
  c.host.epoch = epoch;
  c.host.quorum_threshold = thr;
  c.view = mv::CommitteeView{c.stakes.data(), n, epoch, thr};
}

// ---------------------------------------------------------------- block_walk
struct CountVis {
  uint64_t own_a = 0, own_r = 0, n_inc = 0, n_vr = 0, epoch = 0, sig_pos = 0;
  void own(uint64_t a, uint64_t r, const uint8_t*) { own_a = a, own_r = r; }
  void include(uint64_t, uint64_t, const uint8_t*) { n_inc++; }
  void vote_range(uint64_t, uint64_t) { n_vr++; }
  void meta(uint64_t ep, uint64_t sp) { epoch = ep, sig_pos = sp; }
};
struct VecGather : mv::ByteGather<VecGather> {
  std::vector<uint8_t> out;
  void word(uint64_t w) {
    uint8_t b[8];
    memcpy(b, &w, 8);
    out.insert(out.end(), b, b + 8);
  }
  void finish() {  // the bytes pending in acc
    for (uint32_t k = 0; k < nb; k++) out.push_back(static_cast<uint8_t>(acc >> (8 * k)));
  }
};

// The block at offset d of its allocation; n: the allocation's size.
struct Placed {
  Heap h;
  const uint8_t* p;
  Placed(const uint8_t* b, uint64_t L, uint32_t d, uint64_t n) : h(n, 0xA5), p(h.p + d) {
    if (L) memcpy(h.p + d, b, L);
  }
};

std::string run_walk(const uint8_t* b, uint64_t L, uint32_t d, std::vector<uint8_t>& P) {
  std::string s;
  {
    Placed in(b, L, d, round_up8(d + L) + WALK_SAN_PAD);
    mv::BcReader r{in.p, L, 0, true};
    mv::NoSink sink;
    CountVis v;
    const bool ok = mv::block_walk(r, sink, v);
    s += ok ? fmt("walk=1 own=%" PRIu64 ",%" PRIu64 " n_inc=%" PRIu64 " n_vr=%" PRIu64 " epoch=%" PRIu64 " sig_pos=%" PRIu64,
                  v.own_a, v.own_r, v.n_inc, v.n_vr, v.epoch, v.sig_pos)
            : std::string("walk=0");
  }
  {
    Placed in(b, L, d, round_up8(d + L) + WALK_SAN_PAD);
    mv::BcReader r{in.p, L, 0, true};
    VecGather g;
    CountVis v;
    const bool ok = mv::block_walk(r, g, v);
    g.finish();
    if (ok && g.out.size() != g.len) s += " gather-length-differs";
    s += ok ? fmt(" gather=1 plen=%" PRIu64, g.len) : std::string(" gather=0");
    P = ok ? g.out : std::vector<uint8_t>();
  }
  return s;
}

// ---------------------------------------------------------------- ingest_lane
std::string run_lane(const uint8_t* b, uint64_t L, uint32_t d, const mv::CommitteeView& cv, const std::vector<uint8_t>& P) {
  const uint64_t o = d, so = round_up8(o);
  Placed in(b, L, d, d + L + 16);  // "readable 16 bytes past every block"
  const uint64_t stage_bytes = o + L > so ? o + L - so : 0;
  Heap stage(stage_bytes, 0x5A);  // exactly [round_up(o, 8), o + L): the block's own span
  Heap seen(16 * sizeof(uint32_t)), pre_off(8), pre_len(8), sig(64), key_idx(4), facts(4), claimed(32);
  // (the stage's base is so bytes before its allocation; with o < 8 that is at most 8)
  mv::IngestOut io{stage.p - so,
                   reinterpret_cast<uint64_t*>(pre_off.p),
                   reinterpret_cast<uint64_t*>(pre_len.p),
                   sig.p,
                   reinterpret_cast<uint32_t*>(key_idx.p),
                   reinterpret_cast<uint32_t*>(facts.p),
                   claimed.p};
  mv::ingest_lane(in.h.p, o, L, 0, cv, io, reinterpret_cast<uint32_t*>(seen.p), 1);
  uint64_t plen, poff;
  uint32_t f, key;
  memcpy(&plen, pre_len.p, 8);
  memcpy(&poff, pre_off.p, 8);
  memcpy(&f, facts.p, 4);
  memcpy(&key, key_idx.p, 4);
  if (plen == 0) return fmt(" lane pre_len=0 facts=%u", f);
  std::string s = fmt(" lane pre_len=%" PRIu64 " pre_off=%" PRIu64 " facts=%u key=%u", plen, poff - so, f, key);
  // P || sig || 8 zero bytes at the stage; P is printed once, by the gather
  const bool fits = plen + 72 <= stage_bytes;
  const bool same = fits && plen == P.size() && memcmp(stage.p, P.data(), plen) == 0;
  s += same ? " P=gather" : " P=" + (fits ? hex(stage.p, plen) : std::string("outside"));
  if (fits) s += " sig=" + hex(stage.p + plen, 64) + " zero=" + hex(stage.p + plen + 64, 8);
  s += " sig_out=" + hex(sig.p, 64) + " claimed=" + hex(claimed.p, 32);
  return s;
}

// ---------------------------------------------------------------- the votes walker
struct PrintF {
  std::string s;
  static std::string key(const uint64_t* k) {
    return fmt("%" PRIu64 ",%" PRIu64 ",%016" PRIx64 "%016" PRIx64 "%016" PRIx64 "%016" PRIx64, k[0], k[1], k[2], k[3], k[4], k[5]);
  }
  void share(uint64_t k) { s += fmt(" s%" PRIu64, k); }
  void vote(uint64_t k, const uint64_t* key_, uint64_t lo) { s += fmt(" v%" PRIu64 ":", k) + key(key_) + fmt(":%" PRIu64, lo); }
  void reject(uint64_t k) { s += fmt(" j%" PRIu64, k); }
  void range(uint64_t k, const uint64_t* key_, uint64_t s0, uint64_t s1) {
    s += fmt(" r%" PRIu64 ":", k) + key(key_) + fmt(":%" PRIu64 ":%" PRIu64, s0, s1);
  }
};
// k_vt_scan's two walks: block_walk, then a second reader at INC_OFF + 56 * n_inc
std::string run_votes(const uint8_t* b, uint64_t L, uint32_t d) {
  Placed in(b, L, d, round_up8(d + L) + WALK_SAN_PAD);
  mv::BcReader r{in.p, L, 0, true};
  mv::NoSink sink;
  mv::ix::IncCount vis;
  if (!mv::block_walk(r, sink, vis)) return " votes=0";
  mv::BcReader q{r.p, r.len, mv::br::INC_OFF + mv::br::REF_BYTES * vis.n_inc, true};
  PrintF f;
  uint64_t count = 0;
  if (!mv::ix::walk_statements(q, f, &count)) return " votes=walks-disagree";
  uint64_t key[6];
  mv::ix::ref_key(mv::peek8(r.p), mv::peek8(r.p + 8), r.p + 24, key);
  return fmt(" votes=1 n_st=%" PRIu64 " own=", count) + PrintF::key(key) + f.s;
}

// ---------------------------------------------------------------- parse_block (the host-parse path)
std::string run_codec(const uint8_t* b, uint64_t L, const mvh::Committee& c, const std::vector<uint8_t>& P) {
  mvh::BlockFacts f;
  size_t plen;
  {
    Heap in(L);
    if (L) memcpy(in.p, b, L);
    if (!mvh::parse_block(in.p, L, &c, nullptr, 0, f)) return " codec=0";
    plen = f.preimage_len;
  }
  std::string s = fmt(" codec=1 plen=%zu author=%" PRIu64 " round=%" PRIu64 " epoch=%" PRIu64 " inc=%u vr=%u quorum=%d", plen,
                      f.author, f.round, f.epoch, f.include_error, f.vote_range_error, (int)f.threshold_ok);
  const size_t caps[3] = {plen, plen ? plen - 1 : 0, 0};
  for (int k = 0; k < 3; k++) {
    Heap in(L), pre(caps[k], 0x33);
    if (L) memcpy(in.p, b, L);
    mvh::BlockFacts g;
    const bool ok = mvh::parse_block(in.p, L, &c, pre.p, caps[k], g);
    if (!ok || g.preimage_len != plen) s += fmt(" cap%d-differs", k);
    if (k == 0) {
      const bool same = plen == P.size() && memcmp(pre.p, P.data(), plen) == 0;
      s += same ? " P=gather" : " P=" + hex(pre.p, plen);
      s += " sig=" + hex(g.signature, 64) + " claimed=" + hex(g.claimed_digest, 32);
    }
  }
  return s;
}

void one_block(size_t idx, const uint8_t* b, uint64_t L, const CommitteeFile& c) {
  std::vector<std::string> lines;
  std::vector<uint8_t> P0;
  bool same = true;
  for (uint32_t d = 0; d < 8; d++) {
    std::vector<uint8_t> P;
    std::string s = run_walk(b, L, d, P);
    s += run_lane(b, L, d, c.view, P);
    s += run_votes(b, L, d);
    if (d == 0) P0 = P;
    if (P != P0) s += " gather-P-differs";
    same = same && s == (d ? lines[0] : s);
    lines.push_back(s);
  }
  // (the host codec reads with memcpy: no alignment to vary)
  const std::string tail = run_codec(b, L, c.host, P0) + " P=" + hex(P0.data(), P0.size());
  if (same) {
    printf("B %zu d=* %s%s\n", idx, lines[0].c_str(), tail.c_str());
  } else {
    for (uint32_t d = 0; d < 8; d++) printf("B %zu d=%u %s%s\n", idx, d, lines[d].c_str(), tail.c_str());
  }
}

// ---------------------------------------------------------------- frames
struct PrintSink {
  std::string* s;
  void operator()(uint32_t k, uint64_t off, uint64_t len) const { *s += fmt(" %u:%" PRIu64 ":%" PRIu64, k, off, len); }
};
// k_frame_walk's steps over the whole stream, k_msg_walk's classify of every frame listed (once
// with NoSink, once with a sink, as its two launches do), k_stream_cut's consumed
void one_stream(size_t idx, const uint8_t* b, uint64_t n) {
  namespace fr = mv::fr;
  Heap in(n);
  if (n) memcpy(in.p, b, n);
  uint64_t p = 0, consumed = 0;
  bool cut = false;
  std::string rows;
  for (;;) {
    uint64_t size;
    const fr::Step st = fr::frame_at(in.p, p, n, size);
    if (st == fr::STEP_END) break;
    if (st == fr::STEP_PING) {
      p += 4 + fr::PING_REST;
      continue;
    }
    fr::Msg m{fr::NO_TAG, MV_MSG_BAD_SIZE, 0};
    std::string blocks;
    if (st == fr::STEP_FRAME) {
      m = fr::classify(in.p, p + 4, size, fr::NoSink());
      const fr::Msg m2 = fr::classify(in.p, p + 4, size, PrintSink{&blocks});
      if (m2.tag != m.tag || m2.status != m.status || m2.nblk != m.nblk) blocks += " launches-differ";
    }
    rows += fmt(" | off=%" PRIu64 " size=%" PRIu64 " tag=%u status=%u nblk=%u", p, size, m.tag, m.status, m.nblk) + blocks;
    if (m.status != MV_MSG_OK && !cut) {
      cut = true;
      consumed = st == fr::STEP_BAD_SIZE ? p : p + 4 + size;
    }
    if (st == fr::STEP_BAD_SIZE) break;
    p += 4 + size;
  }
  if (!cut) consumed = p;
  printf("F %zu consumed=%" PRIu64 "%s\n", idx, consumed, rows.c_str());
}

// ---------------------------------------------------------------- wal_entry.h, block_ref.h
int sweep(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) {
    perror(path);
    return 2;
  }
  char kind;
  while (fscanf(f, " %c", &kind) == 1) {
    if (kind == 'w') {
      uint32_t tag;
      uint64_t pos, plen, size;
      if (fscanf(f, "%u %" SCNu64 " %" SCNu64 " %" SCNu64, &tag, &pos, &plen, &size) != 4) return 2;
      const mv::we::Entry e = mv::we::classify(tag, pos, plen, size);
      printf("w %u %" PRIu64 " %" PRIu64 " %" PRIu64 " -> %u %d %" PRIu64 " %" PRIu64 "\n", tag, pos, plen, size, e.status,
             (int)e.block, e.off, e.len);
    } else if (kind == 'r') {
      uint64_t len, k;
      if (fscanf(f, "%" SCNu64 " %" SCNu64, &len, &k) != 2) return 2;
      namespace br = mv::br;
      const bool cnt = br::inc_count_readable(len);
      // (includes_inside asks for len >= INC_OFF)
      printf("r %" PRIu64 " %" PRIu64 " -> %d %d %d %" PRIu64 "\n", len, k, (int)br::own_ref_readable(len), (int)cnt,
             cnt ? (int)br::includes_inside(len, k) : -1, br::include_off(k));
    } else {
      return 2;
    }
  }
  fclose(f);
  printf("k");
  for (int k = 0; k < mv::br::KEY_WORDS; k++) printf(" %" PRIu64, mv::br::key_word_off(k));
  printf("\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "sweep" && argc == 3) return sweep(argv[2]);
  if ((mode == "blocks" || mode == "prefixes") && argc == 4) {
    CommitteeFile c;
    read_committee(argv[3], c);
    size_t idx = 0;
    for (const auto& b : read_corpus(argv[2])) {
      if (mode == "blocks") {
        one_block(idx++, b.data(), b.size(), c);
      } else {
        for (size_t k = 0; k <= b.size(); k++) one_block(idx++, b.data(), k, c);
      }
    }
    return 0;
  }
  if ((mode == "frames" || mode == "frame-prefixes") && argc == 3) {
    size_t idx = 0;
    for (const auto& b : read_corpus(argv[2])) {
      if (mode == "frames") {
        one_stream(idx++, b.data(), b.size());
      } else {
        for (size_t k = 0; k <= b.size(); k++) one_stream(idx++, b.data(), k);
      }
    }
    return 0;
  }
  fprintf(stderr, "usage: walk_san blocks|prefixes CORPUS COMMITTEE | frames|frame-prefixes CORPUS | sweep FILE\n");
  return 2;
}
