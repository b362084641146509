// The rules of mv_encode_blocks under the host sanitizers (tests/test_encode_sanitized.py builds and
// runs this with -fsanitize=address,undefined). It includes encode_walk.h as it ships and restates no
// rule: the payload check, the size pass and the piece table are the header's, driven the way
// encode.hip's kernels drive them -- a check per payload, the scan of the bodies, a size per block,
// the scan of the padded lengths, then every destination word of every OK block from
// BlockSrc::dest_word, stored as one aligned 8-byte word.
//
// Every array is a separate heap allocation of exactly the size the contract grants, so a read or a
// write outside the contract lands in a redzone: heads 80 n bytes, include rows 48 m, the payload
// list 8 p each, the payload buffer its size rounded up to 8 plus 8 (payloads are read as whole
// aligned words), the output exactly cap bytes.
//
//   encode_san IN OUT
// IN:  u64 n, m, p, payload_bytes, cap; heads; include rows; payload offsets; payload lengths; the
//      payload bytes.
// OUT: u64 total, failed checks; per block u64 status, offset, length; the cap output bytes (0xA5
//      where nothing was written).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#define MV_DEV inline
#define MV_VT_DEV inline
#include "../mysticeti_amd/csrc/encode_walk.h"

namespace {

using namespace mv::en;

// An allocation of exactly n bytes (malloc: 16-byte aligned, redzones on both sides).
template <class T>
struct Heap {
  T* p;
  explicit Heap(size_t bytes, int fill = 0) : p(static_cast<T*>(malloc(bytes))) {
    if (bytes && !p) abort();
    if (bytes) memset(p, fill, bytes);
  }
  ~Heap() { free(p); }
  Heap(const Heap&) = delete;
  Heap& operator=(const Heap&) = delete;
};

void get(FILE* f, void* dst, size_t bytes) {
  if (bytes && fread(dst, 1, bytes, f) != bytes) {
    fprintf(stderr, "short input\n");
    exit(2);
  }
}

struct VecPre {
  const uint64_t* s;
  uint64_t operator()(uint64_t j) const { return s[j]; }
};
struct ErrCount {
  uint64_t* n;
  void operator()() const { ++*n; }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t hd[5];
  get(f, hd, sizeof hd);
  const uint64_t n = hd[0], m = hd[1], p = hd[2], bytes = hd[3], cap = hd[4];
  Heap<uint64_t> heads(80 * n), includes(48 * m), poff(8 * p), plen(8 * p);
  Heap<uint8_t> pbuf(round_up8(bytes) + 8, 0xEE), out(cap, 0xA5);
  get(f, heads.p, 80 * n);
  get(f, includes.p, 48 * m);
  get(f, poff.p, 8 * p);
  get(f, plen.p, 8 * p);
  get(f, pbuf.p, bytes);
  fclose(f);

  // k_en_check and the scan of the bodies
  Heap<uint8_t> pay_ok(p);
  Heap<uint64_t> pay_count(8 * p), pay_body(8 * p), pre(8 * (p + 1));
  pre.p[0] = 0;
  for (uint64_t j = 0; j < p; j++) {
    pay_ok.p[j] = check_payload(pbuf.p, bytes, poff.p[j], plen.p[j], &pay_count.p[j], &pay_body.p[j]);
    pre.p[j + 1] = pre.p[j] + pay_body.p[j];
  }
  // k_en_size and the scan of the padded lengths
  std::vector<uint64_t> status(n), off(n), len(n), count(n);
  uint64_t total = 0, errors = 0;
  for (uint64_t i = 0; i < n; i++) {
    status[i] = size_block(heads.p + HEAD_WORDS * i, m, p, pay_ok.p, pay_body.p, pay_count.p, &len[i], &count[i]);
    off[i] = total;
    total += round_up8(len[i]);
  }
  // k_en_write
  const Inputs in{heads.p, includes.p, m, pbuf.p, bytes, poff.p, plen.p, p};
  for (uint64_t i = 0; total <= cap && i < n; i++) {
    if (status[i] != MV_ENCODE_OK) continue;
    Shape sh;
    if (!span_ok(off[i], len[i], cap) || !shape_of(in, i, pre.p, count[i], len[i], &sh)) {
      errors++;
      continue;
    }
    Heap<uint64_t> tile(8 * (sh.np + 1));  // the block's boundaries, as the kernel's LDS holds them
    for (uint64_t j = 0; j <= sh.np; j++) tile.p[j] = pre.p[sh.pay0 + j] - pre.p[sh.pay0];
    const BlockSrc<VecPre, ErrCount> src{in, i, sh, VecPre{tile.p}, ErrCount{&errors}};
    uint64_t* dst = reinterpret_cast<uint64_t*>(out.p + off[i]);
    for (uint64_t w = 0; w < round_up8(len[i]) / 8; w++) dst[w] = src.dest_word(8 * w);
  }

  FILE* g = fopen(argv[2], "wb");
  if (!g) return 2;
  fwrite(&total, 8, 1, g);
  fwrite(&errors, 8, 1, g);
  for (uint64_t i = 0; i < n; i++) {
    const uint64_t row[3] = {status[i], off[i], len[i]};
    fwrite(row, 8, 3, g);
  }
  if (cap) fwrite(out.p, 1, cap, g);
  return fclose(g) == 0 ? 0 : 2;
}
