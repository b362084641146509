// The layout rules of mv_wal_write under the host sanitizers (tests/test_wal_write_sanitized.py
// builds and runs this with -fsanitize=address,undefined; tests/test_wal_write_cases.py builds it
// plain and holds it to mv_wal_layout). It includes wal_layout.h as it ships and restates no rule:
// the checks (entry_ok), the exclusive sums, the map crossings (cross_step, with a binary search
// where the kernel's wave probes 64 places a round), the step table (shift_at), the spans of gap,
// header, next_entry and payload (span_of) and the header words (header_words) are the header's,
// driven in the order wal_write.hip's kernels drive them. The bytes are then placed span by span;
// the crc is a bitwise CRC-32 of the placed body, so it shares nothing with the device's tables.
//
// Every array is a separate heap allocation of exactly the size the contract grants, so a read or a
// write outside the contract lands in a redzone: the rows 32 n bytes, the payload buffer exactly
// buf_bytes, the positions 8 n, the output exactly cap bytes.
//
//   wal_write_san IN OUT
// IN:  u64 cases; per case u64 n, buf_bytes, start, map_bits, cap; the rows; the payload bytes.
// OUT: per case u64 refused (0 / 1), end_pos, crossings; n positions; the cap output bytes (0xA5
//      where nothing was written).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../mysticeti_amd/csrc/wal_layout.h"

namespace {

using namespace mv::wl;

// An allocation of exactly n bytes (malloc: 16-byte aligned, redzones on both sides).
template <class T>
struct Heap {
  T* p;
  explicit Heap(size_t bytes, int fill = 0) : p(static_cast<T*>(malloc(bytes ? bytes : 1))) {
    if (!p) abort();
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

struct Sums {
  const uint64_t* s;  // n + 1 entries
  uint64_t operator()(uint64_t i) const { return s[i]; }
};
struct Find {  // the first i in [lo, n) with S(i + 1) > T, or n
  const uint64_t* s;
  uint64_t n;
  uint64_t operator()(uint64_t lo, uint64_t T) const {
    uint64_t hi = n;
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (s[mid + 1] > T) hi = mid;
      else lo = mid + 1;
    }
    return lo;
  }
};

uint32_t crc32_bitwise(const uint8_t* p, uint64_t n) {
  uint32_t c = 0xffffffffu;
  for (uint64_t i = 0; i < n; i++) {
    c ^= p[i];
    for (int k = 0; k < 8; k++) c = (c & 1) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
  }
  return ~c;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  FILE* g = fopen(argv[2], "wb");
  if (!f || !g) return 2;
  uint64_t cases = 0;
  get(f, &cases, 8);
  for (uint64_t t = 0; t < cases; t++) {
    uint64_t hd[5];
    get(f, hd, sizeof hd);
    const uint64_t n = hd[0], bytes = hd[1], start = hd[2], cap = hd[4];
    const uint32_t bits = (uint32_t)hd[3];
    Heap<uint64_t> rows(8 * ENTRY_WORDS * n), pos(8 * n), sums(8 * (n + 1)), cfirst(8 * n), cshift(8 * n);
    Heap<uint8_t> buf(bytes, 0xEE), out(cap, 0xA5);
    get(f, rows.p, 8 * ENTRY_WORDS * n);
    get(f, buf.p, bytes);

    // the checks and the exclusive sums (LenScan)
    uint64_t refused = 0;
    sums.p[0] = 0;
    for (uint64_t i = 0; i < n; i++) {
      const uint64_t* e = rows.p + ENTRY_WORDS * i;
      const bool ok = entry_ok(e[0], e[1], e[2], bytes, bits);
      refused += !ok;
      sums.p[i + 1] = sums.p[i] + HEADER + (ok ? body_len(e[0], e[2]) : 0);
    }
    uint64_t end = start, nc = 0;
    if (!refused) {
      // the crossings (k_ww_cross), then the positions (k_ww_pos)
      uint64_t cur = 0, shift = 0, gap = 0;
      while (cross_step(n, start, bits, Sums{sums.p}, Find{sums.p, n}, &cur, &shift, &gap)) {
        if (!gap) continue;
        if (nc >= n) return 3;
        cfirst.p[nc] = cur, cshift.p[nc] = shift;
        nc++;
      }
      end = start + shift + sums.p[n];
      for (uint64_t i = 0; i < n; i++) pos.p[i] = start + shift_at(cfirst.p, cshift.p, nc, i) + sums.p[i];
      // the bytes (k_ww_emit), if they fit
      uint64_t prev_end = 0;
      for (uint64_t i = 0; end - start <= cap && i < n; i++) {
        const uint64_t* e = rows.p + ENTRY_WORDS * i;
        const Span sp = span_of(prev_end, pos.p[i] - start, e[0], e[2]);
        if (sp.gap0 > sp.at || sp.end > cap) return 3;
        memset(out.p + sp.gap0, 0, sp.at - sp.gap0);
        uint8_t* body = out.p + sp.at + HEADER;
        if ((uint32_t)e[0] == TAG_OWN) memcpy(body, &e[3], OWN_HEAD);
        memcpy(out.p + sp.body, buf.p + e[1], e[2]);
        uint64_t hw[2];
        header_words(crc32_bitwise(body, sp.end - sp.at - HEADER), e[0], e[2], hw);
        memcpy(out.p + sp.at, hw, HEADER);
        prev_end = sp.end;
      }
    }
    const uint64_t res[3] = {refused ? 1u : 0u, end, nc};
    fwrite(res, 8, 3, g);
    fwrite(pos.p, 8, n, g);
    if (cap) fwrite(out.p, 1, cap, g);
  }
  fclose(f);
  return fclose(g) == 0 ? 0 : 2;
}
