// The wave-wide crc32 (CRC-32/ISO-HDLC, crc32fast::hash) that wal.hip's replay check and
// wal_write.hip's writer share: the LDS tables, the row fold and the lane tree. The scheme is
// described at the top of wal.hip. The build has no relocatable device code: everything here is
// inline or a template.
//
// crc_raw_wave takes a sink: a functor that is handed every word the fold loads, with the word's
// byte offset from the string's first byte (rows 0 and 1 may start before it: q < 0). The replay
// check passes none; the writer stores the words it is handed, so that its payload is read once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef MV_DEV
#define MV_DEV __device__ __forceinline__
#endif

namespace mv {
namespace wal {

#ifndef MV_WAL_REP
#define MV_WAL_REP 8
#endif
constexpr int REP = MV_WAL_REP;              // copies of A256 (bank spread)
constexpr int A_WORDS = 4 * 256 * REP;       // [byte t][value e][copy c]
constexpr int S_LEVELS = 6;                  // shifts by 4 << k bytes, k < 6
constexpr int S_WORDS = S_LEVELS * 4 * 256;  // [k][byte t][value e]
constexpr int T_WORDS = 256;                 // the byte table (1-byte shift), global only
constexpr uint32_t PREFIX = 0x9226f562u;     // crc_raw(0, PREFIX as 4 LE bytes) = 0xFFFFFFFF
constexpr int WG = 1024;                     // threads per crc workgroup
#ifndef MV_WAL_ROWS
#define MV_WAL_ROWS 8  // rows in flight per batch; 8 fits the 64-VGPR budget of 8 waves per SIMD
#endif
constexpr int WAL_ROWS = MV_WAL_ROWS;
#ifndef MV_WAL_WPE
#define MV_WAL_WPE 8  // waves per SIMD the register budget is cut for: two 1024-thread workgroups per CU
#endif
#define MV_WAL_ATTR __attribute__((amdgpu_waves_per_eu(MV_WAL_WPE)))        // 256-B rows in flight per wave

// a wave-uniform 64-bit value from lane 0
MV_DEV uint64_t bcast64(uint64_t x) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)x), hi = __builtin_amdgcn_readfirstlane((uint32_t)(x >> 32));
  return ((uint64_t)hi << 32) | lo;
}

struct Lds {
  uint32_t a[A_WORDS];
#ifndef MV_WAL_SGLOBAL
  uint32_t s[S_WORDS];
#endif
};

MV_DEV void lds_fill(Lds& L, const uint32_t* __restrict__ tables) {
  for (int i = threadIdx.x; i < A_WORDS + S_WORDS; i += blockDim.x) {
    if (i < A_WORDS) L.a[i] = tables[i];
#ifndef MV_WAL_SGLOBAL
    else L.s[i - A_WORDS] = tables[i];
#endif
  }
  __syncthreads();
}

MV_DEV uint32_t adv256(const Lds& L, uint32_t u, uint32_t c) {
  return L.a[(0 * 256 + (u & 255)) * REP + c] ^ L.a[(1 * 256 + ((u >> 8) & 255)) * REP + c] ^
         L.a[(2 * 256 + ((u >> 16) & 255)) * REP + c] ^ L.a[(3 * 256 + (u >> 24)) * REP + c];
}
// the tree's shift maps: in LDS, or (MV_WAL_SGLOBAL) read through the caches
MV_DEV const uint32_t* s_tab(const Lds& L, const uint32_t* __restrict__ tables) {
#ifdef MV_WAL_SGLOBAL
  return tables + A_WORDS;
#else
  return L.s;
#endif
}
MV_DEV uint32_t shiftk(const uint32_t* S, int k, uint32_t u) {
  const uint32_t* s = S + k * 1024;
  return s[u & 255] ^ s[256 + ((u >> 8) & 255)] ^ s[512 + ((u >> 16) & 255)] ^ s[768 + (u >> 24)];
}
MV_DEV uint32_t ld32(const uint8_t* p) { return *reinterpret_cast<const uint32_t*>(p); }  // (nt loads: no gain)

// the sink of a fold that only wants the crc
struct NoSink {
  MV_DEV void operator()(int64_t, uint32_t) const {}
};

// crc_raw(0xFFFFFFFF, base[a, b)) (the CRC register before the final xor), on the whole wave.
// Reads only the aligned dwords that hold bytes of [a, b). sink(q, w): w = the four bytes
// base[a + q, a + q + 4), called once for every q > -4 on the grid b - 4 k (bytes at q < 0 are
// not the string's: their value is unspecified).
template <class Sink = NoSink>
MV_DEV uint32_t crc_raw_wave(const uint8_t* __restrict__ base, uint64_t a, uint64_t b, const Lds& L,
                              const uint32_t* S, const Sink& sink = Sink()) {
  const uint32_t lane = threadIdx.x & 63, c = lane & (REP - 1);
  const uint64_t len = b - a;
  const uint64_t R = (len + 4 + 255) / 256;
  const uint32_t sh = (uint32_t)(b & 3);
  const int64_t a4 = (int64_t)(a & ~3ull);
  const uint64_t Z = (uint64_t)PREFIX << 32;  // virtual bytes a-8 .. a-1: 0 0 0 0 P0 P1 P2 P3
  uint32_t u = 0;
  // rows 0, 1: may hold bytes before a (zeros, then the prefix P); their loads go out first
  uint32_t w01[2] = {0u, 0u};
  int64_t q01[2];
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const int64_t x = (int64_t)b - 256 * (int64_t)(R - j) + 4 * (int64_t)lane;
    q01[j] = x - (int64_t)a;
    if ((uint64_t)j < R && q01[j] > -4) {
      const int64_t xa = x - sh;
      const uint32_t A = xa >= a4 ? ld32(base + xa) : 0u;
      const uint32_t B = sh ? ld32(base + xa + 4) : 0u;
      w01[j] = sh ? __builtin_amdgcn_alignbyte(B, A, sh) : A;
      sink(q01[j], w01[j]);
    }
  }
  // rows 2 .. R-1 in batches of WAL_ROWS loads in flight (the kernel is bound by HBM latency:
  // ~1-2 us per round trip, so each lane keeps a batch outstanding); the last batch is partial,
  // its rows past R neither loaded nor folded: one round trip, not one per leftover row
  const uint8_t* pr = base + (int64_t)b - 256 * (int64_t)(R - 2) + 4 * (int64_t)lane - sh;
  int64_t qr = (int64_t)len - 256 * (int64_t)(R - 2) + 4 * (int64_t)lane;  // of row 2's word
  for (uint64_t j0 = 2;; j0 += WAL_ROWS, pr += 256 * WAL_ROWS, qr += 256 * WAL_ROWS) {
    uint32_t A[WAL_ROWS], B[WAL_ROWS];
#pragma unroll
    for (int k = 0; k < WAL_ROWS; k++) {
      const bool live = j0 + k < R;  // wave-uniform
      A[k] = live ? ld32(pr + 256 * k) : 0u;
      B[k] = live && sh ? ld32(pr + 256 * k + 4) : 0u;
    }
    if (j0 == 2) {
#pragma unroll
      for (int j = 0; j < 2; j++) {
        if ((uint64_t)j >= R) break;
        uint32_t w = w01[j];
        const int64_t q = q01[j];
        if (q < 0) {
          const uint32_t keep = q <= -4 ? 0u : (0xffffffffu << (8 * (uint32_t)(-q)));
          w = q < -8 ? 0u : ((w & keep) | (uint32_t)(Z >> (8 * (q + 8))));
        }
        u = adv256(L, u, c) ^ w;
      }
    }
#pragma unroll
    for (int k = 0; k < WAL_ROWS; k++)
      if (j0 + k < R) {
        const uint32_t w = sh ? __builtin_amdgcn_alignbyte(B[k], A[k], sh) : A[k];
        sink(qr + 256 * k, w);
        u = adv256(L, u, c) ^ w;
      }
    if (j0 + WAL_ROWS >= R) break;
  }
  // lanes: val over [g, g + 2^(k+1)) = shift(val[g, g + 2^k), 4 * 2^k) ^ val[g + 2^k, ...)
#pragma unroll
  for (int k = 0; k < S_LEVELS; k++) {
    const uint32_t v = (uint32_t)__shfl_down((int)u, 1 << k);
    if ((lane & ((2u << k) - 1)) == 0) u = shiftk(S, k, u) ^ v;
  }
  u = shiftk(S, 0, u);  // lane 63's word ends 4 bytes before the end
  return (uint32_t)__shfl((int)u, 0);
}

// state <- state advanced over n zero bytes (crc_raw(state, 0^n)); rare paths only
MV_DEV uint32_t zeros_shift(const Lds& L, const uint32_t* S, const uint32_t* __restrict__ tbyte, uint32_t s,
                            uint64_t n) {
  const uint32_t c = threadIdx.x & (REP - 1);
  for (; n >= 256; n -= 256) s = adv256(L, s, c);
  for (int k = S_LEVELS - 1; k >= 0; k--)
    if (n >= (4u << k)) {
      s = shiftk(S, k, s);
      n -= 4u << k;
    }
  for (; n; n--) s = (s >> 8) ^ tbyte[s & 255];
  return s;
}

// the persistent grid of a one-wave-per-item crc kernel: as many 1024-thread workgroups as the
// LDS lets a CU hold, on every CU
static inline uint32_t crc_grid(uint64_t items, int cus) {
  const uint64_t per_wg = WG / 64;
  uint64_t g = (items + per_wg - 1) / per_wg;
  const uint64_t cap = (uint64_t)(163840 / sizeof(Lds)) * (uint64_t)cus;  // 1024-thread workgroups per CU (LDS)
  return (uint32_t)(g < 1 ? 1 : (g > cap ? cap : g));
}

}  // namespace wal
}  // namespace mv
