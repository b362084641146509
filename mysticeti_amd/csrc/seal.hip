// Block sealing (mv_seal_blocks): the inverse of StatementBlock::verify, which is
// StatementBlock::new_with_signer (mysticeti-core/src/types.rs:155-218) -- Signer::sign_block
// (crypto.rs:199-223) over BLAKE2b-256 of the signed pre-image (crypto.rs:85-128), then
// BlockDigest::new (crypto.rs:38-61) = BLAKE2b-256(pre-image || signature) -- on blocks that are
// already bincode (types.rs:93-114, data.rs:43-52) with placeholder digest and signature fields.
//
//   k_seal_keys   one lane per authority: seed -> (a mod l, prefix, public key), RFC 8032 5.1.5,
//                 once per call
//   k_seal_scan   one lane per block: the bincode walk alone. status (OK, PARSE_ERROR,
//                 UNKNOWN_AUTHOR) and the block's (authority, round), from which the host fills
//                 the (authority, round) -> block hash table and cuts the levels of a linked call
//   k_seal        one lane per block of a level: link the includes through the table, walk the
//                 bincode into BLAKE2b as the pre-image is produced, m = B2(P), sign m, continue
//                 the same hash state with the signature for d = B2(P || sig), store sig and d
//
// One walk serves both hashes: the stream keeps the chaining state after the last full 128-byte
// block of P and its unfinished tail; B2(P) finalises a copy, the signature is then appended to
// the original and finalised as B2(P || sig). Nothing of P is hashed twice.
//
// The walk and its memory-safety argument are bincode_walk.h's; off + len is held against the
// buffer's size before it (block_span). Stores go to the include digests (linked calls), the own
// digest (bytes 24..56) and the signature (the 64 bytes the walk ends on) of a block that passed
// k_seal_scan, and nowhere else in the buffer.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mysti_verify.h"
#include "bincode_walk.h"
#include "blake2b_quad.h"
#include "kernels.h"
#include "tables.h"

namespace mv {
namespace seal {

constexpr uint32_t KEY_WORDS = 24;  // per authority: a mod l (8 words), prefix (8), public key (8)
constexpr uint32_t TAB_NONE = 0xffffffffu;

// The (authority, round) -> block table: open addressing, linear probing, built by the host from
// k_seal_scan's heads (lowest block index per key). max_probe is the longest probe sequence of
// any key the host entered, so a lookup examines at most max_probe + 1 slots.
struct LinkTable {
  const uint4* slots;  // round lo, round hi, authority, block (TAB_NONE: empty)
  uint32_t mask;       // slots - 1 (a power of two), 0 with slots == nullptr: no table
  uint32_t max_probe;
};
MV_DEV uint32_t tab_find(const LinkTable& t, uint64_t a, uint64_t r) {
  if (!t.slots || a > 0xffffffffull) return TAB_NONE;
  uint32_t h = mvk::seal_table_hash(a, r) & t.mask;
  for (uint32_t k = 0; k <= t.max_probe; k++, h = (h + 1) & t.mask) {
    const uint4 s = t.slots[h];
    if (s.w == TAB_NONE) return TAB_NONE;
    if (s.x == (uint32_t)r && s.y == (uint32_t)(r >> 32) && s.z == (uint32_t)a) return s.w;
  }
  return TAB_NONE;
}

// 8 bytes to any address (the compiler picks the widest stores the target allows unaligned)
MV_DEV void poke8(uint8_t* p, uint64_t v) { __builtin_memcpy(p, &v, 8); }

// BLAKE2b-256 over bytes as they are produced. The lane's 128-byte message block lives in LDS,
// word w of lane l at row[64 w + l] (no two lanes of a wave share a bank); a full block is
// compressed only when the next word arrives, so the last block is always still in the row.
struct B2Stream : ByteGather<B2Stream> {
  uint64_t h[8];
  uint64_t* row;
  uint32_t nw = 0;  // whole words in the row (<= 16)

  MV_DEV explicit B2Stream(uint64_t* lane_row) : row(lane_row) { b2q::lane_init256(h); }
  MV_DEV void load(uint64_t (&m)[16], uint32_t words, uint64_t tail) const {
#pragma unroll
    for (uint32_t j = 0; j < 16; j++) m[j] = j < words ? row[64 * j] : (j == words ? tail : 0ull);
  }
  MV_DEV void word(uint64_t w) {
    if (nw == 16) {
      uint64_t m[16];
      load(m, 16, 0);
      b2q::lane_compress(h, m, len - nb, false);  // the bytes in whole words so far (put() counts after word())
      nw = 0;
    }
    row[64 * nw++] = w;
  }
  // the digest of the bytes so far; the stream goes on unchanged
  MV_DEV void digest(uint64_t (&out)[4]) const {
    uint64_t hc[8], m[16];
#pragma unroll
    for (int j = 0; j < 8; j++) hc[j] = h[j];
    if (nw == 16 && nb) {  // a full block, then the tail bytes in a block of their own
      load(m, 16, 0);
      b2q::lane_compress(hc, m, len - nb, false);
      load(m, 0, acc);
    } else {
      load(m, nw, acc);
    }
    b2q::lane_compress(hc, m, len, true);
#pragma unroll
    for (int j = 0; j < 4; j++) out[j] = hc[j];
  }
};

// What sealing takes from the walk: the block's (authority, round), where its signature lies, and
// link(a, r, d), called per include before its digest bytes at d are read.
template <class LinkFn>
struct SealVisitor {
  LinkFn link;
  uint64_t author = 0, round = 0;
  uint32_t sig_pos = 0;  // of the 64 signature bytes in the block
  bool fits = false;     // sig_pos holds the position
  MV_DEV void own(uint64_t a, uint64_t r, const uint8_t*) {
    author = a;
    round = r;
  }
  MV_DEV void include(uint64_t a, uint64_t r, const uint8_t* d) { link(a, r, const_cast<uint8_t*>(d)); }
  MV_DEV void vote_range(uint64_t, uint64_t) {}
  MV_DEV void meta(uint64_t, uint64_t pos) {
    fits = pos <= 0xffffff00ull;
    sig_pos = (uint32_t)pos;
  }
};
template <class Sink, class LinkFn>
MV_DEV bool seal_walk(BcReader& r, Sink& w, SealVisitor<LinkFn>& vis) {
  return block_walk(r, w, vis) && vis.fits;
}

// Where block i lies, or false when its span leaves the buffer.
MV_DEV bool block_span(const uint64_t* off, const uint64_t* len, uint32_t i, uint64_t buf_bytes, uint64_t& o,
                       uint64_t& L) {
  o = off[i];
  L = len[i];
  return o <= buf_bytes && L <= buf_bytes - o;
}

__global__ void __launch_bounds__(64) k_seal_keys(const uint8_t* __restrict__ seeds, uint32_t n_auth,
                                                  const uint4* __restrict__ btab_g, uint32_t* __restrict__ keys) {
  __shared__ uint4 btab[BT_TABLE];
  lds_btab_load(btab, btab_g, BT_TABLE);
  const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= n_auth) return;
  uint32_t sw[8], ared[8], prefix[8], pkw[8];
#pragma unroll
  for (int i = 0; i < 8; i++) sw[i] = reinterpret_cast<const uint32_t*>(seeds)[8 * (size_t)a + i];
  ed25519_expand(ared, prefix, pkw, sw, btab);
  uint32_t* o = keys + KEY_WORDS * (size_t)a;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    o[i] = ared[i];
    o[8 + i] = prefix[i];
    o[16 + i] = pkw[i];
  }
}

__global__ void __launch_bounds__(256) k_seal_scan(const uint8_t* __restrict__ buf, uint64_t buf_bytes,
                                                   const uint64_t* __restrict__ off, const uint64_t* __restrict__ len,
                                                   uint32_t n, uint32_t n_auth, uint8_t* __restrict__ status,
                                                   uint64_t* __restrict__ heads) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t o, L;
  auto no_link = [](uint64_t, uint64_t, uint8_t*) {};
  SealVisitor<decltype(no_link)> hd{no_link};
  bool ok = block_span(off, len, i, buf_bytes, o, L);
  if (ok) {
    BcReader r{buf + o, L, 0, true};
    NoSink ns;
    ok = seal_walk(r, ns, hd);
  }
  status[i] = !ok ? MV_SEAL_PARSE_ERROR : (hd.author >= n_auth ? MV_SEAL_UNKNOWN_AUTHOR : MV_SEAL_OK);
  heads[2 * (size_t)i] = ok ? hd.author : ~0ull;
  heads[2 * (size_t)i + 1] = ok ? hd.round : ~0ull;
}

// Blocks [lo, hi), one lane each, WAVES waves per workgroup (they share the LDS copy of the
// fixed-base table). bd_all: every block's digest, written here and read by later levels.
template <int WAVES>
__global__ void __launch_bounds__(64 * WAVES)
    k_seal(uint8_t* __restrict__ buf, uint64_t buf_bytes, const uint64_t* __restrict__ off,
           const uint64_t* __restrict__ len, uint32_t lo, uint32_t hi, const uint32_t* __restrict__ keys,
           const uint4* __restrict__ btab_g, LinkTable tab, uint8_t* __restrict__ status, uint8_t* __restrict__ md_all,
           uint8_t* __restrict__ bd_all) {
  __shared__ uint4 btab[BT_TABLE];
  __shared__ uint64_t rows[WAVES][16 * 64];
  lds_btab_load(btab, btab_g, BT_TABLE);  // (the only barrier: lanes leave freely after it)
  const uint32_t i = lo + blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= hi || status[i] != MV_SEAL_OK) return;
  uint64_t o, L;
  if (!block_span(off, len, i, buf_bytes, o, L)) return;  // (k_seal_scan said otherwise)
  if (L < 64) return;  // (a block that parsed holds its reference and the include count)
  uint8_t* const blk = buf + o;

  if (tab.slots) {
    // An include that names a block of this call of the same or a later round: not linked, and
    // the block stays as it is. The include region was bounded by k_seal_scan's walk; it is
    // bounded here again before it is read.
    const uint64_t me_r = peek8(blk + 8), n_inc = peek8(blk + 56);
    if (n_inc > (L - 64) / 56) return;
    bool unlinked = false;
    for (uint64_t k = 0; k < n_inc && !unlinked; k++) {
      const uint8_t* p = blk + 64 + 56 * k;
      const uint64_t a = peek8(p), rd = peek8(p + 8);
      if (rd >= me_r && tab_find(tab, a, rd) != TAB_NONE) unlinked = true;
    }
    if (unlinked) {
      status[i] = MV_SEAL_UNLINKED;
      return;
    }
  }

  B2Stream st(&rows[threadIdx.x >> 6][threadIdx.x & 63]);
  BcReader r{blk, L, 0, true};
  const uint64_t my_round = peek8(blk + 8);
  auto link = [&](uint64_t a, uint64_t rd, uint8_t* d) {
    if (!tab.slots || rd >= my_round) return;
    const uint32_t j = tab_find(tab, a, rd);
    // a matched block that was itself left unlinked has no fresh digest: the bytes stay
    if (j == TAB_NONE || status[j] != MV_SEAL_OK) return;
    const uint64_t* dg = reinterpret_cast<const uint64_t*>(bd_all + 32 * (size_t)j);
#pragma unroll
    for (int q = 0; q < 4; q++) poke8(d + 8 * q, dg[q]);
  };
  SealVisitor<decltype(link)> hd{link};
  const bool ok = seal_walk(r, st, hd);
  if (!ok) {  // cannot happen after k_seal_scan: the walk is the same and the link changes no length
    status[i] = MV_SEAL_PARSE_ERROR;
    return;
  }

  uint64_t m64[4];
  st.digest(m64);  // m = B2(P)
  uint32_t mw[8];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    mw[2 * q] = (uint32_t)m64[q];
    mw[2 * q + 1] = (uint32_t)(m64[q] >> 32);
  }
  const uint32_t* key = keys + KEY_WORDS * (size_t)hd.author;  // author < n_auth: status is OK
  uint32_t ared[8], prefix[8], pkw[8], Rw[8], S[8];
#pragma unroll
  for (int q = 0; q < 8; q++) {
    ared[q] = key[q];
    prefix[q] = key[8 + q];
    pkw[q] = key[16 + q];
  }
  ed25519_sign(Rw, S, ared, prefix, pkw, mw, btab);

  uint64_t sg[8];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    sg[q] = ((uint64_t)Rw[2 * q + 1] << 32) | Rw[2 * q];
    sg[4 + q] = ((uint64_t)S[2 * q + 1] << 32) | S[2 * q];
  }
#pragma unroll
  for (int q = 0; q < 8; q++) st.put(sg[q], 8);
  uint64_t d64[4];
  st.digest(d64);  // d = B2(P || sig)

  uint8_t* sp = blk + hd.sig_pos;  // sig_pos + 64 <= L: the walk checked the 64 bytes
#pragma unroll
  for (int q = 0; q < 8; q++) poke8(sp + 8 * q, sg[q]);
#pragma unroll
  for (int q = 0; q < 4; q++) poke8(blk + 24 + 8 * q, d64[q]);  // the reference's digest, bytes 24..56
  uint64_t* mo = reinterpret_cast<uint64_t*>(md_all + 32 * (size_t)i);
  uint64_t* bo = reinterpret_cast<uint64_t*>(bd_all + 32 * (size_t)i);
#pragma unroll
  for (int q = 0; q < 4; q++) {
    mo[q] = m64[q];
    bo[q] = d64[q];
  }
}

}  // namespace seal
}  // namespace mv

namespace mvk {

hipError_t launch_seal_keys(const uint8_t* seeds, uint32_t n_auth, const void* btab, uint32_t* keys, hipStream_t s) {
  if (n_auth == 0) return hipSuccess;
  hipLaunchKernelGGL(mv::seal::k_seal_keys, dim3((n_auth + 63) / 64), dim3(64), 0, s, seeds, n_auth,
                     (const uint4*)btab, keys);
  return hipGetLastError();
}

hipError_t launch_seal_scan(const uint8_t* buf, uint64_t buf_bytes, const uint64_t* off, const uint64_t* len,
                            uint32_t n, uint32_t n_auth, uint8_t* status, uint64_t* heads, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(mv::seal::k_seal_scan, dim3((n + 255) / 256), dim3(256), 0, s, buf, buf_bytes, off, len, n,
                     n_auth, status, heads);
  return hipGetLastError();
}

hipError_t launch_seal_level(uint8_t* buf, uint64_t buf_bytes, const uint64_t* off, const uint64_t* len, uint32_t lo,
                             uint32_t hi, const uint32_t* keys, const void* btab, const SealTable& t, uint8_t* status,
                             uint8_t* md, uint8_t* bd, hipStream_t s) {
  if (hi <= lo) return hipSuccess;
  const uint32_t m = hi - lo;
  const mv::seal::LinkTable tab{(const uint4*)t.slots, t.mask, t.max_probe};
  if (m >= SEAL_THROUGHPUT_MIN)
    hipLaunchKernelGGL(mv::seal::k_seal<4>, dim3((m + 255) / 256), dim3(256), 0, s, buf, buf_bytes, off, len, lo, hi,
                       keys, (const uint4*)btab, tab, status, md, bd);
  else
    hipLaunchKernelGGL(mv::seal::k_seal<1>, dim3((m + 63) / 64), dim3(64), 0, s, buf, buf_bytes, off, len, lo, hi,
                       keys, (const uint4*)btab, tab, status, md, bd);
  return hipGetLastError();
}

}  // namespace mvk
