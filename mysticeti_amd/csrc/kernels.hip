// HIP kernels of the StatementBlock verification engine (gfx950 only).
//
//   k_btable_init    fixed-base tables [j]B and [j](2^124 B), j = 0..128, affine
//                    (y+x, y-x, 2dxy)
//   k_verify         ZIP-215 ed25519 verify, one signature per lane (ed25519-consensus
//                    VerificationKey::verify, called at mysticeti-core/src/crypto.rs:188),
//                    on half-size scalars (scalar25519.h sc_halfsize)
//   k_sign           RFC 8032 signing, one per lane (crypto.rs:199-223, corpus generation)
//   (BLAKE2b: blake2b_quad.hip for small calls, blake2b_lane.hip at batch size; the
//   launch_blake2b / launch_block_hash entry points below route between them)
//   k_selftest       field / scalar primitives for the parity tests
//   k_selftest_wide  field and point functions on raw limbs (the limb-bound contract's tests)
//   k_selftest_scalar  the functions of scalar25519.h one by one (the scalar layer's tests)
//
// The verify kernel is INT32-VALU bound: HBM traffic is 128 B of
// input per signature plus the per-lane variable-base tables (2 x 9 cached points,
// written once, read 32 times each, L2/MALL-resident per wave).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/mysti_verify.h"
#include "fe25519.h"
#include "fe_q4.h"
#include "fe_r16.h"
#include "ge25519.h"
#include "hash_dev.h"
#include "kernels.h"
#include "scalar25519.h"
#include "tables.h"
#include "comb.h"
#include "quad25519.h"
#include "pt_r16.h"

namespace mv {

// Per-wave variable-base table scratch. Lane-major: each lane owns 2 x 81 contiguous
// uint4 ([table][entry][quad]), so one entry gather reads 144 contiguous bytes per lane
// (2 cache lines) and the whole line is used (a wave-major layout coalesces the build's
// stores, but a random-digit gather then touches ~5 partly used lines per 8 lanes per quad).
constexpr int TAB_LANE_STRIDE = 2 * AT_TABLE, TAB_QUAD_STRIDE = 1;
constexpr int TAB_ENTRY_STRIDE = AT_QUADS * TAB_QUAD_STRIDE;
constexpr int TAB_TABLE_STRIDE = AT_ENTRIES * TAB_ENTRY_STRIDE;  // A table -> R table
MV_DEV void atab_put(uint4* tab, int e, const cached& c) {
  uint4* p = tab + e * TAB_ENTRY_STRIDE;
  uint4 q[9];
  cached_to_quads(q, c);
#pragma unroll
  for (int i = 0; i < 9; i++) p[i * TAB_QUAD_STRIDE] = q[i];
}
// raw entry load; the sign is applied at use time (cached_cneg) so the gather's
// latency hides behind the window's doublings
MV_DEV void atab_load(cached& c, const uint4* tab, int digit) {
  int e = digit < 0 ? -digit : digit;
  const uint4* p = tab + e * TAB_ENTRY_STRIDE;
  uint4 q[9];
#pragma unroll
  for (int i = 0; i < 9; i++) q[i] = p[i * TAB_QUAD_STRIDE];
  quads_to_cached(c, q);
}

// ---------------------------------------------------------------- kernels
__global__ void __launch_bounds__(256) k_btable_init(uint4* out) {
  const int j = threadIdx.x;
  const int t = blockIdx.x;  // 0: B, 1: 2^124 B
  if (j >= BT_ENTRIES) return;
  // B = decompress(4/5, sign 0)
  const uint32_t by[8] = {0x66666658, 0x66666666, 0x66666666, 0x66666666,
                          0x66666666, 0x66666666, 0x66666666, 0x66666666};
  p3 B, R;
  bool okB, okR;
  decompress_x2(B, okB, by, R, okR, by);
  if (t == 1) {
    p2 P;
    p1p1 Q;
    P.X = B.X;
    P.Y = B.Y;
    P.Z = B.Z;
    for (int i = 0; i < 123; i++) {
      p2_dbl(Q, P);
      p1p1_to_p2(P, Q);
    }
    p2_dbl(Q, P);
    p1p1_to_p3(B, Q);
  }
  p3 acc;
  p3_identity(acc);
  cached cb;
  p3_to_cached(cb, B);
  for (int i = 0; i < j; i++) {
    p1p1 q;
    p3_add_cached(q, acc, cb);
    p1p1_to_p3(acc, q);
  }
  fe zi, x, y, xy, d2;
  fe_invert(zi, acc.Z);
  fe_mul(x, acc.X, zi);
  fe_mul(y, acc.Y, zi);
  fe_const(d2, K_D2);
  precomp pc;
  fe_add(pc.ypx, y, x);
  fe_sub(pc.ymx, y, x);
  fe_mul(xy, x, y);
  fe_mul(pc.xy2d, xy, d2);
  fe_canon(pc.ypx, pc.ypx);
  fe_canon(pc.ymx, pc.ymx);
  fe_canon(pc.xy2d, pc.xy2d);
  uint4 q[7];
  precomp_to_quads(q, pc);
  uint4* o = out + t * BT_TABLE + j * BT_QUADS;
#pragma unroll
  for (int i = 0; i < 7; i++) o[i] = q[i];
}

// Per-wave scratch layout (uint4 units): the two variable-base tables of the 64 lanes
// ([0..8](-A) or [0..8](A) by the sign of c, then [0..8](-R)), then the recoded
// scalars [group][lane], parked in HBM during the ladder instead of holding 16 VGPRs.
constexpr int SCR_DIG = 2 * AT_TABLE * 64;  // 4 groups x uint4 (c, d, e lo, e hi)
constexpr int WAVE_QUADS = 2 * AT_TABLE + 4;  // 166 per lane

// [0..8]P as cached points into a per-wave table
MV_DEV void vtab_build(uint4* tab, const p3& P) {
  cached c1, c;
  cached_identity(c);
  atab_put(tab, 0, c);
  p3_to_cached(c1, P);
  atab_put(tab, 1, c1);
  p3 cur = P;
  for (int j = 2; j <= 8; j++) {
    p1p1 t;
    p3_add_cached(t, cur, c1);
    p1p1_to_p3(cur, t);
    p3_to_cached(c, cur);
    atab_put(tab, j, c);
  }
}

// What the batch path's k_bv_prep already decoded (the fallback re-verifies from it): R at
// pts[i] and A at pts[n + i] (affine precomp), or A from the committee's comb table entry
// [0][1] = [1](-A) when it was summed per key; status[i] != 0 is prep's final verdict
// (s >= l or a point that does not decode) and stays.
struct PrepView {
  const uint4* pts;   // nullptr: decode A and R here
  uint32_t n;
  const uint4* comb;  // non-null: A of key b from the comb tables
};

// One signature per lane. pk rows are read at key_idx[i] when key_idx != nullptr.
// Two waves per SIMD (<= 256 VGPRs): occupancies 1 and 3 were measured no faster and removed.
//
// Checks [8]([e]B - [c]A - [d]R) == O with e = d*s mod l, (c, d) = sc_halfsize(k),
// which holds iff the ZIP-215 equation [8]([s]B - [k]A - R) == O does (see
// sc_halfsize). e's signed radix-256 digits 0..15 go against [j]B at the even 4-bit
// windows, digits 16..31 against [j](2^124 B) at the odd ones, so every one of the
// 32 windows does 4 doublings and three additions (A, R, B or 2^124 B).
__global__ void __launch_bounds__(256, 2)
    k_verify(const uint8_t* __restrict__ msg, const uint8_t* __restrict__ sig, const uint8_t* __restrict__ pk,
             const uint32_t* __restrict__ key_idx, uint32_t n, const uint4* __restrict__ btab_g,
             uint4* __restrict__ scratch, uint8_t* __restrict__ status, const uint32_t* __restrict__ skip,
             uint32_t skip_group, PrepView pv) {
  // batch fallback (batch.hip): nothing to do for a group whose equation held (skip_group
  // is a multiple of the block size, so the test is uniform over the block)
  if (skip && skip[skip_group ? blockIdx.x * blockDim.x / skip_group : 0]) return;
  __shared__ uint4 btab[2 * BT_TABLE];
  lds_btab_load(btab, btab_g, 2 * BT_TABLE);
  const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t idx = gid < n ? gid : n - 1;
  const int lane = threadIdx.x & 63;
  uint4* wave_tab = scratch + (size_t)(gid >> 6) * (WAVE_QUADS * 64);
  uint4* wave_dig = wave_tab + SCR_DIG;
  uint4* tabA = wave_tab + lane * TAB_LANE_STRIDE;
  uint4* tabR = tabA + TAB_TABLE_STRIDE;

  bool okA, okR, s_ok;
  {
    uint32_t aw[8], rw[8], sw[8], mw[8];
    load8(aw, pk + 32 * (size_t)(key_idx ? key_idx[idx] : idx));
    load8(rw, sig + 64 * (size_t)idx);
    load8(sw, sig + 64 * (size_t)idx + 32);
    load8(mw, msg + 32 * (size_t)idx);

    s_ok = sc_is_canonical(sw);
    // k = SHA-512(R || A || M) mod l over the original encodings
    uint32_t kin[24], h[16], k[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
      kin[i] = rw[i];
      kin[8 + i] = aw[i];
      kin[16 + i] = mw[i];
    }
    sha512_short(h, kin, 96);
    sc_reduce512(k, h);
    uint32_t c[4], d[8], e[8], zero[8];
    bool c_neg;
    sc_halfsize(c, c_neg, d, k);
#pragma unroll
    for (int i = 0; i < 8; i++) zero[i] = 0;
#pragma unroll
    for (int i = 4; i < 8; i++) d[i] = 0;
    sc_muladd(e, d, sw, zero);
    uint32_t cd[4], dd[4], ed[8];
    sc_recode16_128(cd, c);
    sc_recode16_128(dd, d);
    sc_recode256(ed, e);
#pragma unroll
    for (int g = 0; g < 4; g++) wave_dig[g * 64 + lane] = make_uint4(cd[g], dd[g], ed[g], ed[4 + g]);

    p3 A, R, nR;
    if (pv.pts) {  // decoded by k_bv_prep; lanes prep already rejected keep its verdict
      const bool prep_ok = status[idx] == 0;
      okA = prep_ok;
      okR = prep_ok;
      s_ok = s_ok && prep_ok;
      uint4 q[7];
      precomp pc;
      const uint4* pr = pv.pts + (size_t)idx * PT_QUADS;
#pragma unroll
      for (int k = 0; k < 7; k++) q[k] = pr[k];
      quads_to_precomp(pc, q);
      precomp_to_p3(R, pc);
      const uint4* pa = pv.comb ? pv.comb + (size_t)(key_idx ? key_idx[idx] : idx) * CT_TABLE + CT_QUADS
                                : pv.pts + ((size_t)pv.n + idx) * PT_QUADS;
#pragma unroll
      for (int k = 0; k < 7; k++) q[k] = pa[k];
      quads_to_precomp(pc, q);
      if (pv.comb) precomp_cneg(pc, true);  // the tables hold -A
      precomp_to_p3(A, pc);
    } else {
      decompress_x2(A, okA, aw, R, okR, rw);
    }
    // -[c]A = [|c|](-A) for c >= 0, [|c|]A for c < 0
    if (!c_neg) p3_neg(A, A);
    vtab_build(tabA, A);
    p3_neg(nR, R);
    vtab_build(tabR, nR);
  }

  p2 P;
  p3 P3;
  p1p1 Q;
  cached ca, cr;
  precomp pb;
  // 4 groups of 8 windows; a group's digit quad is loaded one group ahead, each
  // window's two table gathers are issued before its doublings and consumed after.
  uint4 dw_next = wave_dig[3 * 64 + lane];
  for (int g = 3; g >= 0; g--) {
    const uint4 dw = dw_next;
    if (g > 0) dw_next = wave_dig[(g - 1) * 64 + lane];
    for (int j = 7; j >= 0; j--) {
      const int w = 8 * g + j;
      const int dc = ((int)(dw.x << (28 - 4 * j))) >> 28;
      const int dd = ((int)(dw.y << (28 - 4 * j))) >> 28;
      atab_load(ca, tabA, dc);
      atab_load(cr, tabR, dd);
      if (w != 31) {
        for (int i = 0; i < 3; i++) {
          p2_dbl(Q, P);
          p1p1_to_p2(P, Q);
        }
        p2_dbl(Q, P);
        p1p1_to_p3(P3, Q);
      } else {
        p3_identity(P3);
      }
      cached_cneg(ca, dc < 0);
      p3_add_cached(Q, P3, ca);
      p1p1_to_p3(P3, Q);
      cached_cneg(cr, dd < 0);
      p3_add_cached(Q, P3, cr);
      p1p1_to_p3(P3, Q);
      // even window 2i: digit i of e (B); odd window 2i+1: digit 16+i (2^124 B)
      const uint32_t ew = (j & 1) ? dw.w : dw.z;
      const int de = ((int)(ew << (24 - 8 * (j >> 1)))) >> 24;
      btab_get(pb, btab + (j & 1) * BT_TABLE, de);
      p3_add_precomp(Q, P3, pb);
      p1p1_to_p2(P, Q);
    }
  }
  // cofactored check: [8]([e]B - [c]A - [d]R) == identity
#pragma unroll 1
  for (int i = 0; i < 3; i++) {
    p2_dbl(Q, P);
    p1p1_to_p2(P, Q);
  }
  const bool ident = fe_is_zero(P.X) && fe_eq(P.Y, P.Z);
  if (gid < n && !(pv.pts && !okA)) {  // (prep's own verdicts stay)
    uint8_t st = !okA ? 2 : ((s_ok && okR && ident) ? 0 : 1);
    status[gid] = st;
  }
}

// RFC 8032: (pk, R || S) from (seed, 32-byte msg)
__global__ void __launch_bounds__(256, 2)
    k_sign(const uint8_t* __restrict__ seed, const uint8_t* __restrict__ msg, uint32_t n,
           const uint4* __restrict__ btab_g, uint8_t* __restrict__ pk_out, uint8_t* __restrict__ sig_out) {
  __shared__ uint4 btab[BT_TABLE];
  lds_btab_load(btab, btab_g, BT_TABLE);
  const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t idx = gid < n ? gid : n - 1;
  uint32_t sw[8], mw[8], ared[8], prefix[8], pkw[8], Rw[8], S[8];
  load8(sw, seed + 32 * (size_t)idx);
  load8(mw, msg + 32 * (size_t)idx);
  ed25519_expand(ared, prefix, pkw, sw, btab);
  ed25519_sign(Rw, S, ared, prefix, pkw, mw, btab);
  if (gid < n) {
    store8(pk_out + 32 * (size_t)gid, pkw);
    store8(sig_out + 64 * (size_t)gid, Rw);
    store8(sig_out + 64 * (size_t)gid + 32, S);
  }
}

// Field / scalar primitives on 16-word lane inputs (parity tests).
__global__ void __launch_bounds__(64) k_selftest(int op, const uint32_t* __restrict__ in, uint32_t n,
                                                 const uint4* __restrict__ btab_g, uint32_t* __restrict__ out) {
  __shared__ uint4 btab[2 * BT_TABLE];
  lds_btab_load(btab, btab_g, 2 * BT_TABLE);
  const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= n) return;
  uint32_t x[16], y[16];
#pragma unroll
  for (int i = 0; i < 16; i++) {
    x[i] = in[16 * (size_t)gid + i];
    y[i] = 0;
  }
  fe a, b, r;
  fe_from_words_full(a, x);
  fe_from_words_full(b, x + 8);
  switch (op) {
    case 0: fe_mul(r, a, b); fe_canon(r, r); break;
    case 1: fe_sq(r, a); fe_canon(r, r); break;
    case 2: fe_add(r, a, b); fe_canon(r, r); break;
    case 3: fe_sub(r, a, b); fe_canon(r, r); break;
    case 4: fe_invert(r, a); fe_canon(r, r); break;
    case 5: fe_pow_p58(r, a); fe_canon(r, r); break;
    case 6: fe_mul_small(r, a, x[8]); fe_canon(r, r); break;
    case 7: {  // ZIP-215 decode of a: x (canonical) and the ok flag in word 8
      p3 A, B;
      bool oa, ob;
      decompress_x2(A, oa, x, B, ob, x);
      fe_canon(r, A.X);
      y[8] = oa ? 1u : 0u;
      break;
    }
    case 8: {
      uint32_t k[8];
      sc_reduce512(k, x);
#pragma unroll
      for (int i = 0; i < 8; i++) out[16 * (size_t)gid + i] = k[i];
#pragma unroll
      for (int i = 8; i < 16; i++) out[16 * (size_t)gid + i] = 0;
      return;
    }
    case 9: {  // sha512 of 64 bytes
      sha512_short(y, x, 64);
#pragma unroll
      for (int i = 0; i < 16; i++) out[16 * (size_t)gid + i] = y[i];
      return;
    }
    case 15: {  // sha512 of 96 bytes (the R || A || M challenge input): the 64 input bytes, then their first 32
      uint32_t m96[24];
#pragma unroll
      for (int i = 0; i < 16; i++) m96[i] = x[i];
#pragma unroll
      for (int i = 0; i < 8; i++) m96[16 + i] = x[i];
      sha512_short(y, m96, 96);
#pragma unroll
      for (int i = 0; i < 16; i++) out[16 * (size_t)gid + i] = y[i];
      return;
    }
    // four lanes per element (fe_q4.h): every lane of a quad must hold the same input
    case 16: {
      feq qa, qb, qr;
      feq_from_fe(qa, a);
      feq_from_fe(qb, b);
      feq_mul(qr, qa, qb);
      fe_from_feq(r, qr);
      fe_canon(r, r);
      break;
    }
    case 17: {
      feq qa, qr;
      feq_from_fe(qa, a);
      feq_pow_p58(qr, qa);
      fe_from_feq(r, qr);
      fe_canon(r, r);
      break;
    }
    case 18: {  // a^(2^50) by repeated squaring
      feq qa, qr;
      feq_from_fe(qa, a);
      feq_sqn(qr, qa, 50);
      fe_from_feq(r, qr);
      fe_canon(r, r);
      break;
    }
    // one DPP row per element (fe_r16.h): every lane of a 16-lane row must hold the same input
    case 19: {
      fer ra, rb, rr;
      fer_from_fe(ra, a);
      fer_from_fe(rb, b);
      fer_mul(rr, ra, rb, r16::consts());
      fe_from_fer(r, rr);
      fe_canon(r, r);
      break;
    }
    case 20: {
      fer ra, rr;
      fer_from_fe(ra, a);
      fer_pow_p58(rr, ra);
      fe_from_fer(r, rr);
      fe_canon(r, r);
      break;
    }
    case 21: {  // a^(2^50) by repeated squaring
      fer ra, rr;
      fer_from_fe(ra, a);
      fer_sqn(rr, ra, 50, r16::consts());
      fe_from_fer(r, rr);
      fe_canon(r, r);
      break;
    }
    case 10: fe_set(r, sc_is_canonical(x) ? 1 : 0); break;
    case 11: {  // [a]B encoding for a scalar a < 2^253
      uint32_t sd[8];
      sc_recode256(sd, x);
      p3 P;
      basemul(P, sd, btab);
      uint32_t enc[8];
      p3_compress(enc, P);
#pragma unroll
      for (int i = 0; i < 8; i++) out[16 * (size_t)gid + i] = enc[i];
#pragma unroll
      for (int i = 8; i < 16; i++) out[16 * (size_t)gid + i] = 0;
      return;
    }
    case 13: {  // sc_halfsize of k < l: c words 0..3, c_neg word 4, d words 8..11
      uint32_t c[4], d[4];
      bool neg;
      sc_halfsize(c, neg, d, x);
#pragma unroll
      for (int i = 0; i < 16; i++) y[i] = 0;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        y[i] = c[i];
        y[8 + i] = d[i];
      }
      y[4] = neg;
#pragma unroll
      for (int i = 0; i < 16; i++) out[16 * (size_t)gid + i] = y[i];
      return;
    }
    case 14: {  // [a](2^124 B) encoding via the second fixed-base table
      uint32_t sd[8];
      sc_recode256(sd, x);
      p3 P;
      basemul(P, sd, btab + BT_TABLE);
      uint32_t enc[8];
      p3_compress(enc, P);
#pragma unroll
      for (int i = 0; i < 8; i++) out[16 * (size_t)gid + i] = enc[i];
#pragma unroll
      for (int i = 8; i < 16; i++) out[16 * (size_t)gid + i] = 0;
      return;
    }
    case 22: {  // sc_recode256 of a scalar a < 2^253: the packed digit words
      uint32_t sd[8];
      sc_recode256(sd, x);
#pragma unroll
      for (int i = 0; i < 8; i++) out[16 * (size_t)gid + i] = sd[i];
#pragma unroll
      for (int i = 8; i < 16; i++) out[16 * (size_t)gid + i] = 0;
      return;
    }
    case 12: {  // fe_canon of raw 255-bit input
      fe_from_words(r, x);
      fe_canon(r, r);
      break;
    }
    default: fe_set(r, 0);
  }
  {
    uint32_t rw[8];
    fe_to_words(rw, r);
#pragma unroll
    for (int i = 0; i < 8; i++) y[i] = rw[i];
  }
#pragma unroll
  for (int i = 0; i < 16; i++) out[16 * (size_t)gid + i] = y[i];
}

// Field and point functions on RAW limbs (ops >= 64, 64-word rows): the tests of the limb-bound
// contract of fe25519.h and of the point formulas (tests/test_gpu_limb_bounds.py,
// tests/test_gpu_points.py). Each op calls the production function directly.
//   in : words 0..35   four operands a, b, c, d as raw limbs (9 words each, used unmasked)
//        word  36      parameter
//        words 40..47  encoding of P, words 48..55 encoding of Q (point ops)
//   out: words 0..35   raw limbs of the result (field ops: words 0..8; point ops: X, Y, Z, T)
//        word  36      flags
//        words 40..47  the canonical value (fe_to_words) / the compressed point
//        words 48..56  point additions: raw limbs of cached(Q).YpX as used
// Field ops (flags only for 72: bit 0 fe_is_zero(a), 1 fe_is_negative(a), 2 fe_eq(a, b)):
//   64 fe_mul(a, b)   65 fe_sq(a)   66 fe_mul_small(a, parameter)   67 fe_add   68 fe_addn
//   69 fe_sub   70 fe_neg(a)   71 fe_normalize(a)   72 fe_canon(a), out words 40..47 fe_to_words(a)
//   73 fe_sqn(a, parameter)   74 fe_invert(a)   75 feq_mul   76 feq_sqn(a, parameter)
//   77 fer_mul   78 fer_sqn(a, parameter)   79 r4::carry(a)   80 r4::addn   81 r4::sub
//   82 fe_mul<MulOrder::split>(a, b), the bucket kernel's order (64 is the default, chained)
//   83 a * b^parameter by fe_mul<MulOrder::split>(r, r, b) in place
// Point ops: P = (a, b, c, d) raw when parameter bit 11 is set, else the decoded P encoding;
// Q is the decoded Q encoding (parameter bits 8..9 = 0), P itself (1) or P's (Y, X, T, Z) (2).
// Parameter bits 0..7: P is doubled that many times first; bit 12: Q = p3_neg(Q) first;
// bit 10: the table entry of Q is negated (cached_cneg / precomp_cneg; quad and row forms: -Q);
// bit 13 (96..98): words 0..35 are the p1p1 result's raw limbs instead of the p3's.
//   96 p2_dbl + p1p1_to_p3   97 p3_to_cached + p3_add_cached   98 p3_add_precomp (Q with Z = 1)
//   99 qp_dbl   100 qp_add   101 qp_in_torsion (flag bit 3; the result is P)
//   102 r4::dbl   103 r4::addp
// flags: bit 0 p3_is_identity(result), bit 1 / 2 P / Q decoded.
// As in k_selftest, every lane of a quad (75, 76, 99..101), of a 16-lane row (77..81) or of a
// wave (102, 103) must carry the same input row; all 64 lanes stay active.
__global__ void __launch_bounds__(64) k_selftest_wide(int op, const uint32_t* __restrict__ in, uint32_t n,
                                                      uint32_t* __restrict__ out) {
  const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t* x = in + 64 * (size_t)(gid < n ? gid : n - 1);
  fe f[4], extra;
#pragma unroll
  for (int k = 0; k < 4; k++)
#pragma unroll
    for (int i = 0; i < 9; i++) f[k].v[i] = x[9 * k + i];
  const uint32_t param = x[36];
  const fe a = f[0], b = f[1];
  uint32_t flags = 0, ow[8];
  fe_set(extra, 0);
  if (op < 96) {
    const int nsq = (int)(param & 0xffu) ? (int)(param & 0xffu) : 1;
    fe r;
    fe_set(r, 0);
    switch (op) {
      case 64: fe_mul(r, a, b); break;
      case 65: fe_sq(r, a); break;
      case 66: fe_mul_small(r, a, param); break;
      case 67: fe_add(r, a, b); break;
      case 68: fe_addn(r, a, b); break;
      case 69: fe_sub(r, a, b); break;
      case 70: fe_neg(r, a); break;
      case 71: r = a; fe_normalize(r); break;
      case 72:
        fe_canon(r, a);
        flags = (fe_is_zero(a) ? 1u : 0u) | (fe_is_negative(a) ? 2u : 0u) | (fe_eq(a, b) ? 4u : 0u);
        break;
      case 73: fe_sqn(r, a, nsq); break;
      case 74: fe_invert(r, a); break;
      case 75: {
        feq qa, qb, qr;
        feq_from_fe(qa, a);
        feq_from_fe(qb, b);
        feq_mul(qr, qa, qb);
        fe_from_feq(r, qr);
        break;
      }
      case 76: {
        feq qa, qr;
        feq_from_fe(qa, a);
        feq_sqn(qr, qa, nsq);
        fe_from_feq(r, qr);
        break;
      }
      case 77: {
        fer ra, rb, rr;
        fer_from_fe(ra, a);
        fer_from_fe(rb, b);
        fer_mul(rr, ra, rb, r16::consts());
        fe_from_fer(r, rr);
        break;
      }
      case 78: {
        fer ra, rr;
        fer_from_fe(ra, a);
        fer_sqn(rr, ra, nsq, r16::consts());
        fe_from_fer(r, rr);
        break;
      }
      case 79: case 80: case 81: {
        const r16::Consts K = r16::consts();
        fer ra, rb, rr;
        fer_from_fe(ra, a);
        fer_from_fe(rb, b);
        rr = op == 79 ? r4::carry(ra.v, K) : (op == 80 ? r4::addn(ra, rb, K) : r4::sub(ra, rb, K));
        fe_from_fer(r, rr);
        break;
      }
      case 82: fe_mul<MulOrder::split>(r, a, b); break;
      case 83:  // in place, the result an operand of the next call
        r = a;
#pragma unroll 1
        for (int i = 0; i < nsq; i++) fe_mul<MulOrder::split>(r, r, b);
        break;
      default: break;
    }
    if (op == 72) fe_to_words(ow, a);
    else fe_to_words(ow, r);
    f[0] = r;
    fe_set(f[1], 0);
    fe_set(f[2], 0);
    fe_set(f[3], 0);
  } else {
    const int kdbl = (int)(param & 0xffu);
    const uint32_t qmode = (param >> 8) & 3u;
    const bool neg = (param >> 10) & 1u, raw = (param >> 11) & 1u, qneg = (param >> 12) & 1u;
    p3 P, Q, R;
    bool okP, okQ;
    {
      uint32_t ep[8], eq[8];
#pragma unroll
      for (int i = 0; i < 8; i++) {
        ep[i] = x[40 + i];
        eq[i] = x[48 + i];
      }
      decompress_x2(P, okP, ep, Q, okQ, eq);
    }
    fe_cmov(P.X, f[0], raw);
    fe_cmov(P.Y, f[1], raw);
    fe_cmov(P.Z, f[2], raw);
    fe_cmov(P.T, f[3], raw);
    {
      const p3 P0 = P;
      fe_cmov(Q.X, P0.X, qmode == 1);
      fe_cmov(Q.Y, P0.Y, qmode == 1);
      fe_cmov(Q.Z, P0.Z, qmode == 1);
      fe_cmov(Q.T, P0.T, qmode == 1);
      fe_cmov(Q.X, P0.Y, qmode == 2);
      fe_cmov(Q.Y, P0.X, qmode == 2);
      fe_cmov(Q.Z, P0.T, qmode == 2);
      fe_cmov(Q.T, P0.Z, qmode == 2);
    }
    if (qneg) p3_neg(Q, Q);
    R = P;
    switch (op) {
      case 96: case 97: case 98: {
        p1p1 t;
#pragma unroll 1
        for (int i = 0; i < kdbl; i++) {
          p3_dbl(t, P);
          p1p1_to_p3(P, t);
        }
        if (op == 96) {
          p2 h;
          h.X = P.X; h.Y = P.Y; h.Z = P.Z;
          p2_dbl(t, h);
        } else if (op == 97) {
          cached c;
          p3_to_cached(c, Q);
          cached_cneg(c, neg);
          extra = c.YpX;
          p3_add_cached(t, P, c);
        } else {
          fe d2;
          fe_const(d2, K_D2);
          precomp c;  // Q has Z = 1: (y + x, y - x, 2dxy)
          fe_add(c.ypx, Q.Y, Q.X);
          fe_sub(c.ymx, Q.Y, Q.X);
          fe_mul(c.xy2d, Q.T, d2);
          precomp_cneg(c, neg);
          extra = c.ypx;
          p3_add_precomp(t, P, c);
        }
        p1p1_to_p3(R, t);
        if ((param >> 13) & 1u) {  // the completed point itself: ge25519.h's bounds on p1p1
          R.X = t.X; R.Y = t.Y; R.Z = t.Z; R.T = t.T;
        }
        break;
      }
      case 99: case 100: case 101: {
        const uint32_t c = qlane();
        fe v, w;
        fe_qsel(v, c, P.X, P.Y, P.Z, P.T);
        fe_qsel(w, c, Q.X, Q.Y, Q.Z, Q.T);
        qp_dbl_n(v, kdbl);
        if (op == 99) {
          qp_dbl(v);
        } else if (op == 100) {
          fe nw;
          fe_neg(nw, w);
          fe_cmov(w, nw, neg && (c == 0u || c == 3u));
          qp_add(v, w);
        } else {
          flags |= qp_in_torsion(v) ? 8u : 0u;
        }
        fe_qget<0>(R.X, v);
        fe_qget<1>(R.Y, v);
        fe_qget<2>(R.Z, v);
        fe_qget<3>(R.T, v);
        break;
      }
      case 102: case 103: {
        const r16::Consts K = r16::consts();
        const uint32_t c = r4::row();
        fe vf, wf;
        fe_qsel(vf, c, P.X, P.Y, P.Z, P.T);
        fe_qsel(wf, c, Q.X, Q.Y, Q.Z, Q.T);
        fer v, w;
        fer_from_fe(v, vf);
        fer_from_fe(w, wf);
#pragma unroll 1
        for (int i = 0; i < kdbl; i++) r4::dbl(v, K);
        if (op == 102) {
          r4::dbl(v, K);
        } else {
          fe d2;
          fe_const(d2, K_D2);
          fer d2r, z;
          fer_from_fe(d2r, d2);
          z.v = 0;
          const fer nw = r4::sub(z, w, K);
          w.v = neg && (c == 0u || c == 3u) ? nw.v : w.v;
          r4::addp(v, w, d2r, K);
        }
        fe_from_fer(R.X, r4::get<0>(v));
        fe_from_fer(R.Y, r4::get<1>(v));
        fe_from_fer(R.Z, r4::get<2>(v));
        fe_from_fer(R.T, r4::get<3>(v));
        break;
      }
      default: break;
    }
    flags |= (p3_is_identity(R) ? 1u : 0u) | (okP ? 2u : 0u) | (okQ ? 4u : 0u);
    p3_compress(ow, R);
    f[0] = R.X; f[1] = R.Y; f[2] = R.Z; f[3] = R.T;
  }
  if (gid >= n) return;
  uint32_t* o = out + 64 * (size_t)gid;
#pragma unroll
  for (int k = 0; k < 4; k++)
#pragma unroll
    for (int i = 0; i < 9; i++) o[9 * k + i] = f[k].v[i];
  o[36] = flags;
  o[37] = o[38] = o[39] = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) o[40 + i] = ow[i];
#pragma unroll
  for (int i = 0; i < 9; i++) o[48 + i] = extra.v[i];
#pragma unroll
  for (int i = 57; i < 64; i++) o[i] = 0;
}

// The scalar layer (scalar25519.h) function by function (ops >= 112, 64-word rows as above;
// tests/test_gpu_scalars.py against tests/scalar_model.py). Each op calls the production function
// and nothing else; output words not named are zero. Word 36 of a row is the parameter.
//   112 sc_muladd(a, b, c)   in : words 0..7 a, 8..15 b, 16..23 c          out: words 0..7
//   113 sc_reduce512(x)      in : words 0..15 x                            out: words 0..7
//   114 sc_is_canonical(s)   in : words 0..7 s                             out: word 0 (0 / 1)
//   115 sc_recode16_128(x)   in : words 0..3 x                             out: words 0..3, packed
//   116 sc_halfsize(k)       in : words 0..7 k                             out: words 0..3 c, word 4 c_neg, words 8..11 d
//   117 shl_var(x, s)        in : words 0..7 x, parameter s (0..255)       out: words 0..7 shl_var<8>(x, s),
//                                                                               words 8..11 shl_var<4>(x[0..3], s)
//   118 len256(x)            in : words 0..7 x                             out: word 0
//   119 digits               in : words 0..7 sd, 8..15 kd (packed)         out: parameter 0: words 0..31 digit256(sd, i);
//                                                                               parameter 1: words 0..63 digit16(kd, i)
//                                                                               (sign-extended to 32 bits)
// One lane per row, no lane looks at another's.
__global__ void __launch_bounds__(64) k_selftest_scalar(int op, const uint32_t* __restrict__ in, uint32_t n,
                                                        uint32_t* __restrict__ out) {
  const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= n) return;
  const uint32_t* row = in + 64 * (size_t)gid;
  uint32_t x[24], y[64];
#pragma unroll
  for (int i = 0; i < 24; i++) x[i] = row[i];
#pragma unroll
  for (int i = 0; i < 64; i++) y[i] = 0;
  const uint32_t param = row[36];
  uint32_t* o = out + 64 * (size_t)gid;
  switch (op) {
    case 112: sc_muladd(y, x, x + 8, x + 16); break;
    case 113: sc_reduce512(y, x); break;
    case 114: y[0] = sc_is_canonical(x) ? 1u : 0u; break;
    case 115: sc_recode16_128(y, x); break;
    case 116: {
      uint32_t c[4], d[4];
      bool neg;
      sc_halfsize(c, neg, d, x);
#pragma unroll
      for (int i = 0; i < 4; i++) {
        y[i] = c[i];
        y[8 + i] = d[i];
      }
      y[4] = neg ? 1u : 0u;
      break;
    }
    case 117: {
      uint32_t a8[8], r8[8], a4[4], r4w[4];
#pragma unroll
      for (int i = 0; i < 8; i++) a8[i] = x[i];
#pragma unroll
      for (int i = 0; i < 4; i++) a4[i] = x[i];
      shl_var<8>(r8, a8, (int)(param & 0xffu));
      shl_var<4>(r4w, a4, (int)(param & 0xffu));
#pragma unroll
      for (int i = 0; i < 8; i++) y[i] = r8[i];
#pragma unroll
      for (int i = 0; i < 4; i++) y[8 + i] = r4w[i];
      break;
    }
    case 118: y[0] = (uint32_t)len256(x); break;
    case 119: {  // the digit index stays a run-time value, as in the callers' loops
      const int nd = (param & 1u) ? 64 : 32;
#pragma unroll 1
      for (int i = 0; i < 64; i++)
        o[i] = i >= nd ? 0u : (uint32_t)((param & 1u) ? digit16(x + 8, i) : digit256(x, i));
      return;
    }
    default: break;
  }
#pragma unroll
  for (int i = 0; i < 64; i++) o[i] = y[i];
}

// The number of invalid signatures (status MV_SIG_INVALID: the failures a combined equation
// can see; s >= l and undecodable points are excluded from it exactly) of n statuses, added to
// *count (zeroed by the launcher): the single-path feedback of the batch policy (engine.cpp
// enqueue_batch), one atomic per wave. 256 threads x 16 bytes per thread per block.
__global__ void __launch_bounds__(256) k_count_rejects(const uint8_t* __restrict__ status, uint32_t n,
                                                       uint32_t* __restrict__ count) {
  const uint32_t base = (blockIdx.x * 256 + threadIdx.x) * 16;
  uint32_t c = 0;
  if (base + 16 <= n) {
    const uint4 w = *reinterpret_cast<const uint4*>(status + base);
    const uint32_t x[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
      // bytes equal to 1 -> y's zero bytes; nonzero bytes of y get their high bit set
      const uint32_t y = x[k] ^ 0x01010101u;
      const uint32_t nz = (((y & 0x7f7f7f7fu) + 0x7f7f7f7fu) | y) & 0x80808080u;
      c += 4u - (uint32_t)__builtin_popcount(nz);
    }
  } else {
    for (uint32_t i = base; i < n && i < base + 16; i++) c += status[i] == MV_SIG_INVALID;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) c += (uint32_t)__shfl_xor((int)c, m);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, c);
}

}  // namespace mv

// ---------------------------------------------------------------- launchers
namespace mvk {

hipError_t launch_count_rejects(const uint8_t* status, uint32_t n, uint32_t* count, hipStream_t s) {
  hipError_t e = hipMemsetAsync(count, 0, sizeof(uint32_t), s);
  if (e != hipSuccess || n == 0) return e;
  hipLaunchKernelGGL(mv::k_count_rejects, dim3((n + 4095) / 4096), dim3(256), 0, s, status, n, count);
  return hipGetLastError();
}

size_t verify_scratch_bytes(uint32_t n) {
  size_t waves = (size_t)((n + 255) / 256) * 4;  // every wave of the 256-thread grid owns a slot
  return waves * mv::WAVE_QUADS * 64 * sizeof(uint4);
}
size_t btable_bytes() { return 2 * mv::BT_TABLE * sizeof(uint4); }

hipError_t launch_btable_init(void* d_btab, hipStream_t s) {
  hipLaunchKernelGGL(mv::k_btable_init, dim3(2), dim3(256), 0, s, (uint4*)d_btab);
  return hipGetLastError();
}
hipError_t launch_verify(const uint8_t* msg, const uint8_t* sig, const uint8_t* pk, const uint32_t* key_idx, uint32_t n,
                         const void* btab, void* scratch, uint8_t* status, hipStream_t s, const uint32_t* skip,
                         uint32_t skip_group, const void* prep_pts, const void* prep_comb) {
  if (n == 0) return hipSuccess;
  const mv::PrepView pv{static_cast<const uint4*>(prep_pts), n, static_cast<const uint4*>(prep_comb)};
  hipLaunchKernelGGL(mv::k_verify, dim3((n + 255) / 256), dim3(256), 0, s, msg, sig, pk, key_idx, n,
                     (const uint4*)btab, (uint4*)scratch, status, skip, skip_group, pv);
  return hipGetLastError();
}
hipError_t launch_sign(const uint8_t* seed, const uint8_t* msg, uint32_t n, const void* btab, uint8_t* pk,
                       uint8_t* sig, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(mv::k_sign, dim3((n + 255) / 256), dim3(256), 0, s, seed, msg, n, (const uint4*)btab, pk, sig);
  return hipGetLastError();
}
// BLAKE2b launchers: four lanes per string on small calls (blake2b_quad.hip), one lane per
// string at batch size (blake2b_lane.hip)
hipError_t launch_blake2b(const Knobs& kn, const uint8_t* buf, const uint64_t* off, const uint64_t* len, uint32_t n,
                          uint8_t* out, hipStream_t s) {
  return launch_blake2b_quad(kn, buf, off, len, n, out, s);
}
hipError_t launch_block_hash(const Knobs& kn, const uint8_t* buf, const uint64_t* off, const uint64_t* len,
                             uint32_t n, uint8_t* msg_out, uint8_t* dig_out, hipStream_t s) {
  return launch_block_hash_quad(kn, buf, off, len, n, msg_out, dig_out, s);
}
hipError_t launch_selftest(int op, const uint32_t* in, uint32_t n, const void* btab, uint32_t* out, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(mv::k_selftest, dim3((n + 63) / 64), dim3(64), 0, s, op, in, n, (const uint4*)btab, out);
  return hipGetLastError();
}
hipError_t launch_selftest_wide(int op, const uint32_t* in, uint32_t n, uint32_t* out, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (op >= SELFTEST_SCALAR_OP) {
    hipLaunchKernelGGL(mv::k_selftest_scalar, dim3((n + 63) / 64), dim3(64), 0, s, op, in, n, out);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(mv::k_selftest_wide,dim3((n + 63) / 64), dim3(64), 0, s, op, in, n, out);
  return hipGetLastError();
}

}  // namespace mvk
