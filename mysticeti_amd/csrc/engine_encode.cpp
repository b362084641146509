// mv_encode_blocks / mv_dev_encode_blocks: the host side of encode.hip. One call = the payload check
// and the scan of the bodies, the sizes and the scan of the padded lengths, the total read back (the
// one synchronise of a call that does not seal), then -- if the total fits cap -- the bytes, and with
// MV_ENCODE_SEAL engine_seal.cpp's seal_run over the image in place.
#include <algorithm>
#include <cstring>
#include <vector>

#include "engine_internal.h"

using namespace mvi;

namespace {

constexpr uint64_t kMaxPayloads = 0xffffffffull;
constexpr uint32_t kMaxBlocks = 0x7fffffffu;  // a workgroup per block has to fit a grid

struct SealOut {
  const uint8_t* d_seeds;
  uint32_t n_auth;
  uint8_t *d_status, *d_md, *d_bd;
};

// The control words read back on s, which is synchronised. A bounds check that failed in this call
// or in the device-buffer call before it (whose bytes were written after it returned) is MV_E_HIP;
// the word is cleared.
mv_status read_encode_ctl(mv_ctx* ctx, Device::Encode& q, hipStream_t s, uint64_t* total, uint64_t* nbig = nullptr) {
  HIPCHK(ctx, hipMemcpyAsync(q.h_ctl.p, q.ctl.p, 8 * mvk::EN_CTL_WORDS, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  const uint64_t* w = q.h_ctl.as<uint64_t>();
  if (total) *total = w[mvk::EN_CTL_TOTAL];
  if (nbig) *nbig = w[mvk::EN_CTL_NBIG];
  if (w[mvk::EN_CTL_ERR]) {
    HIPCHK(ctx, hipMemsetAsync(q.ctl.as<uint64_t>() + mvk::EN_CTL_ERR, 0, 8, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return set_err(ctx, MV_E_HIP, "encode: a bounds check failed on the device");
  }
  return MV_OK;
}

// One call on device arrays (c: the caller's, the scratch is filled in here), on stream s.
// finish: synchronise behind the bytes and report their bounds checks now (the host-buffer call);
// without it a call that does not seal returns with the bytes enqueued.
mv_status encode_run(mv_ctx* ctx, Device& dev, mvk::EncodeCall c, uint32_t flags, const SealOut& so, hipStream_t s,
                     bool finish, uint64_t* out_bytes) {
  Device::Encode& q = dev.encode;
  if (q.done_set) HIPCHK(ctx, hipStreamWaitEvent(s, q.done, 0));
  const hipEvent_t guard = q.done_set ? (hipEvent_t)q.done : nullptr;
  const bool fresh = !q.ctl.p;
  HIPCHK(ctx, q.ctl.ensure(8 * mvk::EN_CTL_WORDS, guard));
  HIPCHK(ctx, q.h_ctl.ensure(8 * mvk::EN_CTL_WORDS));
  HIPCHK(ctx, q.pay_ok.ensure(std::max<uint64_t>(c.p, 1), guard));
  HIPCHK(ctx, q.pay_count.ensure(8 * std::max<uint64_t>(c.p, 1), guard));
  HIPCHK(ctx, q.pay_body.ensure(8 * std::max<uint64_t>(c.p, 1), guard));
  HIPCHK(ctx, q.pre.ensure(8 * (c.p + 1), guard));
  HIPCHK(ctx, q.blk_count.ensure(8 * (size_t)c.n, guard));
  HIPCHK(ctx, q.big.ensure(4 * (size_t)c.n, guard));
  HIPCHK(ctx, q.wg.ensure(mvk::wg_scan_bytes(std::max<uint64_t>(c.n, c.p)), guard));
  HIPCHK(ctx, q.done.ensure());
  c.pay_ok = q.pay_ok.as<uint8_t>();
  c.pay_count = q.pay_count.as<uint64_t>();
  c.pay_body = q.pay_body.as<uint64_t>();
  c.pre = q.pre.as<uint64_t>();
  c.blk_count = q.blk_count.as<uint64_t>();
  c.big = q.big.as<uint32_t>();
  uint64_t* ctl = q.ctl.as<uint64_t>();
  // (the error word outlives a call: see read_encode_ctl)
  HIPCHK(ctx, hipMemsetAsync(ctl, 0, fresh ? 8 * mvk::EN_CTL_WORDS : 8 * mvk::EN_CTL_ERR, s));
  HIPCHK(ctx, mvk::launch_encode_check(c, q.wg.p, ctl, s));
  HIPCHK(ctx, mvk::launch_encode_size(c, q.wg.p, ctl, s));
  uint64_t total = 0, nbig = 0;
  const mv_status rc = read_encode_ctl(ctx, q, s, &total, &nbig);
  q.done_set = false;  // (s has been synchronised behind the wait for it)
  if (rc != MV_OK) return rc;
  *out_bytes = total;
  const bool seal = flags & MV_ENCODE_SEAL;
  if (total > c.cap) {  // nothing is written and nothing sealed
    if (seal) {
      HIPCHK(ctx, hipMemsetAsync(so.d_status, MV_SEAL_PARSE_ERROR, c.n, s));
      if (so.d_md) HIPCHK(ctx, hipMemsetAsync(so.d_md, 0, 32 * (size_t)c.n, s));
      if (so.d_bd) HIPCHK(ctx, hipMemsetAsync(so.d_bd, 0, 32 * (size_t)c.n, s));
    }
    if (finish) HIPCHK(ctx, hipStreamSynchronize(s));
    return MV_OK;
  }
  HIPCHK(ctx, mvk::launch_encode_write(c, nbig, ctl, s));
  if (seal) {
    // a block that is not MV_ENCODE_OK is an empty span: MV_SEAL_PARSE_ERROR, no head, no key
    const mv_status src = seal_run(ctx, dev, c.out, total, c.out_off, c.out_len, c.n, so.d_seeds, so.n_auth,
                                   (flags & MV_ENCODE_LINK) ? MV_SEAL_LINK : 0, so.d_status, so.d_md, so.d_bd, s);
    const mv_status erc = read_encode_ctl(ctx, q, s, nullptr);
    return erc != MV_OK ? erc : src;
  }
  if (finish) return read_encode_ctl(ctx, q, s, nullptr);
  HIPCHK(ctx, hipEventRecord(q.done, s));
  q.done_set = true;
  return MV_OK;
}

bool encode_args_ok(const void* heads, uint32_t n, const void* includes, uint64_t m, const void* payload_buf,
                    uint64_t payload_bytes, const void* payload_off, const void* payload_len, uint64_t p, uint32_t flags,
                    const void* seeds, uint32_t n_auth, const void* out, uint64_t cap, const void* out_off,
                    const void* out_len, const void* status, const void* out_bytes, const void* seal_status) {
  if (flags & ~(MV_ENCODE_SEAL | MV_ENCODE_LINK)) return false;
  if ((flags & MV_ENCODE_LINK) && !(flags & MV_ENCODE_SEAL)) return false;
  if (!out_bytes || p > kMaxPayloads || n > kMaxBlocks) return false;
  if (m > ~0ull / 48 || payload_bytes > ~0ull - 64 || cap > ~0ull - 64) return false;
  if ((m && !includes) || (payload_bytes && !payload_buf) || (p && (!payload_off || !payload_len)) || (cap && !out))
    return false;
  if (n && (!heads || !out_off || !out_len || !status)) return false;
  if (flags & MV_ENCODE_SEAL) {
    if (n_auth > kMaxSealAuth || (n_auth && !seeds) || (n && !seal_status)) return false;
  }
  return true;
}

}  // namespace

extern "C" {

mv_status mv_encode_blocks(mv_ctx* ctx, const uint64_t* heads, uint32_t n, const uint64_t* includes, uint64_t m,
                           const uint8_t* payload_buf, uint64_t payload_bytes, const uint64_t* payload_off,
                           const uint64_t* payload_len, uint64_t p, uint32_t flags, const uint8_t* seeds, uint32_t n_auth,
                           uint8_t* out, uint64_t cap, uint64_t* out_off, uint64_t* out_len, uint8_t* status,
                           uint64_t* out_bytes, uint8_t* seal_status, uint8_t* msg_digest, uint8_t* block_digest) {
  if (!ctx || !encode_args_ok(heads, n, includes, m, payload_buf, payload_bytes, payload_off, payload_len, p, flags, seeds,
                              n_auth, out, cap, out_off, out_len, status, out_bytes, seal_status))
    return set_err(ctx, MV_E_INVALID_ARG, "bad encode args");
  *out_bytes = 0;
  if (n == 0) return MV_OK;
  const bool seal = flags & MV_ENCODE_SEAL;
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device& dev = ctx->devs[0];
  Device::Encode& q = dev.encode;
  Device::Seal& sq = dev.seal;
  hipStream_t s = dev.stream;
  HIPCHK(ctx, hipSetDevice(dev.id));
  HIPCHK(ctx, q.heads.ensure(80 * (size_t)n));
  HIPCHK(ctx, q.inc.ensure(std::max<uint64_t>(48 * m, 8)));
  HIPCHK(ctx, q.pay.ensure(payload_bytes + 16));
  HIPCHK(ctx, q.pol.ensure(std::max<uint64_t>(16 * p, 8)));
  HIPCHK(ctx, q.out.ensure(cap + 16));
  HIPCHK(ctx, q.ool.ensure(16 * (size_t)n));
  HIPCHK(ctx, q.st.ensure(n));
  if (seal) {
    HIPCHK(ctx, q.sst.ensure(n));
    HIPCHK(ctx, sq.seeds.ensure(32 * (size_t)std::max<uint32_t>(n_auth, 1)));
    HIPCHK(ctx, sq.md.ensure(32 * (size_t)n));
    HIPCHK(ctx, sq.bd.ensure(32 * (size_t)n));
  }
  uint8_t* d_pay = q.pay.as<uint8_t>();
  uint64_t* d_pol = q.pol.as<uint64_t>();
  HIPCHK(ctx, hipMemcpyAsync(q.heads.p, heads, 80 * (size_t)n, hipMemcpyHostToDevice, s));
  if (m) HIPCHK(ctx, hipMemcpyAsync(q.inc.p, includes, 48 * m, hipMemcpyHostToDevice, s));
  if (payload_bytes) HIPCHK(ctx, hipMemcpyAsync(d_pay, payload_buf, payload_bytes, hipMemcpyHostToDevice, s));
  HIPCHK(ctx, hipMemsetAsync(d_pay + payload_bytes, 0, 16, s));  // (payloads are read as whole aligned words)
  if (p) {
    HIPCHK(ctx, hipMemcpyAsync(d_pol, payload_off, 8 * p, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(d_pol + p, payload_len, 8 * p, hipMemcpyHostToDevice, s));
  }
  if (seal && n_auth) HIPCHK(ctx, hipMemcpyAsync(sq.seeds.p, seeds, 32 * (size_t)n_auth, hipMemcpyHostToDevice, s));
  mvk::EncodeCall c{};
  c.heads = q.heads.as<uint64_t>(), c.n = n;
  c.includes = q.inc.as<uint64_t>(), c.m = m;
  c.payload_buf = d_pay, c.payload_bytes = payload_bytes;
  c.payload_off = d_pol, c.payload_len = d_pol + p, c.p = p;
  c.out = q.out.as<uint8_t>(), c.cap = cap;
  c.out_off = q.ool.as<uint64_t>(), c.out_len = q.ool.as<uint64_t>() + n;
  c.status = q.st.as<uint8_t>();
  const SealOut so{sq.seeds.as<uint8_t>(), n_auth, q.sst.as<uint8_t>(), sq.md.as<uint8_t>(), sq.bd.as<uint8_t>()};
  const mv_status rc = encode_run(ctx, dev, c, flags, so, s, true, out_bytes);
  // the device copy of the seeds goes with the keys (the copies below synchronise behind it)
  hipError_t we = hipSuccess;
  if (seal) we = hipMemsetAsync(sq.seeds.p, 0, sq.seeds.cap, s);
  if (rc == MV_E_HIP || rc == MV_E_ALLOC) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  HIPCHK(ctx, we);
  // sizes and verdicts come back whatever became of the bytes
  HIPCHK(ctx, hipMemcpyAsync(status, q.st.p, n, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipMemcpyAsync(out_off, c.out_off, 8 * (size_t)n, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipMemcpyAsync(out_len, c.out_len, 8 * (size_t)n, hipMemcpyDeviceToHost, s));
  if (rc == MV_OK) {
    if (*out_bytes && *out_bytes <= cap) HIPCHK(ctx, hipMemcpyAsync(out, c.out, *out_bytes, hipMemcpyDeviceToHost, s));
    if (seal) {
      HIPCHK(ctx, hipMemcpyAsync(seal_status, q.sst.p, n, hipMemcpyDeviceToHost, s));
      if (msg_digest) HIPCHK(ctx, hipMemcpyAsync(msg_digest, sq.md.p, 32 * (size_t)n, hipMemcpyDeviceToHost, s));
      if (block_digest) HIPCHK(ctx, hipMemcpyAsync(block_digest, sq.bd.p, 32 * (size_t)n, hipMemcpyDeviceToHost, s));
    }
  }
  HIPCHK(ctx, hipStreamSynchronize(s));
  return rc;  // (MV_E_INVALID_ARG: rounds out of order under MV_ENCODE_LINK, `out` as it was)
}

mv_status mv_dev_encode_blocks(mv_ctx* ctx, int device, const uint64_t* d_heads, uint32_t n, const uint64_t* d_includes,
                               uint64_t m, const uint8_t* d_payload_buf, uint64_t payload_bytes,
                               const uint64_t* d_payload_off, const uint64_t* d_payload_len, uint64_t p, uint32_t flags,
                               const uint8_t* d_seeds, uint32_t n_auth, uint8_t* d_out, uint64_t cap, uint64_t* d_out_off,
                               uint64_t* d_out_len, uint8_t* d_status, uint64_t* out_bytes, uint8_t* d_seal_status,
                               uint8_t* d_msg_digest, uint8_t* d_block_digest, void* stream) {
  if (!ctx || !encode_args_ok(d_heads, n, d_includes, m, d_payload_buf, payload_bytes, d_payload_off, d_payload_len, p,
                              flags, d_seeds, n_auth, d_out, cap, d_out_off, d_out_len, d_status, out_bytes, d_seal_status))
    return set_err(ctx, MV_E_INVALID_ARG, "bad encode args");
  if (((uintptr_t)d_heads | (uintptr_t)d_includes | (uintptr_t)d_payload_buf | (uintptr_t)d_payload_off |
       (uintptr_t)d_payload_len | (uintptr_t)d_out | (uintptr_t)d_out_off | (uintptr_t)d_out_len) & 7)
    return set_err(ctx, MV_E_INVALID_ARG, "encode: misaligned device pointer");
  const bool seal = flags & MV_ENCODE_SEAL;
  if (seal && ((((uintptr_t)d_msg_digest | (uintptr_t)d_block_digest) & 7) || ((uintptr_t)d_seeds & 3)))
    return set_err(ctx, MV_E_INVALID_ARG, "encode: misaligned device pointer");
  *out_bytes = 0;
  if (n == 0) return MV_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device* dev = find_dev(ctx, device);
  if (!dev || dev != &ctx->devs[0]) return set_err(ctx, MV_E_NO_DEVICE, "encode runs on the context's first device");
  HIPCHK(ctx, hipSetDevice(dev->id));
  hipStream_t s = stream ? (hipStream_t)stream : (hipStream_t)dev->stream;
  mvk::EncodeCall c{};
  c.heads = d_heads, c.n = n;
  c.includes = d_includes, c.m = m;
  c.payload_buf = d_payload_buf, c.payload_bytes = payload_bytes;
  c.payload_off = d_payload_off, c.payload_len = d_payload_len, c.p = p;
  c.out = d_out, c.cap = cap;
  c.out_off = d_out_off, c.out_len = d_out_len;
  c.status = d_status;
  const SealOut so{d_seeds, n_auth, d_seal_status, d_msg_digest, d_block_digest};
  return encode_run(ctx, *dev, c, flags, so, s, false, out_bytes);
}

}  // extern "C"
