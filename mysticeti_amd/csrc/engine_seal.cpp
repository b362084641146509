// mv_seal_blocks / mv_dev_seal_blocks: the host side of seal.hip. One call = the key expansion,
// the scan, and then either one step over every block (unlinked) or, under MV_SEAL_LINK, the
// heads read back once, the order check, the (authority, round) -> block table, and one step per
// distinct round.
#include <algorithm>
#include <cstring>
#include <vector>

#include "engine_internal.h"

using namespace mvi;

namespace {

constexpr uint64_t kNoHead = ~0ull;

// The table of a linked call from the scan's heads (2 words per block: authority, round; all
// ones: a parse error). Keys: the blocks whose authority < n_auth, the lowest index per key.
struct HostTable {
  std::vector<uint32_t> slots;  // 4 words per slot
  uint32_t mask = 0, max_probe = 0;
};
HostTable build_table(const uint64_t* heads, uint32_t n, uint32_t n_auth) {
  HostTable t;
  uint64_t keys = 0;
  for (uint32_t i = 0; i < n; i++) keys += heads[2 * (size_t)i] < n_auth;
  uint64_t cap = 16;
  while (cap < 2 * keys) cap <<= 1;
  t.mask = (uint32_t)(cap - 1);
  t.slots.assign(4 * cap, 0xffffffffu);
  for (uint32_t i = 0; i < n; i++) {
    const uint64_t a = heads[2 * (size_t)i], r = heads[2 * (size_t)i + 1];
    if (a >= n_auth) continue;
    uint32_t h = mvk::seal_table_hash(a, r) & t.mask, probe = 0;
    for (;; h = (h + 1) & t.mask, probe++) {
      uint32_t* s = &t.slots[4 * (size_t)h];
      if (s[3] == 0xffffffffu) {
        s[0] = (uint32_t)r, s[1] = (uint32_t)(r >> 32), s[2] = (uint32_t)a, s[3] = i;
        t.max_probe = std::max(t.max_probe, probe);
        break;
      }
      if (s[0] == (uint32_t)r && s[1] == (uint32_t)(r >> 32) && s[2] == (uint32_t)a) break;  // a lower index holds it
    }
  }
  return t;
}

// The expanded keys are secrets (scalar and prefix): zeroed behind the call's last step, then the
// synchronise every path of seal_run ends on.
mv_status wipe_keys(mv_ctx* ctx, Device::Seal& q, hipStream_t s) {
  hipError_t e = hipMemsetAsync(q.keys.p, 0, q.keys.cap, s);
  const hipError_t e2 = hipStreamSynchronize(s);
  if (e == hipSuccess) e = e2;
  HIPCHK(ctx, e);
  return MV_OK;
}

}  // namespace

// One call on device arrays, on stream s, which it synchronises. d_md / d_bd may be null.
mv_status mvi::seal_run(mv_ctx* ctx, Device& dev, uint8_t* d_buf, uint64_t buf_bytes, const uint64_t* d_off,
                   const uint64_t* d_len, uint32_t n, const uint8_t* d_seeds, uint32_t n_auth, uint32_t flags,
                   uint8_t* d_status, uint8_t* d_md, uint8_t* d_bd, hipStream_t s) {
  Device::Seal& q = dev.seal;
  HIPCHK(ctx, q.keys.ensure(96 * (size_t)std::max<uint32_t>(n_auth, 1)));
  HIPCHK(ctx, q.heads.ensure(16 * (size_t)n));
  if (!d_md) {
    HIPCHK(ctx, q.md.ensure(32 * (size_t)n));
    d_md = q.md.as<uint8_t>();
  }
  if (!d_bd) {
    HIPCHK(ctx, q.bd.ensure(32 * (size_t)n));
    d_bd = q.bd.as<uint8_t>();
  }
  HIPCHK(ctx, hipMemsetAsync(d_md, 0, 32 * (size_t)n, s));
  HIPCHK(ctx, hipMemsetAsync(d_bd, 0, 32 * (size_t)n, s));
  HIPCHK(ctx, mvk::launch_seal_keys(d_seeds, n_auth, dev.tab.btab.p, q.keys.as<uint32_t>(), s));
  HIPCHK(ctx, mvk::launch_seal_scan(d_buf, buf_bytes, d_off, d_len, n, n_auth, d_status, q.heads.as<uint64_t>(), s));
  if (!(flags & MV_SEAL_LINK)) {
    HIPCHK(ctx, mvk::launch_seal_level(d_buf, buf_bytes, d_off, d_len, 0, n, q.keys.as<uint32_t>(), dev.tab.btab.p,
                                       mvk::SealTable{nullptr, 0, 0}, d_status, d_md, d_bd, s));
    return wipe_keys(ctx, q, s);
  }
  // the heads, once: order, table, steps
  HIPCHK(ctx, q.h.ensure(16 * (size_t)n));
  const uint64_t* heads = q.h.as<uint64_t>();
  HIPCHK(ctx, hipMemcpyAsync(q.h.p, q.heads.p, 16 * (size_t)n, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  std::vector<uint32_t> cut;  // the first block of every step, then n
  bool have = false;
  uint64_t cur = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (heads[2 * (size_t)i] == kNoHead && heads[2 * (size_t)i + 1] == kNoHead) continue;
    const uint64_t r = heads[2 * (size_t)i + 1];
    if (have && r < cur) {
      (void)wipe_keys(ctx, q, s);
      return set_err(ctx, MV_E_INVALID_ARG, "MV_SEAL_LINK: blocks not in non-decreasing round order");
    }
    if (!have || r != cur) cut.push_back(have ? i : 0);
    have = true;
    cur = r;
  }
  if (!have) return wipe_keys(ctx, q, s);  // nothing parses: the scan's statuses are the result
  cut.push_back(n);
  const HostTable t = build_table(heads, n, n_auth);
  HIPCHK(ctx, q.tab.ensure(4 * t.slots.size()));
  HIPCHK(ctx, hipMemcpyAsync(q.tab.p, t.slots.data(), 4 * t.slots.size(), hipMemcpyHostToDevice, s));
  const mvk::SealTable st{q.tab.p, t.mask, t.max_probe};
  for (size_t k = 0; k + 1 < cut.size(); k++)
    HIPCHK(ctx, mvk::launch_seal_level(d_buf, buf_bytes, d_off, d_len, cut[k], cut[k + 1], q.keys.as<uint32_t>(),
                                       dev.tab.btab.p, st, d_status, d_md, d_bd, s));
  return wipe_keys(ctx, q, s);  // (its synchronise also ends the copy of t.slots, which is pageable)
}

namespace {

bool seal_args_ok(const void* buf, const void* off, const void* len, uint32_t n, const void* seeds, uint32_t n_auth,
                  uint32_t flags, const void* status) {
  if (flags & ~MV_SEAL_LINK) return false;
  if (n_auth > kMaxSealAuth || (n_auth && !seeds)) return false;
  return n == 0 || (buf && off && len && status);
}

}  // namespace

extern "C" {

mv_status mv_seal_blocks(mv_ctx* ctx, uint8_t* buf, const uint64_t* off, const uint64_t* len, uint32_t n,
                         const uint8_t* seeds, uint32_t n_auth, uint32_t flags, uint8_t* status, uint8_t* msg_digest,
                         uint8_t* block_digest) {
  if (!ctx || !seal_args_ok(buf, off, len, n, seeds, n_auth, flags, status))
    return set_err(ctx, MV_E_INVALID_ARG, "bad seal args");
  if (n == 0) return MV_OK;
  // the span of the blocks: staged as one image, so gaps travel with it (and come back unread)
  uint64_t lo = ~0ull, hi = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (off[i] + len[i] < off[i]) return set_err(ctx, MV_E_INVALID_ARG, "seal: a block's span overflows");
    lo = std::min(lo, off[i]);
    hi = std::max(hi, off[i] + len[i]);
  }
  const uint64_t span = hi - lo;
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device& dev = ctx->devs[0];
  Device::Seal& q = dev.seal;
  hipStream_t s = dev.stream;
  HIPCHK(ctx, hipSetDevice(dev.id));
  HIPCHK(ctx, q.in.ensure(span + 16));
  HIPCHK(ctx, q.ol.ensure(16 * (size_t)n));
  HIPCHK(ctx, q.st.ensure(n));
  HIPCHK(ctx, q.seeds.ensure(32 * (size_t)std::max<uint32_t>(n_auth, 1)));
  HIPCHK(ctx, q.md.ensure(32 * (size_t)n));
  HIPCHK(ctx, q.bd.ensure(32 * (size_t)n));
  std::vector<uint64_t> ol(2 * (size_t)n);
  for (uint32_t i = 0; i < n; i++) {
    ol[i] = off[i] - lo;
    ol[(size_t)n + i] = len[i];
  }
  uint8_t* d_in = q.in.as<uint8_t>();
  if (span) HIPCHK(ctx, hipMemcpyAsync(d_in, buf + lo, span, hipMemcpyHostToDevice, s));
  HIPCHK(ctx, hipMemsetAsync(d_in + span, 0, 16, s));
  HIPCHK(ctx, hipMemcpyAsync(q.ol.p, ol.data(), 16 * (size_t)n, hipMemcpyHostToDevice, s));
  if (n_auth) HIPCHK(ctx, hipMemcpyAsync(q.seeds.p, seeds, 32 * (size_t)n_auth, hipMemcpyHostToDevice, s));
  HIPCHK(ctx, hipStreamSynchronize(s));  // (pageable sources: ol goes out of use only after the copies)
  const mv_status rc = seal_run(ctx, dev, d_in, span, q.ol.as<uint64_t>(), q.ol.as<uint64_t>() + n, n,
                                q.seeds.as<uint8_t>(), n_auth, flags, q.st.as<uint8_t>(), q.md.as<uint8_t>(),
                                q.bd.as<uint8_t>(), s);
  // the device copy of the seeds goes with the keys (the copies below synchronise behind it)
  const hipError_t we = hipMemsetAsync(q.seeds.p, 0, q.seeds.cap, s);
  if (rc != MV_OK) {  // (rounds out of order: no step ran, the caller's buffer is as it was)
    (void)hipStreamSynchronize(s);
    return rc;
  }
  HIPCHK(ctx, we);
  HIPCHK(ctx, hipMemcpyAsync(status, q.st.p, n, hipMemcpyDeviceToHost, s));
  if (msg_digest) HIPCHK(ctx, hipMemcpyAsync(msg_digest, q.md.p, 32 * (size_t)n, hipMemcpyDeviceToHost, s));
  if (block_digest) HIPCHK(ctx, hipMemcpyAsync(block_digest, q.bd.p, 32 * (size_t)n, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  // the sealed blocks' bytes come back, and nothing else: runs of sealed blocks that lie back to
  // back (a packed corpus is one run) in one copy each
  for (uint32_t i = 0; i < n;) {
    if (status[i] != MV_SEAL_OK || len[i] == 0) {
      i++;
      continue;
    }
    uint32_t j = i + 1;
    uint64_t end = off[i] + len[i];
    while (j < n && status[j] == MV_SEAL_OK && off[j] == end) end += len[j++];
    HIPCHK(ctx, hipMemcpyAsync(buf + off[i], d_in + (off[i] - lo), end - off[i], hipMemcpyDeviceToHost, s));
    i = j;
  }
  HIPCHK(ctx, hipStreamSynchronize(s));
  return MV_OK;
}

mv_status mv_dev_seal_blocks(mv_ctx* ctx, int device, uint8_t* d_buf, uint64_t buf_bytes, const uint64_t* d_off,
                             const uint64_t* d_len, uint32_t n, const uint8_t* d_seeds, uint32_t n_auth,
                             uint32_t flags, uint8_t* d_status, uint8_t* d_msg_digest, uint8_t* d_block_digest,
                             void* stream) {
  if (!ctx || !seal_args_ok(d_buf, d_off, d_len, n, d_seeds, n_auth, flags, d_status))
    return set_err(ctx, MV_E_INVALID_ARG, "bad seal args");
  if (((uintptr_t)d_buf | (uintptr_t)d_off | (uintptr_t)d_len | (uintptr_t)d_msg_digest | (uintptr_t)d_block_digest) & 7 ||
      ((uintptr_t)d_seeds & 3))
    return set_err(ctx, MV_E_INVALID_ARG, "seal: misaligned device pointer");
  if (n == 0) return MV_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device* dev = find_dev(ctx, device);
  if (!dev || dev != &ctx->devs[0]) return set_err(ctx, MV_E_NO_DEVICE, "seal runs on the context's first device");
  HIPCHK(ctx, hipSetDevice(dev->id));
  hipStream_t s = stream ? (hipStream_t)stream : (hipStream_t)dev->stream;
  return seal_run(ctx, *dev, d_buf, buf_bytes, d_off, d_len, n, d_seeds, n_auth, flags, d_status, d_msg_digest,
                  d_block_digest, s);
}

}  // extern "C"
