// Host-side launchers for kernels.hip (internal to libmysti_verify.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace mvk {
// The runtime switches. Read from the environment once, at mv_create
// (knobs_from_env in engine.cpp, the only getenv in the library), and stored in the context; the
// diagnostics entry point mv_set_option changes one between calls (the tests select forms that
// way). None changes a verdict, digest or crc. Launchers that choose between kernel forms take
// the context's Knobs as their first argument.
struct Knobs {
  // block path (engine.cpp)
  int64_t blk_pipe = 1;                  // MV_BLK_PIPE: batch-size block calls in two halves on two streams
  int64_t comb_split_bytes = 2048;       // MV_COMB_SPLIT_BYTES: bytes per block from which the split comb path runs
  int64_t hash_in_comb = 1;              // MV_HASH_IN_COMB: online passes hash inside k_verify_comb16
  int64_t ingest_in_comb = 1;            // MV_INGEST_IN_COMB: ... and parse there
  int64_t verdict_fused = 1;             // MV_VERDICT_FUSED: the block verdict inside the comb kernels
  int64_t blk_chunk_bytes = 256ll << 20;  // MV_BLK_CHUNK_BYTES: bytes per host-buffer block chunk
  int64_t pack_threads = 0;              // MV_PACK_THREADS: host threads packing a chunk (0: min(8, cores))
  int64_t blk_trace = 0;                 // MV_BLK_TRACE: host-side timing lines on stderr
  int64_t blk_zerocopy = 1ll << 20;      // MV_BLK_ZEROCOPY: passes up to this size read pinned staging
  int64_t pass_spin = 0;                 // MV_PASS_SPIN: the pass owner polls its event
  int64_t pass_sets = 2;                 // MV_PASS_SETS: submission-queue pass sets (2 .. 4)
  int64_t q_linger_us = 50;              // MV_Q_LINGER_US
  int64_t q_spin_us = 0;                 // MV_Q_SPIN_US
  // the resident online service
  int64_t online = 1;                    // MV_ONLINE: small block calls take the service
  int64_t online_long = 1;               // MV_ONLINE_LONG: long blocks take it too
  int64_t online_prio = 1;               // MV_ONLINE_PRIO: the service stream at the highest priority (its own queue)
  int64_t online_wgs = 0;                // MV_ONLINE_WGS: resident workgroups (0: = CUs)
  int64_t online_idle_us = 10000;        // MV_ONLINE_IDLE_US: the launch ends after this long idle
  int64_t online_trace = 0;              // MV_ONLINE_TRACE: per-stage means on stderr at release
  int64_t online_debug = 0;              // MV_ONLINE_DEBUG: launch lines, long waits on stderr
  int64_t online_inject = 0;             // MV_ONLINE_INJECT: fault injection (tests): launches fail
  int64_t online_spinners = 0;           // MV_ONLINE_SPINNERS: callers spinning on their verdict (0: 1/4 of the CPU share)
  // signature path
  int64_t stream_chunk_log2 = 17;        // MV_STREAM_CHUNK_LOG2: signatures per copy chunk
  int64_t guard_groups = 8;              // MV_GUARD_GROUPS: sub-batches while guarded
  int64_t base_groups = 1;               // MV_BASE_GROUPS: sub-batches when not guarded
  double stream_fracs[8] = {0.7, 0.3};   // MV_STREAM_FRACS: the streamed batches' shares
  int n_stream_fracs = 2;
  // kernel forms (the launchers)
  int64_t no_key_agg = 0;                // MV_NO_KEY_AGG: committee A terms as bucket entries
  int64_t reduce_quad = 16384;           // MV_REDUCE_QUAD: quad-reduce threshold
  int64_t b2_lane = 1;                   // MV_B2_LANE: batch-size BLAKE2b one lane per string
  int64_t comb_quad = -1;                // MV_COMB_QUAD: force k_verify_comb16 (1) / k_verify_comb (0)
  int64_t reduce_rows = 1024;            // MV_REDUCE_ROWS: reduction levels of <= this many elements a wave each (0: none)
  int64_t final_rows = 1;                // MV_FINAL_ROWS: k_bv_final's Horner with one DPP row per coordinate
  int64_t bucket_bal = 1;                // MV_BUCKET_BAL: entries per bucket-kernel lane (<= 1: 64, with the chip-filling floor)
  int64_t sort_wide = 0;                 // MV_SORT_WIDE: 1 = the bucket sort's 8-byte partition entries at any batch size
  int64_t prep_chain = 1;                // MV_PREP_CHAIN: a batch's k_bv_prep starts after the previous batch's
                                         // (1: on the engine's streams; 2: on callers' streams too)
  int64_t blk_walk = 1;                  // MV_BLK_WALK: batch-size block calls in one pass over the bincode (k_block_walk); 0: staged pre-image
  // the index of block references (index.hip)
  int64_t index_tag_bits = 64;           // MV_INDEX_TAG_BITS: bits kept of a slot's tag (1..64; tests force collisions)
};

size_t verify_scratch_bytes(uint32_t n);
size_t btable_bytes();
hipError_t launch_btable_init(void* d_btab, hipStream_t s);
hipError_t launch_verify(const uint8_t* msg, const uint8_t* sig, const uint8_t* pk, const uint32_t* key_idx, uint32_t n,
                         const void* btab, void* scratch, uint8_t* status, hipStream_t s, const uint32_t* skip = nullptr,
                         uint32_t skip_group = 0, const void* prep_pts = nullptr, const void* prep_comb = nullptr);
// skip (optional, device): per-group flags; the signatures of group g = i / skip_group
// (skip_group a multiple of 256; 0 = one group) are not verified when skip[g] != 0.
// prep_pts (the batch path's fallback): R and A as k_bv_prep decoded them (A from the comb
// tables prep_comb when it was summed per key), and prep's nonzero statuses kept.
// *count = the number of items of status[0..n) equal to MV_SIG_INVALID; status 16-byte aligned
hipError_t launch_count_rejects(const uint8_t* status, uint32_t n, uint32_t* count, hipStream_t s);
hipError_t launch_sign(const uint8_t* seed, const uint8_t* msg, uint32_t n, const void* btab, uint8_t* pk,
                       uint8_t* sig, hipStream_t s);
hipError_t launch_blake2b(const Knobs& kn, const uint8_t* buf, const uint64_t* off, const uint64_t* len, uint32_t n, uint8_t* out,
                          hipStream_t s);
hipError_t launch_block_hash(const Knobs& kn, const uint8_t* buf, const uint64_t* off, const uint64_t* len, uint32_t n,
                             uint8_t* msg_out, uint8_t* dig_out, hipStream_t s);
// blake2b_quad.hip: the same two hashes with four lanes per string (launch_blake2b /
// launch_block_hash route to them; at batch size they route on to blake2b_lane.hip)
hipError_t launch_blake2b_quad(const Knobs& kn, const uint8_t* buf, const uint64_t* off, const uint64_t* len, uint32_t n, uint8_t* out,
                               hipStream_t s);
hipError_t launch_block_hash_quad(const Knobs& kn, const uint8_t* buf, const uint64_t* off, const uint64_t* len, uint32_t n,
                                  uint8_t* msg_out, uint8_t* dig_out, hipStream_t s);
// blake2b_lane.hip: one lane per string (batch-size calls; the quad launchers route to it)
hipError_t launch_blake2b_lane(const uint8_t* buf, const uint64_t* off, const uint64_t* len, uint32_t n, uint8_t* out,
                               hipStream_t s);
hipError_t launch_block_hash_lane(const uint8_t* buf, const uint64_t* off, const uint64_t* len, uint32_t n,
                                  uint8_t* msg_out, uint8_t* dig_out, hipStream_t s);
hipError_t launch_selftest(int op, const uint32_t* in, uint32_t n, const void* btab, uint32_t* out, hipStream_t s);
// ops >= SELFTEST_WIDE_OP: raw-limb field and point functions on 64-word rows (kernels.hip k_selftest_wide)
constexpr int SELFTEST_WIDE_OP = 64;
// ops >= SELFTEST_SCALAR_OP: the functions of scalar25519.h, same rows (kernels.hip k_selftest_scalar)
constexpr int SELFTEST_SCALAR_OP = 112;
hipError_t launch_selftest_wide(int op, const uint32_t* in, uint32_t n, uint32_t* out, hipStream_t s);
// batch.hip: random-linear-combination batch verify with exact on-device fallback.
// The batch is cut into `groups` sub-batches (1..BATCH_MAX_GROUPS, whole 1024-signature
// chunks, batch_group_size signatures each), one combined equation per group.
// key = 32-byte secret + 64-bit call counter (the z_i PRF key); *flag_out receives the
// device address of the flag words: [0] = 1 if every group's equation held, [1 + g] = 1
// if group g's held. ev (optional): BATCH_STAGES + 1 events, recorded before the first
// stage and after each stage.
struct ChunkGate {
  const hipEvent_t* ready;
  uint32_t n;
  const uint32_t* end;
};
constexpr int BATCH_STAGES = 6;  // prep, sort, bucket, reduce, final, fallback
constexpr int BATCH_MAX_GROUPS = 16;
size_t batch_scratch_bytes(uint32_t n, uint32_t groups);
uint32_t batch_group_size(uint32_t n, uint32_t groups);
hipError_t launch_verify_batch(const Knobs& kn, const uint8_t* msg, const uint8_t* sig, const uint8_t* pk, const uint32_t* key_idx,
                               uint32_t n, uint32_t groups, const uint32_t key[10], const void* btab,
                               void* bscratch, void* vscratch, uint8_t* status, hipStream_t s,
                               uint32_t** flag_out, hipEvent_t* ev = nullptr, const void* comb_a = nullptr,
                               const uint8_t* key_ok = nullptr, uint32_t n_keys = 0, const void* comb_b = nullptr,
                               const struct ChunkGate* gate = nullptr, const hipEvent_t* chain = nullptr);
// The preparation stage alone (the test entry mv_selftest_batch_prep): the zeroing of the column
// sums and the k_bv_prep launch(es), by the helper launch_verify_batch itself calls
// (launch_prep_stage), into buffers of the caller: pts 2 n rows of 128 bytes (R at i, A at n + i;
// the A rows are not written when A's term is summed per key: a_rows = 0), scal n rows of 48
// bytes, bsum BATCH_MAX_GROUPS x 12 64-bit column sums. Nothing after the preparation runs.
struct BatchPrepInfo {
  uint32_t groups, group_sigs, a_rows;
};
hipError_t launch_batch_prep(const Knobs& kn, const uint8_t* msg, const uint8_t* sig, const uint8_t* pk,
                             const uint32_t* key_idx, uint32_t n, uint32_t groups, const uint32_t key[10], void* pts,
                             void* scal, void* bsum, uint8_t* status, hipStream_t s, const void* comb_a,
                             const uint8_t* key_ok, uint32_t n_keys, const struct ChunkGate* gate,
                             BatchPrepInfo* info);
// The stages after the preparation alone (the test entry mv_selftest_batch_msm): sort, buckets,
// per-key A term, reduction and k_bv_final, by the helper launch_verify_batch itself calls
// (launch_msm_stage), on the caller's host rows: h_scal n rows of 48 bytes (z < 2^127 and z k <
// 2^253: the caller checks, a larger scalar's bucket key would leave the key space), h_pts 2 n
// rows of 128 bytes (n rows in the per-key form), h_bsum BATCH_MAX_GROUPS x 12 column sums. They
// are copied into bscratch (scratch_bytes >= batch_scratch_bytes(n, the group count used)) where
// k_bv_prep writes them. key_idx (device, with comb_a and n_keys <= 512): the per-key form.
// info: the geometry and the device addresses (inside bscratch) of the window sums k_bv_final
// read (groups x nw rows of 9 quads), the groups' per-key A terms (per-key form, else null) and
// the 1 + groups flag words. No fallback runs.
struct BatchMsmInfo {
  uint32_t groups, group_sigs, nw;
  const uint4* win;
  const uint4* asum;
  const uint32_t* flag;
};
hipError_t launch_batch_msm(const Knobs& kn, uint32_t n, uint32_t groups, const void* h_scal, const void* h_pts,
                            const void* h_bsum, const uint32_t* key_idx, uint32_t n_keys, const void* comb_a,
                            const void* comb_b, void* bscratch, size_t scratch_bytes, hipStream_t s,
                            BatchMsmInfo* info);
// chain (optional, unchunked calls): k_bv_prep waits for chain[0] (may be null) and chain[1]
// is recorded after it, so consecutive batches on different streams run their preparations
// one after another and each overlaps the previous batches' narrow tails (sort, reduce, final)
// instead of all starting together and leaving the tails to run side by side.
// gate (optional): the inputs arrive in chunks (H2D copies on another stream). Chunk c =
// signatures [end[c - 1], end[c]) (ends multiples of 256 except the last = n); k_bv_prep runs
// chunk by chunk on s, each launch after hipStreamWaitEvent on ready[c].
// comb_b (required): the comb table of B (mv_create), for the -[sum z s]B term.
// comb_a / key_ok (optional, with key_idx): the committee's comb tables (comb.hip, tables of
// -A) and per-key decode flags; k_bv_prep then reads each signature's A from entry [0][1]
// of its key's table instead of decoding A (the key was decoded once, at mv_set_committee).
// n_keys (committee size, <= 512) > 0 also sums A's term per key: sum_b [c_b] A_b on the
// comb tables replaces the 16 A bucket entries per signature.
// comb.hip: per-key comb tables C[i][j] = [j 256^i](+-P) and the committee-key verify.
// enc == nullptr builds the table of B; negate = 1 stores -P (committee keys).
size_t comb_table_bytes(uint32_t nbases);
hipError_t launch_comb_init(const uint8_t* enc, uint32_t nb, int negate, void* tab, uint8_t* ok, hipStream_t s);
// the block verdict (block_verdict.h) fused into a committee signature kernel's last step on
// the online block path, which then writes status[] instead of the signature status: one
// launch less. Null: signature status only.
struct BlockVerdictOut {
  const uint32_t* facts;
  const uint8_t* claimed;
  uint8_t* msg_digest;
  uint8_t* digest;
  uint8_t* status;
};
// the block hash folded into the online committee verify (k_verify_comb16): the staged
// pre-images P || sig in, both digests out (msg_digest is then the kernel's msg input)
struct BlockHashIn {
  const uint8_t* stage;
  const uint64_t* pre_off;
  const uint64_t* pre_len;
  uint8_t* msg_digest;
  uint8_t* digest;
};
// the block ingest folded into the online committee verify too (k_verify_comb16 parses its own
// blocks first, one wave per block): bincode in, everything launch_block_parse writes out
struct BlockIngestIn {
  const uint8_t* buf;
  const uint64_t* off;
  const uint64_t* len;
  const uint64_t* stakes;
  uint32_t n_auth;
  uint64_t epoch, quorum_thr;
  uint8_t* stage;
  uint64_t* pre_off;
  uint64_t* pre_len;
  uint8_t* sig;
  uint32_t* key_idx;
  uint32_t* facts;
  uint8_t* claimed;
};
// The resident online service (comb.hip k_online): one kernel that stays on the GPU while
// online traffic flows and runs each mv_verify_blocks request of <= ONLINE_MAX_BLOCKS short
// blocks as k_verify_comb16's workgroups would (ingest, both digests, challenge, comb sums,
// verdict), with no launch and no event per request.
//   host     writes request q's input (offsets, lengths, bincode) into ring slot q % SLOTS of
//            page-locked memory and its descriptor, then seq = q + 1; ctl.tail >= q + 1
//   poller   workgroup 0 polls ctl.tail, copies the input of every request whose seq is set
//            into the slot's HBM scratch (one pass for all of them) and appends the request's
//            4-block jobs to a job ring in HBM: the only PCIe reads on the request's path
//   workers  workgroups 1.. each hold a ticket (one atomic add on the ring's head) and start the
//            job as soon as the ring's tail passes it, run it from HBM, copy its blocks' digests
//            and verdicts to the slot's page-locked output; the request's last job stores
//            ctl.done[slot] = q + 1 (system-scope release after the outputs)
// The poller ends the launch (quit) after idle_ticks without a request, on ctl.stop, or after
// max_ticks; workers leave when they see quit. A launch starts by discarding tickets of the
// previous launch's workers (head = tail) before any worker takes one (epoch handshake).
// The slot's HBM scratch layout is fixed (below), so a descriptor is 16 bytes.
#ifndef MV_ONLINE_SLOTS
#define MV_ONLINE_SLOTS 128
#endif
constexpr uint32_t ONLINE_SLOTS = MV_ONLINE_SLOTS;  // request ring (a multiple of 64)
constexpr uint32_t ONLINE_MAX_BLOCKS = 64;  // 16 jobs per request
constexpr uint32_t ONLINE_JOBS = 16 * ONLINE_SLOTS;  // job ring (>= SLOTS x 16)
constexpr uint32_t ONLINE_MAX_WGS = 256;    // resident workgroups at most (the poller + workers)
constexpr uint32_t ONLINE_WG_LEFT = 0x80000000u;
constexpr uint64_t ONLINE_EXIT_STOP = 1, ONLINE_EXIT_IDLE = 2, ONLINE_EXIT_MAX = 3;
constexpr size_t ONLINE_IN_CAP = 128u << 10;  // bincode bytes per request
constexpr size_t online_al(size_t x) { return (x + 255) & ~(size_t)255; }
constexpr size_t ONLINE_IN_STRIDE = online_al(16 * ONLINE_MAX_BLOCKS + ONLINE_IN_CAP + 64);  // off | len | bincode
constexpr size_t ONLINE_OUT_STRIDE = online_al(65 * ONLINE_MAX_BLOCKS);  // md[64][32] | bd[64][32] | status[64]
// slot scratch (HBM): in | out | stage | pre_off | pre_len | sig | key_idx | facts | claimed | sst
constexpr size_t ONLINE_O_OUT = ONLINE_IN_STRIDE;
constexpr size_t ONLINE_O_STAGE = ONLINE_O_OUT + ONLINE_OUT_STRIDE;
constexpr size_t ONLINE_O_POFF = ONLINE_O_STAGE + online_al(ONLINE_IN_CAP + 4096);
constexpr size_t ONLINE_O_PLEN = ONLINE_O_POFF + online_al(8 * ONLINE_MAX_BLOCKS);
constexpr size_t ONLINE_O_SIG = ONLINE_O_PLEN + online_al(8 * ONLINE_MAX_BLOCKS);
constexpr size_t ONLINE_O_KIDX = ONLINE_O_SIG + online_al(64 * ONLINE_MAX_BLOCKS);
constexpr size_t ONLINE_O_FACTS = ONLINE_O_KIDX + online_al(4 * ONLINE_MAX_BLOCKS);
constexpr size_t ONLINE_O_CLAIMED = ONLINE_O_FACTS + online_al(4 * ONLINE_MAX_BLOCKS);
constexpr size_t ONLINE_O_SST = ONLINE_O_CLAIMED + online_al(32 * ONLINE_MAX_BLOCKS);
constexpr size_t ONLINE_SCR_STRIDE = ONLINE_O_SST + online_al(ONLINE_MAX_BLOCKS);
// the wave-parallel ingest's LDS window per block (ingest_dev.h IG_WIN): longer blocks parse on
// one lane, so the online service leaves them to the queue
constexpr uint32_t INGEST_WINDOW_BYTES = 10240;
struct OnlineReq {
  uint64_t seq;         // request number + 1 once the slot's input and n are written (release)
  uint32_t n;           // blocks; 0 = a void request (completed without work)
  uint32_t copy_bytes;  // input bytes of the slot (offsets, lengths, bincode + 16 zero bytes)
};
struct OnlineCtl {
  uint64_t tail;  // requests published so far
  uint64_t stop;  // nonzero: end the launch when idle
  uint64_t done[ONLINE_SLOTS];
  // the kernel's wall clock at: the poller sees the request, its jobs are in the ring, its first
  // job starts, its last job is done; then job 0's barrier 0 (ingest done), B rows done, S done,
  // R decoded, barrier 1, verdict written, outputs fenced, digests done, k published (comb.hip
  // comb16_wg; diagnostics: MV_ONLINE_TRACE sums them)
  uint64_t trace[ONLINE_SLOTS][14];
  // liveness (plain system-scope stores, read by the host's bounded stop): the workgroup's launch
  // number while it runs, | ONLINE_WG_LEFT once it has left; the poller's exit reason and its
  // ring words at exit (ready, jobs_head, jobs_tail)
  uint32_t wg[ONLINE_MAX_WGS];
  uint64_t exit_why, exit_ready, exit_head, exit_tail;
};
struct OnlineDev {
  unsigned long long ready;      // requests moved to HBM by the poller
  unsigned long long jobs_head;  // next ticket
  unsigned long long jobs_tail;  // jobs appended
  uint32_t quit, epoch;          // quit: workers leave; epoch: the launch whose poller is set up
  uint32_t n[ONLINE_SLOTS];
  uint32_t jobs_done[ONLINE_SLOTS];
  unsigned long long moved[ONLINE_SLOTS];  // request + 1 last moved from each slot (the poller's)
  unsigned long long jobs[ONLINE_JOBS];  // (request << 8) | job
  uint64_t sink[2 * 1024];               // 16 B per poller thread: where its copy lanes past the end go
};
struct OnlineArgs {
  OnlineCtl* ctl;                 // page-locked (device view)
  const OnlineReq* reqs;          // page-locked ring of descriptors
  OnlineDev* dev;                 // HBM
  const uint8_t* in_host;         // page-locked inputs, ONLINE_IN_STRIDE per slot
  uint8_t* out_host;              // page-locked outputs, ONLINE_OUT_STRIDE per slot
  uint8_t* scr;                   // HBM scratch, ONLINE_SCR_STRIDE per slot
  const void* combB;
  const void* combA;
  const uint8_t* key_ok;
  const uint8_t* pk;              // committee keys (32 B each)
  const uint64_t* stakes;
  uint64_t epoch, quorum_thr;     // the committee's
  uint32_t n_auth;
  uint32_t launch;                // launch number (the epoch handshake)
  uint64_t idle_ticks, max_ticks;
};
hipError_t launch_online(const OnlineArgs& a, uint32_t grid, hipStream_t s);
hipError_t launch_verify_comb(const Knobs& kn, const uint8_t* msg, const uint8_t* sig, const uint8_t* pk, const uint32_t* key_idx,
                              uint32_t n, const void* combB, const void* combA, const uint8_t* key_ok,
                              uint8_t* status, hipStream_t s, const BlockVerdictOut* bv = nullptr,
                              const BlockHashIn* hin = nullptr, const BlockIngestIn* ing = nullptr);
// whether launch_verify_comb takes the short-chain kernel (the one that can fold the hash in)
bool comb_short_chain(const Knobs& kn, uint32_t n);
// the comb verify split in two, for small batches of long blocks: k_hash_comb_pre is
// launch_block_hash plus, on workgroups of their own, the signature-only terms (R decoded ->
// rbuf, -[s]B -> sbuf, 144 B per signature each, flags: bit 0 s < l, bit 1 R decodes);
// k_comb_post adds the message-dependent [k]A and tests [8](R - R') = O
hipError_t launch_hash_comb_pre(const uint8_t* stage, const uint64_t* poff, const uint64_t* plen, uint32_t n,
                                uint8_t* md, uint8_t* bd, const uint8_t* sig, const void* combB, void* rbuf,
                                void* sbuf, uint8_t* qflags, hipStream_t s);
hipError_t launch_comb_post(const uint8_t* msg, const uint8_t* sig, const uint8_t* pk, const uint32_t* key_idx,
                            uint32_t n, const void* combA, const uint8_t* key_ok, const void* rbuf,
                            const void* sbuf, const uint8_t* qflags, uint8_t* status, hipStream_t s,
                            const BlockVerdictOut* bv = nullptr);
// ingest.hip: device-side bincode parse + pre-image staging, and the final block verdict
hipError_t launch_block_parse(const uint8_t* buf, const uint64_t* off, const uint64_t* len, uint32_t n,
                              const uint64_t* stakes, uint32_t n_auth, uint64_t epoch, uint64_t quorum_thr,
                              uint8_t* stage, uint64_t* pre_off, uint64_t* pre_len, uint8_t* sig, uint32_t* key_idx,
                              uint32_t* facts, uint8_t* claimed, hipStream_t s);
// block_walk.hip: launch_block_parse's outputs (but no staged pre-image) and both digests in
// ONE pass over the bincode, one lane per block; committees of <= 512 authorities
hipError_t launch_block_walk(const uint8_t* buf, const uint64_t* off, const uint64_t* len, uint32_t n,
                             const uint64_t* stakes, uint32_t n_auth, uint64_t epoch, uint64_t quorum_thr,
                             uint8_t* sig, uint32_t* key_idx, uint32_t* facts, uint8_t* claimed, uint8_t* md,
                             uint8_t* bd, hipStream_t s);
// sig[i]'s s := 2^256 - 1 (outside the batch equation) for every parsed block whose computed
// digest differs from its claimed one
hipError_t launch_block_digest_gate(const uint8_t* claimed, const uint8_t* digest, const uint32_t* facts, uint32_t n,
                                    uint8_t* sig, hipStream_t s);
// status in the types.rs order; zeroes both digests of blocks that do not deserialize
hipError_t launch_block_verdict(const uint32_t* facts, const uint8_t* claimed, uint8_t* msg_digest, uint8_t* digest,
                                const uint8_t* sig_status, uint32_t n, uint8_t* status, hipStream_t s);
// wal.hip: crc32fast::hash on the GPU and the WAL replay walk. `tables`
// (wal_table_words() words, built by wal_build_tables on the host) stay resident per device.
// cus = compute units (sizes the persistent crc grids).
size_t wal_table_words();
void wal_build_tables(uint32_t* out);
hipError_t launch_crc32(const uint8_t* buf, const uint64_t* off, const uint64_t* len, uint32_t n,
                        const uint32_t* tables, uint32_t* out, int cus, hipStream_t s);
// one lane per map: records (position | walk status << 60) of map m at rec[m * cap_pm ..], the
// record count (may exceed cap_pm: nothing past it is stored) and how the iteration leaves the map.
// moff (optional, a second walk): map m's records at rec[moff[m] ..], mcount[m] of them (the
// first walk's counts, read by the kernel)
constexpr uint8_t WAL_MAP_EMPTY = 0, WAL_MAP_NEXT = 1, WAL_MAP_END = 2, WAL_MAP_BAD = 3;
hipError_t launch_wal_walk(const uint8_t* img, uint64_t size, uint64_t end_pos, uint32_t map_bits, uint32_t nmaps,
                           uint32_t cap_pm, const uint64_t* moff, unsigned long long* rec, uint32_t* mcount,
                           uint8_t* mflag, hipStream_t s);
hipError_t launch_wal_compact(const unsigned long long* rec, uint32_t cap_pm, const uint32_t* mcount,
                              const uint64_t* moff, uint32_t nmaps, unsigned long long* ent, hipStream_t s);
// one wave per entry: header, payload crc, verdict (MV_WAL_*); *first_fail = min failing index
hipError_t launch_wal_crc(const uint8_t* img, uint64_t size, const unsigned long long* ent, uint64_t total,
                          const uint32_t* tables, uint64_t* out_pos, uint32_t* out_tag, uint32_t* out_len,
                          uint8_t* out_status, uint64_t cap, unsigned long long* first_fail, int cus, hipStream_t s);
// replay.hip: mv_wal_replay after the walk and the crc pass (rules: wal_entry.h). The entry list is
// launch_wal_crc's output in device memory; entry statuses are updated in place.
struct ReplayEntries {
  const uint64_t* pos;
  const uint32_t* tag;
  const uint32_t* len;
  uint8_t* status;
  uint64_t n;  // the walk's entries up to and including its first failing one
};
struct ReplayBlocks {  // the entries that carry a block, in iteration order (lists of cap >= n places)
  uint64_t* off;       // of the block's bincode in the image
  uint64_t* len;
  uint64_t* ent;       // entry index
  uint8_t* status;     // MV_BLOCK_* (enqueue_blocks)
  uint64_t n, cap;
};
// control words (device): the block total, the first failing entry (preset to all ones), the rows
// kept, three maxima (highest round, last own row + 1, last state entry + 1); the rest preset to 0
constexpr int REPLAY_CTL_NB = 0, REPLAY_CTL_FF = 1, REPLAY_CTL_NROWS = 2, REPLAY_CTL_ACC = 3, REPLAY_CTL_WORDS = 6;
uint64_t replay_groups(uint64_t n);  // workgroups of the per-entry kernels: wgcount / wgbase hold one word each
// k_replay_select + launch_index_scan: statuses of unknown tags and short own-block payloads, the
// per-workgroup block counts and their scan, *nb = the block total
hipError_t launch_replay_select(const ReplayEntries& en, uint64_t size, uint64_t* wgcount, uint64_t* wgbase,
                                uint64_t* nb, hipStream_t s);
hipError_t launch_replay_list(const ReplayEntries& en, uint64_t size, const uint64_t* wgbase, const ReplayBlocks& bl,
                              hipStream_t s);
// one lane per listed block: its row (10 words), or its entry's MV_WAL_BLOCK_DECODE /
// MV_WAL_UNKNOWN_AUTHORITY
hipError_t launch_replay_rows(const uint8_t* img, const ReplayEntries& en, const ReplayBlocks& bl, uint32_t n_auth,
                              uint64_t* rows, hipStream_t s);
// k_replay_cut, k_replay_summary, k_replay_finish: summary[3], last_seen[n_auth] (preset to 0),
// counts = {entries, rows} after the cut at the first entry that is not OK
hipError_t launch_replay_summary(const ReplayEntries& en, const ReplayBlocks& bl, const uint64_t* rows, uint32_t n_auth,
                                 uint64_t* ctl, uint64_t* summary, uint64_t* last_seen, uint64_t* counts,
                                 hipStream_t s);
// frames.hip: the walk of received NetworkMessage frames and the per-message / per-connection
// verdicts of mv_verify_frames (rules: frame_walk.h). Stream s = buf[soff[s], soff[s] + slen[s])
// clipped to buf_bytes. Count / scan / list as the WAL walk: the first launch_frame_walk
// (foff == nullptr) writes fcount[s] (frames that get a row) and consumed[s]; the second lists
// stream s's frames at foff[s] (offset of the size word, size, stream).
hipError_t launch_frame_walk(const uint8_t* buf, uint64_t buf_bytes, const uint64_t* soff, const uint64_t* slen,
                             uint32_t ns, const uint64_t* foff, uint64_t* fr_off, uint32_t* fr_size,
                             uint32_t* fr_stream, uint32_t* fcount, uint64_t* consumed, hipStream_t s);
struct FrameList {  // nf frames: the walk's list, and per frame the message's tag, status, blocks
  const uint64_t* off;
  const uint32_t* size;
  const uint32_t* stream;
  uint64_t nf;
  uint32_t* tag;
  uint8_t* status;  // MV_MSG_OK / DECODE_ERROR / TOO_MANY_REQUESTED / BAD_SIZE
  uint32_t* nblk;
};
struct FrameRows {  // the second message walk's inputs (per stream / per frame) and outputs
  const uint64_t* foff;       // per stream: its first frame
  const uint32_t* kept;       // per stream: rows kept (launch_stream_cut)
  const uint32_t* row_base;   // per stream: its first row
  const uint32_t* blk_base;   // per stream: its first block
  const uint64_t* bpre;       // per frame: blocks of the stream's earlier frames
  uint32_t* rows;             // n_rows x 8 words (include/mysti_verify.h)
  uint64_t n_rows;
  uint64_t* blk_off;          // n_blk
  uint64_t* blk_len;
  uint64_t n_blk;
};
// one lane per frame; out == nullptr: tag / status / nblk of every frame, else rows + block lists
hipError_t launch_msg_walk(const uint8_t* buf, const FrameList& fl, const FrameRows* out, hipStream_t s);
// one lane per stream: kept[s] (rows up to and including the first the bytes alone condemn),
// sblocks[s] (their blocks), bpre per frame; consumed[s] ends after a frame-level decode error
hipError_t launch_stream_cut(const uint64_t* soff, uint64_t buf_bytes, uint32_t ns, const uint32_t* fcount,
                             const uint64_t* foff, const FrameList& fl, uint64_t* bpre, uint32_t* kept,
                             uint64_t* sblocks, uint64_t* consumed, hipStream_t s);
// k_msg_verdict (block statuses -> row status, bad_block, bad_status) then k_stream_verdict
// (drop_msg[s], later rows MV_MSG_NOT_REACHED)
hipError_t launch_frame_verdicts(uint32_t* rows, uint64_t n_rows, const uint8_t* blk_status, uint64_t n_blk,
                                 uint32_t ns, const uint32_t* kept, const uint32_t* row_base, uint32_t* drop_msg,
                                 hipStream_t s);
// index.hip: the index of block references and the accept call (rules: block_ref.h; the table, the
// insert protocol and the memory model of all index kernels are described at the top of index_dev.h).
struct IndexTable {
  unsigned long long* slots;  // mask + 1 slots of 8 words (null: no table yet, every lookup is ABSENT)
  uint64_t mask;
  uint64_t k0, k1;    // the context's hash secret
  uint32_t tag_bits;  // MV_INDEX_TAG_BITS as it stood when the table was made
};
// Where the keys of n items lie: item i's six words at base + (off ? off[i] : i * stride) -- an
// off of IX_NO_SRC skips the item -- consecutive, or (ref) laid out as a bincode BlockReference.
struct IndexKeys {
  const uint8_t* base;
  const uint64_t* off;
  uint64_t stride;
  int ref;
};
constexpr uint64_t IX_NO_SRC = ~0ull;
constexpr uint64_t IX_MAX_ITEMS = 0xfffffffeull;  // items of one insert (the owner word holds ~item)
// control words (device, u64): the HAVE and WANTED entries, the longest probe since the last clear,
// items left for another round, probes that ran through the table (sticky: MV_E_HIP), then the
// totals of the accept call's scans and of the WANTED list (zeroed by every accept call), the STORED
// entries (HAVE counts them too), and the connect call's words: blocks and includes appended to or
// kept in the suspended-block store, the rows listed so far, and the rows of each level of the
// levels enqueued together
constexpr int IX_CTL_HAVE = 0, IX_CTL_WANTED = 1, IX_CTL_MAXPROBE = 2, IX_CTL_RETRY = 3, IX_CTL_ERR = 4,
              IX_CTL_NVER = 5, IX_CTL_NHEADS = 6, IX_CTL_NCAND = 7, IX_CTL_NINC = 8, IX_CTL_NMISS = 9,
              IX_CTL_NWANTED = 10, IX_CTL_STORED = 11, IX_CTL_PB_NB = 12, IX_CTL_PB_NI = 13, IX_CTL_PB_ROWS = 14,
              IX_CTL_LV0 = 16, IX_CTL_LEVELS = 16, IX_CTL_PB_END = IX_CTL_LV0 + IX_CTL_LEVELS,
              // the DAG store's words: includes appended by the connect call that is running (or kept by
              // a prune), max of ~round and of round over its records (0: no record), and the voting
              // and decision records a decide call picked
              IX_CTL_DG_NI = IX_CTL_PB_END, IX_CTL_DG_NLO = IX_CTL_DG_NI + 1, IX_CTL_DG_HI = IX_CTL_DG_NI + 2,
              IX_CTL_DG_NVOTE = IX_CTL_DG_NI + 3, IX_CTL_DG_NDEC = IX_CTL_DG_NI + 4, IX_CTL_DG_NB = IX_CTL_DG_NI + 5,
              // a commit call's pass: the walk jobs its chain step emitted, the highest anchor round, the
              // max of ~(lowest target round), the rows the pass moved; and the sequence's length
              IX_CTL_CM_NJOBS = IX_CTL_DG_NI + 8, IX_CTL_CM_QHI = IX_CTL_DG_NI + 9, IX_CTL_CM_NQLO = IX_CTL_DG_NI + 10,
              IX_CTL_CM_MOVED = IX_CTL_DG_NI + 11, IX_CTL_CM_NSEQ = IX_CTL_DG_NI + 12,
              IX_CTL_CM_NSPAN = IX_CTL_DG_NI + 13,  // the records of the rounds a commit call's levels read
              IX_CTL_WORDS = IX_CTL_DG_NI + 16;
constexpr int IX_WG = 256;  // lanes (items) per workgroup of the per-item kernels
inline uint64_t index_groups(uint64_t n) { return (n + IX_WG - 1) / IX_WG; }
// The per-workgroup scratch of a count / scan / list pass over n items: two counts per workgroup and
// their scans, index_groups(n) words each. The host sizes the buffer and the launchers carve it here.
struct WgScan {
  uint64_t *count_a, *count_b, *base_a, *base_b;
};
inline size_t wg_scan_bytes(uint64_t n) { return 4 * 8 * (size_t)index_groups(n); }
inline WgScan wg_scan_of(void* p, uint64_t n) {
  uint64_t* w = (uint64_t*)p;
  const uint64_t g = index_groups(n);
  return WgScan{w, w + g, w + 2 * g, w + 3 * g};
}
// wgbase[g] = the counts of the nwg workgroups before g, *total = all of them. With `running` (may
// be null) the bases stand behind *running, which then grows by the total.
hipError_t launch_index_scan(const uint64_t* wgcount, uint64_t nwg, uint64_t* wgbase, uint64_t* total, uint64_t* running,
                             hipStream_t s);
// one insert round (k_ix_claim, k_ix_fill, k_ix_settle) of n items towards `state`; item: n words
// of per-item records, kept between rounds; round > 0 takes the items the last round left over
// (ctl[IX_CTL_RETRY], zeroed by the caller before each round)
hipError_t launch_index_round(const IndexTable& t, const IndexKeys& ks, uint64_t n, uint64_t* item, uint32_t state,
                              int round, uint64_t* ctl, hipStream_t s);
// ctl[IX_CTL_ERR] += ctl[IX_CTL_RETRY]: ends the rounds of a call that cannot read the counter back
hipError_t launch_index_giveup(uint64_t* ctl, hipStream_t s);
hipError_t launch_index_prior(const uint64_t* item, uint64_t n, uint8_t* prior, hipStream_t s);
hipError_t launch_index_lookup(const IndexTable& t, const IndexKeys& ks, uint64_t n, uint8_t* out, uint64_t* ctl,
                               hipStream_t s);
// every entry of the old table into t (empty, zeroed)
hipError_t launch_index_rebuild(const uint64_t* old_slots, uint64_t n_old, const IndexTable& t, uint64_t* ctl,
                                hipStream_t s);
// after launch_index_rebuild: the n slot numbers a store holds (some may be DG_NO_SLOT, which stays)
// become those of the same keys in t; a number >= n_old or a key without an entry becomes DG_NO_SLOT
// and counts into ctl[IX_CTL_ERR]
hipError_t launch_index_reresolve(const uint64_t* old_slots, uint64_t n_old, const IndexTable& t, uint64_t* slotidx,
                                  uint64_t n, uint64_t* ctl, hipStream_t s);
// count / scan / list of the WANTED entries: *total, the first cap into out (cap x 6 words);
// wg: wg_scan_bytes(slots), as for every launcher below that takes one (of its own item count)
hipError_t launch_index_wanted(const IndexTable& t, uint64_t* wg, uint64_t* total, uint64_t* out, uint64_t cap,
                               hipStream_t s);
struct AcceptArrays {  // one accept call: the caller's blocks and the per-block / per-workgroup scratch
  const uint8_t* buf;
  uint64_t buf_bytes;
  const uint64_t* off;
  const uint64_t* len;
  const uint64_t* grp;  // may be null: every block its own group
  uint64_t n;
  uint8_t* known;       // per block
  uint32_t* rank;       // per block that is not KNOWN: its place in the verify list
  uint64_t* v_off;      // the verify list
  uint64_t* v_len;
  uint8_t* v_status;
  uint8_t* status;      // per block: MV_BLOCK_*
  uint8_t* state;       // per block: MV_ACC_*
  uint32_t* gidx;       // per block: its group's number
  uint32_t* gflag;      // per group: a block of it was rejected (zeroed by the caller)
  uint32_t* kc;         // per block: includes of a candidate
  uint64_t *wg_a, *wg_b, *base_a, *base_b;  // per workgroup: two counts and their scans
  uint32_t* cand_blk;   // per candidate (OK block of an accepted group), in block order: the block,
  uint64_t* cand_src;   // the offset of its own reference,
  uint64_t* inc_base;   // the number of its first include among all candidates' includes
};
// k_acc_probe, scan, k_acc_vlist: known[], ctl[IX_CTL_NVER] and the verify list
hipError_t launch_accept_probe(const IndexTable& t, const AcceptArrays& a, uint64_t* ctl, hipStream_t s);
// after the block pipeline: k_acc_groups, k_acc_states, the candidate list; ctl[IX_CTL_NCAND], ctl[IX_CTL_NINC]
hipError_t launch_accept_groups(const AcceptArrays& a, uint64_t* ctl, hipStream_t s);
hipError_t launch_accept_own_states(const AcceptArrays& a, const uint64_t* item, uint64_t ncand, hipStream_t s);
hipError_t launch_accept_inc_src(const AcceptArrays& a, uint64_t ncand, uint64_t ninc, uint64_t* inc_src, hipStream_t s);
hipError_t launch_accept_missing(const IndexTable& t, const uint64_t* item, uint64_t ninc, uint64_t* wg, uint64_t* ctl,
                                 uint64_t* out, uint64_t cap, hipStream_t s);

// The suspended-block store (mv_connect_blocks; layout and sweep: pending.hip): one record per block
// whose includes are not all MV_REF_STORED, in arrival order. The engine keeps two copies and
// compacts from one into the other. References are held as slots of the table: a rebuild
// re-resolves them (launch_index_reresolve).
struct PendStore {
  uint64_t* slot;   // per block: the slot of its own reference
  uint64_t* ibase;  // the number of its first include in inc
  uint64_t* blk;    // its index in the call that is running, IX_NO_SRC when an earlier call suspended it
  uint32_t* kc;     // its include count
  uint64_t* inc;    // per include: its slot
};
// cand_slot[r] = the slot of candidate r's own reference (its insert's records, before the includes' overwrite them)
hipError_t launch_pend_own_slots(const uint64_t* item, uint64_t ncand, uint64_t* cand_slot, hipStream_t s);
// The NEW blocks of an accept call join the store behind its nb0 blocks and ni0 includes, in block
// order; item: the records of the includes' insert. ctl[IX_CTL_PB_NB], ctl[IX_CTL_PB_NI] = how many.
hipError_t launch_pend_append(const AcceptArrays& a, uint64_t ncand, uint64_t ninc, const uint64_t* item,
                              const uint64_t* cand_slot, uint64_t* cand_dst, const PendStore& p, uint64_t nb0, uint64_t ni0,
                              uint64_t* wg, uint64_t* ctl, hipStream_t s);
// One level of the sweep over the nb records: check (a wave per record), count, scan, list + raise.
// lvl[b]: 0, or 1 + the level that connected b. Rows go to out (cap rows of 8 words) from row
// ctl[IX_CTL_PB_ROWS] on; ctl[lv_word] = the rows of this level. row_of (may be null; per record):
// the row a record connected as, whatever the cap -- the DAG store's record order.
hipError_t launch_pend_level(const IndexTable& t, const PendStore& p, uint64_t nb, uint32_t* lvl, uint8_t* hit,
                             uint64_t level, uint64_t* wg, uint64_t* out, uint64_t cap,
                             uint64_t* ctl, int lv_word, uint32_t* row_of, hipStream_t s);
// Stable compaction of p's records that are not STORED into q; those of the running call become
// MV_ACC_SUSPENDED in state (n_state entries, may be null). ctl[IX_CTL_PB_NB], ctl[IX_CTL_PB_NI] = what q holds.
hipError_t launch_pend_compact(const IndexTable& t, const PendStore& p, const PendStore& q, uint64_t nb, uint64_t* newbase,
                               uint8_t* state, uint64_t n_state, uint64_t* wg, uint64_t* ctl, hipStream_t s);

// The DAG store (mv_dag_reserve, mv_decide_leaders; kernels: dag_store.hip, decide.hip): one
// record per block that mv_connect_blocks stored, in connected-row order, with its includes as
// slots of the table. map: per slot of the table the record of its reference, DG_NONE without one.
struct DagStore {
  uint64_t* slot;   // per record: the slot of its own reference
  uint64_t* round;  // its round and
  uint32_t* auth;   // its authority, as the slot's key has them
  uint64_t* ibase;  // the number of its first include in inc
  uint32_t* kc;     // its include count
  uint64_t* inc;    // per include: its slot
  uint32_t* map;    // per slot of the table: its record
  uint64_t cap_b, cap_i, n_slots;  // what the arrays hold: every index is checked against them
};
constexpr uint32_t DG_NONE = 0xffffffffu;
constexpr uint64_t DG_NO_SLOT = ~0ull;
constexpr uint32_t DG_MAX_AUTH = 512;  // the bitmaps are 16 words (the walk's threshold-clock bitmap)
constexpr int DG_BM_WORDS = DG_MAX_AUTH / 32;
// The rows of a connect call (records of p with lvl != 0, row row_of[b]) join d behind its nb0
// records and ni0 includes: the records, the scan of their include counts (ctl[IX_CTL_DG_NI] = the
// includes), the include slots a wave per row. src: rows words of scratch.
hipError_t launch_dag_append(const IndexTable& t, const PendStore& p, uint64_t nb, const uint32_t* lvl,
                             const uint32_t* row_of, uint64_t rows, const DagStore& d, uint64_t nb0, uint64_t ni0,
                             uint64_t* src, uint64_t* wg, uint64_t* ctl, hipStream_t s);
// map[] = DG_NONE, then map[slot of record b] = b for d's nb records
hipError_t launch_dag_map(const DagStore& d, uint64_t nb, uint64_t* ctl, hipStream_t s);
// Stable compaction of d's records of round >= floor into q (whose map is rebuilt);
// ctl[IX_CTL_DG_NB], ctl[IX_CTL_DG_NI] = what q holds, ctl[IX_CTL_DG_NLO / _HI] its rounds.
hipError_t launch_dag_prune(const DagStore& d, const DagStore& q, uint64_t nb, uint64_t floor, uint64_t* newbase,
                            uint64_t* wg, uint64_t* ctl, hipStream_t s);

// One seed call (mv_dev_dag_seed_rows, mv_wal_recover; kernels: dag_store.hip): the rows of a replay
// (n x SD_ROW_WORDS words: 1 the offset of the block's bincode in img, 2 its length, 3..8 its
// reference) with their block verdicts, and the per-row scratch. Offsets and lengths are the
// caller's: every one is checked against `size` before a byte of img is read.
constexpr int SD_ROW_WORDS = 10;
struct SeedRows {
  const uint8_t* img;
  uint64_t size;
  const uint64_t* rows;
  const uint8_t* status;
  uint64_t n, floor;
  uint8_t* elig;       // per row: 0, 1 (may get a record), 2 (MV_BLOCK_OK, but its bytes do not fit the image)
  uint8_t* first;      // per row: the lowest row of its reference, and that reference had no record
  uint32_t* kc;        // per row: the include count of an eligible row
  uint64_t* own_slot;  // per row: the slot of its own reference
  uint64_t* rec_off;   // per record of the call: where its block lies in img
};
// the call's totals stand in words an accept call uses for its own (both zero them first)
constexpr int IX_CTL_SD_NREC = IX_CTL_NVER, IX_CTL_SD_MISFIT = IX_CTL_NHEADS, IX_CTL_SD_ELIG = IX_CTL_NCAND,
              IX_CTL_SD_EINC = IX_CTL_NINC, IX_CTL_SD_NINC = IX_CTL_NWANTED;
// k_sd_elig and its scans: elig, kc; ctl[IX_CTL_SD_ELIG / _EINC] = the eligible rows and their includes,
// ctl[IX_CTL_SD_MISFIT] += the misfits
hipError_t launch_seed_eligible(const SeedRows& r, uint64_t* wg, uint64_t* ctl, hipStream_t s);
// after the own references' insert (item: its records): k_sd_claim, k_sd_count, the scans, k_sd_list.
// The record rows join d behind its nb0 records and ni0 includes; ctl[IX_CTL_SD_NREC / _NINC] = how many.
hipError_t launch_seed_records(const IndexTable& t, const uint64_t* item, const SeedRows& r, const DagStore& d, uint64_t nb0,
                               uint64_t ni0, uint64_t* wg, uint64_t* ctl, hipStream_t s);
// inc_src[j] = where include item j of the call's nrec records lies in img (IX_NO_SRC for none)
hipError_t launch_seed_inc_src(const SeedRows& r, const DagStore& d, uint64_t nb0, uint64_t ni0, uint64_t nrec, uint64_t ninc,
                               uint64_t* inc_src, uint64_t* ctl, hipStream_t s);
// after the includes' insert (item: its records): their slots into the records
hipError_t launch_seed_inc(const uint64_t* item, const DagStore& d, uint64_t nb0, uint64_t ni0, uint64_t nrec, uint64_t ninc,
                           uint64_t* ctl, hipStream_t s);

// One decide call over n leader rows sorted by round: the distinct rounds (ng of them), where each
// round's rows start (ng + 1 words), and per sorted row its authority, round and place in the
// caller's arrays. gmax: the most rows of one round.
struct DecideIn {
  const uint64_t* g_round;
  const uint64_t* g_start;
  const uint64_t* l_auth;
  const uint64_t* l_round;
  const uint64_t* l_row;
  uint64_t ng, n, gmax;
};
struct DecideState {  // zeroed by the caller except vpos / vlist / dlist / sup
  uint32_t* cand_n;     // per row: leader blocks found
  uint64_t* cand_slot;  // per row x 8: their slots
  uint32_t* blame;      // per row x 16: authors of voting blocks without an include of the authority
  uint32_t* vote;       // per row x 8 x 16: authors of voting blocks that vote for the block
  uint32_t* cert;       // per row x 8 x 16: authors of its certificates
  uint32_t* vpos;       // per record: its place in vlist, DG_NONE outside it
  uint32_t* vlist;      // the voting records, the decision records
  uint32_t* dlist;
  uint64_t* sup;        // per (place in vlist, row of that round): the supported slot, DG_NO_SLOT for none
  uint8_t* cmask;       // null for a decide call; a commit call: per (place in dlist, row of that round) the
                        // candidates the decision record certifies, bit c for candidate c (zeroed by the caller)
};
// PickRoles (decide.hip): vpos, vlist, dlist, the candidates; ctl[IX_CTL_DG_NVOTE], ctl[IX_CTL_DG_NDEC]
hipError_t launch_decide_pick(const DagStore& d, uint64_t nb, const DecideIn& in, const DecideState& st,
                              uint64_t* wg, uint64_t* ctl, hipStream_t s);
// k_dg_vote, k_dg_cert, k_dg_decide: out (n x 8) and stakes_out (n x 3, may be null) in the caller's row order
hipError_t launch_decide_rule(const IndexTable& t, const DagStore& d, uint64_t nb, const DecideIn& in,
                              const DecideState& st, uint64_t nvote, uint64_t ndec, const uint64_t* stakes,
                              uint32_t n_auth, uint64_t quorum_thr, uint64_t* out, uint64_t* stakes_out, uint64_t* ctl,
                              hipStream_t s);

// One commit call (mv_commit_leaders; kernels: decide.hip) on top of a decide call's DecideIn /
// DecideState and its out rows, which must be in non-decreasing round order (l_row[k] = k). All
// arrays are per row unless said otherwise.
struct CommitState {
  uint32_t* fin;        // 0: the direct rule left the row UNDECIDED and nothing ended it yet; 1: final
  uint32_t* act;        // what a pass's chain step found for a row: CM_ACT_*
  uint32_t* anchor;     // the anchor's row (CM_ACT_WALK)
  uint64_t* cslot;      // the slot of a COMMIT row's block, DG_NO_SLOT otherwise
  uint32_t* job_id;     // per anchor row: its walk job in this pass, DG_NONE without one
  uint64_t* job_low;    // per anchor row: the lowest round its walk has to reach
  uint64_t* job_miss;   // per anchor row: 1 + the highest round at which an include of the walk had no record
  uint32_t* jobs;       // per job: its anchor's row
  uint32_t* marks;      // per job: a bitmap over the records (mark_words words each), made per pass
  uint64_t mark_words;
  uint32_t* span;       // the records of the rounds the call's levels can read (per call)
};
constexpr uint32_t CM_ACT_NONE = 0, CM_ACT_UNDECIDED = 1, CM_ACT_BLOCKED = 2, CM_ACT_WALK = 3;
constexpr uint32_t CM_CLAIMED = 0xfffffffeu;
// after launch_decide_rule: fin, cslot and the info rows of the rows the direct rule decided
hipError_t launch_commit_init(const IndexTable& t, const DecideIn& in, const DecideState& st, const CommitState& cs,
                              const uint64_t* out, uint64_t* info, uint64_t* ctl, hipStream_t s);
// one pass's chain step: act, anchor, the jobs; ctl[IX_CTL_CM_NJOBS / _QHI / _NQLO / _MOVED] (zeroed by the caller,
// as job_id (all ones), job_low (all ones) and job_miss (0) are)
hipError_t launch_commit_chain(const DecideIn& in, const CommitState& cs, const uint64_t* out, uint64_t* ctl, hipStream_t s);
// span = the records of rounds lo..hi; ctl[IX_CTL_CM_NSPAN] = how many
hipError_t launch_commit_span(const DagStore& d, uint64_t nb, uint64_t lo, uint64_t hi, uint32_t* span, uint64_t* wg,
                              uint64_t* ctl, hipStream_t s);
// the anchors' records into the (zeroed) marks, then one launch over the span per level of `levels` (descending)
hipError_t launch_commit_reach(const IndexTable& t, const DagStore& d, uint64_t nb, const DecideIn& in,
                               const CommitState& cs, uint64_t njobs, uint64_t nspan, const uint64_t* levels,
                               uint64_t n_levels, uint64_t* ctl, hipStream_t s);
// the rows the chain step moved: status, committed reference, info, fin
hipError_t launch_commit_resolve(const IndexTable& t, const DagStore& d, uint64_t nb, const DecideIn& in,
                                 const DecideState& st, const CommitState& cs, uint64_t nvote, uint64_t ndec, uint64_t njobs,
                                 uint64_t* out, uint64_t* info, uint64_t* ctl, hipStream_t s);
// ctl[IX_CTL_CM_NSEQ] = the rows of the longest prefix of COMMIT / SKIP rows among those of round > 0
hipError_t launch_commit_prefix(const DecideIn& in, const uint64_t* out, uint64_t* ctl, hipStream_t s);

// One linearize call (mv_linearize; kernels: linearize.hip): the leaders' sub-DAGs in one top-down
// sweep over the stored edges. mark is the context's committed mark per slot of the table (kept
// between calls, carried over by a rebuild); everything else is made per call.
constexpr int LN_KEY_WORDS = 5;    // a pick key: cidx | the includer's 16 path components | the include number
constexpr int LN_PATH_WORDS = 4;   // 16 components of 16 bits, the first in the top bits of word 0
constexpr uint32_t LN_MAX_DEPTH = 16, LN_MAX_J = 0xffff, LN_MAX_LEADERS = 0xffff;
// LN_CTL_LO: the lowest rec_low over the nodes so far -- no level below it has work (all ones before the first node)
constexpr int LN_CTL_NNODES = 0, LN_CTL_NOK = 1, LN_CTL_NROWS = 2, LN_CTL_NEWMARK = 3, LN_CTL_LO = 4, LN_CTL_WORDS = 8;
struct LinEdge {
  uint32_t rec, j;  // the including record, the include's number in its list
  uint64_t slot;    // the included reference
};
struct LinState {
  uint32_t* mark;         // per slot: committed (the counterpart of Linearizer::committed)
  uint64_t* best;         // per slot x LN_KEY_WORDS: the least pick key so far, word by word (all ones: none)
  uint32_t* node_of_rec;  // per record: its node in this call, DG_NONE without one
  uint64_t* rec_low;      // per record: the lowest round of an include that was not marked before the call (all ones: none)
  // per node, in the order the take steps made them (the nodes of one level are consecutive)
  uint64_t* n_slot;
  uint64_t* n_round;
  uint64_t* n_path;       // x LN_PATH_WORDS
  uint32_t* n_cidx;       // the sequence number of its leader
  uint32_t* n_depth;
  uint32_t* n_t;          // its number among its leader's nodes, in take order
  uint32_t* n_lvl;        // the level that made it
  uint64_t node_cap;
  // per leader
  const uint64_t* leaders;  // n x 6
  uint64_t* root_slot;      // DG_NO_SLOT: no entry, no record, or marked
  uint32_t* fail;           // 0, or the highest MV_LINEAR_* its sweep met
  uint32_t* total;          // its nodes
  uint64_t* first;          // its first output row
  uint64_t n;
  // per level of the call, and one behind: the nodes made before it
  uint64_t* lvl_start;
  uint64_t n_levels;
  // the edges, bucketed by the included reference's round: bucket 0 holds the rounds below lo
  uint32_t* bk_count;       // per bucket (count pass), then the fill pass's cursors
  const uint64_t* bk_off;   // nbk + 1: where each bucket starts
  LinEdge* edges;
  uint64_t nbk, lo, hi, n_edges;  // buckets, the store's lowest record round, the highest leader round
  uint64_t* lctl;           // LN_CTL_*
};
// the leaders' slots (a probe of the table), their refusals, their root keys into best
hipError_t launch_linear_roots(const IndexTable& t, const DagStore& d, uint64_t nb, const LinState& ls, uint64_t* ctl,
                               hipStream_t s);
// fill == false: bk_count[bucket] += the includes of every record of round <= hi; true: the edges
hipError_t launch_linear_edges(const IndexTable& t, const DagStore& d, uint64_t nb, const LinState& ls, bool fill,
                               uint64_t* ctl, hipStream_t s);
// one level: the edges [e0, e0 + ne) end in it; `round` is its round (roots of that round join), all
// ones for bucket 0. LN_KEY_WORDS pick launches, then the take step.
hipError_t launch_linear_level(const IndexTable& t, const DagStore& d, uint64_t nb, const LinState& ls, uint64_t level,
                               uint64_t round, uint64_t e0, uint64_t ne, uint64_t* ctl, hipStream_t s);
// statuses, first rows, counts and heights (sub: n x 4), the prefix rule; then the OK prefix's nodes
// into blocks (cap x 6) in (leader, round, path) order and into the marks
hipError_t launch_linear_output(const IndexTable& t, const LinState& ls, uint64_t height0, uint64_t cap, uint64_t* sub,
                                uint64_t* blocks, uint64_t* ctl, hipStream_t s);
// mark[slot of item i] = 1 for the n records of an insert; lctl[LN_CTL_NEWMARK] += those newly set
hipError_t launch_linear_mark(const uint64_t* item, uint64_t n, uint32_t* mark, uint64_t n_slots, uint64_t* lctl,
                              uint64_t* ctl, hipStream_t s);
// after launch_index_rebuild: the marks of the old table's slots onto the same keys' slots in t
hipError_t launch_linear_carry(const uint64_t* old_slots, uint64_t n_old, const uint32_t* old_mark, const IndexTable& t,
                               uint32_t* mark, uint64_t* ctl, hipStream_t s);

// propose.hip: mv_propose_* (the threshold clock, the pending queue and the include choice of
// Core::add_blocks / try_new_block, core.rs:181-278). The control words of the state (device, u64):
// the clock -- round, stake, voters, the voters bitmap (DG_BM_WORDS u32 words in PP_CTL_BM..) -- and
// a call's words: rows without a slot, the OR of the rows' rounds and of their complements (a bit set in
// both differs over the call), the zeros of a sort
// pass, the cut, the includes and payloads kept, the include entries taken, the flags, the tag of the
// first entry behind the cut, whether the own record was appended.
constexpr int PP_CTL_ROUND = 0, PP_CTL_STAKE = 1, PP_CTL_VOTERS = 2, PP_CTL_BM = 3, PP_CTL_NMISS = PP_CTL_BM + DG_BM_WORDS / 2,
              PP_CTL_OR = PP_CTL_NMISS + 1, PP_CTL_NOR = PP_CTL_NMISS + 2, PP_CTL_ZEROS = PP_CTL_NMISS + 3,
              PP_CTL_CUT = PP_CTL_NMISS + 4, PP_CTL_NINC = PP_CTL_NMISS + 5, PP_CTL_NPAY = PP_CTL_NMISS + 6,
              PP_CTL_NENT = PP_CTL_NMISS + 7, PP_CTL_FLAGS = PP_CTL_NMISS + 8, PP_CTL_NEXT = PP_CTL_NMISS + 9,
              PP_CTL_APPENDED = PP_CTL_NMISS + 10, PP_CTL_WORDS = PP_CTL_NMISS + 13;
constexpr uint32_t PP_INCLUDE = 1, PP_PAYLOAD = 2;  // an entry's kind
// The queue, entries in arrival order: kind, the slot of an include's reference (DG_NO_SLOT for a
// payload), its round, the caller's tag. The engine keeps two copies; a take moves the tail into the other.
struct PropQueue {
  uint32_t* kind;
  uint64_t* slot;
  uint64_t* round;
  uint64_t* tag;
};
// The rows of one clock step, in the order the automaton takes them, and the per-row scratch of the
// batch form: first (the row is the first of its author in its segment of equal round), and at a
// segment's first row its length, the first row at which the stake of first-seen authors passes the
// quorum (pos0; pos1: the first such row behind the segment's first; DG_NONE: none) and the stake of
// all its authors.
struct PropClock {
  const uint64_t* round;
  const uint32_t* auth;
  uint64_t n;
  uint8_t* first;
  uint32_t* seglen;
  uint32_t* pos0;
  uint32_t* pos1;
  uint64_t* stot;
  const uint64_t* stakes;
  uint32_t n_auth;
  uint64_t quorum;  // quorum <=> stake > it
};
// a lane per row: slot[i] of its key (a probe; none, or an authority outside the committee: pctl[PP_CTL_NMISS]),
// round[i], auth[i]; pctl[PP_CTL_OR / _NOR] their rounds' bits; perm[i] = i
hipError_t launch_propose_resolve(const IndexTable& t, const uint64_t* rows, uint64_t n, uint64_t stride_words, uint32_t n_auth,
                                  uint64_t* slot, uint64_t* round, uint32_t* auth, uint32_t* perm, uint64_t* pctl,
                                  uint64_t* ctl, hipStream_t s);
// one pass of a stable sort of perm by bit `bit` of round[perm[i]]: count, scan, scatter
hipError_t launch_propose_sort_bit(const uint64_t* round, int bit, const uint32_t* perm, uint32_t* perm_out,
                                   uint64_t n, uint64_t* wg, uint64_t* pctl, hipStream_t s);
// entry q0 + j of the queue = row perm[j] (an include with tags[perm[j]], 0 without tags), sauth[j] its
// authority; with `payload` one payload entry carrying `token` behind them
hipError_t launch_propose_append(const uint64_t* slot, const uint64_t* round, const uint32_t* auth, const uint64_t* tags,
                                 const uint32_t* perm, uint64_t n, const PropQueue& q, uint64_t q0, uint64_t qcap,
                                 uint32_t* sauth, bool payload, uint64_t token, uint64_t* ctl, hipStream_t s);
// ThresholdClockAggregator::add_block over the rows of c, in order: the segment scan (a wave per
// segment), then the chain over the segments (one wave); pctl's clock words before and after
hipError_t launch_propose_clock(const PropClock& c, uint64_t* pctl, uint64_t* ctl, hipStream_t s);
// pctl[PP_CTL_CUT] = the first include entry of round >= `round` (qn without one)
hipError_t launch_propose_cut(const PropQueue& q, uint64_t qn, uint64_t round, uint64_t* pctl, hipStream_t s);
// stamp[include slot] = counter for the includes of the records of the include entries before `cut`
// and for the own last block's n_own includes; an entry of round > 0 without a record: MV_PROPOSE_INCOMPLETE
hipError_t launch_propose_stamp(const PropQueue& q, uint64_t cut, const DagStore& d, uint64_t nb, bool dag_on,
                                const uint64_t* own_inc, uint64_t n_own, uint32_t* stamp, uint64_t n_stamp, uint32_t counter,
                                uint64_t* pctl, uint64_t* ctl, hipStream_t s);
// the include entries before `cut` whose slot is not stamped, as references (cap x 6) and as slots
// (choice, cap_choice), and the payload tokens (cap_p), all in queue order; the totals and the next tag
hipError_t launch_propose_keep(const IndexTable& t, const PropQueue& q, uint64_t qn, uint64_t cut, const uint32_t* stamp,
                               uint64_t n_stamp, uint32_t counter, uint64_t* includes, uint64_t cap, uint64_t* choice,
                               uint64_t cap_choice, uint64_t* payloads, uint64_t cap_p, uint64_t* wg, uint64_t* pctl,
                               uint64_t* ctl, hipStream_t s);
// the entries [cut, qn) of q become the entries [0, qn - cut) of to
hipError_t launch_propose_shift(const PropQueue& q, const PropQueue& to, uint64_t cut, uint64_t qn, hipStream_t s);
// own_out = the slot of the insert's item 0, then the includes: `prev` (the own last block's slot, with has_prev)
// and the n_src slots of src
hipError_t launch_propose_own(const uint64_t* item, const uint64_t* prev, bool has_prev, const uint64_t* src, uint64_t n_src,
                              uint64_t* own_out, uint64_t n_slots, uint64_t* ctl, hipStream_t s);
// the own block's record behind d's nb records and ni includes, unless its slot has one: pctl[PP_CTL_APPENDED]
hipError_t launch_propose_record(const IndexTable& t, const DagStore& d, uint64_t nb, uint64_t ni, const uint64_t* own,
                                 uint64_t k, uint64_t* pctl, uint64_t* ctl, hipStream_t s);

// seal.hip: mv_seal_blocks (StatementBlock::new_with_signer on bincode blocks with placeholder
// digest and signature fields). keys: 24 words per authority (a mod l, prefix, public key).
hipError_t launch_seal_keys(const uint8_t* seeds, uint32_t n_auth, const void* btab, uint32_t* keys, hipStream_t s);
// the walk alone: status[i] = MV_SEAL_OK / PARSE_ERROR / UNKNOWN_AUTHOR, heads[2 i] = authority,
// heads[2 i + 1] = round (both all ones for a parse error)
hipError_t launch_seal_scan(const uint8_t* buf, uint64_t buf_bytes, const uint64_t* off, const uint64_t* len,
                            uint32_t n, uint32_t n_auth, uint8_t* status, uint64_t* heads, hipStream_t s);
// The (authority, round) -> block table of a linked call, built on the host: slots of four words
// (round low, round high, authority, block; block = all ones: empty), mask + 1 of them (a power
// of two), linear probing from seal_table_hash & mask, no key further than max_probe slots from
// there. slots == nullptr: an unlinked call.
struct SealTable {
  const void* slots;
  uint32_t mask, max_probe;
};
__host__ __device__ inline uint32_t seal_table_hash(uint64_t a, uint64_t r) {
  uint64_t x = (r * 0x9E3779B97F4A7C15ull) ^ (a * 0xC2B2AE3D27D4EB4Full);
  x ^= x >> 29;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 32;
  return (uint32_t)x;
}
// a step of at least this many blocks runs four waves per workgroup on one LDS copy of the
// fixed-base table (the throughput shape); smaller steps one wave per workgroup
constexpr uint32_t SEAL_THROUGHPUT_MIN = 1u << 15;
// blocks [lo, hi) whose status is MV_SEAL_OK: linked (with a table), hashed, signed, patched in
// place; md / bd: n x 32 bytes, 8-byte aligned, bd read by later levels
hipError_t launch_seal_level(uint8_t* buf, uint64_t buf_bytes, const uint64_t* off, const uint64_t* len, uint32_t lo,
                             uint32_t hi, const uint32_t* keys, const void* btab, const SealTable& t, uint8_t* status,
                             uint8_t* md, uint8_t* bd, hipStream_t s);

// votes.hip: mv_aggregate_votes (TransactionAggregator::process_block, committee.rs:263-482). The
// store: a table of its own (index_dev.h's layout and hashing, another instance than the block
// index) from a sharing block's reference to a row, and per row a run of cells in one arena. A
// cell is cw = 2 + voter words: [0] 0 empty, 1 aggregating, else the mark of the event that
// certified it in the running call (cleared when its row is written); [1] the stake sum; [2..]
// the voters. Cells past the arena's cursor are zero.
struct VoteStore {
  IndexTable t;
  uint32_t* rowmap;  // per slot of t: its row
  uint64_t* row_key;   // 6 words per row
  uint64_t* row_base;  // the row's first cell
  uint32_t* row_n;     // its cells: the statement count of the block that made it
  uint32_t* row_agg;   // of which aggregating
  uint64_t* cells;
  uint64_t cap_rows, cap_cells;
  uint32_t cw;
};
// One call: the blocks, the committee, the per-block arrays of the scan (n entries each) and the
// events (cap_ev entries each). An event is three words: row | kind << 32, start | end << 32 (clipped
// to the row's cells), voter | block << 32; its id is its position, monotone in (block, statement)
// with a block's register events ahead of its votes.
struct VoteCall {
  const uint8_t* buf;
  uint64_t buf_bytes;
  const uint64_t *off, *len;
  uint32_t n, flags;
  const uint64_t* stakes;
  uint32_t n_auth;
  uint64_t quorum;  // certified at a stake sum >= quorum
  uint8_t* status;
  uint64_t *key, *keyoff;  // the own reference's six words; 48 i for a sharing block, else IX_NO_SRC
  uint32_t *author, *n_st, *nreg, *nev, *bflags;
  uint64_t *unk, *evbase;  // unknown offsets counted without an event; the block's first event
  uint8_t* brk;            // the block re-registers a row: a segment starts at it
  uint64_t* ev;
  uint32_t *evc, *evx;  // per event: certified; unknown (votes) or duplicate (register)
  uint64_t cap_ev;
};
// the store's control words, behind the IX_CTL_WORDS of its table's insert rounds
constexpr int VT_CTL_NSHARE = IX_CTL_WORDS, VT_CTL_NEWCELLS = VT_CTL_NSHARE + 1, VT_CTL_NEV = VT_CTL_NSHARE + 2,
              VT_CTL_NROWS = VT_CTL_NSHARE + 3, VT_CTL_NCELLS = VT_CTL_NSHARE + 4, VT_CTL_ERR = VT_CTL_NSHARE + 5,
              VT_CTL_NBRK = VT_CTL_NSHARE + 6, VT_CTL_PENDING = VT_CTL_NSHARE + 7, VT_CTL_AGG = VT_CTL_NSHARE + 8,
              VT_CTL_LIVECELLS = VT_CTL_NSHARE + 9, VT_CTL_NCERT = VT_CTL_NSHARE + 10, VT_CTL_NLIST = VT_CTL_NSHARE + 11,
              VT_CTL_SEGCERT = VT_CTL_NSHARE + 12, VT_CTL_WORDS = VT_CTL_NSHARE + 16;
constexpr uint32_t VT_KIND_NONE = 0, VT_KIND_REG = 1, VT_KIND_VOTE = 2;
// exclusive scan of n u32 counts into u64: out[i], *total; with `running` behind it (launch_index_scan).
// wg: wg_scan_bytes(n)
hipError_t launch_votes_scan_u32(const uint32_t* v, uint64_t n, uint64_t* out, uint64_t* total, uint64_t* running,
                                 void* wg, hipStream_t s);
// the first walk: the per-block arrays but evbase, brk; ctl[VT_CTL_NSHARE / _NEWCELLS] (zeroed by the caller)
hipError_t launch_votes_scan(const VoteCall& c, uint64_t* ctl, hipStream_t s);
// after the insert of the sharing blocks' references (item: its records): the rows of new
// references, brk, ctl[VT_CTL_NBRK]; then the second walk writes the events
hipError_t launch_votes_rows(const VoteStore& v, const VoteCall& c, const uint64_t* item, uint64_t* ctl, hipStream_t s);
hipError_t launch_votes_emit(const VoteStore& v, const VoteCall& c, const uint64_t* item, uint64_t* ctl, hipStream_t s);
// One segment, events [e0, e1): grouped by row in id order (row_cnt, row_cur: nrows words, row_lb
// nrows; list, sorted: e1 - e0 words), applied a wave per row, and the certified rows written behind
// ctl[VT_CTL_NCERT] (which grows), the first cap_cert of the call.
struct VoteSeg {
  uint32_t *row_cnt, *row_cur, *list, *sorted;
  uint64_t *row_lb, *certbase;
  void* wg;
};
hipError_t launch_votes_segment(const VoteStore& v, const VoteCall& c, uint64_t nrows, uint64_t e0, uint64_t e1,
                                const VoteSeg& g, uint64_t* certified, uint64_t cap_cert, uint64_t* ctl, hipStream_t s);
// blk_counts (4 words per block) from the events' counts
hipError_t launch_votes_blockout(const VoteCall& c, uint64_t* blk_counts, hipStream_t s);
// ctl[VT_CTL_PENDING / _AGG / _LIVECELLS] over the rows
hipError_t launch_votes_stats(const VoteStore& v, uint64_t nrows, uint64_t* ctl, hipStream_t s);
// the rows of v with an aggregating cell into q (empty, zeroed); ctl[VT_CTL_NROWS / _NCELLS] = what q holds
hipError_t launch_votes_move(const VoteStore& v, uint64_t nrows, const VoteStore& q, uint64_t* ctl, hipStream_t s);

// encode.hip: mv_encode_blocks (the bincode of Core::try_new_block's block; rules: encode_walk.h).
// One call: the caller's arrays, the per-payload results of the check (p entries each; pre p + 1:
// the exclusive scan of the body lengths and their total, modulo 2^64 -- a block that is OK has a
// body below MV_ENCODE_MAX_LEN, so the difference of two entries of its run is exact), the
// statement count per block, and the outputs.
struct EncodeCall {
  const uint64_t* heads;
  uint32_t n;
  const uint64_t* includes;
  uint64_t m;
  const uint8_t* payload_buf;
  uint64_t payload_bytes;
  const uint64_t *payload_off, *payload_len;
  uint64_t p;
  uint8_t* pay_ok;
  uint64_t *pay_count, *pay_body, *pre;
  uint64_t* blk_count;
  uint32_t* big;  // the blocks of at least EN_WG_BYTES, in block order (n entries of room)
  uint8_t* out;
  uint64_t cap;
  uint64_t *out_off, *out_len;
  uint8_t* status;
};
// control words: the scan of the bodies, the span of the blocks, the failed bounds checks
// (the words before EN_CTL_ERR are zeroed by every call; that one outlives a call, engine_encode.cpp)
constexpr int EN_CTL_BODY = 0, EN_CTL_TOTAL = 1, EN_CTL_NBIG = 2, EN_CTL_ERR = 3, EN_CTL_WORDS = 4;
// a block of at least this many bytes is written by a workgroup, a shorter one by a wave
constexpr uint64_t EN_WG_BYTES = 4096;
// a block of at most this many payloads keeps its piece boundaries in LDS
constexpr uint32_t EN_TILE = 512;
// k_en_check and the scan of the bodies: pay_ok, pay_count, pay_body, pre; wg: wg_scan_bytes(max(n, p))
hipError_t launch_encode_check(const EncodeCall& c, void* wg, uint64_t* ctl, hipStream_t s);
// k_en_size and the scan of the padded lengths: status, out_len, blk_count, out_off, big; ctl[EN_CTL_TOTAL],
// ctl[EN_CTL_NBIG] = the entries of big
hipError_t launch_encode_size(const EncodeCall& c, void* wg, uint64_t* ctl, hipStream_t s);
// k_en_write: the bytes of the OK blocks and their padding (the caller has held ctl[EN_CTL_TOTAL]
// against cap). A wave per block, unless all nbig = ctl[EN_CTL_NBIG] blocks are large; a workgroup per
// entry of big, if there is one.
hipError_t launch_encode_write(const EncodeCall& c, uint64_t nbig, uint64_t* ctl, hipStream_t s);

// wal_write.hip: mv_wal_write (WalWriter::writev for n entries; layout rule: wal_layout.h, crc: wal_crc.h).
// One call: the caller's arrays and the layout's scratch.
struct WalWriteCall {
  const uint8_t* buf;       // the payloads' bytes: 8-byte aligned, 16 readable bytes past buf_bytes
  uint64_t buf_bytes;
  const uint64_t* entries;  // n rows: tag | payload offset | payload length | next_entry
  uint64_t n;
  uint64_t start;
  uint32_t map_bits;
  uint8_t* out;             // cap bytes, 8-byte aligned; byte 0 is writer position `start`
  uint64_t cap;
  uint64_t* pos;            // n positions (absolute)
  uint64_t* sums;           // n: the exclusive sums of the entry lengths
  uint64_t *cross_first, *cross_shift;  // n each: the step table of the map crossings
};
// control words: entries refused (a payload outside buf, a body no map holds) | the writer position
// after the call | the steps of the crossing table | the sum of the entry lengths | a bounds check of
// the byte pass failed (it outlives a call: the device-buffer call returns with the bytes enqueued)
enum { WW_CTL_BAD = 0, WW_CTL_END = 1, WW_CTL_NC = 2, WW_CTL_TOTAL = 3, WW_CTL_ERR = 4, WW_CTL_WORDS = 5 };
// checks, sums, crossings, pos; ctl[WW_CTL_BAD / _END / _NC / _TOTAL] (zeroed by the caller). wg: wg_scan_bytes(n)
hipError_t launch_wal_write_layout(const WalWriteCall& c, void* wg, uint64_t* ctl, hipStream_t s);
// k_ww_emit: gap, header and body of every entry (the caller has held the span against cap and
// ctl[WW_CTL_BAD] against 0); tables: wal_build_tables'
hipError_t launch_wal_write_emit(const WalWriteCall& c, const uint32_t* tables, uint64_t* ctl, int cus, hipStream_t s);
}  // namespace mvk
