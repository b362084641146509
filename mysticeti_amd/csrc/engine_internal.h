// What the engine's source files share (host only): the per-device state and the context, the
// error plumbing, the sharding helpers, and the declarations of the functions that cross files
// (engine.cpp, engine_blocks.cpp, engine_online.cpp, engine_wal.cpp, engine_frames.cpp,
// engine_index.cpp, engine_connect.cpp, engine_dag.cpp, engine_decide.cpp, engine_linearize.cpp,
// engine_propose.cpp, engine_seal.cpp, engine_encode.cpp, engine_votes.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mysti_verify.h"
#include "block_codec.h"
#include "dev_resources.h"
#include "kernels.h"

namespace mvi {

constexpr int kBlockStage0 = mvk::BATCH_STAGES;  // parse, hash, verify, verdict

constexpr int kBlockStages = 4;
constexpr int kWalStage0 = kBlockStage0 + kBlockStages;  // walk, crc
static_assert(kWalStage0 + 2 == MV_NSTAGES, "stage count");

using mvr::DevBuf;
using mvr::HostBuf;

struct OnlineSvc;

// One logical device: the engine stream and, grouped by the feature that uses them, the
// resources of each path. Every group is made of owning types (dev_resources.h), so mv_destroy
// releases a group as a whole (mvr::reset) and names no single buffer or event.
struct Device {
  int id = 0;
  int cus = 0;
  bool committee_loaded = false;
  mvr::Stream stream;

  // the fixed-base tables ([0..128]B and [0..128](2^124 B) for the ladders, the comb table C_B)
  // and the committee: key encodings, stakes, per-key comb tables C_A, per-key decode flags
  struct Tables {
    DevBuf btab, combB;
    DevBuf committee_pk, stakes, combA, keyok;
  } tab;

  // staging of the synchronous host-buffer calls (signatures, hashes, crc, host-parsed blocks)
  struct HostCall {
    DevBuf msg, sig, pk, keyidx, status, bytes, off, len, out2;
    HostBuf h_in, h_out;
  } hc;

  // scratch rings: consecutive calls rotate over kSlots slots (mvr::ScratchRing)
#ifndef MV_SLOTS
#define MV_SLOTS 3
#endif
  static constexpr int kSlots = MV_SLOTS;
  static constexpr int kFlagWords = 1 + mvk::BATCH_MAX_GROUPS;
  // the batch flags of each call, copied to pinned host words behind it, in a ring larger
  // than the scratch ring: read (without blocking) once flag_ev has completed;
  // flag_groups[e] groups pending. A call blocks the host only with kFlagRing calls in flight.
  static constexpr int kFlagRing = 16;
  struct BatchPath {
    struct Scratch {
      DevBuf b, v;  // batch.hip's scratch, k_verify's per-wave tables (the fallback)
    };
    mvr::ScratchRing<Scratch, kSlots> ring;
    // the single-path batches' rejected-signature counts, one device word per flag-ring entry
    DevBuf rejects;
    HostBuf h_flags;  // kFlagRing x kFlagWords, pinned
    uint32_t flag_groups[kFlagRing] = {};
    mvr::Event flag_ev[kFlagRing];
    int flag_next = 0;
    // the preparation chain (MV_PREP_CHAIN): recorded after each batch's k_bv_prep; the next
    // batch's k_bv_prep waits for it (prep_chained: recorded at least once)
    mvr::Event prep_chain;
    bool prep_chained = false;
    const uint32_t* flags(int e) const { return h_flags.as<uint32_t>() + e * kFlagWords; }
    uint32_t* flags(int e) { return h_flags.as<uint32_t>() + e * kFlagWords; }
  } batch;

  // single-verify scratch (k_verify's per-wave tables)
  struct SinglePath {
    mvr::ScratchRing<DevBuf, kSlots> ring;
  } single;

  // device-API block-pipeline scratch: a ring whose slots are all grown together on first use,
  // so no slot is allocated inside a caller's steady state (a 2^21-block slot is ~21 GB; round
  // 3's four lazily grown slots put one ~0.8 s allocation into the driver's timed steps)
#ifndef MV_BLK_SLOTS
#define MV_BLK_SLOTS 3
#endif
  static constexpr int kBlkSlots = MV_BLK_SLOTS;
  // batch-size block calls: the second half's parse on an aux stream beside the first half's
  // hash (enqueue_blocks). One aux stream and event pair per scratch owner (ring slot or pass
  // set), so two calls in flight never queue their second halves behind each other.
  struct BlkAux {
    mvr::Event ev[2];
    mvr::Stream stream;
  };
  struct BlockPath {
    mvr::ScratchRing<DevBuf, kBlkSlots> ring;
    BlkAux aux[kBlkSlots];
  } blk;

  // pinned signature calls (verify_host_streamed)
  static constexpr int kPinBufs = 3;
  static constexpr int kMaxChunks = 64;
  static constexpr int kSigCalls = 4;
  struct PinnedPath {
    // three input buffer sets: the batches rotate over them (four measured the same for two
    // concurrent callers, profiles/r06/e2e_two_callers.txt)
    DevBuf pin_msg[kPinBufs], pin_sig[kPinBufs], pin_pk[kPinBufs], pin_st[kPinBufs];
    // Calls in flight: each holds one of kSigCalls status staging slots from its enqueue until
    // its verdicts are copied out; the enqueue runs under ctx->mu, the wait does not, so one
    // caller's copies run beside another's verification.
    HostBuf sig_stage[kSigCalls];
    mvr::Event sig_done[kSigCalls][2];
    bool sig_busy[kSigCalls] = {};
    mvr::Event pin_free[kPinBufs];
    mvr::EventSet chunk_ev[kPinBufs];  // kMaxChunks per-chunk "copied" events of each input buffer
    int pin_next = 0;  // the next batch's input buffer and compute stream (rotating across calls)
    // two compute streams: the H2D of one batch runs beside the previous batch's verification
    mvr::Stream pstream[2];
  } pin;

  // mv_verify_blocks passes (the submission queue): kPassSets sets of pinned staging, device
  // buffers and a stream each, so pass k + 1 is packed and enqueued while passes k, k - 1, ...
  // run (an online pass is a few workgroups: passes on distinct hardware queues run side by side)
  static constexpr int kPassSets = 4;
  struct PassSet {
    HostBuf h_in, h_out;
    DevBuf bytes, out2, scr;  // scr: the block pipeline's scratch for this set's passes
    BlkAux aux;               // the two-halves parse of a large host-fed chunk
    mvr::Event done;
    hipStream_t stream = nullptr;  // qstream[k] (not owned)
    // the chunk in flight: items [lo, lo + m) of `it`, outputs in h_out when finished
    const void* it = nullptr;
    uint64_t lo = 0;
    uint32_t m = 0;
    bool inflight = false;
  };
  struct PassSets {
    PassSet set[kPassSets];
    mvr::Stream qstream[kPassSets];  // one per pass set
  } pass;

  // WAL replay (wal.hip): crc tables, walk records, per-map counts / flags / offsets, entries,
  // the image and outputs of host-buffer calls (mv_wal_replay keeps its whole entry list in them)
  struct Wal {
    DevBuf tab, rec, mcount, mflag, moff, ent, ff, img, pos, tag, len, st;
    // mv_wal_replay (replay.hip): control words, per-workgroup scans and the block lists, the
    // block rows, and the summary / last_seen of host-buffer calls
    DevBuf rctl, rscr, rows, rsum;
    // mv_wal_write (wal_write.hip): the sums, the crossing table, the per-workgroup scan and the
    // control words; payload bytes, entry rows, image and positions of host-buffer calls
    DevBuf wsum, wcross, wwg, wctl, wbuf, went, wout, wpos;
  } wal;

  // mv_verify_frames (frames.hip): per-stream and per-frame walk arrays, the row and block
  // lists, and the bytes and stream table of host-buffer calls (calls are synchronous)
  struct Frames {
    DevBuf s, f, o, in, tab;
  } frm;

  // the index of block references (index.hip, engine_index.cpp and the files beside them), made on first use: the table
  // and its control words, and the scratch of insert, lookup, list and accept calls
  struct Index {
    DevBuf tab, ctl;
    DevBuf item, keys, out, wg;  // per-item records, staged keys / sources, results, per-workgroup scans
    DevBuf acc, accv, in, tab_in, miss;  // mv_accept_blocks: per-block arrays, the verify list, bytes, off | len | grp, the list
    HostBuf h_ctl;               // the control words read back
    uint64_t slots = 0;          // a power of two, 0: no table
    uint64_t used = 0;           // entries: exact after every call that synchronises, else an upper bound
    bool used_exact = true;
    // recorded behind every mv_dev_index_insert (which only enqueues, maybe on a caller's stream):
    // the next index call's stream waits for it, and it guards the per-item records when they grow
    mvr::Event ahead;
    bool ahead_set = false;
    uint64_t rebuilds = 0;
    uint32_t tag_bits = 64;      // of the table in force
    // mv_connect_blocks: the suspended-block store (mvk::PendStore), two copies -- blk[k] holds
    // slot | ibase | blk | kc for cap_b records, inc[k] cap_i include slots -- of which `cur` is in
    // force; a call compacts into the other and swaps
    struct Pending {
      DevBuf blk[2], inc[2];
      int cur = 0;
      uint64_t nb = 0, ni = 0, cap_b = 0, cap_i = 0, levels = 0;
      DevBuf cand_slot, cand_dst, lvl, hit, newbase, rows;  // per candidate | per record scratch, the rows
      DevBuf row_of;  // per record: the row it connected as (only with a DAG store)
    } pend;
    // mv_dag_reserve / mv_decide_leaders: the DAG store (mvk::DagStore), made by mv_dag_reserve
    // only -- rec holds slot | round | ibase | auth | kc for cap_b records, inc cap_i include
    // slots, map a u32 per slot of the table (remade with it). Growing and pruning fill a fresh
    // copy and swap.
    struct Dag {
      bool on = false;
      DevBuf rec, inc, map;
      uint64_t nb = 0, ni = 0, cap_b = 0, cap_i = 0, map_slots = 0;
      // a connect call's row -> record scratch, a prune's new bases, and a decide call's sorted
      // rows, per-row state, per-record lists, supports and results; a commit call's certificate
      // masks, per-row chain state, per-job marks and the records of its round span
      DevBuf src, newbase, lead, state, lists, sup, res, cmask, cm, marks, span;
      // mv_linearize: the committed mark per slot of the table (as long as map, remade with it and
      // carried over), the marked references and last_height; a call's control words, leaders, per-slot
      // keys, per-record and per-node arrays, buckets, edges and results
      DevBuf lmark;
      uint64_t lin_marked = 0, lin_height = 0;
      DevBuf lctl, llead, lbest, lnode, lbk, ledge, lres;
    } dag;
    // mv_propose_*: the proposer's state (propose.hip), made by mv_propose_reserve only -- the clock in
    // the control words ctl (mvk::PP_CTL_*), the queue in two copies (kind | slot | round | tag for
    // cap entries) of which `cur` is in force, the own last block (own[own_cur]: its slot, then own_k
    // include slots; mv_propose_own fills the other copy and flips), the outstanding choice (slots), and a stamp per slot of the table. Slots are those of the
    // table in force: a rebuild re-resolves them and the stamps are remade for the next take.
    struct Propose {
      bool on = false;
      uint32_t authority = 0;
      DevBuf ctl, q[2], own[2], choice, stamp;
      int cur = 0, own_cur = 0;
      uint64_t qn = 0, cap = 0;
      bool has_own = false, outstanding = false;
      uint64_t round = 0;  // the clock round as of the last call (the control words', read back)
      uint64_t own_round = 0, own_k = 0, n_choice = 0, take_round = 0;
      uint64_t stamp_slots = 0;
      uint32_t counter = 0;
      uint64_t takes = 0, dropped = 0;
      // a call's scratch: per row slot | round | tag (u64), auth | sauth | perm x 2 | seglen | pos0 | pos1
      // (u32), first (u8), stot (u64); the results of a take; the staged rows
      DevBuf rows, res, in;
    } prop;
  } index;

  // mv_seal_blocks (seal.hip): the expanded keys, the scan's heads, the link table, both digest
  // arrays, and the bytes, off | len, status and seeds of host-buffer calls (calls are synchronous)
  struct Seal {
    DevBuf keys, heads, tab, md, bd, in, ol, st, seeds;
    HostBuf h;
  } seal;

  // mv_encode_blocks (encode.hip): the per-payload results of the check and the scan of their
  // bodies, the statement count per block, the list of the large blocks, the scans' per-workgroup words, the control words and
  // their pinned copy; the inputs and outputs of host-buffer calls (heads, include rows, payload
  // bytes, payload off | len, the image, out_off | out_len, status, seal status). `done` is
  // recorded behind every device-buffer call (whose bytes are written after it returned): the next
  // call's stream waits for it, and it guards the scratch when it grows.
  struct Encode {
    DevBuf pay_ok, pay_count, pay_body, pre, blk_count, big, wg, ctl;
    HostBuf h_ctl;
    DevBuf heads, inc, pay, pol, out, ool, st, sst;
    mvr::Event done;
    bool done_set = false;
  } encode;

  // mv_aggregate_votes (votes.hip): the store -- its own table, the slot -> row map, the rows and
  // the cell arena, made by mv_votes_reserve only; growing and reclaiming fill a fresh copy and
  // swap -- its control words, and a call's per-block, per-event and per-segment scratch, the
  // insert's records, and the bytes, off | len and results of host-buffer calls
  struct Votes {
    bool on = false;
    DevBuf tab, rowmap, row_key, row_base, row_n, row_agg, cells, ctl;
    HostBuf h_ctl;
    uint64_t slots = 0, cap_rows = 0, cap_cells = 0, nrows = 0, ncells = 0;
    uint32_t voter_words = 0;
    uint64_t pending = 0, agg = 0, live_cells = 0, certified = 0;  // as of the last call
    DevBuf blk, evs, seg, item, in, ol, out;
  } votes;

  // the resident online service (k_online) of this device, made on first use
  std::shared_ptr<OnlineSvc> online;
};

struct PendingEvents {
  int device;
  int first_stage;  // stage index of events[0] -> events[1]
  mvr::EventSet events;
};

}  // namespace mvi

struct mv_ctx {
  std::mutex mu;
  std::vector<mvi::Device> devs;
  std::string err;
  uint32_t max_batch = 1u << 20;
  uint32_t flags = 0;
  uint32_t secret[8] = {0};         // batch-path z_i PRF key (from /dev/urandom)
  uint64_t index_secret[2] = {0};   // the index's hash key (index_dev.h), drawn with it
  std::atomic<uint64_t> calls{0};   // batch calls, the PRF's per-call input
  std::atomic<uint64_t> batches{0}, fallbacks{0}, groups_run{0}, groups_failed{0};
  // sub-batch equations per batch: groups_fixed != 0 forces that many; 0 = adaptive:
  // base_groups equations (one: every group adds 16 x 2^15 buckets to the bucket and reduce
  // kernels; config 2 measured 267 M/s at one group against 241 M/s at four), and after a
  // batch whose equation failed, the next kGuardBatches batches are cut into guard_groups
  // (a failure then re-verifies 1/8 of the batch).
  uint32_t groups_fixed = 0;
  uint32_t base_groups = 1;
  uint32_t guard_groups = 8;
  std::atomic<int> guard_left{0};
  // batches still to send straight to the single path (dense failures, kSingleRun), and the
  // counts of batches by route
  std::atomic<int> single_left{0};
  std::atomic<uint64_t> single_batches{0}, dense_failures{0};
  // stage timing (mv_set_stage_timing): event sets of calls not yet read back
  bool stage_timing = false;
  std::mutex tmu;
  std::vector<mvi::PendingEvents> pending;
  double stage_ms[MV_NSTAGES] = {0};
  uint64_t stage_calls[MV_NSTAGES] = {0};
  std::atomic<bool> has_committee{false};
  std::condition_variable sig_cv;  // a pinned signature call released its staging slot (Device::sig_busy)
  mvh::Committee committee;
  // block submission queue (mv_verify_blocks): concurrent callers' requests are merged into
  // one device pass by whichever caller finds the engine idle (flat combining)
  struct BlockReq;
  std::mutex q_mu;
  std::condition_variable q_cv;
  std::deque<BlockReq*> q;
  bool q_packing = false;                // a combining caller is packing / enqueueing a pass
  bool q_set_busy[mvi::Device::kPassSets] = {};  // pass sets with a pass in flight
  int q_sets = 0;                          // pass sets in use (MV_PASS_SETS, default kPassSets)
  // linger (MV_Q_LINGER_US): a combining caller that finds fewer requests queued than the last
  // finished pass carried waits briefly for the rest of that pass's callers to come back
  std::condition_variable q_linger_cv;
  bool q_lingering = false;
  size_t q_last_calls = 0;
  std::atomic<uint64_t> q_calls{0}, q_passes{0};
  // online requests hold it shared for their whole life; mv_set_committee and mv_destroy take it
  // exclusively (the resident kernel reads the committee's tables)
  std::shared_mutex com_mu;
  std::atomic<uint64_t> online_rr{0};
  std::vector<size_t> online_devs;  // devs[] index of the first logical shard of each GPU
  // the runtime switches, read from the environment at mv_create (knobs_from_env) and changed
  // only by mv_set_option (diagnostics, between calls)
  mvk::Knobs kn;
};

struct mv_ctx::BlockReq {
  const uint8_t* buf;
  const uint64_t *off, *len;
  uint32_t n;
  uint8_t *status, *md, *bd;
  mv_status rc = MV_OK;
  std::string err;
  bool taken = false;             // in a pass (q_mu)
  std::atomic<bool> done{false};  // verdicts delivered (set under q_mu, may be polled without it)
};

namespace mvi {

// Errors are recorded in the calling thread's slot (shard threads of one call each own
// one) and published to ctx->err by the thread that returns to the caller.
inline thread_local std::string* t_err = nullptr;

inline void record_err(mv_ctx* ctx, const std::string& msg) {
  if (t_err) *t_err = msg;
  else if (ctx) ctx->err = msg;
}

#define HIPCHK(ctx, expr)                                                                          \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) {                                                                        \
      record_err((ctx), std::string(#expr) + ": " + hipGetErrorString(e_));                        \
      return MV_E_HIP;                                                                             \
    }                                                                                              \
  } while (0)

// HIPCHK for functions that carry the status in `rc` (the first error is kept, no early return)
#define HIPCHK_RC(ctx, rc, expr)                                                  \
  do {                                                                            \
    hipError_t e_ = (expr);                                                       \
    if (e_ != hipSuccess && (rc) == MV_OK) {                                      \
      record_err((ctx), std::string(#expr) + ": " + hipGetErrorString(e_));       \
      (rc) = MV_E_HIP;                                                            \
    }                                                                             \
  } while (0)

inline mv_status set_err(mv_ctx* ctx, mv_status code, const std::string& msg) {
  record_err(ctx, msg);
  return code;
}

// Runs fn(device, cut[d], cut[d + 1]) for every device with a non-empty shard, one thread
// per device (cut: nd + 1 ascending item indices from 0 to n).
template <class Fn>
mv_status for_each_cut(mv_ctx* ctx, const std::vector<uint64_t>& cut, Fn fn) {
  const size_t nd = ctx->devs.size();
  std::vector<mv_status> rc(nd, MV_OK);
  std::vector<std::string> errs(nd);
  std::vector<std::thread> th;
  for (size_t d = 0; d < nd; d++) {
    const uint64_t lo = cut[d], hi = cut[d + 1];
    if (lo == hi) continue;
    th.emplace_back([&, d, lo, hi] {
      t_err = &errs[d];
      rc[d] = fn(ctx->devs[d], lo, hi);
      t_err = nullptr;
    });
  }
  for (auto& t : th) t.join();
  for (size_t d = 0; d < nd; d++)
    if (rc[d] != MV_OK) {
      ctx->err = errs[d];
      return rc[d];
    }
  return MV_OK;
}

// Runs fn(device, lo, hi) for each device's contiguous shard of [0, n) (equal counts).
template <class Fn>
mv_status for_each_shard(mv_ctx* ctx, uint64_t n, Fn fn) {
  const size_t nd = ctx->devs.size();
  if (nd == 1 || n < 2 * 256) return fn(ctx->devs[0], 0, n);
  std::vector<uint64_t> cut(nd + 1);
  for (size_t d = 0; d <= nd; d++) cut[d] = n * d / nd;
  return for_each_cut(ctx, cut, fn);
}

// count + 1 timing events (empty when stage timing is off)
inline mv_status make_events(mv_ctx* ctx, int count, mvr::EventSet& evs) {
  evs.release();
  if (!ctx->stage_timing) return MV_OK;
  HIPCHK(ctx, evs.ensure(count + 1, hipEventDefault));
  return MV_OK;
}

inline void keep_events(mv_ctx* ctx, int device, int first_stage, mvr::EventSet& evs) {
  if (evs.empty()) return;
  std::lock_guard<std::mutex> lk(ctx->tmu);
  ctx->pending.push_back(PendingEvents{device, first_stage, std::move(evs)});
}

constexpr uint32_t kOnSlots = mvk::ONLINE_SLOTS, kOnMax = mvk::ONLINE_MAX_BLOCKS;
constexpr size_t kOnInCap = mvk::ONLINE_IN_CAP;        // bincode bytes per request
constexpr size_t kOnInStride = mvk::ONLINE_IN_STRIDE;  // off[n] | len[n] | bincode | 16 zero B
constexpr size_t kOnOutStride = mvk::ONLINE_OUT_STRIDE;  // md[64] | bd[64] | status[64]

struct OnlineSvc {
  std::mutex mu;
  bool ready = false, launched = false;
  // set once the service cannot serve (a failed launch, a timed-out request): later requests
  // take the submission queue; read without o.mu by callers waiting for a slot or a verdict
  std::atomic<bool> failed{false};
  bool stuck = false;  // a launch that would not end: its stream and memory are never released
  // Everything the resident kernel touches. mvr::reset frees it once the kernel has ended;
  // abandon() gives it up unfreed when the kernel would not end (leaked on purpose).
  struct Resources {
    HostBuf ctl, req, in, out;  // pinned, coherent: the host views below point into them
    DevBuf dctl, scr;
    mvr::Event exited;
    mvr::Stream stream;
    void abandon() {
      for (HostBuf* b : {&ctl, &req, &in, &out}) b->abandon();
      dctl.abandon();
      scr.abandon();
      exited.abandon();
      stream.abandon();
    }
  } res;
  mvk::OnlineCtl* ctl = nullptr;  // host view
  mvk::OnlineReq* req = nullptr;
  uint8_t* in = nullptr;
  uint8_t* out = nullptr;
  void *ctl_d = nullptr, *req_d = nullptr, *in_d = nullptr, *out_d = nullptr;  // device views
  std::unique_ptr<std::atomic<uint64_t>[]> freed;  // slot released by its owner: request + 1
  // Waiting callers (round 5). At most max_spinners callers spin on their done word; the others
  // sleep on a futex word of their slot, which the reaper thread sets and wakes once the done
  // word holds their request (99 callers spinning on a 16-CPU share descheduled one another
  // for milliseconds: p99 81 ms). A caller waiting for its slot to be freed sleeps the same way.
  int max_spinners = 4;
  std::atomic<int> spinners{0}, sleepers{0};
  std::unique_ptr<std::atomic<uint32_t>[]> dwake;  // per slot: set by the reaper (futex word)
  std::unique_ptr<std::atomic<uint64_t>[]> sleep_q;  // per slot: request + 1 its sleeper waits for, 0: none
  std::unique_ptr<std::atomic<uint32_t>[]> fseq, fwait;  // per slot: frees so far (futex word), sleepers on it
  std::thread reaper;
  std::mutex rmu;
  std::condition_variable rcv;
  bool rstop = false;
  uint64_t next_q = 0;
  uint32_t grid = 0, launch_no = 0;
  std::atomic<uint64_t> requests{0}, launches{0};
  uint64_t idle_us = 10000;
  // MV_ONLINE_TRACE: per-stage sums (us) -- host publish to done seen, and on the kernel's
  // clock seen -> ready -> first claim -> last job done -- printed at release
  bool trace = false, debug = false;  // MV_ONLINE_TRACE, MV_ONLINE_DEBUG
  double ticks_per_us = 100.0;
  std::mutex tr_mu;
  double tr_sum[14] = {};
  uint64_t tr_n = 0;
};

inline Device* find_dev(mv_ctx* ctx, int device) {
  for (auto& d : ctx->devs)
    if (d.id == device) return &d;
  return nullptr;
}

// engine.cpp: the batch policy, the single paths, what every path shares
void poll_flags(mv_ctx* ctx, Device& dev);
mv_status enqueue_batch(mv_ctx* ctx, Device& dev, const uint8_t* d_msg, const uint8_t* d_sig, const uint8_t* d_pk,
                        const uint32_t* d_key_idx, uint32_t n, uint8_t* d_status, hipStream_t s,
                        uint32_t* flag_dst, const mvk::ChunkGate* gate = nullptr, bool caller_stream = false);
mv_status enqueue_verify(mv_ctx* ctx, Device& dev, const uint8_t* d_msg, const uint8_t* d_sig, const uint8_t* d_pk,
                         const uint32_t* d_key_idx, uint32_t n, uint8_t* d_status, hipStream_t s);
mv_status enqueue_committee_verify(mv_ctx* ctx, Device& dev, const uint8_t* d_msg, const uint8_t* d_sig,
                                   const uint32_t* d_kidx, uint32_t n, uint8_t* d_status, hipStream_t s,
                                   const mvk::BlockVerdictOut* bv = nullptr, const mvk::BlockHashIn* hin = nullptr,
                                   const mvk::BlockIngestIn* ing = nullptr);
bool committee_ready(mv_ctx* ctx);
bool host_pinned(const void* p);
bool pinned_range_holds(const void* p, uint64_t bytes);
void reap_idle(mv_ctx* ctx, Device& dev);

// engine_blocks.cpp
mv_status enqueue_blocks(mv_ctx* ctx, Device& dev, const uint8_t* d_buf, uint64_t buf_bytes, const uint64_t* d_off,
                         const uint64_t* d_len, uint32_t n, uint8_t* d_status, uint8_t* d_md, uint8_t* d_bd,
                         hipStream_t s, DevBuf* own = nullptr, Device::BlkAux* own_aux = nullptr);
std::vector<uint64_t> balanced_cuts(const uint64_t* w, uint64_t n, uint32_t parts);

// engine_index.cpp: the table and the accept call, which the three files below build on (each
// function is described where it is defined)
constexpr size_t ix_al(size_t x) { return (x + 255) & ~(size_t)255; }
using Index = Device::Index;
using Pending = Device::Index::Pending;
using Dag = Device::Index::Dag;
mvk::IndexTable table_of(mv_ctx* ctx, const Index& ix);
mv_status index_dev(mv_ctx* ctx, Device*& dev);
mv_status index_ctl(mv_ctx* ctx, Device& dev, hipStream_t s);
mv_status read_ctl(mv_ctx* ctx, Device& dev, hipStream_t s, const uint64_t** words);
mv_status order_behind_ahead(mv_ctx* ctx, Device& dev, hipStream_t s);
mv_status index_room_for_more(mv_ctx* ctx, Device& dev, uint64_t more, bool can_grow, hipStream_t s);
mv_status insert_rounds(mv_ctx* ctx, Device& dev, const mvk::IndexKeys& ks, uint64_t n, uint32_t state, hipStream_t s);
// Where accept_run leaves its results (device memory of dev.index)
struct AcceptOut {
  uint64_t n_missing = 0;
  const uint8_t *status = nullptr, *state = nullptr;
  const uint64_t* missing = nullptr;
  // for the connect call: the call's arrays, the candidates (their slots are in pend.cand_slot) and
  // their includes (whose insert's records are in index.item)
  mvk::AcceptArrays a{};
  uint64_t ncand = 0, ninc = 0;
};
mv_status accept_run(mv_ctx* ctx, Device& dev, const uint8_t* d_buf, uint64_t buf_bytes, const uint64_t* d_off,
                     const uint64_t* d_len, const uint64_t* d_grp, uint32_t n32, uint64_t cap_missing, bool can_grow,
                     hipStream_t s, AcceptOut& out, bool connect = false);
mv_status stage_blocks(mv_ctx* ctx, Device& dev, const uint8_t* buf, const uint64_t* off, const uint64_t* len,
                       const uint64_t* grp, uint32_t n, uint64_t cap_missing, hipStream_t s, AcceptOut& ao, bool connect);

// engine_connect.cpp: the suspended-block store
mvk::PendStore pend_view(const Pending& pd, int k);
mv_status pending_room(mv_ctx* ctx, Device& dev, uint64_t more_b, uint64_t more_i, bool can_grow, hipStream_t s);

// engine_dag.cpp: the DAG store; one seed call (mv_dev_dag_seed_rows) on stream s, which it synchronises; the image,
// the rows and their block verdicts are device memory, seeded (5 words) is the host's
mvk::DagStore dag_view(const Dag& dg, const DevBuf& rec, const DevBuf& inc, uint64_t cap_b, uint64_t cap_i);
mvk::DagStore dag_view(const Dag& dg);
mv_status dag_room(mv_ctx* ctx, Device& dev, uint64_t more_b, uint64_t more_i, hipStream_t s, bool can_grow = true);
mv_status dag_seed_run(mv_ctx* ctx, Device& dev, const uint8_t* d_img, uint64_t size, const uint64_t* d_rows,
                       const uint8_t* d_status, uint64_t n, uint64_t floor_round, bool can_grow, hipStream_t s,
                       uint64_t* seeded);

// engine_linearize.cpp: the committed marks follow the table -- a zeroed array for `slots` slots that, with
// marks set, takes over those of the table in force (old_slots of them) under the new table nt. The
// caller swaps it into dg.lmark once s has been synchronised.
mv_status linear_marks_for(mv_ctx* ctx, Device& dev, uint64_t old_slots, const mvk::IndexTable& nt, uint64_t slots,
                           DevBuf& fresh, hipStream_t s);

// engine_propose.cpp: the proposer's state follows the table -- its slots (queue, own last block,
// outstanding choice) of the table in force (old_slots of them) become those of the same keys under
// the new table nt, on s; the stamps are remade by the next take. And mv_index_clear's part.
using Propose = Device::Index::Propose;
mv_status propose_follow_table(mv_ctx* ctx, Device& dev, uint64_t old_slots, const mvk::IndexTable& nt, hipStream_t s);
mv_status propose_clear(mv_ctx* ctx, Device& dev, hipStream_t s);

// engine_seal.cpp: one seal call on device arrays, on stream s, which it synchronises (d_md / d_bd may
// be null); mv_encode_blocks seals its image through it
constexpr uint32_t kMaxSealAuth = 1u << 20;
mv_status seal_run(mv_ctx* ctx, Device& dev, uint8_t* d_buf, uint64_t buf_bytes, const uint64_t* d_off,
                   const uint64_t* d_len, uint32_t n, const uint8_t* d_seeds, uint32_t n_auth, uint32_t flags,
                   uint8_t* d_status, uint8_t* d_md, uint8_t* d_bd, hipStream_t s);

// engine_online.cpp
bool online_eligible(mv_ctx* ctx, uint32_t n, uint64_t bytes, uint64_t longest);
mv_status online_verify(mv_ctx* ctx, Device& dev, const uint8_t* buf, const uint64_t* off, const uint64_t* len,
                        uint32_t n, uint8_t* status, uint8_t* md, uint8_t* bd);
bool online_stop(OnlineSvc& o);
void online_release(OnlineSvc& o);

}  // namespace mvi
