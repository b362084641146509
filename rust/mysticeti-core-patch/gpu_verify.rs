//! mysticeti-core/src/gpu_verify.rs (new file): StatementBlock::verify on the MI355X engine.
//!
//! One `mv_verify_blocks` call checks a whole message worth of blocks on the GPU (bincode
//! parse, both BLAKE2b-256 digests, the ZIP-215 signature and every structural check, in the
//! order of types.rs:315-376). The engine returns one status per block; this wrapper turns a
//! failing status back into the exact `eyre` error `StatementBlock::verify` would have
//! returned. The message text needs the failing values (digests, the include, the range), so
//! for a rejected block the wrapper re-reads them host-side -- only on that failure path.
use std::sync::atomic::{AtomicU64, Ordering};
use std::sync::Arc;

use eyre::{bail, ensure};
use mysti_verify_sys as sys;

use crate::committee::Committee;
use crate::crypto::BlockDigest;
use crate::data::Data;
use crate::serde::ByteRepr; // serde.rs:8-14
use crate::types::{BaseStatement, StatementBlock};

pub struct GpuVerifier {
    ctx: *mut sys::mv_ctx,
    // the blocks `connect_blocks` left suspended (an upper bound): sizes its row buffer without a
    // device round trip. Connect calls are the core's and come one at a time.
    suspended: AtomicU64,
}
// mv_* calls are thread-safe on one context; concurrent callers are merged by the engine's
// submission queue (one device pass serves all of them)
unsafe impl Send for GpuVerifier {}
unsafe impl Sync for GpuVerifier {}

impl Drop for GpuVerifier {
    fn drop(&mut self) {
        unsafe { sys::mv_destroy(self.ctx) }
    }
}

impl GpuVerifier {
    /// Opens the devices in `device_mask` and loads the committee (keys decoded once per
    /// device, as Committee::load decodes each VerificationKey once, committee.rs:83-87).
    pub fn new(committee: &Committee, device_mask: u32) -> eyre::Result<Arc<Self>> {
        let mut ctx = std::ptr::null_mut();
        let cfg = sys::mv_config { device_mask, ..Default::default() };
        ensure!(unsafe { sys::mv_create(&cfg, &mut ctx) } == sys::MV_OK, "no gfx950 device in mask {device_mask:#x}");
        let me = Self { ctx, suspended: AtomicU64::new(0) };
        let pks: Vec<u8> = committee
            .authorities()
            .flat_map(|a| committee.get_public_key(a).unwrap().0.as_bytes().to_vec())
            .collect();
        let stakes: Vec<u64> = committee.authorities().map(|a| committee.get_stake(a).unwrap()).collect();
        let rc = unsafe {
            sys::mv_set_committee(me.ctx, pks.as_ptr(), stakes.as_ptr(), stakes.len() as u32, committee.epoch(),
                                  std::ptr::null_mut())
        };
        ensure!(rc == sys::MV_OK, "mv_set_committee: {}", me.last_error());
        Ok(Arc::new(me))
    }

    fn last_error(&self) -> String {
        unsafe { std::ffi::CStr::from_ptr(sys::mv_last_error(self.ctx)) }.to_string_lossy().into_owned()
    }

    /// StatementBlock::verify (types.rs:315-376) for every block, same results, same errors.
    pub fn verify_blocks(&self, blocks: &[Data<StatementBlock>], committee: &Committee) -> Vec<eyre::Result<()>> {
        let mut buf = Vec::new();
        let mut off = Vec::with_capacity(blocks.len());
        let mut len = Vec::with_capacity(blocks.len());
        for b in blocks {
            off.push(buf.len() as u64);
            len.push(b.serialized_bytes().len() as u64);
            buf.extend_from_slice(b.serialized_bytes());
        }
        let mut status = vec![0u8; blocks.len()];
        let mut digest = vec![0u8; 32 * blocks.len()];
        let rc = unsafe {
            sys::mv_verify_blocks(self.ctx, buf.as_ptr(), off.as_ptr(), len.as_ptr(), blocks.len() as u32,
                                  status.as_mut_ptr(), std::ptr::null_mut(), digest.as_mut_ptr())
        };
        if rc != sys::MV_OK {
            let e = self.last_error();
            return blocks.iter().map(|_| Err(eyre::eyre!("GPU verifier failed: {e}"))).collect();
        }
        blocks
            .iter()
            .zip(status)
            .zip(digest.chunks(32))
            .map(|((b, s), d)| verdict_to_result(b, s, d, committee))
            .collect()
    }

    /// What the reference does with the received bytes of many connections, per message
    /// (handle_read_stream + the NetworkMessage decode, network.rs:400-457; process_blocks,
    /// net_sync.rs:314-383): `streams[s]` = (offset, length) of connection s's bytes in `buf`.
    /// One mv_verify_frames call walks the frames, verifies the blocks in place and returns the
    /// message rows (8 words each, include/mysti_verify.h), per connection the consumed bytes and
    /// the first row that is not MV_MSG_OK (u32::MAX: keep the connection), and the listed blocks.
    pub fn verify_frames(&self, buf: &[u8], streams: &[(u64, u64)]) -> eyre::Result<FrameVerdicts> {
        let soff: Vec<u64> = streams.iter().map(|s| s.0).collect();
        let slen: Vec<u64> = streams.iter().map(|s| s.1).collect();
        ensure!(streams.iter().all(|s| s.0 <= buf.len() as u64 && s.1 <= buf.len() as u64 - s.0), "stream out of buf");
        let ns = streams.len();
        let mut out = FrameVerdicts { consumed: vec![0; ns], drop_msg: vec![0; ns], ..Default::default() };
        let (mut cap_m, mut cap_b) = (1024usize, 4096usize);
        loop {
            out.rows.resize(8 * cap_m, 0);
            out.blk_off.resize(cap_b, 0);
            out.blk_len.resize(cap_b, 0);
            out.blk_status.resize(cap_b, 0);
            let (mut n_msgs, mut n_blocks) = (0u64, 0u64);
            let rc = unsafe {
                sys::mv_verify_frames(self.ctx, buf.as_ptr(), soff.as_ptr(), slen.as_ptr(), ns as u32,
                                      out.consumed.as_mut_ptr(), out.drop_msg.as_mut_ptr(), out.rows.as_mut_ptr(),
                                      cap_m as u64, &mut n_msgs, out.blk_off.as_mut_ptr(), out.blk_len.as_mut_ptr(),
                                      out.blk_status.as_mut_ptr(), cap_b as u64, &mut n_blocks)
            };
            ensure!(rc == sys::MV_OK, "mv_verify_frames: {}", self.last_error());
            let (m, b) = (n_msgs as usize, n_blocks as usize);
            if m <= cap_m && b <= cap_b {
                out.rows.truncate(8 * m);
                out.blk_off.truncate(b);
                out.blk_len.truncate(b);
                out.blk_status.truncate(b);
                return Ok(out);
            }
            // the totals always come back: once more with room for all of them
            cap_m = cap_m.max(m);
            cap_b = cap_b.max(b);
        }
    }

    /// The replay loop of BlockStore::open (block_store.rs:50-116) over a WAL image, up to the
    /// writer position `end_pos`: one mv_wal_replay call walks the entries, checks their crc,
    /// decodes and verifies every WAL_ENTRY_BLOCK / WAL_ENTRY_OWN_BLOCK block in place and returns
    /// the entries, one row per block (its BlockReference for add_unloaded, next_entry of an own
    /// block), highest_round, last_seen_by_authority and the positions RecoveredStateBuilder
    /// wants. The caller still decodes payload, state and commit entries (tags 2, 4, 5) and keeps
    /// the `pending` map from pos, the tags and next_entry (state.rs:39-59). An entry whose
    /// status is not MV_WAL_OK -- always the last -- is where the reference panics.
    pub fn wal_replay(&self, wal: &[u8], end_pos: u64, map_bits: u32, committee_size: usize) -> eyre::Result<WalReplay> {
        let cap = wal.len() / 16 + 1; // an entry takes at least its 16-byte header
        let mut out = WalReplay {
            pos: vec![0; cap],
            tag: vec![0; cap],
            len: vec![0; cap],
            status: vec![0; cap],
            rows: vec![0; 10 * cap],
            blk_status: vec![0; cap],
            summary: [0; 3],
            last_seen: vec![0; committee_size],
        };
        let (mut count, mut n_blocks) = (0u64, 0u64);
        let rc = unsafe {
            sys::mv_wal_replay(self.ctx, wal.as_ptr(), wal.len() as u64, end_pos, map_bits, out.pos.as_mut_ptr(),
                               out.tag.as_mut_ptr(), out.len.as_mut_ptr(), out.status.as_mut_ptr(), cap as u64,
                               &mut count, out.rows.as_mut_ptr(), out.blk_status.as_mut_ptr(), cap as u64,
                               &mut n_blocks, out.summary.as_mut_ptr(), out.last_seen.as_mut_ptr())
        };
        ensure!(rc == sys::MV_OK, "mv_wal_replay: {}", self.last_error());
        let (n, b) = (count as usize, n_blocks as usize);
        out.pos.truncate(n);
        out.tag.truncate(n);
        out.len.truncate(n);
        out.status.truncate(n);
        out.rows.truncate(10 * b);
        out.blk_status.truncate(b);
        Ok(out)
    }

    /// `wal_replay`, then the replayed blocks become stored blocks with records in the DAG store
    /// (mv_wal_recover: BlockStore::open with add_unloaded, block_store.rs:398-404, as what makes a
    /// replayed block visible to BaseCommitter). Needs `dag_reserve`. `floor_round`: rows of lower
    /// rounds get no record, as after `dag_prune`. The five words: the references raised to
    /// MV_REF_STORED, the records appended and their includes, the includes no row of the WAL holds
    /// (0 for a WAL this node wrote), and verified rows whose bytes did not fit the image.
    pub fn wal_recover(&self, wal: &[u8], end_pos: u64, map_bits: u32, committee_size: usize,
                       floor_round: u64) -> eyre::Result<(WalReplay, [u64; 5])> {
        let cap = wal.len() / 16 + 1;
        let mut out = WalReplay {
            pos: vec![0; cap],
            tag: vec![0; cap],
            len: vec![0; cap],
            status: vec![0; cap],
            rows: vec![0; 10 * cap],
            blk_status: vec![0; cap],
            summary: [0; 3],
            last_seen: vec![0; committee_size],
        };
        let (mut count, mut n_blocks, mut seeded) = (0u64, 0u64, [0u64; 5]);
        let rc = unsafe {
            sys::mv_wal_recover(self.ctx, wal.as_ptr(), wal.len() as u64, end_pos, map_bits, out.pos.as_mut_ptr(),
                                out.tag.as_mut_ptr(), out.len.as_mut_ptr(), out.status.as_mut_ptr(), cap as u64,
                                &mut count, out.rows.as_mut_ptr(), out.blk_status.as_mut_ptr(), cap as u64,
                                &mut n_blocks, out.summary.as_mut_ptr(), out.last_seen.as_mut_ptr(), floor_round,
                                seeded.as_mut_ptr())
        };
        ensure!(rc == sys::MV_OK, "mv_wal_recover: {}", self.last_error());
        let (n, b) = (count as usize, n_blocks as usize);
        out.pos.truncate(n);
        out.tag.truncate(n);
        out.len.truncate(n);
        out.status.truncate(n);
        out.rows.truncate(10 * b);
        out.blk_status.truncate(b);
        Ok((out, seeded))
    }

    /// Seeds the index of block references with references the store holds (MV_REF_HAVE): the
    /// genesis references, and after a replay the rows' words 3..8 (BlockStore::open's
    /// add_unloaded, block_store.rs:398-404). `refs` holds six words per reference: authority,
    /// round, the four little-endian digest words.
    pub fn index_insert_have(&self, refs: &[u64]) -> eyre::Result<()> {
        ensure!(refs.len() % 6 == 0, "six words per reference");
        let rc = unsafe {
            sys::mv_index_insert(self.ctx, refs.as_ptr(), (refs.len() / 6) as u64, sys::MV_REF_HAVE as u32,
                                 std::ptr::null_mut())
        };
        ensure!(rc == sys::MV_OK, "mv_index_insert: {}", self.last_error());
        Ok(())
    }

    /// Seeds references of blocks that are in the store as MV_REF_STORED: what a caller of
    /// `connect_blocks` uses in place of `index_insert_have` for the genesis references and a
    /// replay's rows, and for its own proposed block (then `connect_blocks` with no blocks sweeps).
    /// A context seeded with MV_REF_HAVE never connects anything.
    pub fn index_insert_stored(&self, refs: &[u64]) -> eyre::Result<()> {
        ensure!(refs.len() % 6 == 0, "six words per reference");
        let rc = unsafe {
            sys::mv_index_insert_stored(self.ctx, refs.as_ptr(), (refs.len() / 6) as u64, std::ptr::null_mut())
        };
        ensure!(rc == sys::MV_OK, "mv_index_insert_stored: {}", self.last_error());
        Ok(())
    }

    /// BlockManager::missing_blocks (block_manager.rs:138-140) as the index holds it: the
    /// MV_REF_WANTED references, six words each, in no particular order.
    pub fn index_wanted(&self) -> eyre::Result<Vec<u64>> {
        let mut n = 0u64;
        let rc = unsafe { sys::mv_index_wanted(self.ctx, std::ptr::null_mut(), 0, &mut n) };
        ensure!(rc == sys::MV_OK, "mv_index_wanted: {}", self.last_error());
        let mut out = vec![0u64; 6 * n as usize];
        let rc = unsafe { sys::mv_index_wanted(self.ctx, out.as_mut_ptr(), n, &mut n) };
        ensure!(rc == sys::MV_OK, "mv_index_wanted: {}", self.last_error());
        out.truncate(6 * n as usize);
        Ok(out)
    }

    /// process_blocks (net_sync.rs:314-386) for the blocks of several received messages in one
    /// call: the `processed` query and skip (:325-336), StatementBlock::verify of the others, the
    /// early return of a message with a rejected block (:352-361), and the include lookups of
    /// BlockManager::add_blocks (block_manager.rs:62-98) whose result the syncer requests from
    /// peers (net_sync.rs:388-398). `groups[i]` names the message of block i (non-decreasing).
    /// The caller hands the MV_ACC_NEW blocks to the core, which keeps the suspend / unlock
    /// cascade (blocks_pending) and the WAL write; `connect_blocks` runs the cascade too.
    pub fn accept_blocks(&self, buf: &[u8], blocks: &[(u64, u64)], groups: &[u64]) -> eyre::Result<Accepted> {
        ensure!(groups.len() == blocks.len(), "one group word per block");
        let n = blocks.len();
        let off: Vec<u64> = blocks.iter().map(|b| b.0).collect();
        let len: Vec<u64> = blocks.iter().map(|b| b.1).collect();
        let mut out = Accepted { blk_status: vec![0; n], blk_state: vec![0; n], missing: Vec::new() };
        let cap = 64 * n.max(1);
        out.missing.resize(6 * cap, 0);
        let mut n_missing = 0u64;
        let rc = unsafe {
            sys::mv_accept_blocks(self.ctx, buf.as_ptr(), off.as_ptr(), len.as_ptr(), groups.as_ptr(), n as u32,
                                  out.blk_status.as_mut_ptr(), out.blk_state.as_mut_ptr(), out.missing.as_mut_ptr(),
                                  cap as u64, &mut n_missing)
        };
        ensure!(rc == sys::MV_OK, "mv_accept_blocks: {}", self.last_error());
        if n_missing as usize <= cap {
            out.missing.truncate(6 * n_missing as usize);
        } else {
            // the list was cut: the index holds these references as WANTED already (a second accept
            // call would find every block KNOWN), so the whole set comes from there
            out.missing = self.index_wanted()?;
        }
        Ok(out)
    }

    /// The whole of BlockManager::add_blocks but the block bodies and the WAL write
    /// (mv_connect_blocks): `accept_blocks`, then the suspend / unlock cascade
    /// (block_manager.rs:102-131) over the suspended blocks the context keeps in device memory.
    /// The rows name the blocks the core may process now, in an order in which every include comes
    /// before its includer: the caller appends them to its WAL and hands them on in that order,
    /// keeping the bodies of MV_ACC_SUSPENDED blocks by reference until a later call lists them.
    /// No blocks: a sweep alone.
    pub fn connect_blocks(&self, buf: &[u8], blocks: &[(u64, u64)], groups: &[u64]) -> eyre::Result<Connected> {
        ensure!(groups.len() == blocks.len(), "one group word per block");
        let n = blocks.len();
        let off: Vec<u64> = blocks.iter().map(|b| b.0).collect();
        let len: Vec<u64> = blocks.iter().map(|b| b.1).collect();
        let before = self.suspended.load(Ordering::Relaxed);
        let cap_rows = n + before as usize; // every row: this call's blocks and the suspended ones
        let mut acc = Accepted { blk_status: vec![0; n], blk_state: vec![0; n], missing: Vec::new() };
        let cap = 64 * n.max(1);
        acc.missing.resize(6 * cap, 0);
        let mut connected = vec![0u64; 8 * cap_rows.max(1)];
        let (mut n_missing, mut n_connected) = (0u64, 0u64);
        let rc = unsafe {
            sys::mv_connect_blocks(self.ctx, buf.as_ptr(), off.as_ptr(), len.as_ptr(), groups.as_ptr(), n as u32,
                                   acc.blk_status.as_mut_ptr(), acc.blk_state.as_mut_ptr(), acc.missing.as_mut_ptr(),
                                   cap as u64, &mut n_missing, connected.as_mut_ptr(), cap_rows as u64,
                                   &mut n_connected)
        };
        ensure!(rc == sys::MV_OK, "mv_connect_blocks: {}", self.last_error());
        if n_missing as usize <= cap {
            acc.missing.truncate(6 * n_missing as usize);
        } else {
            acc.missing = self.index_wanted()?;
        }
        connected.truncate(8 * n_connected as usize);
        // every NEW block joined the store (parked ones say SUSPENDED), every row left it
        let joined = acc.blk_state.iter().filter(|&&s| s == sys::MV_ACC_NEW || s == sys::MV_ACC_SUSPENDED).count() as u64;
        self.suspended.store((before + joined).saturating_sub(n_connected), Ordering::Relaxed);
        Ok(Connected { accepted: acc, connected })
    }
}

impl GpuVerifier {
    /// Keeps the edges of what `connect_blocks` connects in device memory (mv_dag_reserve): the
    /// store `decide_leaders` reads. Call once, before the first connect call.
    pub fn dag_reserve(&self, blocks: u64, includes: u64) -> eyre::Result<()> {
        let rc = unsafe { sys::mv_dag_reserve(self.ctx, blocks, includes) };
        ensure!(rc == sys::MV_OK, "mv_dag_reserve: {}", self.last_error());
        Ok(())
    }

    /// BlockStore::cleanup for the DAG store (mv_dag_prune): drops the records below `round`.
    pub fn dag_prune(&self, round: u64) -> eyre::Result<()> {
        let rc = unsafe { sys::mv_dag_prune(self.ctx, round) };
        ensure!(rc == sys::MV_OK, "mv_dag_prune: {}", self.last_error());
        Ok(())
    }

    /// BaseCommitter::try_direct_decide (consensus/base_committer.rs:323-357) for every elected
    /// leader (authority, round) of `leaders`, on the GPU (mv_decide_leaders). The caller elects
    /// the leaders, and runs try_indirect_decide and the longest-decided-prefix rule on the rows
    /// (`commit_leaders` does both; the linearizer is `linearize`); an MV_LEADER_OVERFLOW row it
    /// decides itself.
    pub fn decide_leaders(&self, leaders: &[(u64, u64)]) -> eyre::Result<Decided> {
        let n = leaders.len();
        let flat: Vec<u64> = leaders.iter().flat_map(|&(a, r)| [a, r]).collect();
        let mut d = Decided { rows: vec![0u64; 8 * n], stakes: vec![0u64; 3 * n] };
        let rc = unsafe {
            sys::mv_decide_leaders(self.ctx, flat.as_ptr(), n as u32, d.rows.as_mut_ptr(), d.stakes.as_mut_ptr())
        };
        ensure!(rc == sys::MV_OK, "mv_decide_leaders: {}", self.last_error());
        Ok(d)
    }

    /// UniversalCommitter::try_commit (consensus/universal_committer.rs:30-90) on the GPU
    /// (mv_commit_leaders): the direct rule, try_indirect_decide and the decided prefix for the
    /// elected leaders (authority, round) of `leaders`, which stand in the order try_commit's deque
    /// ends in: ascending round, within a round in committer order, after last_decided. The caller
    /// elects the leaders, keeps last_decided and hands the committed references of the first
    /// `n_sequence` rows of round > 0 to `linearize`; a row with MV_COMMIT_INCOMPLETE it decides
    /// itself once the store holds the missing blocks.
    pub fn commit_leaders(&self, leaders: &[(u64, u64)]) -> eyre::Result<Committed> {
        let n = leaders.len();
        let flat: Vec<u64> = leaders.iter().flat_map(|&(a, r)| [a, r]).collect();
        let mut c = Committed { rows: vec![0u64; 8 * n], info: vec![0u64; 4 * n], n_sequence: 0 };
        let rc = unsafe {
            sys::mv_commit_leaders(self.ctx, flat.as_ptr(), n as u32, c.rows.as_mut_ptr(), c.info.as_mut_ptr(),
                                   &mut c.n_sequence)
        };
        ensure!(rc == sys::MV_OK, "mv_commit_leaders: {}", self.last_error());
        Ok(c)
    }

    /// Linearizer::handle_commit (consensus/linearizer.rs:125-166) on the GPU (mv_linearize): the
    /// sub-DAG of every committed leader block of `leaders` (six words per reference, in sequence
    /// order), in the reference's order; at most `cap` blocks in all. The committed marks and
    /// last_height live in the engine. A row that is not MV_LINEAR_OK the caller linearizes itself
    /// and reports with `linearize_mark`.
    pub fn linearize(&self, leaders: &[[u64; 6]], cap: usize) -> eyre::Result<Linearized> {
        let n = leaders.len();
        let flat: Vec<u64> = leaders.iter().flatten().copied().collect();
        let mut l = Linearized { blocks: vec![0u64; 6 * cap.max(1)], sub: vec![0u64; 4 * n], n_rows: 0 };
        let rc = unsafe {
            sys::mv_linearize(self.ctx, flat.as_ptr(), n as u32, l.blocks.as_mut_ptr(), cap as u64, l.sub.as_mut_ptr(),
                              &mut l.n_rows)
        };
        ensure!(rc == sys::MV_OK, "mv_linearize: {}", self.last_error());
        l.blocks.truncate(6 * l.n_rows as usize);
        Ok(l)
    }

    /// Linearizer::recover_state (linearizer.rs:108-121): marks `refs` as committed and raises
    /// last_height to `height` (mv_linearize_mark).
    pub fn linearize_mark(&self, refs: &[[u64; 6]], height: u64) -> eyre::Result<()> {
        let flat: Vec<u64> = refs.iter().flatten().copied().collect();
        let rc = unsafe { sys::mv_linearize_mark(self.ctx, flat.as_ptr(), refs.len() as u64, height) };
        ensure!(rc == sys::MV_OK, "mv_linearize_mark: {}", self.last_error());
        Ok(())
    }

    /// (marked references, last_height) (mv_linearize_stats)
    pub fn linearize_stats(&self) -> eyre::Result<(u64, u64)> {
        let mut out = [0u64; 2];
        let rc = unsafe { sys::mv_linearize_stats(self.ctx, out.as_mut_ptr()) };
        ensure!(rc == sys::MV_OK, "mv_linearize_stats: {}", self.last_error());
        Ok((out[0], out[1]))
    }

    /// Opts in to the proposer's state for `authority` (mv_propose_reserve): the clock of
    /// ThresholdClockAggregator::new(0), an empty `pending` queue with room for `entries`.
    pub fn propose_reserve(&self, authority: u32, entries: u64) -> eyre::Result<()> {
        let rc = unsafe { sys::mv_propose_reserve(self.ctx, authority, entries) };
        ensure!(rc == sys::MV_OK, "mv_propose_reserve: {}", self.last_error());
        Ok(())
    }

    /// The loop of Core::add_blocks (core.rs:181-200) over `rows` (`stride` words each, the reference
    /// in words 0-5: `Connected::connected` at a stride of 8) with their WAL positions `tags`, and with
    /// `payload` the entry of run_block_handler (core.rs:223-224). `in_order` skips the sort by round
    /// (Core::open's replay, core.rs:90-94, 104-109). Returns (clock round, stake, voters, queue length).
    pub fn propose_add(&self, rows: &[u64], stride: usize, tags: Option<&[u64]>, in_order: bool,
                       payload: Option<u64>) -> eyre::Result<[u64; 4]> {
        ensure!(stride >= 6 && rows.len() % stride == 0, "propose_add: rows of {stride} words");
        let n = rows.len() / stride;
        ensure!(tags.map_or(true, |t| t.len() == n), "propose_add: one tag per row");
        let flags = if in_order { sys::MV_PROPOSE_IN_ORDER } else { 0 } | if payload.is_some() { sys::MV_PROPOSE_PAYLOAD } else { 0 };
        let mut out = [0u64; 4];
        let rc = unsafe {
            sys::mv_propose_add(self.ctx, rows.as_ptr(), n as u64, stride as u64, tags.map_or(std::ptr::null(), |t| t.as_ptr()),
                                flags, payload.unwrap_or(0), out.as_mut_ptr())
        };
        ensure!(rc == sys::MV_OK, "mv_propose_add: {}", self.last_error());
        Ok(out)
    }

    /// The include choice of Core::try_new_block (core.rs:232-278) (mv_propose_take). The own last
    /// block is not among the includes: the caller puts it first (:264).
    pub fn propose_take(&self, cap: usize, cap_payloads: usize) -> eyre::Result<Proposal> {
        let mut p = Proposal { includes: vec![0u64; 6 * cap.max(1)], payloads: vec![0u64; cap_payloads.max(1)], out: [0u64; 6] };
        let (mut ni, mut np) = (0u64, 0u64);
        let rc = unsafe {
            sys::mv_propose_take(self.ctx, p.includes.as_mut_ptr(), cap as u64, &mut ni, p.payloads.as_mut_ptr(),
                                 cap_payloads as u64, &mut np, p.out.as_mut_ptr())
        };
        ensure!(rc == sys::MV_OK, "mv_propose_take: {}", self.last_error());
        p.includes.truncate(6 * (ni as usize).min(cap));
        p.payloads.truncate((np as usize).min(cap_payloads));
        Ok(p)
    }

    /// The own block after it was sealed (core.rs:307-320) (mv_propose_own); `includes` None: the own
    /// last block followed by the outstanding take's choice. Returns as `propose_add`.
    pub fn propose_own(&self, block_ref: &[u64; 6], includes: Option<&[[u64; 6]]>) -> eyre::Result<[u64; 4]> {
        let flat: Vec<u64> = includes.map_or(vec![], |i| i.iter().flatten().copied().collect());
        let mut out = [0u64; 4];
        let dummy = [0u64; 6];
        let ptr = match includes {
            None => std::ptr::null(),
            Some(i) if i.is_empty() => dummy.as_ptr(),
            Some(_) => flat.as_ptr(),
        };
        let rc = unsafe { sys::mv_propose_own(self.ctx, block_ref.as_ptr(), ptr, includes.map_or(0, |i| i.len()) as u64, out.as_mut_ptr()) };
        ensure!(rc == sys::MV_OK, "mv_propose_own: {}", self.last_error());
        Ok(out)
    }

    /// (clock round, stake, voters, queue length, own last round, outstanding, takes, dropped) (mv_propose_stats)
    pub fn propose_stats(&self) -> eyre::Result<[u64; 8]> {
        let mut out = [0u64; 8];
        let rc = unsafe { sys::mv_propose_stats(self.ctx, out.as_mut_ptr()) };
        ensure!(rc == sys::MV_OK, "mv_propose_stats: {}", self.last_error());
        Ok(out)
    }
}

/// Result of `GpuVerifier::propose_take` (layout: include/mysti_verify.h, mv_propose_take).
pub struct Proposal {
    pub includes: Vec<u64>, // six words per reference, in queue order, without the own last block
    pub payloads: Vec<u64>, // the tokens of the taken payload entries
    pub out: [u64; 6],      // proposed, the clock round, entries taken, MV_PROPOSE_* flags, next_entry, queue length
}

/// Result of `GpuVerifier::linearize` (layout: include/mysti_verify.h, mv_linearize).
pub struct Linearized {
    pub blocks: Vec<u64>, // six words per block, the sub-DAGs one behind the other
    pub sub: Vec<u64>,    // four per leader: MV_LINEAR_*, first row, count, height
    pub n_rows: u64,
}

/// Result of `GpuVerifier::commit_leaders` (layout: include/mysti_verify.h, mv_commit_leaders).
pub struct Committed {
    pub rows: Vec<u64>,  // eight words per leader, as Decided's
    pub info: Vec<u64>,  // four per leader: MV_COMMIT_KIND_*, the anchor's row or u64::MAX, the flags, the reach
    pub n_sequence: u64, // the decided prefix over the rows of round > 0
}

/// Result of `GpuVerifier::decide_leaders` (layout: include/mysti_verify.h, mv_decide_leaders).
pub struct Decided {
    pub rows: Vec<u64>,   // eight words per leader: the committed reference, MV_LEADER_*, leader blocks found
    pub stakes: Vec<u64>, // three per leader: blame, vote and certificate stake
}

/// Result of `GpuVerifier::connect_blocks` (layout: include/mysti_verify.h, mv_connect_blocks).
pub struct Connected {
    pub accepted: Accepted,  // blk_state: MV_ACC_SUSPENDED for the blocks that wait in the store
    pub connected: Vec<u64>, // eight words per row, in causal order: the reference, the block's index
                             // in this call or u64::MAX (an earlier call suspended it), its level
}

/// Result of `GpuVerifier::accept_blocks` (layout: include/mysti_verify.h, mv_accept_blocks).
pub struct Accepted {
    pub blk_status: Vec<u8>, // MV_BLOCK_*, MV_BLOCK_OK for blocks skipped as known
    pub blk_state: Vec<u8>,  // MV_ACC_*
    pub missing: Vec<u64>,   // six words per reference to request from peers
}

/// Result of `GpuVerifier::wal_replay` (layout: include/mysti_verify.h, mv_wal_replay).
pub struct WalReplay {
    pub pos: Vec<u64>,       // per entry: WalPosition.start
    pub tag: Vec<u32>,
    pub len: Vec<u32>,       // payload bytes
    pub status: Vec<u8>,     // MV_WAL_*; only the last entry can be other than MV_WAL_OK
    pub rows: Vec<u64>,      // 10 words per block: entry, offset, length, authority, round, digest[4], next_entry
    pub blk_status: Vec<u8>, // MV_BLOCK_* of StatementBlock::verify (the reference's replay does not verify)
    pub summary: [u64; 3],   // highest_round, last own row or u64::MAX, last state entry or u64::MAX
    pub last_seen: Vec<u64>, // last_seen_by_authority
}

/// Result of `GpuVerifier::verify_frames` (layout: include/mysti_verify.h, mv_verify_frames).
#[derive(Default)]
pub struct FrameVerdicts {
    pub rows: Vec<u32>,      // 8 words per message
    pub consumed: Vec<u64>,  // per connection
    pub drop_msg: Vec<u32>,  // per connection: first row not MV_MSG_OK, or u32::MAX
    pub blk_off: Vec<u64>,
    pub blk_len: Vec<u64>,
    pub blk_status: Vec<u8>, // MV_BLOCK_*
}

impl FrameVerdicts {
    /// MV_MSG_* of row r.
    pub fn status(&self, r: usize) -> u32 {
        self.rows[8 * r + 6] & 0xff
    }
}

/// The blocks of one stream of received network frames (network.rs:400-447: u32 BE size + bincode
/// NetworkMessage) as a flat list of (offsets, lengths) into `buf`, and the bytes of the complete
/// frames, for mv_verify_blocks on the same buffer. This is NOT what the reference does with a
/// connection: the list carries no message index (so "the first rejected block ends its message",
/// net_sync.rs:352-361, has to be rebuilt by the caller), an unparsable block's siblings are still
/// listed although the reference fails the whole message (data.rs:83-96, network.rs:454-457), and
/// Subscribe / RequestBlocks / BlockNotFound bodies are skipped unchecked. Use
/// `GpuVerifier::verify_frames` (mv_verify_frames) for the reference's per-message behaviour. An
/// error where a size, a tag or a block length makes handle_read_stream drop the connection.
pub fn frame_blocks(buf: &[u8]) -> eyre::Result<(Vec<u64>, Vec<u64>, usize)> {
    let mut consumed = 0u64;
    let n = unsafe {
        sys::mv_frame_blocks(buf.as_ptr(), buf.len() as u64, std::ptr::null_mut(), std::ptr::null_mut(), 0,
                             &mut consumed)
    };
    ensure!(n >= 0, "malformed frame stream");
    let mut off = vec![0u64; n as usize];
    let mut len = vec![0u64; n as usize];
    unsafe {
        sys::mv_frame_blocks(buf.as_ptr(), buf.len() as u64, off.as_mut_ptr(), len.as_mut_ptr(), n as u64,
                             &mut consumed)
    };
    Ok((off, len, consumed as usize))
}

/// The error StatementBlock::verify returns for the check the engine reports as failing.
fn verdict_to_result(block: &StatementBlock, status: u8, digest: &[u8], committee: &Committee) -> eyre::Result<()> {
    let round = block.round();
    match status {
        sys::MV_BLOCK_OK => Ok(()),
        // types.rs:327-332
        sys::MV_BLOCK_DIGEST_MISMATCH => bail!(
            "Digest does not match, calculated {:?}, provided {:?}",
            <BlockDigest as ByteRepr>::try_copy_from_slice::<serde::de::value::Error>(digest).unwrap(),
            block.digest()
        ),
        // types.rs:333-338
        sys::MV_BLOCK_EPOCH_MISMATCH => bail!(
            "Block's epoch {} doesn't match committee epoch {}",
            block.epoch(),
            committee.epoch()
        ),
        // types.rs:339-342
        sys::MV_BLOCK_UNKNOWN_AUTHOR => bail!("Unknown block author {}", block.author()),
        // types.rs:343-345
        sys::MV_BLOCK_GENESIS => bail!("Genesis block should not go through verification"),
        // types.rs:346-348 (committee keys decode at Committee::load, so the error is InvalidSignature)
        sys::MV_BLOCK_SIG_INVALID => bail!(
            "Block signature verification has failed: {:?}",
            ed25519_consensus::Error::InvalidSignature
        ),
        // types.rs:349-362: the first failing include, checked in the reference's order
        sys::MV_BLOCK_INCLUDE_UNKNOWN_AUTHORITY | sys::MV_BLOCK_INCLUDE_ROUND => {
            for include in block.includes() {
                ensure!(
                    committee.known_authority(include.authority),
                    "Include {:?} references unknown authority",
                    include
                );
                ensure!(
                    include.round < round,
                    "Include {:?} round is greater or equal to own round {}",
                    include,
                    round
                );
            }
            unreachable!("engine reported a failing include")
        }
        // types.rs:363-370 -> VoteRange::verify (types.rs:440-460): its own error, first failing range
        sys::MV_BLOCK_VOTE_RANGE | sys::MV_BLOCK_VOTE_RANGE_TOO_LONG | sys::MV_BLOCK_VOTE_RANGE_END_TOO_LARGE => {
            for statement in block.statements() {
                if let BaseStatement::VoteRange(range) = statement {
                    range.verify()?;
                }
            }
            unreachable!("engine reported a failing VoteRange")
        }
        // types.rs:371-374
        sys::MV_BLOCK_THRESHOLD_CLOCK => bail!("Threshold clock is not valid"),
        // bincode::deserialize failed (Data::from_bytes, data.rs:43-52, happens before verify in
        // the reference); blocks arriving here were already deserialized, so this is unreachable
        _ => bail!("block bytes do not deserialize"),
    }
}
