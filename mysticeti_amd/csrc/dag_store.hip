// The DAG store (mv_dag_reserve, mv_dag_prune, mv_dev_dag_seed_rows): the edges of the blocks
// mv_connect_blocks stored. A record holds slots of the table, as PendStore does; map[] gives the
// record of a slot. The memory model is index_dev.h's. Every slot number is checked against the
// table size and every record number against the store's count before it is an address; a number
// out of range counts into the error word (MV_E_HIP) and is not followed.
//   k_dg_app_*   a connect call's rows join the store: records (and map[]), the scan of their
//                include counts (AppendBases, a compaction pass of index_dev.h), the include slots
//                a wave per row
//   KeepRecords, k_dg_keep_inc   mv_dag_prune: pending.hip's KeepPending over "round >= floor"
//   k_sd_*       mv_dev_dag_seed_rows: the rows of a replay become stored blocks with records (below)
#include "index_dev.h"

namespace mv::ix {

__global__ void __launch_bounds__(WG) k_dg_app_rows(const u64* __restrict__ slots, PendStore p, uint64_t nb,
                                                    const uint32_t* __restrict__ lvl, const uint32_t* __restrict__ row_of,
                                                    uint64_t rows, DagStore d, uint64_t nb0, uint64_t* __restrict__ src,
                                                    u64* __restrict__ ctl) {
  const uint64_t b = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool bad = false;
  if (b < nb && lvl[b] != 0) {
    const uint64_t r = row_of[b], s = p.slot[b], rec = nb0 + r;
    bad = r >= rows || rec >= d.cap_b || s >= d.n_slots;
    if (!bad) {
      const u64* slot = slots + SLOT_WORDS * s;  // (the key: written by an earlier launch)
      const u64 a = slot[2], rd = slot[3];
      d.slot[rec] = s;
      d.auth[rec] = a < DG_MAX_AUTH ? (uint32_t)a : DG_NONE;
      d.round[rec] = rd;
      d.kc[rec] = p.kc[b];
      d.map[s] = (uint32_t)rec;
      src[r] = b;
      atomicMax(ctl + mvk::IX_CTL_DG_NLO, ~rd);
      atomicMax(ctl + mvk::IX_CTL_DG_HI, rd);
    }
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
}
// where each row's includes start: the scan of the rows' include counts
// (src[r] is IX_NO_SRC for a row k_dg_app_rows refused: its record is not read)
struct AppendBases {
  static constexpr int WEIGHTS = 1;
  DagStore d;
  uint64_t nb0, ni0, rows;
  const uint64_t* src;
  __device__ bool has(uint64_t r) const { return r < rows && src[r] != mvk::IX_NO_SRC; }
  __device__ void weigh(uint64_t r, uint64_t* kc) const { *kc = has(r) ? d.kc[nb0 + r] : 0; }
  __device__ void place(uint64_t r, uint64_t, uint64_t ib) const {
    if (has(r)) d.ibase[nb0 + r] = ni0 + ib;
  }
};
__global__ void __launch_bounds__(WG) k_dg_app_inc(PendStore p, uint64_t nb, DagStore d, uint64_t nb0, uint64_t rows,
                                                   const uint64_t* __restrict__ src, u64* __restrict__ ctl) {
  const uint64_t r = ((uint64_t)blockIdx.x * WG + threadIdx.x) / 64;  // a wave per row
  if (r >= rows) return;
  const uint64_t b = src[r];
  bool bad = b >= nb;
  if (!bad) {
    const uint64_t from = p.ibase[b], to = d.ibase[nb0 + r];
    const uint32_t kc = d.kc[nb0 + r];
    bad = to > d.cap_i || kc > d.cap_i - to;
    if (!bad)
      for (uint32_t i = threadIdx.x & 63; i < kc; i += 64) d.inc[to + i] = p.inc[from + i];
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad && (threadIdx.x & 63) == 0);
}

__global__ void __launch_bounds__(WG) k_dg_map(DagStore d, uint64_t nb, u64* __restrict__ ctl) {
  const uint64_t b = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool bad = false;
  if (b < nb) {
    const uint64_t s = d.slot[b];
    bad = s >= d.n_slots;
    if (!bad) d.map[s] = (uint32_t)b;
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
}

// the records of round >= floor stay, in order; weights: the record, its includes
struct KeepRecords {
  static constexpr int WEIGHTS = 2;
  DagStore d, q;
  uint64_t nb, floor;
  uint64_t* newbase;
  u64* ctl;
  __device__ void weigh(uint64_t b, uint64_t* keep, uint64_t* kc) const {
    *keep = b < nb && d.round[b] >= floor;
    *kc = *keep ? d.kc[b] : 0;
  }
  __device__ void place(uint64_t b, uint64_t kept, uint64_t rb, uint64_t kc, uint64_t ib) const {
    bool keep = kept, bad = false;
    if (b < nb) {
      const uint64_t s = keep ? d.slot[b] : 0;
      bad = keep && (rb >= q.cap_b || ib > q.cap_i || kc > q.cap_i - ib || s >= q.n_slots);
      keep = keep && !bad;
      newbase[b] = keep ? ib : mvk::IX_NO_SRC;
      if (keep) {
        const uint64_t rd = d.round[b];
        q.slot[rb] = s;
        q.auth[rb] = d.auth[b];
        q.round[rb] = rd;
        q.ibase[rb] = ib;
        q.kc[rb] = (uint32_t)kc;
        q.map[s] = (uint32_t)rb;
        atomicMax(ctl + mvk::IX_CTL_DG_NLO, ~rd);
        atomicMax(ctl + mvk::IX_CTL_DG_HI, rd);
      }
    }
    wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
  }
};
__global__ void __launch_bounds__(WG) k_dg_keep_inc(DagStore d, DagStore q, uint64_t nb, const uint64_t* __restrict__ newbase) {
  const uint64_t b = ((uint64_t)blockIdx.x * WG + threadIdx.x) / 64;  // a wave per record
  if (b >= nb || newbase[b] == mvk::IX_NO_SRC) return;
  const uint64_t from = d.ibase[b], to = newbase[b];
  const uint32_t kc = d.kc[b];
  if (from > d.cap_i || kc > d.cap_i - from) return;  // (KeepRecords checked the other side)
  for (uint32_t i = threadIdx.x & 63; i < kc; i += 64) q.inc[to + i] = d.inc[from + i];
}

// ---------------------------------------------------------------- seeding the DAG store from a replay's rows
// mv_dev_dag_seed_rows / mv_wal_recover: the rows of mv_wal_replay become stored blocks with records
// (BlockStore::open with add_unloaded, block_store.rs:50-116, 398-404; the wording of every rule is
// the header's). The blocks are read in place in the image; a row's offset and length are the
// caller's, so they are checked against the image before a byte is read, and the include count
// against the length before it counts. Between the kernels stand the two inserts of the call (the
// rows' own references towards STORED, the record rows' includes towards WANTED), both by
// k_ix_claim / fill / settle.
//   k_sd_elig     a lane per row: may it get a record (OK, round >= floor, its bytes fit), its include
//                 count; the eligible rows and their includes per workgroup (they decide about room)
//   k_sd_claim    after the own references' insert: a row's slot, and atomicMin of nb0 + row into
//                 map[slot] -- a record from before the call is below nb0 and stays, otherwise the
//                 lowest row of a reference wins, as the lowest item owns a slot in k_ix_claim
//   k_sd_count    first[row] = map[slot] == nb0 + row (what k_sd_claim left), the record rows and
//                 their includes per workgroup
//   k_sd_list     a record row writes its record, map[slot] and where its block lies; a first row
//                 without a record puts map[slot] back to DG_NONE. It reads first[], not map[].
//   k_sd_inc_src  a wave per record: where its includes lie in the image, for the includes' insert
//   k_sd_inc      a wave per record: the slots that insert found, in batches of 64
using mvk::SeedRows;
constexpr uint8_t SD_ELIGIBLE = 1, SD_MISFIT = 2;

__global__ void __launch_bounds__(WG) k_sd_elig(SeedRows r, uint64_t* __restrict__ wg_a, uint64_t* __restrict__ wg_b,
                                                u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool el = false, misfit = false;
  uint64_t k = 0;
  if (i < r.n) {
    const uint64_t* row = r.rows + mvk::SD_ROW_WORDS * i;
    if (r.status[i] == MV_BLOCK_OK) {
      const uint64_t off = row[1], len = row[2];
      bool fits = off <= r.size && len <= r.size - off && br::inc_count_readable(len);
      if (fits) {
        k = ld64(r.img + off + br::INC_COUNT_OFF);
        fits = br::includes_inside(len, k) && k <= 0xffffffffull;
      }
      misfit = !fits;
      el = fits && row[4] >= r.floor;
    }
    if (!el) k = 0;
    r.elig[i] = el ? SD_ELIGIBLE : misfit ? SD_MISFIT : 0;
    r.kc[i] = (uint32_t)k;
  }
  uint64_t te, tk;
  (void)wg_excl(el, &te);
  (void)wg_excl(k, &tk);
  if (threadIdx.x == 0) {
    wg_a[blockIdx.x] = te;
    wg_b[blockIdx.x] = tk;
  }
  wave_count_to(ctl + mvk::IX_CTL_SD_MISFIT, misfit);
}

__global__ void __launch_bounds__(WG) k_sd_claim(const u64* __restrict__ item, SeedRows r, DagStore d, uint64_t nb0,
                                                 u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool bad = false;
  if (i < r.n) {
    const u64 it = item[i];
    const uint64_t s = it & SLOT_MASK;
    bad = !item_has_slot(it) || s >= d.n_slots;
    r.own_slot[i] = bad ? mvk::IX_NO_SRC : s;
    if (!bad) atomicMin(d.map + s, (uint32_t)(nb0 + i));
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
}

// a first row (of the call, i < r.n) gets a record when it is eligible: *k = the includes it brings
__device__ inline bool seed_rec(const SeedRows& r, uint64_t i, bool first, uint64_t* k) {
  const bool rec = first && r.elig[i] == SD_ELIGIBLE;
  *k = rec ? r.kc[i] : 0;
  return rec;
}
__global__ void __launch_bounds__(WG) k_sd_count(SeedRows r, DagStore d, uint64_t nb0, uint64_t* __restrict__ wg_a,
                                                 uint64_t* __restrict__ wg_b) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool rec = false;
  uint64_t k = 0;
  if (i < r.n) {
    const uint64_t s = r.own_slot[i];
    const bool first = s < d.n_slots && d.map[s] == (uint32_t)(nb0 + i);  // (k_sd_claim's atomics, an earlier kernel)
    r.first[i] = first;
    rec = seed_rec(r, i, first, &k);
  }
  uint64_t tb, tk;
  (void)wg_excl(rec, &tb);
  (void)wg_excl(k, &tk);
  if (threadIdx.x == 0) {
    wg_a[blockIdx.x] = tb;
    wg_b[blockIdx.x] = tk;
  }
}

__global__ void __launch_bounds__(WG) k_sd_list(const u64* __restrict__ slots, SeedRows r, DagStore d, uint64_t nb0,
                                                uint64_t ni0, const uint64_t* __restrict__ base_a,
                                                const uint64_t* __restrict__ base_b, u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  const bool first = i < r.n && r.first[i];
  uint64_t k, tb, tk;
  const bool rec = seed_rec(r, i, first, &k);
  const uint64_t rb = nb0 + base_a[blockIdx.x] + wg_excl(rec, &tb);
  const uint64_t ib = ni0 + base_b[blockIdx.x] + wg_excl(k, &tk);
  bool bad = false;
  if (first) {
    const uint64_t s = r.own_slot[i];  // (below the table's size: k_sd_count checked it)
    bad = rec && (rb >= d.cap_b || rb - nb0 >= r.n || ib > d.cap_i || k > d.cap_i - ib);
    if (rec && !bad) {
      const u64* slot = slots + SLOT_WORDS * s;  // (the key: written by an earlier launch)
      const u64 a = slot[2], rd = slot[3];
      d.slot[rb] = s;
      d.auth[rb] = a < DG_MAX_AUTH ? (uint32_t)a : DG_NONE;
      d.round[rb] = rd;
      d.kc[rb] = (uint32_t)k;
      d.ibase[rb] = ib;
      d.map[s] = (uint32_t)rb;
      r.rec_off[rb - nb0] = r.rows[mvk::SD_ROW_WORDS * i + 1];
      atomicMax(ctl + mvk::IX_CTL_DG_NLO, ~rd);
      atomicMax(ctl + mvk::IX_CTL_DG_HI, rd);
    } else {
      d.map[s] = DG_NONE;  // the claim of a row that gets no record
    }
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
}

// where the includes of the call's record `rec` stand among the call's include items; false: out of range
__device__ inline bool seed_span(const DagStore& d, uint64_t nb0, uint64_t ni0, uint64_t ninc, uint64_t rec, uint64_t* base,
                                 uint32_t* kc) {
  const uint64_t ib = d.ibase[nb0 + rec];
  *kc = d.kc[nb0 + rec];
  *base = ib - ni0;
  return ib >= ni0 && ib - ni0 <= ninc && *kc <= ninc - (ib - ni0) && ib <= d.cap_i && *kc <= d.cap_i - ib;
}
__global__ void __launch_bounds__(WG) k_sd_inc_src(SeedRows r, DagStore d, uint64_t nb0, uint64_t ni0, uint64_t nrec,
                                                   uint64_t ninc, uint64_t* __restrict__ inc_src, u64* __restrict__ ctl) {
  const uint64_t rec = ((uint64_t)blockIdx.x * WG + threadIdx.x) / 64;  // a wave per record
  if (rec >= nrec) return;
  uint64_t base;
  uint32_t kc;
  const bool bad = !seed_span(d, nb0, ni0, ninc, rec, &base, &kc);
  if (!bad) {
    const uint64_t off = r.rec_off[rec];  // (k_sd_elig checked off + 64 + 56 kc against the image)
    for (uint32_t q = threadIdx.x & 63; q < kc; q += 64) inc_src[base + q] = off + br::include_off(q);
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad && (threadIdx.x & 63) == 0);
}
__global__ void __launch_bounds__(WG) k_sd_inc(const u64* __restrict__ item, DagStore d, uint64_t nb0, uint64_t ni0,
                                               uint64_t nrec, uint64_t ninc, u64* __restrict__ ctl) {
  const uint64_t rec = ((uint64_t)blockIdx.x * WG + threadIdx.x) / 64;  // a wave per record
  if (rec >= nrec) return;
  const uint32_t lane = threadIdx.x & 63;
  uint64_t base;
  uint32_t kc;
  bool bad = !seed_span(d, nb0, ni0, ninc, rec, &base, &kc);
  uint64_t nbad = bad && lane == 0;
  if (!bad) {
    for (uint32_t q0 = 0; q0 < kc; q0 += 64) {  // bounded by the include count; the wave stays together
      const uint32_t q = q0 + lane;
      if (q >= kc) continue;
      const u64 it = item[base + q];
      const uint64_t s = it & SLOT_MASK;
      const bool ok = item_has_slot(it) && s < d.n_slots;
      d.inc[ni0 + base + q] = ok ? s : DG_NO_SLOT;
      nbad += !ok;
    }
  }
  nbad = wave_sum64(nbad);
  if (lane == 0 && nbad) atomicAdd(ctl + mvk::IX_CTL_ERR, (u64)nbad);
}

}  // namespace mv::ix

namespace mvk {
using namespace mv::ix;

hipError_t launch_dag_append(const IndexTable& t, const PendStore& p, uint64_t nb, const uint32_t* lvl,
                             const uint32_t* row_of, uint64_t rows, const DagStore& d, uint64_t nb0, uint64_t ni0,
                             uint64_t* src, uint64_t* wg, uint64_t* ctl, hipStream_t s) {
  if (rows == 0 || nb == 0) return hipSuccess;
  const dim3 b(WG);
  hipError_t e = hipMemsetAsync(src, 0xff, 8 * rows, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_dg_app_rows, dim3(grid_of(nb)), b, 0, s, (const u64*)t.slots, p, nb, lvl, row_of, rows, d, nb0, src,
                     (u64*)ctl);
  compact_pass(AppendBases{d, nb0, ni0, rows, src}, rows, wg_scan_of(wg, rows), ctl + IX_CTL_DG_NI, nullptr, nullptr, s);
  hipLaunchKernelGGL(k_dg_app_inc, dim3(grid_of(64 * rows)), b, 0, s, p, nb, d, nb0, rows, src, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_dag_map(const DagStore& d, uint64_t nb, uint64_t* ctl, hipStream_t s) {
  if (d.n_slots == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(d.map, 0xff, 4 * d.n_slots, s);
  if (e != hipSuccess || nb == 0) return e;
  hipLaunchKernelGGL(k_dg_map, dim3(grid_of(nb)), dim3(WG), 0, s, d, nb, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_dag_prune(const DagStore& d, const DagStore& q, uint64_t nb, uint64_t floor, uint64_t* newbase,
                            uint64_t* wg, uint64_t* ctl, hipStream_t s) {
  if (nb == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(q.map, 0xff, 4 * q.n_slots, s);
  if (e != hipSuccess) return e;
  compact_pass(KeepRecords{d, q, nb, floor, newbase, (u64*)ctl}, nb, wg_scan_of(wg, nb), ctl + IX_CTL_DG_NB, ctl + IX_CTL_DG_NI,
               nullptr, s);
  hipLaunchKernelGGL(k_dg_keep_inc, dim3(grid_of(64 * nb)), dim3(WG), 0, s, d, q, nb, newbase);
  return hipGetLastError();
}

hipError_t launch_seed_eligible(const SeedRows& r, uint64_t* wg, uint64_t* ctl, hipStream_t s) {
  if (r.n == 0) return hipSuccess;
  const uint64_t nwg = index_groups(r.n);
  const WgScan w = wg_scan_of(wg, r.n);
  hipLaunchKernelGGL(k_sd_elig, dim3(grid_of(r.n)), dim3(WG), 0, s, r, w.count_a, w.count_b, (u64*)ctl);
  (void)launch_index_scan(w.count_a, nwg, w.base_a, ctl + IX_CTL_SD_ELIG, nullptr, s);
  (void)launch_index_scan(w.count_b, nwg, w.base_b, ctl + IX_CTL_SD_EINC, nullptr, s);
  return hipGetLastError();
}

hipError_t launch_seed_records(const IndexTable& t, const uint64_t* item, const SeedRows& r, const DagStore& d, uint64_t nb0,
                               uint64_t ni0, uint64_t* wg, uint64_t* ctl, hipStream_t s) {
  if (r.n == 0) return hipSuccess;
  const uint64_t nwg = index_groups(r.n);
  const WgScan w = wg_scan_of(wg, r.n);
  const dim3 g(grid_of(r.n)), b(WG);
  hipLaunchKernelGGL(k_sd_claim, g, b, 0, s, (const u64*)item, r, d, nb0, (u64*)ctl);
  hipLaunchKernelGGL(k_sd_count, g, b, 0, s, r, d, nb0, w.count_a, w.count_b);
  (void)launch_index_scan(w.count_a, nwg, w.base_a, ctl + IX_CTL_SD_NREC, nullptr, s);
  (void)launch_index_scan(w.count_b, nwg, w.base_b, ctl + IX_CTL_SD_NINC, nullptr, s);
  hipLaunchKernelGGL(k_sd_list, g, b, 0, s, (const u64*)t.slots, r, d, nb0, ni0, w.base_a, w.base_b, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_seed_inc_src(const SeedRows& r, const DagStore& d, uint64_t nb0, uint64_t ni0, uint64_t nrec, uint64_t ninc,
                               uint64_t* inc_src, uint64_t* ctl, hipStream_t s) {
  if (nrec == 0 || ninc == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(inc_src, 0xff, 8 * ninc, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_sd_inc_src, dim3(grid_of(64 * nrec)), dim3(WG), 0, s, r, d, nb0, ni0, nrec, ninc, inc_src, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_seed_inc(const uint64_t* item, const DagStore& d, uint64_t nb0, uint64_t ni0, uint64_t nrec, uint64_t ninc,
                           uint64_t* ctl, hipStream_t s) {
  if (nrec == 0 || ninc == 0) return hipSuccess;
  hipLaunchKernelGGL(k_sd_inc, dim3(grid_of(64 * nrec)), dim3(WG), 0, s, (const u64*)item, d, nb0, ni0, nrec, ninc, (u64*)ctl);
  return hipGetLastError();
}

}  // namespace mvk
