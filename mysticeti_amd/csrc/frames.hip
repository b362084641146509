// mv_verify_frames on the device: the walk of received NetworkMessage frames and the
// per-message / per-connection verdicts ("first failing block terminates the
// message"). The rules are those of frame_walk.h; the blocks found are verified in place by the
// block pipeline (engine.cpp enqueue_blocks) between k_msg_walk and k_msg_verdict.
//
// Two levels, so that a dependent chain of loads is one hop per frame of a stream and then one
// hop per block of ONE frame (a single chain over every block of a stream would be ~100x
// longer at 100 blocks a frame), each in the count / scan / list form of k_wal_walk:
//
//   k_frame_walk     one lane per stream, size word to size word: counts the frames that get a
//                    row (pings get none), then (second launch, foff set) lists each one's
//                    offset, size and stream at the scanned positions
//   k_msg_walk       one lane per frame: the message's tag, frame-level status and block count;
//                    second launch (rows set): the message row and each block's (off, len)
//   k_stream_cut     one lane per stream: the rows it keeps (the walk stops a stream at the first
//                    row the bytes alone condemn), its consumed bytes, block prefix sums
//   k_msg_verdict    one lane per row: the first unparsable block (a decode error, which wins),
//                    else the first rejected one
//   k_stream_verdict one lane per stream: drop_msg, later rows MV_MSG_NOT_REACHED
//
// The scans between them run on the host (engine.cpp frames_run), as the WAL replay's do: the
// row and block counts are needed there anyway to size the lists.
// Every load is bounded by the stream's end (clipped to buf_bytes): frame_at admits a frame only
// when all of it lies before the end, and classify reads inside the frame only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frame_walk.h"
#include "kernels.h"

namespace mv {
namespace fr {

// stream s = buf[soff[s], soff[s] + slen[s]) clipped to the buffer
__device__ inline void stream_span(const uint64_t* soff, const uint64_t* slen, uint32_t s, uint64_t buf_bytes,
                                   uint64_t& start, uint64_t& end) {
  start = soff[s] < buf_bytes ? soff[s] : buf_bytes;
  const uint64_t l = slen[s];
  end = l > buf_bytes - start ? buf_bytes : start + l;
}

__global__ void __launch_bounds__(64) k_frame_walk(const uint8_t* __restrict__ buf, uint64_t buf_bytes,
                                                   const uint64_t* __restrict__ soff,
                                                   const uint64_t* __restrict__ slen, uint32_t ns,
                                                   const uint64_t* __restrict__ foff, uint64_t* __restrict__ fr_off,
                                                   uint32_t* __restrict__ fr_size, uint32_t* __restrict__ fr_stream,
                                                   uint32_t* __restrict__ fcount, uint64_t* __restrict__ consumed) {
  const uint32_t s = blockIdx.x * 64 + threadIdx.x;
  if (s >= ns) return;
  uint64_t start, end;
  stream_span(soff, slen, s, buf_bytes, start, end);
  // the second walk lists as many frames as the first one counted, at foff[s]
  const uint32_t cap = foff ? fcount[s] : 0;
  const uint64_t base = foff ? foff[s] : 0;
  uint64_t p = start;
  uint32_t count = 0;
  for (;;) {
    uint64_t size;
    const Step st = frame_at(buf, p, end, size);
    if (st == STEP_END) break;
    if (st == STEP_PING) {
      p += 4 + PING_REST;
      continue;
    }
    if (count < cap) {
      fr_off[base + count] = p;
      fr_size[base + count] = (uint32_t)size;
      fr_stream[base + count] = s;
    }
    if (count == 0xffffffffu) break;  // (a stream of 2^32 frames: the host refuses the call)
    count++;
    if (st == STEP_BAD_SIZE) break;  // the connection is dropped: consumed ends before the frame
    p += 4 + size;
  }
  if (!foff) {
    fcount[s] = count;
    consumed[s] = p - start;
  }
}

// (n: the count of the first walk, so that bytes changed under the call cannot widen the list)
struct BlockSink {
  uint64_t* off;
  uint64_t* len;
  uint32_t n;
  __device__ void operator()(uint32_t k, uint64_t o, uint64_t l) const {
    if (k < n) {
      off[k] = o;
      len[k] = l;
    }
  }
};

// First launch (rows == nullptr): fr_tag / fr_status / fr_nblk of every frame.
// Second launch: the rows of the frames their stream keeps, and the block lists of the messages
// that decode. row_base / blk_base: the stream's first row and block; fr_bpre: the blocks of
// the stream's earlier frames. The lists hold n_rows rows and n_blk blocks.
__global__ void __launch_bounds__(64) k_msg_walk(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ fr_off,
                                                 const uint32_t* __restrict__ fr_size,
                                                 const uint32_t* __restrict__ fr_stream, uint64_t nf,
                                                 uint32_t* __restrict__ fr_tag, uint8_t* __restrict__ fr_status,
                                                 uint32_t* __restrict__ fr_nblk, const uint64_t* __restrict__ foff,
                                                 const uint32_t* __restrict__ kept,
                                                 const uint32_t* __restrict__ row_base,
                                                 const uint32_t* __restrict__ blk_base,
                                                 const uint64_t* __restrict__ fr_bpre, uint32_t* __restrict__ rows,
                                                 uint64_t n_rows, uint64_t* __restrict__ blk_off,
                                                 uint64_t* __restrict__ blk_len, uint64_t n_blk) {
  const uint64_t f = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  if (f >= nf) return;
  const uint64_t off = fr_off[f], size = fr_size[f];
  if (!rows) {
    Msg m{NO_TAG, MV_MSG_BAD_SIZE, 0};
    if (size <= MAX_SIZE) m = classify(buf, off + 4, size, NoSink());
    fr_tag[f] = m.tag;
    fr_status[f] = (uint8_t)m.status;
    fr_nblk[f] = m.nblk;
    return;
  }
  const uint32_t s = fr_stream[f];
  const uint64_t j = f - foff[s];
  if (j >= kept[s]) return;  // after the row that stopped the stream's walk
  const uint64_t row = row_base[s] + j;
  const uint64_t first = blk_base[s] + fr_bpre[f];
  const uint32_t nblk = fr_nblk[f];
  if (row >= n_rows) return;
  put_row(rows + ROW_WORDS * row, s, fr_tag[f], off, (uint32_t)first, nblk, fr_status[f], 0, NONE);
  if (nblk && first <= n_blk && nblk <= n_blk - first)
    (void)classify(buf, off + 4, size, BlockSink{blk_off + first, blk_len + first, nblk});
}

__global__ void __launch_bounds__(64) k_stream_cut(const uint64_t* __restrict__ soff, uint64_t buf_bytes, uint32_t ns,
                                                   const uint32_t* __restrict__ fcount,
                                                   const uint64_t* __restrict__ foff,
                                                   const uint64_t* __restrict__ fr_off,
                                                   const uint32_t* __restrict__ fr_size,
                                                   const uint8_t* __restrict__ fr_status,
                                                   const uint32_t* __restrict__ fr_nblk, uint64_t* __restrict__ fr_bpre,
                                                   uint32_t* __restrict__ kept, uint64_t* __restrict__ sblocks,
                                                   uint64_t* __restrict__ consumed) {
  const uint32_t s = blockIdx.x * 64 + threadIdx.x;
  if (s >= ns) return;
  const uint64_t start = soff[s] < buf_bytes ? soff[s] : buf_bytes;
  const uint64_t base = foff[s];
  const uint32_t n = fcount[s];
  uint64_t acc = 0;
  uint32_t k = 0;
  while (k < n) {
    const uint64_t f = base + k;
    fr_bpre[f] = acc;
    acc += fr_nblk[f];
    k++;
    const uint32_t st = fr_status[f];
    if (st != MV_MSG_OK) {  // BAD_SIZE: k_frame_walk stopped before the frame; else just after it
      if (st != MV_MSG_BAD_SIZE) consumed[s] = fr_off[f] + 4 + fr_size[f] - start;
      break;
    }
  }
  kept[s] = k;
  sblocks[s] = acc;
}

__global__ void __launch_bounds__(64) k_msg_verdict(uint32_t* __restrict__ rows, uint64_t n_rows,
                                                    const uint8_t* __restrict__ blk_status, uint64_t n_blk) {
  const uint64_t r = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  if (r >= n_rows) return;
  uint32_t* row = rows + ROW_WORDS * r;
  const uint32_t first = row[4], n = row[5];
  if ((row[6] & 0xff) != MV_MSG_OK || n == 0 || first > n_blk || n > n_blk - first) return;
  uint32_t bad = NONE, bad_status = 0;
  for (uint32_t k = 0; k < n; k++) {
    const uint32_t st = blk_status[(uint64_t)first + k];
    if (st == MV_BLOCK_PARSE_ERROR) {  // the message does not deserialize: before any verify
      bad = k;
      bad_status = st;
      break;
    }
    if (st != MV_BLOCK_OK && bad == NONE) {
      bad = k;
      bad_status = st;
    }
  }
  if (bad == NONE) return;
  row[6] = (bad_status == MV_BLOCK_PARSE_ERROR ? MV_MSG_DECODE_ERROR : MV_MSG_BLOCK_REJECTED) | (bad_status << 8);
  row[7] = bad;
}

__global__ void __launch_bounds__(64) k_stream_verdict(uint32_t* __restrict__ rows, uint64_t n_rows, uint32_t ns,
                                                       const uint32_t* __restrict__ kept,
                                                       const uint32_t* __restrict__ row_base,
                                                       uint32_t* __restrict__ drop_msg) {
  const uint32_t s = blockIdx.x * 64 + threadIdx.x;
  if (s >= ns) return;
  const uint64_t base = row_base[s];
  uint32_t drop = NONE;
  for (uint32_t k = 0; k < kept[s]; k++) {
    const uint64_t r = base + k;
    if (r >= n_rows) break;
    uint32_t* row = rows + ROW_WORDS * r;
    if (drop != NONE) {
      row[6] = MV_MSG_NOT_REACHED;
      row[7] = NONE;
    } else if ((row[6] & 0xff) != MV_MSG_OK) {
      drop = (uint32_t)r;
    }
  }
  drop_msg[s] = drop;
}

}  // namespace fr
}  // namespace mv

namespace mvk {

hipError_t launch_frame_walk(const uint8_t* buf, uint64_t buf_bytes, const uint64_t* soff, const uint64_t* slen,
                             uint32_t ns, const uint64_t* foff, uint64_t* fr_off, uint32_t* fr_size,
                             uint32_t* fr_stream, uint32_t* fcount, uint64_t* consumed, hipStream_t s) {
  if (ns == 0) return hipSuccess;
  hipLaunchKernelGGL(mv::fr::k_frame_walk, dim3((ns + 63) / 64), dim3(64), 0, s, buf, buf_bytes, soff, slen, ns, foff,
                     fr_off, fr_size, fr_stream, fcount, consumed);
  return hipGetLastError();
}

hipError_t launch_msg_walk(const uint8_t* buf, const FrameList& fl, const FrameRows* out, hipStream_t s) {
  if (fl.nf == 0) return hipSuccess;
  const FrameRows none{};
  const FrameRows& o = out ? *out : none;
  hipLaunchKernelGGL(mv::fr::k_msg_walk, dim3((uint32_t)((fl.nf + 63) / 64)), dim3(64), 0, s, buf, fl.off, fl.size,
                     fl.stream, fl.nf, fl.tag, fl.status, fl.nblk, o.foff, o.kept, o.row_base, o.blk_base, o.bpre,
                     o.rows, o.n_rows, o.blk_off, o.blk_len, o.n_blk);
  return hipGetLastError();
}

hipError_t launch_stream_cut(const uint64_t* soff, uint64_t buf_bytes, uint32_t ns, const uint32_t* fcount,
                             const uint64_t* foff, const FrameList& fl, uint64_t* bpre, uint32_t* kept,
                             uint64_t* sblocks, uint64_t* consumed, hipStream_t s) {
  if (ns == 0) return hipSuccess;
  hipLaunchKernelGGL(mv::fr::k_stream_cut, dim3((ns + 63) / 64), dim3(64), 0, s, soff, buf_bytes, ns, fcount, foff,
                     fl.off, fl.size, fl.status, fl.nblk, bpre, kept, sblocks, consumed);
  return hipGetLastError();
}

hipError_t launch_frame_verdicts(uint32_t* rows, uint64_t n_rows, const uint8_t* blk_status, uint64_t n_blk,
                                 uint32_t ns, const uint32_t* kept, const uint32_t* row_base, uint32_t* drop_msg,
                                 hipStream_t s) {
  if (n_rows) {
    hipLaunchKernelGGL(mv::fr::k_msg_verdict, dim3((uint32_t)((n_rows + 63) / 64)), dim3(64), 0, s, rows, n_rows,
                       blk_status, n_blk);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (ns == 0) return hipSuccess;
  hipLaunchKernelGGL(mv::fr::k_stream_verdict, dim3((ns + 63) / 64), dim3(64), 0, s, rows, n_rows, ns, kept, row_base,
                     drop_msg);
  return hipGetLastError();
}

}  // namespace mvk
