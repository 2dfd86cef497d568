/* reclaim_kernels.h — the copy kernel of gra_reclaim. Included by engine.hip
 * inside namespace gra.
 *
 * gra_reclaim slides every live segment of the store arena down; the plan
 * (gra::plan_reclaim, host_store.h) cuts the moved segments into pieces and
 * the pieces into batches whose loads cannot see their own stores. One batch
 * is one launch of k_rc_move over the batch's task list — a reclaim behind a
 * few hundred compactions moves thousands of small segments, which as one
 * hipMemcpyAsync each would cost their launches, not their bytes. The same
 * kernel serves store -> store (direct batches), store -> bounce buffer and
 * bounce buffer -> store through its two base pointers.
 *
 * src_off == dst_off (mod 16) and every length is a multiple of 8, so a piece
 * is an optional 8-B head, whole 16-B chunks and an optional 8-B tail: there
 * are no byte loops. A wave moves kRcUnroll chunks per lane a step
 * (kRcUnitBytes), the loads of a step issued before its stores, as
 * part_copy.h does. The launch deals every piece to `units` workers: worker
 * u % units of piece u / units takes steps u % units, + units, + 2 units, ...
 * of that piece, and the waves of a capped grid stride over the workers. The
 * host picks `units` per launch (rc_units): 1 when the batch has pieces
 * enough to fill the grid, so that a small piece costs no idle worker, and
 * up to a piece's step count when it has few, so that one large piece does
 * not land on one block. */
#pragma once

struct RcTask {
  uint64_t src_off, dst_off; /* from src_base / dst_base; equal mod 16 */
  uint64_t nbytes;           /* multiple of 8, at most the plan's piece size */
};

constexpr uint32_t kRcUnroll = 4;
constexpr uint32_t kRcUnitBytes = 64 * 16 * kRcUnroll; /* 4 KiB per wave-step */

__global__ void __launch_bounds__(256) k_rc_move(const uint8_t *src_base,
                                                 uint8_t *dst_base,
                                                 const RcTask *__restrict__ tasks,
                                                 uint32_t ntasks,
                                                 uint32_t units) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint64_t total = (uint64_t)ntasks * units;
  for (uint64_t u = wave; u < total; u += nwaves) {
    const RcTask t = tasks[u / units]; /* wave-uniform */
    const uint32_t slot = (uint32_t)(u % units);
    const uint64_t head = (0 - t.src_off) & 15; /* 0 or 8 */
    const uint8_t *s = src_base + t.src_off;
    uint8_t *d = dst_base + t.dst_off;
    if (slot == 0 && lane == 0 && head) /* nbytes >= 8 */
      *(uint2 *)d = *(const uint2 *)s;
    if (t.nbytes <= head) continue;
    const uint64_t body = t.nbytes - head;
    const uint64_t nchunks = body >> 4;
    if (slot == 0 && lane == 1 && (body & 8))
      *(uint2 *)(d + head + 16 * nchunks) =
          *(const uint2 *)(s + head + 16 * nchunks);
    const uint4 *s4 = (const uint4 *)(s + head);
    uint4 *d4 = (uint4 *)(d + head);
    for (uint64_t base = (uint64_t)slot * (64 * kRcUnroll); base < nchunks;
         base += (uint64_t)units * (64 * kRcUnroll)) {
      const uint64_t c0 = base + lane;
      uint4 v[kRcUnroll];
#pragma unroll
      for (uint32_t k = 0; k < kRcUnroll; k++)
        if (c0 + 64 * k < nchunks) v[k] = s4[c0 + 64 * k];
#pragma unroll
      for (uint32_t k = 0; k < kRcUnroll; k++)
        if (c0 + 64 * k < nchunks) d4[c0 + 64 * k] = v[k];
    }
  }
}

/* workers per piece for a launch of `ntasks` pieces of at most `piece_bytes`:
 * enough to put kRcGridWaves waves to work, at most one per step */
constexpr uint32_t kRcGridBlocks = 2048; /* 8 per CU, 4 waves each */
constexpr uint32_t kRcGridWaves = 4 * kRcGridBlocks;
inline uint32_t rc_units(uint32_t ntasks, uint64_t piece_bytes) {
  uint64_t steps = (piece_bytes + kRcUnitBytes - 1) / kRcUnitBytes;
  uint64_t want = (kRcGridWaves + ntasks - 1) / (ntasks ? ntasks : 1);
  uint64_t u = want < steps ? want : steps;
  return u < 1 ? 1u : (uint32_t)u;
}
