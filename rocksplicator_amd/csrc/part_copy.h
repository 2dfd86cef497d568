/* part_copy.h — the partition-copy device code: gathers every record's key
 * and value slice from the blob arena into the tick's payload region.
 *
 * Shared by engine.hip (k_copy) and scripts/micro_copy.hip, so the
 * microbenchmark times exactly what the engine runs.
 *
 * Shape of the work (one 64-lane wave), G lanes per record, R steps deep:
 *  - a batch is (64/G)*R consecutive records; batches are dealt to the waves
 *    of the grid round-robin (grid stride), so at any moment the whole grid
 *    works inside one window of a few MB of the source and the destination.
 *    (A contiguous range of records per wave measured 7 to 30 % slower.)
 *  - a wave fetches a batch's CopyTasks with one coalesced load, one task
 *    per lane, and issues the NEXT batch's fetch behind the current batch's
 *    data loads, so the task fetch is never waited on alone;
 *  - a task is broadcast out of the batch registers: with G == 64 by
 *    v_readlane, which makes addresses, lengths and alignment cases scalar
 *    (SGPR values, scalar branches); with G < 64 by ds_bpermute, 64/G
 *    records per wave-step, G lanes each;
 *  - R wave-steps are in flight: the 16 B/lane loads of R steps (key and
 *    value slice of each record) are all issued before the first store.
 *
 * A slice [dst, dst+n) is written byte-exactly as
 *    head (< 16 B, up to dst's next 16 B boundary) | 16 B chunks | tail (< 16 B)
 * so a destination of any alignment takes the same path; only head and tail
 * use byte accesses. Chunk sources have arbitrary byte alignment: they are
 * read either with one unaligned dwordx4 load (UNAL) or with a dword-aligned
 * dwordx4 + one dword and a v_alignbyte funnel. Neither starts before
 * src & ~3, and the funnel reaches at most 3 B past the end of its slice
 * (the arenas are over-allocated by 16 B). Lanes with nothing to copy are
 * predicated off. */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gra {

struct CopyTask {
  uint64_t src_off; /* into blob arena */
  uint32_t dst_rel; /* into tick payload region */
  uint32_t nbytes;
};

namespace pcopy {

typedef uint32_t v4u __attribute__((ext_vector_type(4)));
typedef v4u v4u_a1 __attribute__((aligned(1)));
typedef v4u v4u_a4 __attribute__((aligned(4)));

template <int G>
__device__ __forceinline__ uint32_t bcast(uint32_t v, uint32_t src_lane) {
  if (G == 64) return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)src_lane);
  return (uint32_t)__shfl((int)v, (int)src_lane, 64);
}

struct Slice {
  uint8_t *d;       /* destination of the slice */
  const uint8_t *s; /* source of the slice */
  uint32_t n;       /* bytes */
  uint32_t head;    /* bytes before d's next 16 B boundary (capped at n) */
  uint32_t nc;      /* whole 16 B chunks after the head */
};

struct Chunk {
  v4u lo;
  uint32_t hi; /* funnel only: the dword after lo */
};

/* NT: bit 0 = nontemporal loads, bit 1 = nontemporal stores */
template <bool UNAL, int NT>
__device__ __forceinline__ Chunk load16(const uint8_t *p) {
  Chunk c;
  c.hi = 0;
  if (UNAL) {
    c.lo = (NT & 1) ? __builtin_nontemporal_load((const v4u_a1 *)p)
                    : *(const v4u_a1 *)p;
  } else {
    uint32_t r = (uint32_t)(uintptr_t)p & 3u;
    const uint8_t *a = p - r;
    c.lo = (NT & 1) ? __builtin_nontemporal_load((const v4u_a4 *)a)
                    : *(const v4u_a4 *)a;
    if (r) c.hi = *(const uint32_t *)(a + 16);
  }
  return c;
}

template <bool UNAL, int NT>
__device__ __forceinline__ void store16(uint8_t *d, const uint8_t *p,
                                        const Chunk &c) {
  v4u o = c.lo;
  if (!UNAL) {
    uint32_t r = (uint32_t)(uintptr_t)p & 3u; /* alignbyte: ({b,a} >> 8r) */
    o.x = __builtin_amdgcn_alignbyte(c.lo.y, c.lo.x, r);
    o.y = __builtin_amdgcn_alignbyte(c.lo.z, c.lo.y, r);
    o.z = __builtin_amdgcn_alignbyte(c.lo.w, c.lo.z, r);
    o.w = __builtin_amdgcn_alignbyte(c.hi, c.lo.w, r);
  }
  if (NT & 2)
    __builtin_nontemporal_store(o, (v4u *)d);
  else
    *(v4u *)d = o;
}

/* Copy this wave's share of the tick's records. `wave` / `nwaves` index the
 * waves of the whole grid; blockDim.x must be a multiple of 64. */
template <int G, int R, bool UNAL, int NT = 0>
__device__ __forceinline__ void part_copy(const uint8_t *__restrict__ blobs,
                                          uint8_t *__restrict__ pay_region,
                                          const CopyTask *__restrict__ tasks,
                                          uint32_t nrec, uint32_t wave,
                                          uint32_t nwaves) {
  constexpr uint32_t S = 64 / G; /* records per wave-step */
  constexpr uint32_t B = S * R;  /* records per batch */
  static_assert(2 * B <= 64, "a batch's tasks are fetched one per lane");
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t sl = lane & (G - 1), sub = lane / G;
  wave = __builtin_amdgcn_readfirstlane(wave);
  const uint32_t nbatch = (nrec + B - 1) / B;
  if (wave >= nbatch) return;
  const uint4 *t4 = (const uint4 *)tasks;
  auto fetch = [&](uint32_t b) { /* lane l <- task 2*B*b + l */
    uint32_t t = 2 * B * b + lane;
    return (lane < 2 * B && t < 2 * nrec) ? t4[t]
                                          : make_uint4(0, 0, 0, 0); /* 0 B */
  };
  auto slice_of = [&](const uint4 &batch, uint32_t src_lane) {
    Slice x;
    uint64_t so = (uint64_t)bcast<G>(batch.x, src_lane) |
                  ((uint64_t)bcast<G>(batch.y, src_lane) << 32);
    x.s = blobs + so;
    x.d = pay_region + bcast<G>(batch.z, src_lane);
    x.n = bcast<G>(batch.w, src_lane);
    uint32_t h = (0u - (uint32_t)(uintptr_t)x.d) & 15u;
    x.head = h < x.n ? h : x.n;
    x.nc = (x.n - x.head) >> 4;
    return x;
  };
  uint4 cur = fetch(wave);
  /* Settle the first fetch HERE. Left to the compiler, the wait lands at the
   * top of the loop as vmcnt(0), where it would also drain the previous
   * batch's stores before the next batch's loads may issue. */
  asm volatile("" ::"v"(cur.x), "v"(cur.y), "v"(cur.z), "v"(cur.w));
  for (uint32_t b = wave; b < nbatch; b += nwaves) {
    Slice sv[2 * R];
    Chunk ch[2 * R];
    /* first G chunks of every slice: all loads, then all stores */
#pragma unroll
    for (int q = 0; q < 2 * R; q++) {
      uint32_t rec = (q >> 1) * S + sub; /* in batch; absent records are 0 B */
      sv[q] = slice_of(cur, 2 * rec + (q & 1));
      if (sl < sv[q].nc)
        ch[q] = load16<UNAL, NT>(sv[q].s + sv[q].head + 16 * sl);
    }
    /* the next batch's tasks ride behind this batch's loads and are settled
     * by the same wait */
    uint4 nxt = make_uint4(0, 0, 0, 0);
    if (b + nwaves < nbatch) nxt = fetch(b + nwaves);
#pragma unroll
    for (int q = 0; q < 2 * R; q++) {
      const uint8_t *p = sv[q].s + sv[q].head + 16 * sl;
      if (sl < sv[q].nc)
        store16<UNAL, NT>(sv[q].d + sv[q].head + 16 * sl, p, ch[q]);
    }
    /* the rest of each slice, if any: head and tail bytes (at most 30) and
     * chunks past the first G. Rolled up: the common shapes have neither. */
#pragma unroll 1
    for (uint32_t q = 0; q < 2 * R; q++) {
      uint32_t rec = (q >> 1) * S + sub;
      Slice x = slice_of(cur, 2 * rec + (q & 1));
      uint32_t e = x.n - 16 * x.nc;
      for (uint32_t i = sl; i < e; i += G) {
        uint32_t off = i < x.head ? i : x.n - e + i;
        x.d[off] = x.s[off];
      }
      for (uint32_t c0 = G; c0 < x.nc; c0 += 4 * G) { /* 4 loads in flight */
        Chunk t[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          uint32_t c = c0 + k * G + sl;
          if (c < x.nc) t[k] = load16<UNAL, NT>(x.s + x.head + 16 * (size_t)c);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
          uint32_t c = c0 + k * G + sl;
          if (c < x.nc)
            store16<UNAL, NT>(x.d + x.head + 16 * (size_t)c,
                              x.s + x.head + 16 * (size_t)c, t[k]);
        }
      }
    }
    cur = nxt;
  }
}

} // namespace pcopy
} // namespace gra
