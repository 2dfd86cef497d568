/* image_kernels.h — device side of gra_import (and of gra_export's content
 * sum): prove a staged shard image well-formed, reserve its place in the
 * store and put it there (≅ restoreDBHelper's ingest of a backup,
 * rocksdb_admin/admin_handler.cpp:865-943, without the file transport).
 * Included by engine.hip inside namespace gra, after compact_kernels.h.
 * gfx950, wave64, 256-thread blocks.
 *
 * The image body (host_store.h has the format and THE VERDICT RULE) is
 * untrusted bytes in a staging buffer: n RecHdr, padded to 16 B, then the
 * payload. Nothing reads it before k_img_check has passed it:
 *
 *   k_img_check    one thread per entry: the RECORD, LAYOUT and ORDER rules
 *                  on entry i (ORDER against i-1). Every offset is bounds-
 *                  checked in 64-bit arithmetic before a key is read. A
 *                  failing entry posts (index << 3 | reason) with atomicMin,
 *                  so the lowest index decides; a passing entry hashes its
 *                  record (rec_hash_cs) from whole uint4 loads and the wave's
 *                  sum goes out in one atomic
 *   k_img_reserve  one thread: verdict and sum against the header's; then the
 *                  bump reservation from the store cursor, k_cp_finish's
 *                  tail. A rejected image or a full arena reserves nothing
 *   k_img_place    headers with a fresh kpref and the payload as whole uint4s
 *                  into the reservation
 *
 * k_checksum is one block per run and would put a whole image on one block;
 * these are grids over the entries. */
#pragma once

constexpr unsigned long long kImgClean = ~0ull; /* no entry has failed */

/* control block, one D2H at the end of the chain */
struct ImgCtl {
  unsigned long long verdict; /* min over failing entries of index << 3 |
                                 reason; kImgClean when none */
  unsigned long long sum;     /* content sum of the passing entries */
  uint64_t hdr_off, payload_off; /* absolute store offsets of the new run */
  uint32_t reason;   /* kImg*: what k_img_reserve decided */
  uint32_t overflow; /* arena full: nothing reserved, nothing written */
};

/* FNV-1a-64 of one byte; the record hash is rec_hash_cs's, byte for byte */
__device__ inline uint64_t img_fold(uint64_t h, uint32_t b) {
  return (h ^ (uint64_t)(b & 0xFFu)) * 1099511628211ULL;
}

/* hdrs/pay: the image body (staging buffer), or a run in the store whose
 * kv_off are run-relative (gra_export's scratch run). pay is 16-B aligned
 * and payload_bytes a multiple of 16, so with kv_off a multiple of 16 and
 * kv_off + key_len + val_len <= payload_bytes every uint4 a record touches
 * lies inside the payload. */
__global__ void __launch_bounds__(256) k_img_check(
    const wb::RecHdr *__restrict__ hdrs, const uint8_t *__restrict__ pay,
    uint64_t n, uint64_t payload_bytes, uint64_t last_seq,
    ImgCtl *__restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint64_t local = 0;
  if (i < n) {
    const wb::RecHdr h = hdrs[i];
    const uint64_t bytes = (uint64_t)h.key_len + h.val_len;
    const bool in = (uint64_t)h.kv_off + bytes <= payload_bytes;
    uint32_t bad = kImgOk;
    if (h.type != wb::kValue || h.flags != 0 || h.seq < 1 ||
        h.seq > last_seq || h.val_len >= 0xFFFF0000u) {
      bad = kImgBadRecord;
    } else {
      uint64_t want = 0;
      bool prev_in = false;
      wb::RecHdr p = {};
      if (i > 0) {
        p = hdrs[i - 1];
        const uint64_t pbytes = (uint64_t)p.key_len + p.val_len;
        want = (uint64_t)p.kv_off + ((pbytes + 15) & ~15ull);
        prev_in = (uint64_t)p.kv_off + pbytes <= payload_bytes;
      }
      if ((h.kv_off & 15u) || (uint64_t)h.kv_off != want || !in ||
          (i == n - 1 &&
           (uint64_t)h.kv_off + ((bytes + 15) & ~15ull) != payload_bytes))
        bad = kImgBadLayout;
      /* both keys are inside the payload here, and only here */
      else if (i > 0 && prev_in &&
               sc_cmp_bytes(pay + p.kv_off, p.key_len, pay + h.kv_off,
                            h.key_len) >= 0)
        bad = kImgBadOrder;
    }
    if (bad != kImgOk) {
      atomicMin(&ctl->verdict, (unsigned long long)((i << 3) | bad));
    } else {
      /* in bounds, 16-B aligned: the record as whole uint4s, bytes folded
       * from registers */
      uint64_t hsh = 1469598103934665603ULL;
      for (int b = 0; b < 8; b++) hsh = img_fold(hsh, (uint32_t)(h.seq >> (8 * b)));
      hsh = img_fold(hsh, h.type);
      for (int b = 0; b < 4; b++) hsh = img_fold(hsh, (uint32_t)h.key_len >> (8 * b));
      for (int b = 0; b < 4; b++) hsh = img_fold(hsh, h.val_len >> (8 * b));
      const uint4 *rec = (const uint4 *)(pay + h.kv_off);
      const uint64_t n16 = bytes >> 4;
      for (uint64_t w = 0; w < n16; w++) {
        const uint4 v = rec[w];
        const uint32_t q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int d = 0; d < 4; d++)
#pragma unroll
          for (int b = 0; b < 4; b++) hsh = img_fold(hsh, q[d] >> (8 * b));
      }
      const uint32_t rem = (uint32_t)(bytes & 15);
      if (rem) {
        const uint4 v = rec[n16];
        const uint32_t q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int b = 0; b < 16; b++)
          if ((uint32_t)b < rem) hsh = img_fold(hsh, q[b >> 2] >> (8 * (b & 3)));
      }
      local = hsh;
    }
  }
  /* wave-reduce, then one atomic per wave (every lane gets here) */
  for (int ofs = 32; ofs > 0; ofs >>= 1) local += __shfl_down(local, ofs, 64);
  if ((threadIdx.x & 63) == 0 && local)
    atomicAdd(&ctl->sum, (unsigned long long)local);
}

/* Single writer of the store cursor, stream-ordered behind the ticks and
 * compactions queued before it, as k_cp_finish. */
__global__ void k_img_reserve(ImgCtl *__restrict__ ctl, uint64_t n,
                              uint64_t payload_bytes, uint64_t content_sum,
                              uint64_t *__restrict__ cursor,
                              uint64_t store_cap) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  ctl->hdr_off = ctl->payload_off = 0;
  ctl->overflow = 0;
  if (ctl->verdict != kImgClean) {
    ctl->reason = (uint32_t)(ctl->verdict & 7);
    return;
  }
  if (ctl->sum != content_sum) {
    ctl->reason = kImgBadSum;
    return;
  }
  ctl->reason = kImgOk;
  const uint64_t need_hdr = (n * sizeof(wb::RecHdr) + 15) & ~15ull;
  const uint64_t need = need_hdr + payload_bytes;
  const uint64_t cur = *cursor;
  if (need > store_cap || cur + need > store_cap) {
    ctl->overflow = 1;
    return;
  }
  ctl->hdr_off = cur;
  ctl->payload_off = cur + need_hdr;
  *cursor = cur + need;
}

/* Grid-stride: the payload as whole uint4s, then one thread per header. The
 * staged image passed k_img_check, so every key lies inside the payload. */
__global__ void __launch_bounds__(256) k_img_place(
    uint8_t *__restrict__ store, const ImgCtl *__restrict__ ctl,
    const wb::RecHdr *__restrict__ hdrs, const uint8_t *__restrict__ pay,
    uint64_t n, uint64_t payload_bytes) {
  if (ctl->reason != kImgOk || ctl->overflow) return;
  const uint64_t tid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * 256;
  uint4 *dst = (uint4 *)(store + ctl->payload_off);
  const uint4 *src = (const uint4 *)pay;
  for (uint64_t w = tid; w < (payload_bytes >> 4); w += nthreads)
    dst[w] = src[w];
  wb::RecHdr *out = (wb::RecHdr *)(store + ctl->hdr_off);
  for (uint64_t i = tid; i < n; i += nthreads) {
    wb::RecHdr h = hdrs[i];
    h.kpref = wb::key_fnv_fold(wb::kFnvBasis32, pay + h.kv_off, h.key_len);
    out[i] = h;
  }
}
