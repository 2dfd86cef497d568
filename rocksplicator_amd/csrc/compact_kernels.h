/* compact_kernels.h — device side of gra_compact: replace a shard's oldest
 * device runs with one key-sorted run (≅ ApplicationDB::CompactRange(nullptr,
 * nullptr), rocksdb_admin/application_db.cpp:138-143). Included by engine.hip
 * inside namespace gra, after scan_kernels.h.
 *
 * The scan chain over the unbounded range already computes what a full
 * compaction keeps: k_sc_collect -> bitonic sort by (key asc, seq desc) ->
 * k_sc_heads -> k_sc_fold leave, per key, its newest entry first and every
 * live Merge head's folded size. The three kernels here write that result
 * back into the store as a run in the tick path's record layout:
 *
 *   k_cp_resolve   a live head costs (1 record, align16(klen + folded vlen))
 *                  instead of the scan's page cost; fused with the in-block
 *                  half of the prefix sum, like k_sc_resolve
 *   k_cp_finish    single block: block partials + carry, then the header and
 *                  payload space is bump-reserved from the store cursor the
 *                  way k_scan2 reserves a tick (single writer, stream-
 *                  ordered). A full arena sets `overflow` and reserves nothing
 *   k_cp_emit      one lane group per live head: header (kpref filled, as
 *                  k_kpref would) + key + value. A Put head is one 16-B
 *                  aligned vector copy of its padded source record
 *   k_cp_emit_chain  concat only: one wave per live Merge head walks the
 *                  chain from its far end, 64 entries a step, so a chain of
 *                  any length is written
 *
 * Dead keys, Deletes, SingleDeletes, shadowed versions and range tombstones
 * cost nothing and are not written. */
#pragma once

enum : uint32_t {
  kCpTooManyTombs = 1,   /* > kScTombCap range tombstones in the prefix */
  kCpTooManyEntries = 2, /* candidate buffer too small (host sizing bug) */
  kCpPayloadTooBig = 4,  /* kv_off is 32 bits: payload must stay < 4 GiB */
  kCpValueTooBig = 8,    /* a value of 0xFFFF0000 bytes or more */
};

/* result block, one D2H at the end of the chain */
struct CpCtl {
  uint64_t hdr_off, payload_off; /* absolute store offsets of the new run */
  uint64_t payload_bytes;
  uint32_t n_out;
  uint32_t overflow;    /* arena full: nothing reserved, nothing written */
  uint32_t unsupported; /* kCp* bits: nothing reserved, nothing written */
  uint32_t ncand, ntomb, _pad;
};

__host__ __device__ inline uint32_t cp_align16(uint64_t n) {
  return (uint32_t)((n + 15) & ~15ULL);
}

/* One thread per sorted candidate; the liveness rules are k_sc_resolve's. A
 * live Merge head must have been folded (k_sc_fold leaves it unfolded only
 * when its value would not fit 32 bits). */
__global__ void __launch_bounds__(256) k_cp_resolve(
    const uint8_t *__restrict__ store, const ScCand *__restrict__ cands,
    const ScTomb *__restrict__ tombs, const ScCtl *__restrict__ ctl,
    uint32_t cap, uint32_t tomb_cap, ScItem *__restrict__ items,
    ScSum *__restrict__ bsums, const ScFold *__restrict__ folds,
    CpCtl *__restrict__ cp) {
  __shared__ ScSum sh[256];
  uint32_t n = sc_count(ctl, cap);
  uint32_t ntomb = ctl->ntomb < tomb_cap ? ctl->ntomb : tomb_cap;
  uint32_t i = blockIdx.x * 256 + threadIdx.x;
  ScSum v = {0, 0, 0};
  if (i < n) {
    ScCand c = cands[i];
    bool head = i == 0 || !sc_same_key(store, cands[i - 1], c);
    uint64_t bytes = 0;
    bool live = false;
    if (head && c.type == wb::kMerge) {
      ScFold f = folds[i];
      if (f.flags & kScFoldLive) {
        live = true;
        if (f.flags & kScFoldFolded)
          bytes = (uint64_t)c.klen + f.vlen;
        else
          bytes = 0xFFFF0000ull;
      }
    } else if (head && c.type == wb::kValue) {
      /* sc_tomb_kills, written out: through the helper this kernel compiles
       * to two more SGPRs (profiles/readpath) */
      const uint8_t *key = store + c.koff;
      live = true;
      for (uint32_t t = 0; t < ntomb && live; t++) {
        ScTomb tb = tombs[t];
        if (tb.seq < c.seq) continue;
        const uint8_t *b = store + tb.boff;
        if (sc_cmp_bytes(b, tb.bl, key, c.klen) <= 0 &&
            sc_cmp_bytes(key, c.klen, b + tb.bl, tb.el) < 0)
          live = false;
      }
      bytes = (uint64_t)c.klen + c.vlen;
    }
    if (live) {
      if (bytes >= 0xFFFF0000ull) {
        atomicOr(&cp->unsupported, (uint32_t)kCpValueTooBig);
      } else {
        v.cnt = 1;
        v.bytes = cp_align16(bytes);
      }
    }
  }
  ScSum inc = sc_block_scan(v, sh);
  if (i < n)
    items[i] = {inc.bytes - v.bytes, (inc.cnt - v.cnt) | (v.cnt << 31),
                (uint32_t)v.bytes};
  if (threadIdx.x == 255) bsums[blockIdx.x] = inc;
}

/* single block: block sums -> exclusive in place with a carry across
 * 256-wide chunks (as k_sc_scan2), then the reservation. store_cap is the
 * linear arena's size; the cursor only grows and stays 16-B aligned. */
__global__ void __launch_bounds__(256) k_cp_finish(
    ScSum *__restrict__ bsums, uint32_t nblocks,
    const ScCtl *__restrict__ ctl, uint32_t cap, uint32_t tomb_cap,
    uint64_t *__restrict__ cursor, uint64_t store_cap,
    CpCtl *__restrict__ cp) {
  __shared__ ScSum sh[256];
  __shared__ ScSum carry;
  if (threadIdx.x == 0) carry = {0, 0, 0};
  __syncthreads();
  for (uint32_t base = 0; base < nblocks; base += 256) {
    uint32_t i = base + threadIdx.x;
    ScSum v = i < nblocks ? bsums[i] : ScSum{0, 0, 0};
    ScSum inc = sc_add(sc_block_scan(v, sh), carry);
    if (i < nblocks) bsums[i] = {inc.bytes - v.bytes, inc.cnt - v.cnt, 0};
    __syncthreads();
    if (threadIdx.x == 255) carry = inc;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    uint32_t bad = cp->unsupported;
    if (ctl->ntomb > tomb_cap) bad |= kCpTooManyTombs;
    if (ctl->ncand > cap) bad |= kCpTooManyEntries;
    if (carry.bytes >= (1ULL << 32)) bad |= kCpPayloadTooBig;
    uint64_t need_hdr = cp_align16((uint64_t)carry.cnt * sizeof(wb::RecHdr));
    uint64_t need = need_hdr + carry.bytes;
    uint64_t cur = *cursor;
    cp->unsupported = bad;
    cp->ncand = ctl->ncand;
    cp->ntomb = ctl->ntomb;
    cp->n_out = carry.cnt;
    cp->payload_bytes = carry.bytes;
    cp->hdr_off = cp->payload_off = 0;
    cp->overflow = 0;
    if (bad) return;
    if (need > store_cap || cur + need > store_cap) {
      cp->overflow = 1;
      return;
    }
    cp->hdr_off = cur;
    cp->payload_off = cur + need_hdr;
    *cursor = cur + need;
  }
}

__device__ inline void cp_write_hdr(uint8_t *store, const CpCtl *cp,
                                    uint32_t rank, uint64_t off,
                                    const ScCand &c, uint32_t vlen) {
  wb::RecHdr h;
  h.seq = c.seq;
  h.kv_off = (uint32_t)off; /* run-relative: pay_rel_base = 0 */
  h.val_len = vlen;
  h.key_len = c.klen;
  h.type = wb::kValue;
  h.flags = 0;
  h.kpref = wb::key_fnv_fold(wb::kFnvBasis32, store + c.koff, c.klen);
  ((wb::RecHdr *)(store + cp->hdr_off))[rank] = h;
}

/* G lanes per sorted candidate. MODE: 1 = concat (live Merge heads are left
 * to k_cp_emit_chain), 2 = u64add (a Merge head's value is the 8 counter
 * bytes). Source and destination records are both 16-B aligned and padded
 * to 16 B, so a Put head moves as whole uint4s. */
template <int G, int MODE>
__global__ void __launch_bounds__(256) k_cp_emit(
    uint8_t *__restrict__ store, const ScCand *__restrict__ cands,
    const ScItem *__restrict__ items, const ScSum *__restrict__ bsums,
    const ScCtl *__restrict__ ctl, const CpCtl *__restrict__ cp, uint32_t cap,
    const ScFold *__restrict__ folds) {
  if (cp->overflow || cp->unsupported) return;
  uint32_t g = (blockIdx.x * blockDim.x + threadIdx.x) / G;
  uint32_t lane = threadIdx.x & (G - 1);
  if (g >= sc_count(ctl, cap)) return;
  ScItem it = items[g];
  if (!(it.excl_cnt >> 31)) return;
  ScCand c = cands[g];
  if (MODE == 1 && c.type == wb::kMerge) return;
  ScSum bs = bsums[g >> 8];
  uint32_t rank = (it.excl_cnt & 0x7FFFFFFFu) + bs.cnt;
  uint64_t off = it.excl_bytes + bs.bytes;
  uint8_t *dst = store + cp->payload_off + off;
  const uint8_t *src = store + c.koff;
  uint32_t vlen = c.vlen;
  if (c.type == wb::kValue) {
    uint32_t n16 = it.cost >> 4;
    for (uint32_t w = lane; w < n16; w += G)
      ((uint4 *)dst)[w] = ((const uint4 *)src)[w];
  } else { /* MODE 2: folded counter */
    uint64_t sum = folds[g].sum;
    vlen = 8;
    copy_dword<G>(dst, src, c.klen, lane);
    if (lane < 8) dst[c.klen + lane] = (uint8_t)(sum >> (8 * lane));
    for (uint32_t p = c.klen + 8u + lane; p < it.cost; p += G) dst[p] = 0;
  }
  if (lane == 0) cp_write_hdr(store, cp, rank, off, c, vlen);
}

/* Concat: one wave per live Merge head (the list k_sc_heads built), strided
 * over the launched waves. The chain's entries follow the head newest first:
 * operands idx .. idx+nops-1, then the base. Output order is oldest first,
 * so entry e of the output is candidate idx + E-1-e. Each step loads 64
 * entries at once, wave-scans their lengths into output positions and then
 * copies them one by one with all 64 lanes. */
__global__ void __launch_bounds__(256) k_cp_emit_chain(
    uint8_t *__restrict__ store, const ScCand *__restrict__ cands,
    const ScItem *__restrict__ items, const ScSum *__restrict__ bsums,
    const ScHead *__restrict__ heads, const ScCtl *__restrict__ ctl,
    const CpCtl *__restrict__ cp, uint32_t cap,
    const ScFold *__restrict__ folds) {
  if (cp->overflow || cp->unsupported) return;
  uint32_t nheads = ctl->nheads < cap ? ctl->nheads : cap;
  uint32_t lane = threadIdx.x & 63;
  uint32_t wave = (blockIdx.x * 256 + threadIdx.x) >> 6;
  uint32_t nwaves = gridDim.x * 4;
  for (uint32_t h = wave; h < nheads; h += nwaves) { /* wave-uniform */
    uint32_t g = heads[h].idx;
    ScItem it = items[g];
    if (!(it.excl_cnt >> 31)) continue;
    ScFold f = folds[g];
    ScCand c = cands[g];
    ScSum bs = bsums[g >> 8];
    uint32_t rank = (it.excl_cnt & 0x7FFFFFFFu) + bs.cnt;
    uint64_t off = it.excl_bytes + bs.bytes;
    uint8_t *dst = store + cp->payload_off + off;
    copy_dword<64>(dst, store + c.koff, c.klen, lane);
    uint8_t *val = dst + c.klen;
    uint32_t E = (uint32_t)f.sum + ((f.flags & kScFoldBase) ? 1u : 0u);
    uint64_t o = 0; /* value bytes written so far */
    for (uint32_t e0 = 0; e0 < E; e0 += 64) {
      uint32_t e = e0 + lane;
      unsigned long long src = 0, len = 0, sep = 0;
      if (e < E) {
        ScCand p = cands[g + (E - 1 - e)];
        src = p.koff + p.klen;
        len = p.vlen;
        sep = e > 0 ? 1 : 0; /* ',' in front of all but the first entry */
      }
      unsigned long long incl = len + sep;
      for (int ofs = 1; ofs < 64; ofs <<= 1) {
        unsigned long long x = __shfl_up(incl, ofs, 64);
        if (lane >= (uint32_t)ofs) incl += x;
      }
      unsigned long long start = o + incl - len;
      uint32_t m = E - e0 < 64 ? E - e0 : 64;
      for (uint32_t l = 0; l < m; l++) {
        unsigned long long s = __shfl(src, l, 64), n = __shfl(len, l, 64),
                           st = __shfl(start, l, 64);
        if (e0 + l > 0 && lane == 0) val[st - 1] = ',';
        copy_dword<64>(val + st, store + s, (uint32_t)n, lane);
      }
      o += __shfl(incl, 63, 64);
    }
    for (uint32_t p = c.klen + f.vlen + lane; p < it.cost; p += 64) dst[p] = 0;
    if (lane == 0) cp_write_hdr(store, cp, rank, off, c, f.vlen);
  }
}
