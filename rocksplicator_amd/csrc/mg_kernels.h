/* mg_kernels.h — device side of gra_multiget: the per-query scan kernel, the
 * lazy read-index build (k_kpref) and the hash-join chain. Included by
 * engine.hip inside namespace gra; RunView, the run descriptor every read
 * path stages, lives here too. */
#pragma once

/* ---------------- device read serving (multiget) ----------------
 * One block per query: scan the shard's runs newest->oldest; per matching
 * entry track the max-seq terminator (Put/Delete/SingleDelete), whether any
 * Merge sits above it (=> host fold), and the max covering range-tombstone
 * seq. Followers serve reads in rocksplicator deployments; with the
 * memtable resident in HBM the lookup runs there too. */
struct RunView {
  uint64_t hdr_off, payload_off;
  uint32_t n_entries, pay_rel_base;
};

__device__ inline int dev_memcmp(const uint8_t *a, const uint8_t *b, uint32_t n) {
  for (uint32_t i = 0; i < n; i++) {
    if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
  }
  return 0;
}

/* per-query raw seq info so mixed device/host shards can merge the device
 * verdict with a host-run probe (gra_multiget) */
struct MgExtra {
  uint64_t term_seq, merge_seq, rd_seq;
  uint32_t term_type, _pad;
};

__global__ void k_multiget(const uint8_t *__restrict__ store,
                           const RunView *__restrict__ runs, uint32_t nruns,
                           const GraKeyRef *__restrict__ keys,
                           const uint8_t *__restrict__ keybuf, uint32_t nq,
                           uint8_t *__restrict__ valbuf, uint32_t val_stride,
                           GraGetResult *__restrict__ out,
                           MgExtra *__restrict__ extra, int fold_u64) {
  __shared__ uint64_t sh_term_seq[256];
  __shared__ uint64_t sh_term_ref[256]; /* (run<<32)|entry, ~0 = none */
  __shared__ uint64_t sh_merge_seq[256];
  __shared__ uint64_t sh_rd_seq[256];
  uint32_t q = blockIdx.x;
  if (q >= nq) return;
  const uint8_t *key = keybuf + keys[q].off;
  uint32_t klen = keys[q].len;
  uint32_t qpref = wb::key_fnv_fold(wb::kFnvBasis32, key, klen);
  uint64_t term_seq = 0, term_ref = ~0ULL, merge_seq = 0, rd_seq = 0;
  for (uint32_t r = 0; r < nruns; r++) {
    RunView rv = runs[r];
    const wb::RecHdr *hdrs = (const wb::RecHdr *)(store + rv.hdr_off);
    const uint8_t *pay = store + rv.payload_off;
    for (uint32_t i = threadIdx.x; i < rv.n_entries; i += blockDim.x) {
      wb::RecHdr h = hdrs[i];
      if (h.type != wb::kRangeDeletion &&
          (h.key_len != klen || h.kpref != qpref))
        continue; /* header-only reject: no payload touch */
      uint32_t rel = h.kv_off - rv.pay_rel_base;
      if (h.type == wb::kRangeDeletion) {
        const uint8_t *b = pay + rel, *e2 = pay + rel + h.key_len;
        uint32_t bl = h.key_len, el = h.val_len;
        int c1 = dev_memcmp(b, key, bl < klen ? bl : klen);
        if (c1 > 0 || (c1 == 0 && bl > klen)) continue;
        int c2 = dev_memcmp(key, e2, klen < el ? klen : el);
        if (c2 > 0 || (c2 == 0 && klen >= el)) continue;
        if (h.seq > rd_seq) rd_seq = h.seq;
        continue;
      }
      if (dev_memcmp(pay + rel, key, klen) != 0) /* len+prefix pre-checked */
        continue;
      if (h.type == wb::kMerge) {
        if (h.seq > merge_seq) merge_seq = h.seq;
      } else if (h.seq > term_seq) {
        term_seq = h.seq;
        term_ref = ((uint64_t)r << 32) | i;
      }
    }
  }
  uint32_t tid = threadIdx.x;
  sh_term_seq[tid] = term_seq;
  sh_term_ref[tid] = term_ref;
  sh_merge_seq[tid] = merge_seq;
  sh_rd_seq[tid] = rd_seq;
  __syncthreads();
  for (uint32_t ofs = blockDim.x / 2; ofs > 0; ofs >>= 1) {
    if (tid < ofs) {
      if (sh_term_seq[tid + ofs] > sh_term_seq[tid]) {
        sh_term_seq[tid] = sh_term_seq[tid + ofs];
        sh_term_ref[tid] = sh_term_ref[tid + ofs];
      }
      if (sh_merge_seq[tid + ofs] > sh_merge_seq[tid])
        sh_merge_seq[tid] = sh_merge_seq[tid + ofs];
      if (sh_rd_seq[tid + ofs] > sh_rd_seq[tid])
        sh_rd_seq[tid] = sh_rd_seq[tid + ofs];
    }
    __syncthreads();
  }
  uint64_t T = sh_term_seq[0], M = sh_merge_seq[0], RD = sh_rd_seq[0];
  uint64_t ref = sh_term_ref[0];
  uint8_t term_type = 0xFF;
  wb::RecHdr h = {};
  RunView rv = {};
  if (ref != ~0ULL) {
    rv = runs[ref >> 32];
    h = ((const wb::RecHdr *)(store + rv.hdr_off))[(uint32_t)ref];
    term_type = h.type;
  }
  if (tid == 0 && extra) { /* raw verdict for host-side merging */
    extra[q].term_seq = T;
    extra[q].merge_seq = M;
    extra[q].rd_seq = RD;
    extra[q].term_type = term_type;
  }
  uint64_t floor_seq = T > RD ? T : RD;
  if (M > floor_seq && fold_u64) {
    /* fold_on_device, u64add: a second pass over the runs sums the operands
     * above the floor (integer adds commute: any order). Long chains land
     * here — they overflow the hash join's candidate cap. */
    uint64_t acc = 0;
    for (uint32_t r = 0; r < nruns; r++) {
      RunView rv2 = runs[r];
      const wb::RecHdr *hdrs = (const wb::RecHdr *)(store + rv2.hdr_off);
      const uint8_t *pay = store + rv2.payload_off;
      for (uint32_t i = tid; i < rv2.n_entries; i += blockDim.x) {
        wb::RecHdr h2 = hdrs[i];
        if (h2.type != wb::kMerge || h2.seq <= floor_seq ||
            h2.key_len != klen || h2.kpref != qpref)
          continue;
        const uint8_t *k2 = pay + (h2.kv_off - rv2.pay_rel_base);
        if (dev_memcmp(k2, key, klen) != 0) continue;
        acc = fold::add_wrap(acc, fold::load_u64le(k2 + klen, h2.val_len));
      }
    }
    __syncthreads(); /* the shared arrays were read above */
    sh_term_seq[tid] = acc;
    __syncthreads();
    for (uint32_t ofs = blockDim.x / 2; ofs > 0; ofs >>= 1) {
      if (tid < ofs)
        sh_term_seq[tid] =
            fold::add_wrap(sh_term_seq[tid], sh_term_seq[tid + ofs]);
      __syncthreads();
    }
    if (tid == 0) {
      uint64_t v = sh_term_seq[0];
      if (T > RD && term_type == wb::kValue) /* base: the Put above RD */
        v = fold::add_wrap(
            v, fold::load_u64le(store + rv.payload_off +
                                    (h.kv_off - rv.pay_rel_base) + h.key_len,
                                h.val_len));
      fold::store_u64le(valbuf + (size_t)q * val_stride, v, val_stride);
      out[q].status = GRA_GET_FOUND;
      out[q].vlen = 8; /* true length (caller sees truncation) */
    }
    return;
  }
  if (M > floor_seq) { /* live merge operands: fold on the host */
    if (tid == 0) {
      out[q].status = GRA_GET_NEEDS_HOST;
      out[q].vlen = 0;
    }
    return;
  }
  if (T == 0 || T <= RD || ref == ~0ULL) {
    if (tid == 0) {
      out[q].status = GRA_GET_MISS;
      out[q].vlen = 0;
    }
    return;
  }
  if (h.type != wb::kValue) { /* Delete/SingleDelete terminator */
    if (tid == 0) {
      out[q].status = GRA_GET_MISS;
      out[q].vlen = 0;
    }
    return;
  }
  uint32_t vlen = h.val_len < val_stride ? h.val_len : val_stride;
  const uint8_t *src = store + rv.payload_off + (h.kv_off - rv.pay_rel_base) +
                       h.key_len;
  uint8_t *dst = valbuf + (size_t)q * val_stride;
  for (uint32_t b = tid; b < vlen; b += blockDim.x) dst[b] = src[b];
  if (tid == 0) {
    out[q].status = GRA_GET_FOUND;
    out[q].vlen = h.val_len; /* true length (caller sees truncation) */
  }
}

/* Lazy read-index build: one coalesced pass over a run fills every
 * header's key fingerprint from the STORED key bytes (contiguous in the
 * payload). Launched at a run's first multiget — apply-time fills all
 * measured 160-480 us/tick against the headline (see k_emit). */
__global__ void k_kpref(uint8_t *__restrict__ store,
                        const RunView *__restrict__ runs) {
  RunView rv = runs[blockIdx.y];
  wb::RecHdr *hdrs = (wb::RecHdr *)(store + rv.hdr_off);
  const uint8_t *pay = store + rv.payload_off;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < rv.n_entries;
       i += gridDim.x * blockDim.x) {
    wb::RecHdr h = hdrs[i];
    hdrs[i].kpref =
        (h.type == wb::kRangeDeletion)
            ? 0 /* tombstones are range-matched, not hash-matched */
            : wb::key_fnv_fold(wb::kFnvBasis32,
                               pay + (h.kv_off - rv.pay_rel_base), h.key_len);
  }
}

/* ---------------- hash-join multiget ----------------
 * The linear per-query scan is header-bandwidth bound (nq × entries × 24 B).
 * Invert it: ONE coalesced pass over all entries probes an open-addressed
 * query-fingerprint table (kpref -> query idx) and appends the rare
 * matches to a candidate list; tiny resolve kernels then pick per-query
 * winners by seq. Traffic: O(entries + matches) instead of O(nq × entries).
 * Range tombstones are collected in the same pass and tested per query
 * separately (they cover key RANGES — not hash-matchable). Overflow of
 * either list falls back to the per-query scan kernel. */
struct MgCand {
  uint32_t qidx, run, entry, type;
  uint64_t seq;
};
struct MgTomb {
  uint32_t run, entry, _pad0, _pad1;
  uint64_t seq;
};

__global__ void k_mg_scan(const uint8_t *__restrict__ store,
                          const RunView *__restrict__ runs,
                          const uint64_t *__restrict__ qtab, uint32_t qmask,
                          const GraKeyRef *__restrict__ keys,
                          const uint8_t *__restrict__ keybuf,
                          MgCand *__restrict__ cands,
                          uint32_t *__restrict__ ncand, uint32_t cand_cap,
                          MgTomb *__restrict__ tombs,
                          uint32_t *__restrict__ ntomb, uint32_t tomb_cap) {
  uint32_t r = blockIdx.y;
  RunView rv = runs[r];
  const wb::RecHdr *hdrs = (const wb::RecHdr *)(store + rv.hdr_off);
  const uint8_t *pay = store + rv.payload_off;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < rv.n_entries;
       i += gridDim.x * blockDim.x) {
    wb::RecHdr h = hdrs[i];
    if (h.type == wb::kRangeDeletion) {
      uint32_t slot = atomicAdd(ntomb, 1u);
      if (slot < tomb_cap) tombs[slot] = {r, i, 0, 0, h.seq};
      continue;
    }
    uint32_t s = h.kpref & qmask;
    while (true) { /* linear probe; duplicates of a fingerprint chain on */
      uint64_t e = qtab[s];
      if (e == 0) break;
      if ((uint32_t)(e >> 32) == h.kpref) {
        uint32_t qidx = (uint32_t)e - 1;
        uint32_t klen = keys[qidx].len;
        if (h.key_len == klen &&
            dev_memcmp(pay + (h.kv_off - rv.pay_rel_base),
                       keybuf + keys[qidx].off, klen) == 0) {
          uint32_t slot = atomicAdd(ncand, 1u);
          if (slot < cand_cap) cands[slot] = {qidx, r, i, h.type, h.seq};
        }
      }
      s = (s + 1) & qmask;
    }
  }
}

__global__ void k_mg_resolve1(const MgCand *__restrict__ cands,
                              const uint32_t *__restrict__ ncand_p,
                              uint32_t cap,
                              unsigned long long *__restrict__ term_pack,
                              unsigned long long *__restrict__ merge_seq) {
  uint32_t n = *ncand_p < cap ? *ncand_p : cap; /* device-side bound: no
                                                   host sync between scan
                                                   and resolve */
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  MgCand c = cands[i];
  if (c.type == wb::kMerge)
    atomicMax(&merge_seq[c.qidx], (unsigned long long)c.seq);
  else /* seqs are unique per shard: the packed max has ONE winner */
    atomicMax(&term_pack[c.qidx],
              (unsigned long long)((c.seq << 8) | c.type));
}

__global__ void k_mg_tombs(const uint8_t *__restrict__ store,
                           const RunView *__restrict__ runs,
                           const MgTomb *__restrict__ tombs,
                           const uint32_t *__restrict__ ntomb_p, uint32_t cap,
                           const GraKeyRef *__restrict__ keys,
                           const uint8_t *__restrict__ keybuf, uint32_t nq,
                           unsigned long long *__restrict__ rd_seq) {
  uint32_t ntomb = *ntomb_p < cap ? *ntomb_p : cap;
  uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const uint8_t *key = keybuf + keys[q].off;
  uint32_t klen = keys[q].len;
  uint64_t best = 0;
  for (uint32_t t = 0; t < ntomb; t++) {
    MgTomb mt = tombs[t];
    RunView rv = runs[mt.run];
    const wb::RecHdr *hdrs = (const wb::RecHdr *)(store + rv.hdr_off);
    wb::RecHdr h = hdrs[mt.entry];
    const uint8_t *pay = store + rv.payload_off;
    uint32_t rel = h.kv_off - rv.pay_rel_base;
    const uint8_t *b = pay + rel, *e2 = pay + rel + h.key_len;
    uint32_t bl = h.key_len, el = h.val_len;
    int c1 = dev_memcmp(b, key, bl < klen ? bl : klen);
    if (c1 > 0 || (c1 == 0 && bl > klen)) continue;
    int c2 = dev_memcmp(key, e2, klen < el ? klen : el);
    if (c2 > 0 || (c2 == 0 && klen >= el)) continue;
    if (h.seq > best) best = h.seq;
  }
  rd_seq[q] = best;
}

__global__ void k_mg_resolve2(const MgCand *__restrict__ cands,
                              const uint32_t *__restrict__ ncand_p,
                              uint32_t cap,
                              const unsigned long long *__restrict__ term_pack,
                              unsigned long long *__restrict__ winner_ref) {
  uint32_t n = *ncand_p < cap ? *ncand_p : cap;
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  MgCand c = cands[i];
  if (c.type != wb::kMerge &&
      term_pack[c.qidx] == (unsigned long long)((c.seq << 8) | c.type))
    winner_ref[c.qidx] = ((unsigned long long)c.run << 32) | c.entry;
}

/* fold_on_device, u64add: every Merge candidate above its query's floor
 * max(T, RD) adds its operand into acc[qidx]. Hot counters put most of a
 * wave on one query, so lanes that share a qidx are summed in the wave
 * first and their leader issues the one global atomic; a lane alone on its
 * query adds directly. Integer adds commute: arrival order is immaterial. */
__global__ void __launch_bounds__(256) k_mg_fold(
    const uint8_t *__restrict__ store, const RunView *__restrict__ runs,
    const MgCand *__restrict__ cands, const uint32_t *__restrict__ ncand_p,
    uint32_t cap, const unsigned long long *__restrict__ term_pack,
    const unsigned long long *__restrict__ rd_seq,
    unsigned long long *__restrict__ acc) {
  uint32_t n = *ncand_p < cap ? *ncand_p : cap;
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t lane = threadIdx.x & 63;
  bool active = false;
  uint32_t q = 0;
  uint64_t v = 0;
  if (i < n) {
    MgCand c = cands[i];
    if (c.type == wb::kMerge) {
      uint64_t T = term_pack[c.qidx] >> 8, RD = rd_seq[c.qidx];
      if (c.seq > (T > RD ? T : RD)) {
        RunView rv = runs[c.run];
        wb::RecHdr h = ((const wb::RecHdr *)(store + rv.hdr_off))[c.entry];
        v = fold::load_u64le(store + rv.payload_off +
                                 (h.kv_off - rv.pay_rel_base) + h.key_len,
                             h.val_len);
        q = c.qidx;
        active = true;
      }
    }
  }
  /* wave-uniform loop: peel one query per turn */
  for (unsigned long long m = __ballot(active); m; m = __ballot(active)) {
    uint32_t leader = (uint32_t)__ffsll((long long)m) - 1;
    uint32_t lq = __shfl(q, leader, 64);
    bool mine = active && q == lq;
    unsigned long long grp = __ballot(mine);
    uint64_t sum = v;
    if (grp & (grp - 1)) { /* more than one lane: wave-reduce the group */
      sum = mine ? v : 0;
      for (int ofs = 32; ofs > 0; ofs >>= 1)
        sum = fold::add_wrap(
            sum, (uint64_t)__shfl_xor((unsigned long long)sum, ofs, 64));
    }
    if (lane == leader) atomicAdd(&acc[lq], (unsigned long long)sum);
    if (mine) active = false;
  }
}

__global__ void k_mg_emit(const uint8_t *__restrict__ store,
                          const RunView *__restrict__ runs,
                          const unsigned long long *__restrict__ term_pack,
                          const unsigned long long *__restrict__ merge_seq,
                          const unsigned long long *__restrict__ rd_seq,
                          const unsigned long long *__restrict__ winner_ref,
                          uint32_t nq, uint8_t *__restrict__ valbuf,
                          uint32_t val_stride, GraGetResult *__restrict__ out,
                          MgExtra *__restrict__ extra,
                          const unsigned long long *__restrict__ acc) {
  uint32_t q = blockIdx.x;
  if (q >= nq) return;
  uint64_t tp = term_pack[q];
  uint64_t T = tp >> 8, M = merge_seq[q], RD = rd_seq[q];
  uint8_t ttype = tp ? (uint8_t)tp : 0xFF;
  if (threadIdx.x == 0 && extra) {
    extra[q].term_seq = T;
    extra[q].merge_seq = M;
    extra[q].rd_seq = RD;
    extra[q].term_type = ttype;
  }
  uint64_t fl = T > RD ? T : RD;
  if (M > fl && acc) { /* fold_on_device, u64add: base + k_mg_fold's sum */
    if (threadIdx.x == 0) {
      uint64_t v = acc[q];
      if (T > RD && ttype == wb::kValue) {
        unsigned long long ref = winner_ref[q];
        RunView rv = runs[ref >> 32];
        wb::RecHdr h = ((const wb::RecHdr *)(store + rv.hdr_off))[(uint32_t)ref];
        v = fold::add_wrap(
            v, fold::load_u64le(store + rv.payload_off +
                                    (h.kv_off - rv.pay_rel_base) + h.key_len,
                                h.val_len));
      }
      fold::store_u64le(valbuf + (size_t)q * val_stride, v, val_stride);
      out[q].status = GRA_GET_FOUND;
      out[q].vlen = 8; /* true length (caller sees truncation) */
    }
    return;
  }
  if (M > fl) {
    if (threadIdx.x == 0) {
      out[q].status = GRA_GET_NEEDS_HOST;
      out[q].vlen = 0;
    }
    return;
  }
  if (T == 0 || T <= RD || ttype != wb::kValue) {
    if (threadIdx.x == 0) {
      out[q].status = GRA_GET_MISS;
      out[q].vlen = 0;
    }
    return;
  }
  unsigned long long ref = winner_ref[q];
  RunView rv = runs[ref >> 32];
  const wb::RecHdr *hdrs = (const wb::RecHdr *)(store + rv.hdr_off);
  wb::RecHdr h = hdrs[(uint32_t)ref];
  uint32_t vlen = h.val_len < val_stride ? h.val_len : val_stride;
  const uint8_t *src =
      store + rv.payload_off + (h.kv_off - rv.pay_rel_base) + h.key_len;
  uint8_t *dst = valbuf + (size_t)q * val_stride;
  for (uint32_t b = threadIdx.x; b < vlen; b += blockDim.x) dst[b] = src[b];
  if (threadIdx.x == 0) {
    out[q].status = GRA_GET_FOUND;
    out[q].vlen = h.val_len;
  }
}
