/* scan_kernels.h — device side of gra_scan: ordered range scans served from
 * the device run store (≅ ApplicationDB::NewIterator, rocksdb_admin/
 * application_db.h:55). Included by engine.hip inside namespace gra, after
 * RunView, dev_memcmp and copy_dword.
 *
 * Runs are sorted by seq, not by key, so a scan is collect → sort → resolve:
 *
 *   k_sc_collect      one coalesced pass over every run's headers; in-range
 *                     point entries are appended to a candidate list, range
 *                     tombstones meeting [lo, hi) to a tombstone list
 *   k_sc_sort_tile /  bitonic sort of the candidates by (key asc, seq desc);
 *   k_sc_sort_global  1024-record tiles in LDS, wider strides in global memory
 *   k_sc_resolve      a key's first candidate is its newest entry: it alone
 *                     and the covering tombstones decide the key (fused with
 *                     the in-block half of the prefix sum, like k_decode)
 *   k_sc_scan2        block partials + carry (like k_scan2)
 *   k_sc_emit         one lane group per emitted entry copies key and value
 *                     into the output buffer
 *
 * Every kernel sizes itself from the device-side candidate count, so the
 * host enqueues the whole chain without a sync in between. Work per call is
 * O(entries in the shard), whatever the range. */
#pragma once

constexpr uint32_t kScTile = 1024;     /* records per LDS tile: 32 KB */
constexpr uint32_t kScTileThreads = kScTile / 2;
constexpr uint32_t kScFirstCap = 16384; /* first-use candidate capacity */
constexpr uint32_t kScTombCap = 4096;
constexpr uint64_t kScInfOff = ~0ULL;   /* koff of a +infinity pad record */
constexpr uint32_t kScMaxBound = 65536; /* stored keys are < 64 KiB (u16
                                           key_len): a longer bound compares
                                           the same once cut to this */

/* One in-range point entry. The key is referenced by its absolute store
 * offset rather than (run, entry): the sort's comparator reaches the key
 * bytes on every prefix tie, and two dependent loads (run view, header) in
 * front of each would dominate it for key families sharing 8 bytes. */
struct ScCand {
  uint64_t pref; /* first 8 key bytes, big-endian, zero-padded: integer
                    order == bytewise order whenever two prefixes differ */
  uint64_t seq;
  uint64_t koff; /* key bytes at store + koff (16-B aligned), value after */
  uint32_t vlen;
  uint16_t klen;
  uint8_t type;
  uint8_t _pad;
};
static_assert(sizeof(ScCand) == 32, "ScCand must be 32 bytes");

struct ScTomb {
  uint64_t seq;
  uint64_t boff; /* begin key at store + boff, end key right after it */
  uint32_t bl, el;
};

struct ScSum {
  uint64_t bytes;
  uint32_t cnt, _pad;
};
__host__ __device__ inline ScSum sc_add(ScSum a, ScSum b) {
  return {a.bytes + b.bytes, a.cnt + b.cnt, 0};
}

/* per sorted candidate: exclusive-in-block prefix + own contribution */
struct ScItem {
  uint64_t excl_bytes;
  uint32_t excl_cnt; /* bit 31: this candidate is a live key head */
  uint32_t cost;     /* output bytes: klen (+ vlen when FOUND) */
};

/* counters + result header, one D2H at the end of the chain */
struct ScCtl {
  uint32_t ncand, ntomb; /* keep counting past the caps */
  uint32_t n, more, too_small, _pad;
  uint64_t buf_used;
};

struct ScBounds {
  const uint8_t *lo, *hi; /* device copies, 16-B aligned, zero-padded */
  uint64_t lo_pref, hi_pref;
  uint32_t lo_len, hi_len;
  uint32_t has_hi, _pad;
};

/* bytewise order, byte loop (unaligned operands: tombstone end keys) */
__device__ inline int sc_cmp_bytes(const uint8_t *a, uint32_t al,
                                   const uint8_t *b, uint32_t bl) {
  int c = dev_memcmp(a, b, al < bl ? al : bl);
  if (c != 0) return c;
  return al < bl ? -1 : (al > bl ? 1 : 0);
}

/* Bytewise order of two keys whose first `from` bytes are known equal
 * (from % 8 == 0), 8 bytes per step. Both pointers are 8-B aligned with at
 * least 7 readable bytes behind the key: stored keys start a 16-B aligned
 * record that is padded to 16 B, bounds are staged zero-padded. */
__device__ inline int sc_key_cmp_from(const uint8_t *a, uint32_t al,
                                      const uint8_t *b, uint32_t bl,
                                      uint32_t from) {
  uint32_t n = al < bl ? al : bl;
  for (uint32_t o = from; o < n; o += 8) {
    uint64_t x = __builtin_bswap64(*(const uint64_t *)(a + o));
    uint64_t y = __builtin_bswap64(*(const uint64_t *)(b + o));
    uint32_t rem = n - o;
    if (rem < 8) {
      uint64_t m = ~0ULL << (8 * (8 - rem));
      x &= m;
      y &= m;
    }
    if (x != y) return x < y ? -1 : 1;
  }
  return al < bl ? -1 : (al > bl ? 1 : 0);
}

/* (key asc, seq desc), pad records last. Total: seqs are unique per shard. */
__device__ inline bool sc_less(const uint8_t *store, const ScCand &a,
                               const ScCand &b) {
  if (a.koff == kScInfOff) return false;
  if (b.koff == kScInfOff) return true;
  if (a.pref != b.pref) return a.pref < b.pref;
  int c = sc_key_cmp_from(store + a.koff, a.klen, store + b.koff, b.klen, 8);
  if (c != 0) return c < 0;
  return a.seq > b.seq;
}

/* candidate count the sort works on, and its padded power-of-two size */
__device__ inline uint32_t sc_count(const ScCtl *ctl, uint32_t cap) {
  uint32_t n = ctl->ncand;
  return n < cap ? n : cap;
}
__device__ inline uint32_t sc_padded(uint32_t n) {
  uint32_t N = kScTile;
  while (N < n) N <<= 1;
  return N; /* <= cap: cap is a power of two >= kScTile */
}

__global__ void __launch_bounds__(256) k_sc_collect(
    const uint8_t *__restrict__ store, const RunView *__restrict__ runs,
    ScBounds bd, ScCand *__restrict__ cands, uint32_t cand_cap,
    ScTomb *__restrict__ tombs, uint32_t tomb_cap, ScCtl *__restrict__ ctl) {
  RunView rv = runs[blockIdx.y];
  const wb::RecHdr *hdrs = (const wb::RecHdr *)(store + rv.hdr_off);
  uint32_t lane = threadIdx.x & 63;
  /* block-uniform trip count: every lane reaches the ballot below */
  for (uint32_t base = blockIdx.x * blockDim.x; base < rv.n_entries;
       base += gridDim.x * blockDim.x) {
    uint32_t i = base + threadIdx.x;
    bool take = false;
    ScCand c = {};
    if (i < rv.n_entries) {
      wb::RecHdr h = hdrs[i];
      uint64_t koff = rv.payload_off + (h.kv_off - rv.pay_rel_base);
      const uint8_t *k = store + koff;
      if (h.type == wb::kRangeDeletion) {
        /* [begin, end) meets [lo, hi): end > lo and begin < hi */
        if (sc_cmp_bytes(k + h.key_len, h.val_len, bd.lo, bd.lo_len) > 0 &&
            (!bd.has_hi ||
             sc_cmp_bytes(k, h.key_len, bd.hi, bd.hi_len) < 0)) {
          uint32_t slot = atomicAdd(&ctl->ntomb, 1u);
          if (slot < tomb_cap) tombs[slot] = {h.seq, koff, h.key_len, h.val_len};
        }
      } else {
        /* records are 16-B aligned: one aligned load yields the key's
         * first 8 bytes, which decide most entries against both bounds */
        uint2 w = *(const uint2 *)k;
        uint64_t pref =
            __builtin_bswap64((uint64_t)w.x | ((uint64_t)w.y << 32));
        pref = h.key_len >= 8 ? pref
               : h.key_len == 0
                   ? 0
                   : pref & (~0ULL << (8 * (8 - h.key_len)));
        bool ge_lo =
            pref > bd.lo_pref ||
            (pref == bd.lo_pref &&
             sc_key_cmp_from(k, h.key_len, bd.lo, bd.lo_len, 8) >= 0);
        bool lt_hi =
            !bd.has_hi || pref < bd.hi_pref ||
            (pref == bd.hi_pref &&
             sc_key_cmp_from(k, h.key_len, bd.hi, bd.hi_len, 8) < 0);
        take = ge_lo && lt_hi;
        c.pref = pref;
        c.seq = h.seq;
        c.koff = koff;
        c.vlen = h.val_len;
        c.klen = h.key_len;
        c.type = h.type;
      }
    }
    /* one atomic per wave, not per candidate */
    unsigned long long m = __ballot(take);
    if (m) {
      uint32_t leader = (uint32_t)__ffsll((long long)m) - 1;
      uint32_t first = 0;
      if (lane == leader) first = atomicAdd(&ctl->ncand, (uint32_t)__popcll(m));
      first = __shfl(first, leader, 64);
      if (take) {
        uint32_t slot = first + (uint32_t)__popcll(m & ((1ULL << lane) - 1));
        if (slot < cand_cap) cands[slot] = c;
      }
    }
  }
}

/* Bitonic stages k_first..k_last restricted to strides < kScTile, on one
 * tile in LDS. first_pass: k runs 2..kScTile and slots past the candidate
 * count load as +infinity pads; later calls merge one stage k > kScTile
 * after its global strides. */
__global__ void __launch_bounds__(kScTileThreads) k_sc_sort_tile(
    const uint8_t *__restrict__ store, ScCand *__restrict__ cands,
    const ScCtl *__restrict__ ctl, uint32_t cap, uint32_t k_first,
    uint32_t k_last, int first_pass) {
  __shared__ ScCand sh[kScTile];
  uint32_t n = sc_count(ctl, cap), N = sc_padded(n);
  uint32_t tile = blockIdx.x * kScTile;
  if (tile >= N || k_first > N) return; /* block-uniform */
  for (uint32_t t = threadIdx.x; t < kScTile; t += kScTileThreads) {
    uint32_t gi = tile + t;
    if (first_pass && gi >= n) {
      ScCand pad = {};
      pad.koff = kScInfOff;
      sh[t] = pad;
    } else {
      sh[t] = cands[gi];
    }
  }
  __syncthreads();
  uint32_t t = threadIdx.x;
  for (uint32_t k = k_first; k <= k_last && k <= N; k <<= 1) {
    uint32_t j = k >> 1;
    if (j > kScTile / 2) j = kScTile / 2;
    for (; j > 0; j >>= 1) {
      uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
      bool asc = ((tile + i) & k) == 0;
      ScCand a = sh[i], b = sh[l];
      if (asc ? sc_less(store, b, a) : sc_less(store, a, b)) {
        sh[i] = b;
        sh[l] = a;
      }
      __syncthreads();
    }
  }
  for (uint32_t u = threadIdx.x; u < kScTile; u += kScTileThreads)
    cands[tile + u] = sh[u];
}

/* one compare-exchange stride j >= kScTile of stage k, in global memory */
__global__ void __launch_bounds__(256) k_sc_sort_global(
    const uint8_t *__restrict__ store, ScCand *__restrict__ cands,
    const ScCtl *__restrict__ ctl, uint32_t cap, uint32_t j, uint32_t k) {
  uint32_t N = sc_padded(sc_count(ctl, cap));
  if (k > N) return;
  uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= N / 2) return;
  uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
  bool asc = (i & k) == 0;
  ScCand a = cands[i], b = cands[l];
  if (asc ? sc_less(store, b, a) : sc_less(store, a, b)) {
    cands[i] = b;
    cands[l] = a;
  }
}

/* One thread per sorted candidate. A candidate whose key differs from its
 * predecessor's is the key's newest entry; with RD = max seq of the range
 * tombstones covering the key:
 *   Put: live iff seq > RD; Delete/SingleDelete: dead;
 *   Merge: seq > RD live (host fold), else dead — every older entry has a
 *   smaller seq and is covered too.
 * seq > RD only asks whether ANY covering tombstone is newer, so tombstones
 * older than the head are skipped without touching their keys. */
__global__ void __launch_bounds__(256) k_sc_resolve(
    const uint8_t *__restrict__ store, const ScCand *__restrict__ cands,
    const ScTomb *__restrict__ tombs, const ScCtl *__restrict__ ctl,
    uint32_t cap, uint32_t tomb_cap, ScItem *__restrict__ items,
    ScSum *__restrict__ bsums) {
  __shared__ ScSum sh[256];
  uint32_t n = sc_count(ctl, cap);
  uint32_t ntomb = ctl->ntomb < tomb_cap ? ctl->ntomb : tomb_cap;
  uint32_t i = blockIdx.x * 256 + threadIdx.x;
  ScSum v = {0, 0, 0};
  if (i < n) {
    ScCand c = cands[i];
    bool head = i == 0;
    if (!head) {
      ScCand p = cands[i - 1];
      head = p.pref != c.pref || p.klen != c.klen ||
             sc_key_cmp_from(store + p.koff, p.klen, store + c.koff, c.klen,
                             8) != 0;
    }
    if (head && (c.type == wb::kValue || c.type == wb::kMerge)) {
      const uint8_t *key = store + c.koff;
      bool live = true;
      for (uint32_t t = 0; t < ntomb && live; t++) {
        ScTomb tb = tombs[t];
        if (tb.seq < c.seq) continue;
        const uint8_t *b = store + tb.boff;
        if (sc_cmp_bytes(b, tb.bl, key, c.klen) <= 0 &&
            sc_cmp_bytes(key, c.klen, b + tb.bl, tb.el) < 0)
          live = false;
      }
      if (live) {
        v.cnt = 1;
        v.bytes = (uint64_t)c.klen + (c.type == wb::kValue ? c.vlen : 0u);
      }
    }
  }
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int ofs = 1; ofs < 256; ofs <<= 1) {
    ScSum a = sh[threadIdx.x];
    ScSum b = threadIdx.x >= (uint32_t)ofs ? sh[threadIdx.x - ofs]
                                           : ScSum{0, 0, 0};
    __syncthreads();
    sh[threadIdx.x] = sc_add(a, b);
    __syncthreads();
  }
  if (i < n) {
    ScSum inc = sh[threadIdx.x];
    items[i] = {inc.bytes - v.bytes, (inc.cnt - v.cnt) | (v.cnt << 31),
                (uint32_t)v.bytes};
  }
  if (threadIdx.x == 255) bsums[blockIdx.x] = sh[255];
}

/* single block: block sums -> exclusive in place, with a carry across
 * 256-wide chunks; then the result header for "everything fit" (k_sc_emit
 * overwrites it at the cut, if there is one) */
__global__ void __launch_bounds__(256) k_sc_scan2(ScSum *__restrict__ bsums,
                                                  uint32_t nblocks,
                                                  ScCtl *__restrict__ ctl) {
  __shared__ ScSum sh[256];
  __shared__ ScSum carry;
  if (threadIdx.x == 0) carry = {0, 0, 0};
  __syncthreads();
  for (uint32_t base = 0; base < nblocks; base += 256) {
    uint32_t i = base + threadIdx.x;
    ScSum v = i < nblocks ? bsums[i] : ScSum{0, 0, 0};
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int ofs = 1; ofs < 256; ofs <<= 1) {
      ScSum a = sh[threadIdx.x];
      ScSum b = threadIdx.x >= (uint32_t)ofs ? sh[threadIdx.x - ofs]
                                             : ScSum{0, 0, 0};
      __syncthreads();
      sh[threadIdx.x] = sc_add(a, b);
      __syncthreads();
    }
    ScSum inc = sc_add(sh[threadIdx.x], carry);
    if (i < nblocks) bsums[i] = {inc.bytes - v.bytes, inc.cnt - v.cnt, 0};
    __syncthreads();
    if (threadIdx.x == 255) carry = inc;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    ctl->n = carry.cnt;
    ctl->buf_used = carry.bytes;
    ctl->more = 0;
    ctl->too_small = 0;
  }
}

/* G lanes per sorted candidate; live heads inside the cut copy their key
 * (and value) to out + byte offset and write entry[rank]. Emitted heads form
 * a prefix (rank and bytes are monotone), so exactly one live head — the
 * first that does not fit — sees its predecessor inside the cut and records
 * where the page ended. */
template <int G>
__global__ void __launch_bounds__(256) k_sc_emit(
    const uint8_t *__restrict__ store, const ScCand *__restrict__ cands,
    const ScItem *__restrict__ items, const ScSum *__restrict__ bsums,
    ScCtl *__restrict__ ctl, uint32_t cap, uint32_t max_entries,
    uint64_t byte_cap, uint8_t *__restrict__ out,
    GraScanEntry *__restrict__ ents) {
  uint32_t g = (blockIdx.x * blockDim.x + threadIdx.x) / G;
  uint32_t lane = threadIdx.x & (G - 1);
  if (g >= sc_count(ctl, cap)) return;
  ScItem it = items[g];
  if (!(it.excl_cnt >> 31)) return;
  ScSum bs = bsums[g >> 8];
  uint32_t rank = (it.excl_cnt & 0x7FFFFFFFu) + bs.cnt;
  uint64_t off = it.excl_bytes + bs.bytes;
  if (rank >= max_entries || off + it.cost > byte_cap) {
    if (lane == 0 && rank <= max_entries && off <= byte_cap) {
      ctl->n = rank;
      ctl->buf_used = off;
      ctl->more = 1;
      ctl->too_small = (rank == 0 && max_entries > 0) ? 1u : 0u;
    }
    return;
  }
  ScCand c = cands[g];
  const uint8_t *src = store + c.koff;
  bool found = c.type == wb::kValue;
  copy_dword<G>(out + off, src, c.klen, lane);
  if (found) copy_dword<G>(out + off + c.klen, src + c.klen, c.vlen, lane);
  if (lane == 0) {
    GraScanEntry e;
    e.key_off = (uint32_t)off;
    e.key_len = c.klen;
    e.val_off = found ? (uint32_t)off + c.klen : 0u;
    e.val_len = found ? c.vlen : 0u;
    e.status = found ? GRA_GET_FOUND : GRA_GET_NEEDS_HOST;
    e._pad = 0;
    ents[rank] = e;
  }
}
