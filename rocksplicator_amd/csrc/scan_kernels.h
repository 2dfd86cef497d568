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
 *   k_sc_heads /      fold_on_device only: list the live Merge heads with
 *   k_sc_fold         their RD, then fold each head's operand chain, one
 *                     wave per head, 64 successors a step
 *   k_sc_resolve      a key's first candidate is its newest entry: it alone
 *                     and the covering tombstones decide the key (fused with
 *                     the in-block half of the prefix sum, like k_decode)
 *   k_sc_scan2        block partials + carry (like k_scan2)
 *   k_sc_emit         one lane group per emitted entry copies key and value
 *                     into the output buffer
 *
 * Every kernel sizes itself from the device-side candidate count, so the
 * host enqueues the whole chain without a sync in between. Work per call is
 * O(entries in the shard), whatever the range — except for a shard's sorted
 * run (gra_compact, compact_kernels.h): k_sc_collect enters it by binary
 * search and reads only the slice [lo, hi). */
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
  uint32_t n, more, too_small;
  uint32_t nheads; /* fold_on_device: live Merge heads listed by k_sc_heads */
  uint64_t buf_used;
};

/* fold_on_device: a live Merge head waiting for its fold, and the verdict.
 * Both arrays are indexed like the sorted candidates / the head list and
 * hold at most one record per candidate. */
struct ScHead {
  uint64_t rd;  /* max seq of the range tombstones covering the key */
  uint32_t idx; /* the head's position in the sorted candidates */
  uint32_t _pad;
};
struct ScFold {
  uint64_t sum;   /* u64add: the folded counter */
  uint32_t vlen;  /* folded value length */
  uint32_t flags; /* kScFold* | operand count << 8 */
};
constexpr uint32_t kScFoldLive = 1;   /* head.seq > RD */
constexpr uint32_t kScFoldFolded = 2; /* value computable here: FOUND */
constexpr uint32_t kScFoldBase = 4;   /* a Put base ends the chain */
constexpr uint32_t kScFoldWaves = 1024; /* waves the fold kernel is launched
                                           with; heads are strided over them */

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

/* first 8 key bytes as ScCand::pref; records are 16-B aligned, so one
 * aligned load yields them */
__device__ inline uint64_t sc_key_pref(const uint8_t *k, uint32_t klen) {
  uint2 w = *(const uint2 *)k;
  uint64_t pref = __builtin_bswap64((uint64_t)w.x | ((uint64_t)w.y << 32));
  return klen >= 8 ? pref
         : klen == 0 ? 0
                     : pref & (~0ULL << (8 * (8 - klen)));
}

/* Sorted run (gra_compact: point records only, strictly ascending keys):
 * index of its first key >= bound, with the collect pass's comparator,
 * searched by one whole wave. Every step the 64 lanes probe 64 evenly spaced
 * entries of [lo, hi) and a ballot keeps the one gap the answer lies in, so
 * the range shrinks 64-fold for two dependent loads (header, then key):
 * three steps for 100K entries where a binary search takes seventeen. All
 * 64 lanes must call it; the result is wave-uniform. */
__device__ inline uint32_t sc_lower_bound(const uint8_t *store,
                                          const RunView &rv,
                                          const uint8_t *b, uint32_t bl,
                                          uint64_t bpref, uint32_t lane) {
  const wb::RecHdr *hdrs = (const wb::RecHdr *)(store + rv.hdr_off);
  uint32_t lo = 0, hi = rv.n_entries;
  while (lo < hi) { /* wave-uniform */
    uint32_t step = (hi - lo + 63) / 64;
    uint64_t p = (uint64_t)lo + (uint64_t)lane * step;
    bool less = false;
    if (p < hi) {
      wb::RecHdr h = hdrs[p];
      const uint8_t *k = store + rv.payload_off + (h.kv_off - rv.pay_rel_base);
      uint64_t pref = sc_key_pref(k, h.key_len);
      less = pref < bpref ||
             (pref == bpref && sc_key_cmp_from(k, h.key_len, b, bl, 8) < 0);
    }
    /* keys ascend, so the lanes that see a smaller key are the leading ones */
    uint32_t c = (uint32_t)__popcll(__ballot(less));
    if (c == 0) return lo;
    /* probe c-1 is below the bound, probe c (if there is one) is not */
    uint64_t next_hi = (uint64_t)lo + (uint64_t)c * step;
    lo = lo + (c - 1) * step + 1;
    if (next_hi < hi) hi = (uint32_t)next_hi;
  }
  return lo;
}

/* sorted0: row 0 of `runs` is the shard's sorted run. Its in-range entries
 * are the slice between the lower bounds of lo and hi, and it holds no
 * tombstones, so the block strides over that slice only. */
__global__ void __launch_bounds__(256) k_sc_collect(
    const uint8_t *__restrict__ store, const RunView *__restrict__ runs,
    ScBounds bd, ScCand *__restrict__ cands, uint32_t cand_cap,
    ScTomb *__restrict__ tombs, uint32_t tomb_cap, ScCtl *__restrict__ ctl,
    uint32_t sorted0) {
  __shared__ uint32_t slice[2];
  RunView rv = runs[blockIdx.y];
  const wb::RecHdr *hdrs = (const wb::RecHdr *)(store + rv.hdr_off);
  uint32_t lane = threadIdx.x & 63;
  uint32_t begin = 0, end = rv.n_entries;
  if (sorted0 && blockIdx.y == 0) { /* block-uniform */
    uint32_t wave = threadIdx.x >> 6; /* wave 0 finds lo, wave 1 finds hi */
    if (wave == 0) {
      uint32_t b = bd.lo_len ? sc_lower_bound(store, rv, bd.lo, bd.lo_len,
                                              bd.lo_pref, lane)
                             : 0u;
      if (lane == 0) slice[0] = b;
    } else if (wave == 1) {
      uint32_t e = bd.has_hi ? sc_lower_bound(store, rv, bd.hi, bd.hi_len,
                                              bd.hi_pref, lane)
                             : rv.n_entries;
      if (lane == 0) slice[1] = e;
    }
    __syncthreads();
    begin = slice[0];
    end = slice[1];
  }
  /* block-uniform trip count: every lane reaches the ballot below */
  for (uint32_t base = begin + blockIdx.x * blockDim.x; base < end;
       base += gridDim.x * blockDim.x) {
    uint32_t i = base + threadIdx.x;
    bool take = false;
    ScCand c = {};
    if (i < end) {
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
        /* the key's first 8 bytes decide most entries against both bounds */
        uint64_t pref = sc_key_pref(k, h.key_len);
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

__device__ inline bool sc_same_key(const uint8_t *store, const ScCand &a,
                                   const ScCand &b) {
  return a.pref == b.pref && a.klen == b.klen &&
         sc_key_cmp_from(store + a.koff, a.klen, store + b.koff, b.klen, 8) ==
             0;
}

/* Is the key's newest entry covered by a range tombstone at least as new as
 * it is? Tombstones older than the head are skipped without touching their
 * keys. */
__device__ inline bool sc_tomb_kills(const uint8_t *store,
                                     const ScTomb *__restrict__ tombs,
                                     uint32_t ntomb, const ScCand &c) {
  const uint8_t *key = store + c.koff;
  for (uint32_t t = 0; t < ntomb; t++) {
    ScTomb tb = tombs[t];
    if (tb.seq < c.seq) continue;
    const uint8_t *b = store + tb.boff;
    if (sc_cmp_bytes(b, tb.bl, key, c.klen) <= 0 &&
        sc_cmp_bytes(key, c.klen, b + tb.bl, tb.el) < 0)
      return true;
  }
  return false;
}

/* inclusive scan of one ScSum per thread over a block of 256 */
__device__ inline ScSum sc_block_scan(ScSum v, ScSum *sh) {
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
  return sh[threadIdx.x];
}

/* ---- fold_on_device: fold merge chains before the prefix sum ----
 * Two passes in front of k_sc_resolve, launched only when the engine option
 * is set, so the default chain is the one above, kernel for kernel.
 *
 * k_sc_heads: one thread per sorted candidate. A Merge that leads its key
 * computes RD = max seq over ALL covering tombstones (an older tombstone
 * does not kill the head but cuts its chain) and, when live, is appended to
 * the head list — one atomic per wave, as k_sc_collect does. */
__global__ void __launch_bounds__(256) k_sc_heads(
    const uint8_t *__restrict__ store, const ScCand *__restrict__ cands,
    const ScTomb *__restrict__ tombs, ScCtl *ctl, uint32_t cap,
    uint32_t tomb_cap, ScHead *__restrict__ heads,
    ScFold *__restrict__ folds) {
  uint32_t n = sc_count(ctl, cap);
  uint32_t ntomb = ctl->ntomb < tomb_cap ? ctl->ntomb : tomb_cap;
  uint32_t i = blockIdx.x * 256 + threadIdx.x;
  uint32_t lane = threadIdx.x & 63;
  bool take = false;
  uint64_t rd = 0;
  if (i < n) {
    ScCand c = cands[i];
    if (c.type == wb::kMerge &&
        (i == 0 || !sc_same_key(store, cands[i - 1], c))) {
      const uint8_t *key = store + c.koff;
      for (uint32_t t = 0; t < ntomb; t++) {
        ScTomb tb = tombs[t];
        if (tb.seq <= rd) continue;
        const uint8_t *b = store + tb.boff;
        if (sc_cmp_bytes(b, tb.bl, key, c.klen) <= 0 &&
            sc_cmp_bytes(key, c.klen, b + tb.bl, tb.el) < 0)
          rd = tb.seq;
      }
      take = c.seq > rd;
      if (!take) folds[i] = {0, 0, 0}; /* dead: every older entry is too */
    }
  }
  /* every lane of the wave reaches the ballot */
  unsigned long long m = __ballot(take);
  if (m) {
    uint32_t leader = (uint32_t)__ffsll((long long)m) - 1;
    uint32_t first = 0;
    if (lane == leader) first = atomicAdd(&ctl->nheads, (uint32_t)__popcll(m));
    first = __shfl(first, leader, 64);
    if (take) {
      uint32_t slot = first + (uint32_t)__popcll(m & ((1ULL << lane) - 1));
      if (slot < cap) heads[slot] = {rd, i, 0};
    }
  }
}

__device__ inline uint64_t sc_wave_sum(uint64_t v) {
  for (int ofs = 32; ofs > 0; ofs >>= 1)
    v += (uint64_t)__shfl_xor((unsigned long long)v, ofs, 64);
  return v;
}

/* k_sc_fold: one wave per listed head (heads strided over the launched
 * waves; the count is read on the device). The head's versions follow it in
 * (seq desc) order, so the wave takes 64 successors a step, ballots for the
 * first that is not an operand — another key, a non-Merge, or seq <= RD —
 * and wave-reduces the operand sum (MODE 2, u64add) or the operand lengths
 * and count (MODE 1, concat). The entry that ends the chain is the base iff
 * it is a Put of the same key above RD. A hot counter's chain costs
 * chain/64 steps of one wave rather than chain steps of one lane; after the
 * first 64 (most chains end there) a turn takes 4 x 64 successors with their
 * candidate, key and value loads all in flight before the first ballot, so
 * the three dependent loads are paid once per 256 operands. */
struct ScFoldAcc {
  uint64_t acc; /* u64add: operand sum; concat: value bytes */
  uint32_t cnt, base;
  bool over; /* concat: no chain end within kFoldMaxConcatOps */
};

/* U x 64 successors from pos; true when the chain ended (wave-uniform) */
template <int MODE, int U, bool UNBOUNDED>
__device__ __forceinline__ bool sc_fold_step(
    const uint8_t *__restrict__ store, const ScCand *__restrict__ cands,
    uint32_t n, const ScCand &hc, const ScHead &hd, uint32_t pos,
    uint32_t lane, ScFoldAcc &a) {
  bool op[U], isbase[U];
  uint64_t val[U];
#pragma unroll
  for (int u = 0; u < U; u++) {
    uint32_t j = pos + u * 64 + lane;
    op[u] = isbase[u] = false;
    val[u] = 0;
    if (j < n) {
      ScCand c = cands[j];
      bool mine = c.seq > hd.rd && sc_same_key(store, hc, c);
      op[u] = mine && c.type == wb::kMerge;
      isbase[u] = mine && c.type == wb::kValue;
      if (op[u] || isbase[u]) /* loaded ahead of the ballots */
        val[u] = MODE == 2
                     ? fold::load_u64le(store + c.koff + c.klen, c.vlen)
                     : (uint64_t)c.vlen;
    }
  }
#pragma unroll
  for (int u = 0; u < U; u++) {
    unsigned long long stop = __ballot(!op[u]);
    uint32_t first = stop ? (uint32_t)__ffsll((long long)stop) - 1 : 64u;
    if (lane < first) {
      a.acc = fold::add_wrap(a.acc, val[u]);
      a.cnt++;
    } else if (lane == first && isbase[u]) {
      a.acc = fold::add_wrap(a.acc, val[u]);
      a.base = 1;
    }
    if (stop) return true;
    if (MODE == 1 && !UNBOUNDED &&
        pos - hd.idx + (u + 1) * 64 > fold::kFoldMaxConcatOps) {
      a.over = true;
      return true;
    }
  }
  return false;
}

/* UNBOUNDED (gra_compact, MODE 1): a concat chain of any length folds; its
 * operand count goes to ScFold::sum, which concat leaves free, instead of
 * the 24 flag bits. */
template <int MODE, bool UNBOUNDED = false>
__global__ void __launch_bounds__(256) k_sc_fold(
    const uint8_t *__restrict__ store, const ScCand *__restrict__ cands,
    const ScHead *__restrict__ heads, const ScCtl *__restrict__ ctl,
    uint32_t cap, ScFold *__restrict__ folds) {
  uint32_t n = sc_count(ctl, cap);
  uint32_t nheads = ctl->nheads < cap ? ctl->nheads : cap;
  uint32_t lane = threadIdx.x & 63;
  uint32_t wave = (blockIdx.x * 256 + threadIdx.x) >> 6;
  uint32_t nwaves = gridDim.x * 4;
  for (uint32_t h = wave; h < nheads; h += nwaves) { /* wave-uniform */
    ScHead hd = heads[h];
    ScCand hc = cands[hd.idx];
    ScFoldAcc a = {0, 0, 0, false};
    bool done = sc_fold_step<MODE, 1, UNBOUNDED>(store, cands, n, hc, hd,
                                                 hd.idx, lane, a);
    for (uint32_t pos = hd.idx + 64; !done; pos += 256)
      done = sc_fold_step<MODE, 4, UNBOUNDED>(store, cands, n, hc, hd, pos,
                                              lane, a);
    bool over = a.over;
    uint64_t acc = sc_wave_sum(a.acc);
    uint32_t nops = (uint32_t)sc_wave_sum(a.cnt);
    uint32_t has_base = (uint32_t)sc_wave_sum(a.base);
    if (lane == 0) {
      ScFold f = {0, 0, kScFoldLive};
      if (MODE == 2) {
        f.sum = acc;
        f.vlen = 8;
        f.flags |= kScFoldFolded;
      } else if (UNBOUNDED || (!over && nops <= fold::kFoldMaxConcatOps)) {
        /* acc already holds the base's bytes along with the operands' */
        uint64_t len = fold::concat_len(has_base != 0, 0, acc, nops);
        if (len + hc.klen < 0xFFFF0000ull) { /* ScItem.cost is 32 bits */
          f.vlen = (uint32_t)len;
          f.flags |= kScFoldFolded | (has_base ? kScFoldBase : 0) |
                     (UNBOUNDED ? 0u : nops << 8);
          if (UNBOUNDED) f.sum = nops;
        }
      }
      folds[hd.idx] = f;
    }
  }
}

/* One thread per sorted candidate. A candidate whose key differs from its
 * predecessor's is the key's newest entry; with RD = max seq of the range
 * tombstones covering the key:
 *   Put: live iff seq > RD; Delete/SingleDelete: dead;
 *   Merge: seq > RD live (host fold), else dead — every older entry has a
 *   smaller seq and is covered too.
 * seq > RD only asks whether ANY covering tombstone is newer, so tombstones
 * older than the head are skipped without touching their keys.
 * FOLD (fold_on_device): a Merge head takes k_sc_fold's verdict instead —
 * its folded size feeds the prefix sum, so pagination runs on it. */
template <bool FOLD>
__global__ void __launch_bounds__(256) k_sc_resolve(
    const uint8_t *__restrict__ store, const ScCand *__restrict__ cands,
    const ScTomb *__restrict__ tombs, const ScCtl *__restrict__ ctl,
    uint32_t cap, uint32_t tomb_cap, ScItem *__restrict__ items,
    ScSum *__restrict__ bsums, const ScFold *__restrict__ folds) {
  __shared__ ScSum sh[256];
  uint32_t n = sc_count(ctl, cap);
  uint32_t ntomb = ctl->ntomb < tomb_cap ? ctl->ntomb : tomb_cap;
  uint32_t i = blockIdx.x * 256 + threadIdx.x;
  ScSum v = {0, 0, 0};
  if (i < n) {
    ScCand c = cands[i];
    bool head = i == 0 || !sc_same_key(store, cands[i - 1], c);
    if (FOLD && head && c.type == wb::kMerge) {
      ScFold f = folds[i];
      if (f.flags & kScFoldLive) {
        v.cnt = 1;
        v.bytes = (uint64_t)c.klen + ((f.flags & kScFoldFolded) ? f.vlen : 0u);
      }
    } else if (head && (c.type == wb::kValue || c.type == wb::kMerge)) {
      if (!sc_tomb_kills(store, tombs, ntomb, c)) {
        v.cnt = 1;
        v.bytes = (uint64_t)c.klen + (c.type == wb::kValue ? c.vlen : 0u);
      }
    }
  }
  ScSum inc = sc_block_scan(v, sh);
  if (i < n)
    items[i] = {inc.bytes - v.bytes, (inc.cnt - v.cnt) | (v.cnt << 31),
                (uint32_t)v.bytes};
  if (threadIdx.x == 255) bsums[blockIdx.x] = inc;
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
    ScSum inc = sc_add(sc_block_scan(v, sh), carry);
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
 * where the page ended.
 * FOLD: 0 = off; 1 = concat, 2 = u64add (fold_on_device). A folded Merge
 * head writes its value here: the 8 counter bytes, or base and operands
 * oldest to newest joined by ',' — the group walks its (bounded) chain from
 * the far end, one cooperative copy per entry. */
template <int G, int FOLD>
__global__ void __launch_bounds__(256) k_sc_emit(
    const uint8_t *__restrict__ store, const ScCand *__restrict__ cands,
    const ScItem *__restrict__ items, const ScSum *__restrict__ bsums,
    ScCtl *__restrict__ ctl, uint32_t cap, uint32_t max_entries,
    uint64_t byte_cap, uint8_t *__restrict__ out,
    GraScanEntry *__restrict__ ents, const ScFold *__restrict__ folds) {
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
  uint32_t vlen = c.vlen;
  copy_dword<G>(out + off, src, c.klen, lane);
  if (found) copy_dword<G>(out + off + c.klen, src + c.klen, c.vlen, lane);
  if (FOLD && c.type == wb::kMerge) {
    ScFold f = folds[g];
    if (f.flags & kScFoldFolded) {
      found = true;
      vlen = f.vlen;
      uint8_t *dst = out + off + c.klen;
      if (FOLD == 2) {
        if (lane < 8) dst[lane] = (uint8_t)(f.sum >> (8 * lane));
      } else {
        uint32_t nops = f.flags >> 8; /* <= kFoldMaxConcatOps */
        uint64_t o = 0;
        bool first = true;
        if (f.flags & kScFoldBase) {
          ScCand b = cands[g + nops];
          copy_dword<G>(dst, store + b.koff + b.klen, b.vlen, lane);
          o = b.vlen;
          first = false;
        }
        for (uint32_t j = nops; j-- > 0;) { /* oldest operand first */
          ScCand p = cands[g + j];
          if (!first) {
            if (lane == 0) dst[o] = ',';
            o++;
          }
          first = false;
          copy_dword<G>(dst + o, store + p.koff + p.klen, p.vlen, lane);
          o += p.vlen;
        }
      }
    }
  }
  if (lane == 0) {
    GraScanEntry e;
    e.key_off = (uint32_t)off;
    e.key_len = c.klen;
    e.val_off = found ? (uint32_t)off + c.klen : 0u;
    e.val_len = found ? vlen : 0u;
    e.status = found ? GRA_GET_FOUND : GRA_GET_NEEDS_HOST;
    e._pad = 0;
    ents[rank] = e;
  }
}
