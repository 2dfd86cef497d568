/* host_store.cpp — run-format Get + leader-side host apply, the ingest rule
 * and the plans of gra_compact / gra_reclaim.
 * Semantics cites: rocksdb_wrapper.cpp:5-8 (WriteToLeader = DB::Write),
 * rocksdb_assumption_test.cpp:136-187 (seq accounting). */
#include "host_store.h"

#include <algorithm>
#include <queue>

namespace gra {

namespace {

/* bytewise comparator (rocksdb default): begin <= key < end */
bool range_covers(const uint8_t *b, size_t bl, const uint8_t *e, size_t el,
                  const uint8_t *k, size_t kl) {
  int c1 = memcmp(b, k, bl < kl ? bl : kl);
  if (c1 > 0 || (c1 == 0 && bl > kl)) return false;
  int c2 = memcmp(k, e, kl < el ? kl : el);
  if (c2 > 0 || (c2 == 0 && kl >= el)) return false;
  return true;
}

/* bytewise key order: memcmp on the common prefix, then shorter first */
int key_cmp(const uint8_t *a, size_t al, const uint8_t *b, size_t bl) {
  size_t n = al < bl ? al : bl;
  int c = n ? memcmp(a, b, n) : 0; /* an empty bound may be a null pointer */
  if (c != 0) return c;
  return al < bl ? -1 : (al > bl ? 1 : 0);
}

using Operand = std::pair<const uint8_t *, uint32_t>;

/* Value of a key from its base Put (if any) and the merge operands above
 * it, newest..oldest. Caller guarantees have_base || !ops.empty(). */
void fold_value(bool have_base, const uint8_t *base, uint32_t base_len,
                const std::vector<Operand> &ops, int merge_op,
                std::string *out) {
  if (ops.empty()) {
    /* no operands above the base: the Put's value verbatim (rocksdb
     * FullMerge only runs when merge records are newer — mirrored in the
     * oracle and the device path) */
    out->assign((const char *)base, base_len);
    return;
  }
  if (merge_op == 1 /* u64add */) {
    uint64_t acc = 0;
    if (have_base) memcpy(&acc, base, base_len < 8 ? base_len : 8);
    for (auto it = ops.rbegin(); it != ops.rend(); ++it) {
      uint64_t v = 0;
      memcpy(&v, it->first, it->second < 8 ? it->second : 8);
      acc += v;
    }
    out->assign((const char *)&acc, 8);
  } else { /* concat with ',' oldest→newest */
    out->clear();
    bool first = true;
    if (have_base) {
      out->append((const char *)base, base_len);
      first = false;
    }
    for (auto it = ops.rbegin(); it != ops.rend(); ++it) {
      if (!first) out->push_back(',');
      first = false;
      out->append((const char *)it->first, it->second);
    }
  }
}

} /* namespace */

void roll_back_locked(ShardState &ss) {
  ss.next_seq = ss.durable_seq + 1;
  while (!ss.log.empty() && ss.log.back().base_seq > ss.durable_seq) {
    ss.log_used -= ss.log.back().rep.size();
    ss.log.pop_back();
  }
}

GroupKeep settle_group_locked(ShardState &ss, const GroupFacts &f) {
  if (f.base_seq == 0 || ss.poisoned) { /* overflow / stale */
    if (f.base_seq == 0) {
      ss.poisoned = true;
      ss.cnt_failures++;
    }
    roll_back_locked(ss);
    return {0, 0, false};
  }
  GroupKeep keep = {f.n_entries, f.last_seq, true};
  if (f.ok) {
    uint32_t recs = 0, i = 0;
    for (; i < f.n_upds && f.ok[i]; i++) recs += f.counts[i];
    if (i < f.n_upds) keep = {recs, f.base_seq - 1 + recs, false};
  }
  if (keep.last_seq > ss.durable_seq) ss.durable_seq = keep.last_seq;
  if (!keep.whole) {
    ss.poisoned = true;
    ss.cnt_failures++;
    roll_back_locked(ss);
  }
  return keep;
}

int run_get(const std::vector<std::shared_ptr<Run>> &runs, const void *key_,
            size_t klen, int merge_op, std::string *out) {
  const uint8_t *key = (const uint8_t *)key_;
  /* operand collection: entry pointers into run payloads (runs stay alive
   * for the duration of this call — caller holds shared_ptrs) */
  std::vector<std::pair<const uint8_t *, uint32_t>> ops; /* newest..oldest */
  const uint8_t *base = nullptr;
  uint32_t base_len = 0;
  bool have_base = false, stopped = false;

  for (auto it = runs.rbegin(); it != runs.rend() && !stopped; ++it) {
    const Run &r = **it;
    if (r.n_entries == 0) continue;
    const wb::RecHdr *hdrs = (const wb::RecHdr *)r.hdrs_data();
    const uint8_t *pay = r.payload_data();
    for (int32_t i = (int32_t)r.n_entries - 1; i >= 0; i--) {
      const wb::RecHdr &h = hdrs[i];
      if (h.type == wb::kRangeDeletion) {
        /* covers key? begin = key slice, end = value slice */
        if (range_covers(pay + h.kv_off, h.key_len,
                         pay + h.kv_off + h.key_len, h.val_len, key, klen)) {
          stopped = true; /* everything below this seq is deleted */
          break;
        }
        continue;
      }
      if (h.key_len != klen || memcmp(pay + h.kv_off, key, klen) != 0) continue;
      if (h.type == wb::kMerge) {
        ops.emplace_back(pay + h.kv_off + h.key_len, h.val_len);
        continue;
      }
      if (h.type == wb::kValue) {
        base = pay + h.kv_off + h.key_len;
        base_len = h.val_len;
        have_base = true;
      }
      stopped = true; /* Value / Deletion / SingleDeletion end the walk */
      break;
    }
  }

  if (!have_base && ops.empty()) return 1;
  fold_value(have_base, base, base_len, ops, merge_op, out);
  return 0;
}

void run_probe(const std::vector<std::shared_ptr<Run>> &runs, const void *key_,
               size_t klen, ProbeResult *out) {
  const uint8_t *key = (const uint8_t *)key_;
  *out = ProbeResult();
  for (const auto &rp : runs) {
    const Run &r = *rp;
    if (r.n_entries == 0) continue;
    const wb::RecHdr *hdrs = (const wb::RecHdr *)r.hdrs_data();
    const uint8_t *pay = r.payload_data();
    for (uint32_t i = 0; i < r.n_entries; i++) {
      const wb::RecHdr &h = hdrs[i];
      if (h.type == wb::kRangeDeletion) {
        if (range_covers(pay + h.kv_off, h.key_len,
                         pay + h.kv_off + h.key_len, h.val_len, key, klen) &&
            h.seq > out->rd_seq)
          out->rd_seq = h.seq;
        continue;
      }
      if (h.key_len != klen || memcmp(pay + h.kv_off, key, klen) != 0)
        continue;
      if (h.type == wb::kMerge) {
        if (h.seq > out->merge_seq) out->merge_seq = h.seq;
      } else if (h.seq > out->term_seq) {
        out->term_seq = h.seq;
        out->term_type = h.type;
        out->val = pay + h.kv_off + h.key_len;
        out->vlen = h.val_len;
      }
    }
  }
}

namespace {

struct Point {
  const uint8_t *key, *val;
  uint64_t seq;
  uint32_t klen, vlen;
  uint8_t type;
};

/* The sweep run_scan and run_compact share: every stored key k with
 * lo <= k < hi that run_get finds, ascending, with its folded value.
 * visit(head, value) gets the key's newest entry; returning false ends the
 * sweep. One sort of the in-range point entries by (key asc, seq desc) plus
 * a sweep over the range tombstones. */
template <class Visit>
void sweep_live(const std::vector<std::shared_ptr<Run>> &runs,
                const uint8_t *lo, size_t lo_len, const uint8_t *hi,
                size_t hi_len, int merge_op, Visit &&visit) {
  struct Tomb {
    const uint8_t *b, *e;
    uint32_t bl, el;
    uint64_t seq;
  };
  std::vector<Point> pts;
  std::vector<Tomb> tombs;
  for (const auto &rp : runs) {
    const Run &r = *rp;
    if (r.n_entries == 0) continue;
    const wb::RecHdr *hdrs = (const wb::RecHdr *)r.hdrs_data();
    const uint8_t *pay = r.payload_data();
    for (uint32_t i = 0; i < r.n_entries; i++) {
      const wb::RecHdr &h = hdrs[i];
      const uint8_t *k = pay + h.kv_off;
      if (h.type == wb::kRangeDeletion) {
        /* keep only tombstones whose [begin, end) meets [lo, hi) */
        const uint8_t *e = k + h.key_len;
        if (key_cmp(e, h.val_len, lo, lo_len) <= 0) continue;
        if (hi && key_cmp(k, h.key_len, hi, hi_len) >= 0) continue;
        tombs.push_back({k, e, h.key_len, h.val_len, h.seq});
        continue;
      }
      if (key_cmp(k, h.key_len, lo, lo_len) < 0) continue;
      if (hi && key_cmp(k, h.key_len, hi, hi_len) >= 0) continue;
      pts.push_back({k, k + h.key_len, h.seq, h.key_len, h.val_len, h.type});
    }
  }
  /* (key asc, seq desc): each key's newest entry leads its group */
  std::sort(pts.begin(), pts.end(), [](const Point &a, const Point &b) {
    int c = key_cmp(a.key, a.klen, b.key, b.klen);
    return c != 0 ? c < 0 : a.seq > b.seq;
  });
  /* tombstone sweep: keys ascend, so a tombstone enters once its begin is
   * reached and is dropped for good once its end is; the heap's top is RD,
   * the max seq among the tombstones covering the current key */
  std::sort(tombs.begin(), tombs.end(), [](const Tomb &a, const Tomb &b) {
    return key_cmp(a.b, a.bl, b.b, b.bl) < 0;
  });
  auto by_seq = [](const Tomb *a, const Tomb *b) { return a->seq < b->seq; };
  std::priority_queue<const Tomb *, std::vector<const Tomb *>,
                      decltype(by_seq)> open(by_seq);
  size_t next_tomb = 0;

  std::vector<Operand> ops;
  std::string val;
  for (size_t i = 0; i < pts.size();) {
    const Point &head = pts[i];
    size_t end = i + 1;
    while (end < pts.size() &&
           key_cmp(pts[end].key, pts[end].klen, head.key, head.klen) == 0)
      end++;
    while (next_tomb < tombs.size() &&
           key_cmp(tombs[next_tomb].b, tombs[next_tomb].bl, head.key,
                   head.klen) <= 0)
      open.push(&tombs[next_tomb++]);
    while (!open.empty() &&
           key_cmp(open.top()->e, open.top()->el, head.key, head.klen) <= 0)
      open.pop();
    uint64_t rd = open.empty() ? 0 : open.top()->seq;
    bool live = (head.type == wb::kValue || head.type == wb::kMerge) &&
                head.seq > rd;
    if (live) {
      /* fold: operands above the newest terminator, all above RD */
      ops.clear();
      const uint8_t *base = nullptr;
      uint32_t base_len = 0;
      bool have_base = false;
      for (size_t j = i; j < end && pts[j].seq > rd; j++) {
        if (pts[j].type == wb::kMerge) {
          ops.emplace_back(pts[j].val, pts[j].vlen);
          continue;
        }
        if (pts[j].type == wb::kValue) {
          base = pts[j].val;
          base_len = pts[j].vlen;
          have_base = true;
        }
        break;
      }
      fold_value(have_base, base, base_len, ops, merge_op, &val);
      if (!visit(head, val)) return;
    }
    i = end;
  }
}

} /* namespace */

int run_scan(const std::vector<std::shared_ptr<Run>> &runs, const void *lo_,
             size_t lo_len, const void *hi_, size_t hi_len, int merge_op,
             uint32_t max_entries, size_t cap, ScanResult *out) {
  const uint8_t *lo = (const uint8_t *)lo_, *hi = (const uint8_t *)hi_;
  out->items.clear();
  out->buf.clear();
  out->more = false;
  if (hi && key_cmp(lo, lo_len, hi, hi_len) >= 0) return 0; /* empty range */
  int rc = 0;
  sweep_live(runs, lo, lo_len, hi, hi_len, merge_op,
             [&](const Point &head, const std::string &val) {
               if (out->items.size() >= max_entries) {
                 out->more = true;
                 return false;
               }
               if (out->buf.size() + head.klen + val.size() > cap) {
                 if (out->items.empty())
                   rc = 2;
                 else
                   out->more = true;
                 return false;
               }
               ScanItem it;
               it.key_off = (uint32_t)out->buf.size();
               it.key_len = head.klen;
               out->buf.append((const char *)head.key, head.klen);
               it.val_off = (uint32_t)out->buf.size();
               it.val_len = (uint32_t)val.size();
               out->buf.append(val);
               out->items.push_back(it);
               return true;
             });
  return rc;
}

int run_compact(const std::vector<std::shared_ptr<Run>> &runs, int merge_op,
                Run *out) {
  *out = Run();
  if (runs.empty()) return 0;
  uint64_t entries = 0, tombs = 0;
  for (const auto &rp : runs) {
    const wb::RecHdr *h = (const wb::RecHdr *)rp->hdrs_data();
    for (uint32_t i = 0; i < rp->n_entries; i++)
      tombs += h[i].type == wb::kRangeDeletion;
    entries += rp->n_entries;
  }
  if (tombs > 4096 || entries > (1ull << 30)) return 1;
  std::vector<wb::RecHdr> hdrs;
  std::vector<uint8_t> pay;
  bool too_big = false;
  sweep_live(runs, nullptr, 0, nullptr, 0, merge_op,
             [&](const Point &head, const std::string &val) {
               uint64_t rec = (uint64_t)head.klen + val.size();
               if (rec >= 0xFFFF0000ull ||
                   pay.size() + ((rec + 15) & ~15ull) >= (1ull << 32)) {
                 too_big = true;
                 return false;
               }
               wb::RecHdr h;
               h.seq = head.seq; /* a folded chain carries its head's seq */
               h.kv_off = (uint32_t)pay.size(); /* run-relative */
               h.val_len = (uint32_t)val.size();
               h.key_len = (uint16_t)head.klen;
               h.type = wb::kValue;
               h.flags = 0;
               h.kpref = wb::key_fnv_fold(wb::kFnvBasis32, head.key, head.klen);
               hdrs.push_back(h);
               pay.insert(pay.end(), head.key, head.key + head.klen);
               pay.insert(pay.end(), val.begin(), val.end());
               pay.resize((pay.size() + 15) & ~(size_t)15, 0);
               return true;
             });
  if (too_big) return 1;
  out->base_seq = runs.front()->base_seq;
  out->last_seq = runs.back()->last_seq;
  out->n_entries = (uint32_t)hdrs.size();
  out->payload_bytes = (uint32_t)pay.size();
  out->hdrs.assign((const uint8_t *)hdrs.data(),
                   (const uint8_t *)(hdrs.data() + hdrs.size()));
  out->payload = std::move(pay);
  out->kpref_built = true;
  out->sorted = true;
  return 0;
}

/* ---- shard images: the host statement of the format and its verdict rule
 * (host_store.h) ---- */

namespace {

const char kImgMagic[8] = {'G', 'R', 'A', 'S', 'H', 'I', 'M', 'G'};

uint64_t fnv64(const uint8_t *p, size_t n) {
  uint64_t h = 1469598103934665603ULL;
  for (size_t i = 0; i < n; i++) h = (h ^ p[i]) * 1099511628211ULL;
  return h;
}

uint64_t rd64(const uint8_t *p) { return wb::fixed64_le(p); }
uint32_t rd32(const uint8_t *p) { return wb::fixed32_le(p); }
void wr64(uint8_t *p, uint64_t v) {
  for (int i = 0; i < 8; i++) p[i] = (uint8_t)(v >> (8 * i));
}
void wr32(uint8_t *p, uint32_t v) {
  for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (8 * i));
}

} /* namespace */

uint64_t rec_hash_host(uint64_t seq, uint8_t type, uint32_t klen, uint32_t vlen,
                       const uint8_t *key, const uint8_t *val) {
  uint8_t pre[17];
  wr64(pre, seq);
  pre[8] = type;
  wr32(pre + 9, klen);
  wr32(pre + 13, vlen);
  uint64_t h = 1469598103934665603ULL;
  for (size_t i = 0; i < sizeof(pre); i++) h = (h ^ pre[i]) * 1099511628211ULL;
  for (uint32_t i = 0; i < klen; i++) h = (h ^ key[i]) * 1099511628211ULL;
  for (uint32_t i = 0; i < vlen; i++) h = (h ^ val[i]) * 1099511628211ULL;
  return h;
}

void image_write_header(uint8_t *dst, uint32_t merge_op, uint64_t last_seq,
                        uint64_t n_entries, uint64_t payload_bytes,
                        uint64_t content_sum) {
  memcpy(dst, kImgMagic, 8);
  wr32(dst + 8, kImgVersion);
  wr32(dst + 12, merge_op);
  wr64(dst + 16, last_seq);
  wr64(dst + 24, n_entries);
  wr64(dst + 32, payload_bytes);
  wr64(dst + 40, content_sum);
  wr64(dst + 48, 0);
  wr64(dst + 56, fnv64(dst, 56));
}

uint32_t check_image_header(const uint8_t *img, size_t len, ImageInfo *out) {
  *out = ImageInfo();
  auto verdict = [&](uint32_t r) { return out->reason = r; };
  if (!img || len < kImgHeaderBytes) return verdict(kImgBadHeader);
  if (memcmp(img, kImgMagic, 8) != 0) return verdict(kImgBadHeader);
  out->version = rd32(img + 8);
  out->merge_op = rd32(img + 12);
  if (out->version != kImgVersion || rd64(img + 56) != fnv64(img, 56) ||
      rd64(img + 48) != 0 || out->merge_op > 1)
    return verdict(kImgBadHeader);
  out->last_seq = rd64(img + 16);
  out->n_entries = rd64(img + 24);
  out->payload_bytes = rd64(img + 32);
  out->content_sum = rd64(img + 40);
  if (out->n_entries > kImgMaxEntries || (out->payload_bytes & 15) ||
      out->payload_bytes >= (1ull << 32) ||
      (out->n_entries == 0 && out->payload_bytes != 0))
    return verdict(kImgBadSize);
  out->image_bytes = kImgHeaderBytes +
                     img_align16(out->n_entries * sizeof(wb::RecHdr)) +
                     out->payload_bytes;
  if ((uint64_t)len != out->image_bytes) return verdict(kImgBadSize);
  return verdict(kImgOk);
}

uint32_t check_image(const uint8_t *img, size_t len, ImageInfo *out) {
  if (check_image_header(img, len, out) != kImgOk) return out->reason;
  const uint64_t n = out->n_entries, pb = out->payload_bytes;
  const uint8_t *hdrs = img + kImgHeaderBytes;
  const uint8_t *pay = hdrs + img_align16(n * sizeof(wb::RecHdr));
  uint64_t sum = 0;
  wb::RecHdr prev = {};
  bool prev_in = false;
  for (uint64_t i = 0; i < n; i++) {
    wb::RecHdr h; /* the image may sit at any alignment */
    memcpy(&h, hdrs + i * sizeof(wb::RecHdr), sizeof(h));
    const uint64_t bytes = (uint64_t)h.key_len + h.val_len;
    const bool in = (uint64_t)h.kv_off + bytes <= pb;
    uint32_t bad = kImgOk;
    if (h.type != wb::kValue || h.flags != 0 || h.seq < 1 ||
        h.seq > out->last_seq || h.val_len >= 0xFFFF0000u) {
      bad = kImgBadRecord;
    } else {
      const uint64_t want =
          i == 0 ? 0
                 : (uint64_t)prev.kv_off +
                       img_align16((uint64_t)prev.key_len + prev.val_len);
      if ((h.kv_off & 15) || h.kv_off != want || !in ||
          (i == n - 1 && (uint64_t)h.kv_off + img_align16(bytes) != pb))
        bad = kImgBadLayout;
      else if (i > 0 && prev_in &&
               key_cmp(pay + prev.kv_off, prev.key_len, pay + h.kv_off,
                       h.key_len) >= 0)
        bad = kImgBadOrder;
    }
    if (bad != kImgOk) {
      out->bad_index = i;
      return out->reason = bad;
    }
    sum += rec_hash_host(h.seq, h.type, h.key_len, h.val_len, pay + h.kv_off,
                         pay + h.kv_off + h.key_len);
    prev = h;
    prev_in = in;
  }
  if (sum != out->content_sum) return out->reason = kImgBadSum;
  return out->reason = kImgOk;
}

void image_from_run(const Run &run, uint64_t last_seq, uint32_t merge_op,
                    std::vector<uint8_t> *out) {
  const uint64_t n = run.n_entries;
  const uint64_t hb = img_align16(n * sizeof(wb::RecHdr));
  out->assign(kImgHeaderBytes + hb + run.payload_bytes, 0);
  uint8_t *hdrs = out->data() + kImgHeaderBytes, *pay = hdrs + hb;
  if (n) memcpy(hdrs, run.hdrs_data(), n * sizeof(wb::RecHdr));
  uint64_t sum = 0;
  for (uint64_t i = 0; i < n; i++) {
    wb::RecHdr h;
    memcpy(&h, hdrs + i * sizeof(wb::RecHdr), sizeof(h));
    const uint8_t *src = run.payload_data() + h.kv_off;
    /* key and value only: the padding stays 0 */
    memcpy(pay + h.kv_off, src, (size_t)h.key_len + h.val_len);
    sum += rec_hash_host(h.seq, h.type, h.key_len, h.val_len, src,
                         src + h.key_len);
  }
  image_write_header(out->data(), merge_op, last_seq, n, run.payload_bytes,
                     sum);
}

bool host_build_run(const uint8_t *rep, size_t len, uint64_t base_seq, Run *out) {
  wb::WalkTotals tot = wb::walk(rep, (uint32_t)len, nullptr, 0);
  if (!tot.ok) return false;
  out->n_entries = tot.n_records;
  out->base_seq = base_seq;
  out->last_seq = base_seq + tot.hdr_count - 1;
  out->hdrs.resize((size_t)tot.n_records * sizeof(wb::RecHdr));
  /* same 16-byte record alignment the GPU emit kernel uses */
  size_t pay_need = 0;
  {
    uint32_t i = 0;
    std::vector<wb::Rec> recs(tot.n_records);
    wb::WalkTotals t2 = wb::walk(rep, (uint32_t)len, recs.data(), tot.n_records);
    (void)t2;
    /* CF range tombstones prefix BOTH slices (begin and end key live in the
     * cf-namespaced key space) — mirrors k_emit and the oracle */
    auto cfv_of = [](const wb::Rec &rc) {
      return (rc.cf_id && wb::base_tag(rc.tag) == wb::kRangeDeletion) ? 4u : 0u;
    };
    for (i = 0; i < tot.n_records; i++) {
      const wb::Rec &rc = recs[i];
      uint32_t cf4 = rc.cf_id ? 4u : 0u;
      pay_need += (cf4 + rc.key_len + cfv_of(rc) + rc.val_len + 15u) & ~15u;
    }
    out->payload.resize(pay_need);
    out->payload_bytes = (uint32_t)pay_need;
    wb::RecHdr *hd = (wb::RecHdr *)out->hdrs.data();
    uint32_t off = 0;
    for (i = 0; i < tot.n_records; i++) {
      const wb::Rec &rc = recs[i];
      uint32_t cf4 = rc.cf_id ? 4u : 0u;
      uint32_t cfv = cfv_of(rc);
      wb::RecHdr h;
      h.seq = base_seq + i;
      h.kv_off = off;
      h.val_len = rc.val_len + cfv;
      h.key_len = (uint16_t)(rc.key_len + cf4);
      h.type = wb::base_tag(rc.tag);
      h.flags = cf4 ? 1 : 0;
      hd[i] = h;
      uint8_t *p = out->payload.data() + off;
      if (cf4) memcpy(p, &rc.cf_id, 4);
      memcpy(p + cf4, rep + rc.key_off, rc.key_len);
      /* fingerprint over the STORED key bytes just written (host runs pay
       * it eagerly — CPU cost is trivial; device runs build theirs lazily
       * at first multiget via k_kpref) */
      hd[i].kpref = wb::key_fnv_fold(wb::kFnvBasis32, p, cf4 + rc.key_len);
      if (cfv) memcpy(p + cf4 + rc.key_len, &rc.cf_id, 4);
      memcpy(p + cf4 + rc.key_len + cfv, rep + rc.val_off, rc.val_len);
      off += (cf4 + rc.key_len + cfv + rc.val_len + 15u) & ~15u;
    }
  }
  return true;
}

int plan_reclaim(const std::vector<RcSegment> &segments, uint64_t used,
                 uint64_t bounce_bytes, uint64_t piece_bytes, RcPlan *plan,
                 std::string *err) {
  *plan = RcPlan();
  auto fail = [&](const char *msg) {
    if (err) *err = msg;
    *plan = RcPlan();
    return 1;
  };
  if (piece_bytes == 0 || piece_bytes % 16 != 0 || piece_bytes > 0xFFFFFFF0ull)
    return fail("piece size must be a positive multiple of 16 below 4 GiB");
  if (bounce_bytes < piece_bytes)
    return fail("bounce buffer smaller than one piece");
  std::vector<RcSegment> &segs = plan->segs;
  segs = segments;
  std::sort(segs.begin(), segs.end(), [](const RcSegment &a, const RcSegment &b) {
    return a.src != b.src ? a.src < b.src : a.nbytes < b.nbytes;
  });
  uint64_t src_end = 0; /* end of the segments seen so far */
  for (const RcSegment &s : segs) {
    if (s.src % 8 != 0 || s.nbytes % 8 != 0)
      return fail("segment not 8-byte aligned");
    if (s.nbytes > used || s.src > used - s.nbytes)
      return fail("segment reaches past the cursor");
    if (s.src < src_end) return fail("segments overlap");
    src_end = s.src + s.nbytes;
  }
  /* destinations */
  uint64_t running = 0;
  for (RcSegment &s : segs) {
    uint64_t dst = (running & ~15ull) | (s.src & 15);
    if (dst < running) dst += 16;
    s.dst = dst;
    running = dst + s.nbytes;
  }
  plan->new_cursor = (running + 15) & ~15ull;
  /* pieces of the moved segments */
  for (size_t i = 0; i < segs.size(); i++) {
    const RcSegment &s = segs[i];
    if (s.dst == s.src || s.nbytes == 0) continue;
    plan->bytes_moved += s.nbytes;
    for (uint64_t done = 0; done < s.nbytes;) {
      /* the first piece of a segment at 8 mod 16 stops at a 16-B boundary */
      uint64_t room = piece_bytes - ((s.src + done) & 15);
      uint64_t n = s.nbytes - done < room ? s.nbytes - done : room;
      plan->pieces.push_back(
          {s.src + done, s.dst + done, 0, (uint32_t)n, (uint32_t)i});
      done += n;
    }
  }
  /* batches */
  std::vector<RcPiece> &pc = plan->pieces;
  for (size_t i = 0; i < pc.size();) {
    RcBatch b = {};
    b.first = (uint32_t)i;
    if (pc[i].src - pc[i].dst >= piece_bytes) {
      b.kind = kRcDirect;
      const uint64_t src_begin = pc[i].src;
      while (i < pc.size() && pc[i].dst + pc[i].nbytes <= src_begin) {
        b.bytes += pc[i].nbytes;
        i++;
      }
    } else {
      b.kind = kRcBounce;
      uint64_t fill = 0; /* bytes of the bounce buffer taken */
      /* until the buffer is full or the gap has grown to hold a piece */
      while (i < pc.size() && pc[i].src - pc[i].dst < piece_bytes) {
        uint64_t bnc = ((fill + 15) & ~15ull) + (pc[i].src & 15);
        if (bnc + pc[i].nbytes > bounce_bytes) break;
        pc[i].bnc = bnc;
        fill = bnc + pc[i].nbytes;
        b.bytes += pc[i].nbytes;
        i++;
      }
      plan->bytes_bounced += b.bytes;
    }
    b.count = (uint32_t)i - b.first;
    plan->batches.push_back(b);
  }
  return 0;
}

} /* namespace gra */
