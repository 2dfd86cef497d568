/* host_store.h — host-side run registry standing behind the DbWrapper seam.
 *
 * MI355X-first design: the follower "memtable" is a sequence of GPU-produced
 * sorted-by-seq runs resident in device HBM (288 GB/GPU); the host keeps only
 * run descriptors and lazily fetches run bytes for parity probes (gra_get).
 * Leader-side writes (WriteToLeader, rocksdb_wrapper.cpp:5-8) produce
 * host-built runs in the identical format.
 *
 * Get semantics must equal the oracle's (tests/test_oracle.py): walk runs
 * newest→oldest, entries newest→oldest; Put = base, Delete/SingleDelete =
 * tombstone, Merge = operand collected then folded oldest→newest with the
 * engine merge operator, RangeDeletion = tombstone for covered keys below
 * its seq.
 */
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "wb_format.h"

namespace gra {

struct Run {
  uint64_t base_seq = 0, last_seq = 0;
  uint32_t n_entries = 0;
  uint32_t payload_bytes = 0;
  /* device-resident location (absolute offsets into the store arena);
   * UINT64_MAX for host-origin (leader-write) runs */
  uint64_t hdr_cur = UINT64_MAX, payload_cur = UINT64_MAX;
  uint32_t pay_rel_base = 0; /* device runs: kv_off rebase at fetch time */
  /* host copies — always set for host runs, lazily fetched for device runs */
  std::vector<uint8_t> hdrs;     /* n_entries × wb::RecHdr */
  std::vector<uint8_t> payload;
  /* drain-host mode: runs are SPANS of a tick-shared pinned arena drained
   * by k_drain (no per-run host copy). kv_off stays tick-relative; pay_p
   * points at the tick's payload base so pay_p + kv_off is correct. */
  std::shared_ptr<uint8_t> hbuf;
  const uint8_t *hdr_p = nullptr, *pay_p = nullptr;
  bool kpref_built = false; /* device read index (k_kpref) done; guarded by
                               the engine mutex at build time */
  bool sorted = false; /* written by gra_compact / run_compact: one Put per
                          key, ascending bytewise key order, no tombstones.
                          A shard holds at most one, as its oldest run */
  /* its bytes are in the store arena, at hdr_cur / payload_cur */
  bool on_device() const { return hdr_cur != UINT64_MAX; }
  const uint8_t *hdrs_data() const { return hdr_p ? hdr_p : hdrs.data(); }
  const uint8_t *payload_data() const { return pay_p ? pay_p : payload.data(); }
  bool resident() const {
    return hdr_p != nullptr || !hdrs.empty() || n_entries == 0;
  }
};

/* One retained batch for downstream serving (leader update log — the WAL
 * retention analog; replicated_db.cpp:435-575). */
struct LogEnt {
  uint64_t base_seq = 0;
  uint32_t count = 0;
  int64_t ts = 0;
  std::vector<uint8_t> rep;
};

struct ShardState {
  mutable std::mutex mu;
  uint64_t durable_seq = 0;   /* last seq applied & synced on device */
  uint64_t next_seq = 1;      /* next seq to assign at submission */
  bool poisoned = false;      /* corrupt batch seen; next HRR returns false */
  std::vector<std::shared_ptr<Run>> runs; /* oldest .. newest */
  std::deque<LogEnt> log;     /* retained batches (retain_log mode) */
  uint64_t log_used = 0;      /* bytes retained in this shard's log */
  /* follower-ACK box ≅ MaxNumberBox (max_number_box.h:38-83): serving a
   * pull carries the follower's progress — the request's seq_no is the
   * confirmed ack (mode 2, replicated_db.cpp:452-456), and everything sent
   * is the sent ack (mode 1, :543-546). */
  uint64_t acked_sent = 0, acked_confirmed = 0;
  std::condition_variable ack_cv;
  /* per-db counters ≅ replicator_stats.cpp:33-102's per-db fan-out
   * (replicator_in_bytes / _out_bytes / latency / failure counters);
   * relaxed atomics so the hot ingest path never takes a lock for them */
  std::atomic<uint64_t> cnt_updates{0}, cnt_in_bytes{0}, cnt_failures{0};
  std::atomic<uint64_t> cnt_served{0}, cnt_out_bytes{0};
  std::atomic<uint64_t> lat_sum_ms{0}, lat_n{0};
};

/* Roll the shard's submission seq back to the durable boundary and drop
 * retained-log entries past it: a batch that failed validation (or was
 * staged on top of one that did) must never be re-served downstream — the
 * reference's WAL only ever contains accepted batches. Caller holds ss.mu. */
void roll_back_locked(ShardState &ss);

/* The ingest rule: what a finished tick leaves of ONE shard group, and what
 * it does to the shard's seq state. Plain host arithmetic, so a CPU test
 * holds every decision to account; the engine's ingest is one loop over a
 * tick's groups (in tick order) that calls this under ss.mu and materialises
 * the kept records as a run. */
struct GroupFacts {
  uint64_t base_seq, last_seq; /* from the run descriptor; base_seq == 0: the
                                  tick found no room in the store */
  uint32_t n_entries;
  const uint8_t *ok;      /* the group's n_upds validity bytes, or nullptr:
                             the tick reported no error */
  const uint32_t *counts; /* the group's n_upds record counts */
  uint32_t n_upds;
};
struct GroupKeep {
  uint32_t n_entries; /* leading records of the group that stay readable */
  uint64_t last_seq;  /* seq of the last of them */
  bool whole;         /* the group was clean */
};
/*  - overflow (base_seq == 0; real seqs start at 1): NOTHING of the tick was
 *    applied. Poison the shard, count a failure, roll back, keep nothing.
 *    The condition persists until the operator gives the store room, like
 *    the reference's repeated DB::Write failures on a full disk. k_scan2
 *    raises the tick's error word wherever it sets the overflow flag the
 *    descriptors get their base_seq == 0 from, so the case needs no `ok`;
 *  - stale (the shard is already poisoned, by an earlier group of this tick
 *    or an earlier tick): the group was staged BEFORE the failure was
 *    detected and its base_seqs assumed the corrupt batch applied. Such
 *    ticks always ingest while the shard is still poisoned
 *    (gra_handle_replicate_response's failure report drains pending ticks
 *    before clearing the flag). Roll back and keep nothing, durable_seq left
 *    alone: advancing it would skip the failed batch on re-pull (follower
 *    divergence);
 *  - clean (no `ok`, or every byte set): keep the group whole,
 *    durable_seq = max(durable_seq, last_seq);
 *  - corrupt (first clear byte at update i): keep the records of the updates
 *    before it — keep_recs = sum(counts[0..i)), their seqs are final, up to
 *    keep_seq = base_seq - 1 + keep_recs — set durable_seq = max(durable_seq,
 *    keep_seq), poison the shard, count a failure (≅
 *    kReplicatorHandleResponseFailure) and roll back: the reference's
 *    failed-apply -> re-pull-from-LatestSequenceNumber cadence
 *    (replicated_db.cpp:378-382). */
GroupKeep settle_group_locked(ShardState &ss, const GroupFacts &f);

/* Get over a run list (newest last). merge_op: 0 concat, 1 u64add.
 * Returns 0 found, 1 not found. Found value appended to out. */
int run_get(const std::vector<std::shared_ptr<Run>> &runs, const void *key,
            size_t klen, int merge_op, std::string *out);

/* Raw probe over a run list: max-seq terminator (Put/Delete/SingleDelete),
 * max merge-operand seq and max covering range-tombstone seq for `key` —
 * the same per-query verdict k_multiget computes, so a mixed shard can
 * merge the device and host halves by seq. */
struct ProbeResult {
  uint64_t term_seq = 0, merge_seq = 0, rd_seq = 0;
  uint8_t term_type = 0xFF;          /* wb tag of the terminator */
  const uint8_t *val = nullptr;      /* terminator value (kValue only) */
  uint32_t vlen = 0;
};
void run_probe(const std::vector<std::shared_ptr<Run>> &runs, const void *key,
               size_t klen, ProbeResult *out);

/* Ordered range scan over a run list (the host side of gra_scan, and the
 * plain-C++ restatement of the device path): every stored key k with
 * lo <= k < hi (bytewise; lo_len == 0 = from the first key, hi == nullptr =
 * unbounded) for which run_get(k) finds a value, ascending, with that value
 * — merges folded with merge_op. One sort of the in-range point entries by
 * (key asc, seq desc) plus a sweep over the range tombstones: O(entries log
 * entries), never one run_get per key. Emission stops at max_entries or when
 * the next key+value no longer fits in cap bytes (more = true when live keys
 * remain). Returns 0, or 2 when the very first entry exceeds cap. */
struct ScanItem {
  uint32_t key_off, key_len, val_off, val_len; /* into ScanResult::buf */
};
struct ScanResult {
  std::vector<ScanItem> items;
  std::string buf;
  bool more = false;
};
int run_scan(const std::vector<std::shared_ptr<Run>> &runs, const void *lo,
             size_t lo_len, const void *hi, size_t hi_len, int merge_op,
             uint32_t max_entries, size_t cap, ScanResult *out);

/* Compaction of a run list (oldest first) into one sorted run: the plain-C++
 * statement of what gra_compact's device chain writes, result and layout.
 * out gets one Put record per key run_get finds over `runs`, in ascending
 * bytewise key order — a live Put as it stands, a live merge chain folded
 * with merge_op and carrying its newest operand's seq — in the apply path's
 * layout: RecHdr array, 16-B aligned and padded records, run-relative kv_off,
 * flags 0, kpref filled. base_seq / last_seq span the input. Returns 0, or 1
 * where gra_compact reports GRA_COMPACT_UNSUPPORTED (more than 4096 range
 * tombstones or 2^30 entries, a payload of 4 GiB, a record of 0xFFFF0000
 * bytes); out is then empty. */
int run_compact(const std::vector<std::shared_ptr<Run>> &runs, int merge_op,
                Run *out);

/* ---- shard images (gra_export / gra_import / gra_image_check) ----
 *
 * A shard image is what run_compact leaves of a shard — one Put per live
 * key, key-sorted, in the store's own layout — behind a 64-byte header.
 * Version 1, little-endian:
 *
 *    0  8 B  magic "GRASHIMG"
 *    8  u32  version = 1
 *   12  u32  merge_op (GRA_MERGE_* the values were folded with)
 *   16  u64  last_seq: the shard's durable seq at capture; the importer
 *            resumes from it
 *   24  u64  n_entries (<= 2^30)
 *   32  u64  payload_bytes (multiple of 16, < 4 GiB)
 *   40  u64  content_sum: rec_hash_cs of every record, summed mod 2^64 (what
 *            gra_shard_checksum reports for a shard holding just the image)
 *   48  u64  reserved, 0
 *   56  u64  header_sum: FNV-1a-64 over bytes 0..55
 *   64  n_entries x wb::RecHdr (24 B), zero-padded to a multiple of 16
 *       payload_bytes of records
 *
 * image_bytes = 64 + align16(24 n) + payload_bytes. Rules per entry i:
 *   RECORD  type == kValue, flags == 0, 1 <= seq <= last_seq,
 *           val_len < 0xFFFF0000;
 *   LAYOUT  kv_off is a multiple of 16 and dense: kv_off[0] == 0, kv_off[i] ==
 *           kv_off[i-1] + align16(key_len[i-1] + val_len[i-1]) (64-bit);
 *           kv_off + key_len + val_len <= payload_bytes (in bounds); the last
 *           entry's kv_off + align16(key_len + val_len) == payload_bytes;
 *   ORDER   key[i-1] < key[i] in gra_scan's order (memcmp on the common
 *           prefix, the shorter key first, over the stored key). Looked at
 *           only when entries i and i-1 are both in bounds: an entry out of
 *           bounds has failed LAYOUT at a lower or the same index.
 * kpref is the 32-bit key fingerprint: exporters write it, importers
 * recompute it and ignore the stored value. Exporters write every padding
 * byte as 0, so the same content always gives the same bytes; importers do
 * not look at padding.
 *
 * THE VERDICT RULE, one for check_image, k_img_check and the tests. Header
 * first: kImgBadHeader for fewer than 64 bytes, a wrong magic, version,
 * header_sum, reserved word or a merge_op outside the enum; then kImgBadSize
 * when a limit is exceeded (n_entries, payload_bytes) or len differs from
 * image_bytes. Otherwise the failing entry with the lowest index decides; if
 * it fails several rules the order is RECORD, LAYOUT, ORDER. kImgBadSum only
 * when every entry passes and the records do not sum to content_sum.
 * n_entries == 0 with payload_bytes != 0 is kImgBadSize. */
enum : uint32_t {
  kImgOk = 0,
  kImgBadHeader = 1,
  kImgBadSize = 2,
  kImgBadRecord = 3,
  kImgBadLayout = 4,
  kImgBadOrder = 5,
  kImgBadSum = 6,
};
constexpr size_t kImgHeaderBytes = 64;
constexpr uint32_t kImgVersion = 1;
constexpr uint64_t kImgMaxEntries = 1ull << 30;
constexpr uint64_t kImgNoIndex = ~0ull;

struct ImageInfo {
  uint32_t version = 0, merge_op = 0;
  uint64_t last_seq = 0, n_entries = 0, payload_bytes = 0, image_bytes = 0,
           content_sum = 0;
  uint32_t reason = kImgOk;
  uint64_t bad_index = kImgNoIndex; /* lowest failing entry */
};

inline uint64_t img_align16(uint64_t n) { return (n + 15) & ~15ull; }

/* rec_hash_cs, the record hash of gra_shard_checksum and the oracle: FNV-1a-64
 * over (seq LE8 | type | key_len LE4 | val_len LE4 | key | value). */
uint64_t rec_hash_host(uint64_t seq, uint8_t type, uint32_t klen, uint32_t vlen,
                       const uint8_t *key, const uint8_t *val);

/* The header half of the verdict rule: fills the header fields of *out and
 * returns kImgOk, kImgBadHeader or kImgBadSize. Reads at most min(len, 64)
 * bytes. */
uint32_t check_image_header(const uint8_t *img, size_t len, ImageInfo *out);

/* The whole rule over an untrusted byte string: never reads outside
 * [img, img + len). Returns out->reason. */
uint32_t check_image(const uint8_t *img, size_t len, ImageInfo *out);

/* Serialise a run_compact result (sorted, run-relative kv_off, resident) as
 * an image: header, headers, payload, padding zeroed, content_sum and
 * header_sum computed. */
void image_from_run(const Run &run, uint64_t last_seq, uint32_t merge_op,
                    std::vector<uint8_t> *out);

/* Write the 64-byte header (header_sum included) at dst. */
void image_write_header(uint8_t *dst, uint32_t merge_op, uint64_t last_seq,
                        uint64_t n_entries, uint64_t payload_bytes,
                        uint64_t content_sum);

/* The plan of gra_reclaim: where every live segment of the store arena goes
 * when the arena is slid down, and in which copies. Plain host code, so a CPU
 * test can hold every decision to account; the engine runs exactly this plan.
 *
 * A segment is a byte range [src, src + nbytes) of the arena that some
 * device-resident run owns (its header array or its payload); src and nbytes
 * are multiples of 8. The segments are sorted by src and walked with a running
 * offset that starts at 0: dst is the smallest offset >= running with
 * dst == src (mod 16), so dst <= src by induction, every 16-B chunk of the
 * source is a 16-B chunk of the destination, and no reader meets an alignment
 * it did not meet before. A segment with dst == src is not moved; once one
 * moves, every later one does, and the gap src - dst never shrinks along the
 * walk. new_cursor is the end of the last segment rounded up to 16.
 *
 * Moved segments are cut into pieces of at most piece_bytes (a multiple of
 * 16; a piece of a segment at 8 mod 16 ends on a 16-B boundary, so only a
 * segment's first piece has an 8-B head). Consecutive pieces form batches:
 *  - kRcDirect: dst_end(batch) <= src_begin(batch), so no load of the batch
 *    can see a store of the batch (later sources lie higher, earlier batches
 *    are ordered before it). Taken whenever the gap at the batch's first
 *    piece is at least piece_bytes;
 *  - kRcBounce: otherwise. The pieces go store -> bounce buffer, then bounce
 *    buffer -> store; RcPiece::bnc is the piece's place in the buffer
 *    (bnc == src (mod 16)), and a batch ends before bounce_bytes.
 * Returns 0, or 1 with *err set (plan untouched apart from being cleared)
 * when two segments overlap, one reaches past `used`, a src or nbytes is not
 * a multiple of 8, piece_bytes is 0 or not a multiple of 16, or bounce_bytes
 * is smaller than piece_bytes. */
enum : uint32_t { kRcDirect = 0, kRcBounce = 1 };
struct RcSegment {
  uint64_t src = 0, nbytes = 0;
  uint64_t dst = 0;  /* filled by plan_reclaim */
  uint64_t tag = 0;  /* the caller's: carried through the sort */
};
struct RcPiece {
  uint64_t src, dst, bnc; /* bnc: bounce batches only, else 0 */
  uint32_t nbytes;
  uint32_t seg; /* index into RcPlan::segs */
};
struct RcBatch {
  uint32_t kind;  /* kRcDirect / kRcBounce */
  uint32_t first, count; /* pieces */
  uint32_t _pad;
  uint64_t bytes; /* sum of the pieces' nbytes */
};
struct RcPlan {
  std::vector<RcSegment> segs; /* sorted by src, dst filled */
  std::vector<RcPiece> pieces; /* of the moved segments, in source order */
  std::vector<RcBatch> batches;
  uint64_t new_cursor = 0;
  uint64_t bytes_moved = 0, bytes_bounced = 0;
};
int plan_reclaim(const std::vector<RcSegment> &segments, uint64_t used,
                 uint64_t bounce_bytes, uint64_t piece_bytes, RcPlan *plan,
                 std::string *err);

/* Host apply of one rep blob (leader write path): decodes with wb::walk and
 * builds a Run in the same format the GPU emits. Returns false on corrupt
 * rep. base_seq = first seq to assign. */
bool host_build_run(const uint8_t *rep, size_t len, uint64_t base_seq, Run *out);

} /* namespace gra */
