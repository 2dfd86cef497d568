/* rocksplicator_gpu.h — C-ABI boundary of the MI355X-native replication
 * apply path.
 *
 * This is the drop-in seam for pinterest/rocksplicator's follower-side
 * WriteBatch ingest. Each entry point states the reference interface it
 * replaces (file:line in /root/reference). A C++ adapter implementing
 * replicator::DbWrapper (rocksdb_replicator/db_wrapper.h:6-15) on top of
 * these calls is shown in INTEGRATION.md, so that
 * RocksDBReplicator::addDB/write (rocksdb_replicator/rocksdb_replicator.h:
 * 175-216) stay source-compatible.
 *
 * Threading contract (mirrors the reference executor model,
 * rocksdb_replicator.cpp:41-67): calls on ONE GraDb are sequential per
 * shard; calls across different GraDb handles may be concurrent.
 * gra_handle_replicate_response enqueues and completes asynchronously;
 * gra_flush is the drain barrier after which gra_latest_seq/gra_get are
 * linearizable per shard.
 *
 * The follower apply path is GPU-only BY DESIGN: gra_engine_create fails
 * loudly when no MI355X (HIP device) is present — there is no CPU fallback
 * for gra_handle_replicate_response.
 */
#ifndef ROCKSPLICATOR_GPU_H
#define ROCKSPLICATOR_GPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct GraEngine GraEngine;   /* one per GPU; owns streams + device store */
typedef struct GraDb GraDb;           /* per-shard handle ≅ one replicator::DbWrapper */
typedef struct GraReplay GraReplay;   /* pre-uploaded replay stream (harness) */

enum { GRA_MERGE_CONCAT = 0, GRA_MERGE_U64ADD = 1 };

/* Status codes (gra_* return int unless noted): */
enum {
  GRA_OK = 0,
  GRA_NOT_FOUND = 1,      /* gra_get: key absent/deleted */
  GRA_BUF_TOO_SMALL = 2,  /* gra_get: value larger than cap */
  GRA_ERR = -1,           /* see gra_last_error() */
  GRA_CORRUPT = -2,       /* malformed WriteBatch rep */
  GRA_NO_GPU = -3,        /* no HIP device — the apply path refuses to run */
  GRA_FULL = -4,          /* staging or store arena exhausted */
};

typedef struct GraEngineOpts {
  uint32_t nshards;
  int device;              /* HIP device ordinal; -1 = current device */
  int merge_op;            /* GRA_MERGE_* — Get-time merge-operator fold */
  int store_ring;          /* 1: device run arena recycles oldest ticks (bench);
                              0: GRA_FULL when exhausted */
  uint64_t store_bytes;    /* device run-arena capacity (0 = 4 GiB default) */
  uint64_t staging_bytes;  /* pinned staging per buffer (0 = 256 MiB default) */
  uint32_t max_wb_records; /* per-batch record cap (0 = 1024 default) */
  int retain_log;          /* 1: retain applied/written rep blobs per shard so
                              this node can serve downstream pulls (the WAL-
                              retention analog; replicated_db.cpp:435-575) */
  uint64_t log_bytes;      /* retained-log cap across shards (0 = 256 MiB);
                              oldest batches evicted first (WAL_ttl analog,
                              performance.cpp:99) */
  int drain_host;          /* 1: eagerly drain each run's bytes to host
                              memtable buffers at flush (the literal
                              "drain to host memtables" mode; default 0 =
                              device-resident store with lazy fetch) */
  int fold_on_device;      /* 1: gra_multiget and gra_scan fold live merge
                              operands on the device and report GRA_GET_FOUND
                              (see both for what still reports NEEDS_HOST);
                              default 0 = every such key is GRA_GET_NEEDS_HOST */
} GraEngineOpts;

void gra_engine_opts_init(GraEngineOpts *opts); /* fill defaults */

/* Create/destroy the per-GPU engine. Returns GRA_OK or GRA_NO_GPU/GRA_ERR. */
int gra_engine_create(const GraEngineOpts *opts, GraEngine **out);
void gra_engine_destroy(GraEngine *e);

/* Thread-local message for the last GRA_ERR/GRA_CORRUPT/GRA_NO_GPU. */
const char *gra_last_error(void);

/* ---------------- per-shard handles (the DbWrapper seam) ---------------- */

/* ≅ constructing a RocksDbWrapper for one shard and registering it via
 * RocksDBReplicator::addDB (rocksdb_replicator.cpp:96-133). */
GraDb *gra_open(GraEngine *e, uint32_t shard_id);
void gra_close(GraDb *db);

/* ≅ DbWrapper::HandleReplicateResponse (db_wrapper.h:13; reference impl
 * rocksdb_wrapper.cpp:13-28): apply one Update's raw_data (WriteBatch rep
 * bytes) + timestamp to this shard. Returns 1 (true) when accepted, 0 on
 * failure — same bool contract the pull loop checks (replicated_db.cpp:378).
 * Acceptance is an enqueue; a later corruption detected on-GPU poisons the
 * shard: the NEXT call returns 0 and the shard's seq rolls back to the last
 * durable batch boundary, mirroring the reference's delayed re-pull
 * (replicated_db.cpp:378-382,412-431). */
int gra_handle_replicate_response(GraDb *db, const uint8_t *rep, size_t len,
                                  int64_t timestamp_ms);

/* ≅ DbWrapper::LatestSequenceNumber (db_wrapper.h:12; rocksdb_wrapper.cpp:4).
 * Returns the seq the pull loop should resume from: submitted seq while the
 * shard is healthy, last durable seq after a failure. */
uint64_t gra_latest_seq(GraDb *db);

/* ≅ DbWrapper::WriteToLeader (db_wrapper.h:8; rocksdb_wrapper.cpp:5-8):
 * leader-side local write of a WriteBatch rep. Host path (WAL+memtable is
 * host work in the reference; GPU leader batching is a later row — SURVEY
 * §8f f1). Fills *seq_out with the batch's last seq. */
int gra_write_leader(GraDb *db, const uint8_t *rep, size_t len, uint64_t *seq_out);

/* Parity probe ≅ rocksdb::DB::Get with the engine's merge operator folded.
 * GRA_OK (value in buf, *vlen set) / GRA_NOT_FOUND / GRA_BUF_TOO_SMALL. */
int gra_get(GraDb *db, const void *key, size_t klen, void *buf, size_t cap,
            size_t *vlen);

/* Drain barrier: every update submitted so far is applied and durable; after
 * this, gra_latest_seq and gra_get are linearizable per shard. */
int gra_flush(GraEngine *e);

/* drain_host mode setup: pre-pin `count` host arenas of `bytes` each so no
 * hipHostMalloc happens inside a timed region. */
int gra_drain_prewarm(GraEngine *e, size_t bytes, uint32_t count);

/* Batched point reads served FROM THE DEVICE STORE (followers serve reads
 * in rocksplicator deployments — ApplicationDB::Get routes to the local db;
 * here the memtable lives in HBM, so the search runs there too: one block
 * per query scanning the shard's runs newest->oldest). Each result value is
 * written at valbuf[q*val_stride] (the copy is capped at val_stride; vlen is
 * the true length). Call gra_flush first for linearizable results.
 *
 * Merge operands. With T = the key's newest Put/Delete/SingleDelete, RD =
 * the newest range tombstone covering it and floor = max(T.seq, RD.seq), a
 * key is "live merge" when it has Merge entries above the floor.
 *   fold_on_device = 0 (default): every live-merge query reports
 *     GRA_GET_NEEDS_HOST with vlen 0; answer it with gra_get.
 *   fold_on_device = 1, GRA_MERGE_U64ADD: the device folds — the base (T's
 *     value iff T is a Put above RD, else 0) plus every operand above the
 *     floor, each read as its first min(8, len) bytes little-endian and
 *     zero-extended, added modulo 2^64. The query reports GRA_GET_FOUND,
 *     vlen = 8, with the 8 little-endian bytes (min(8, val_stride) copied).
 *     Chains of any length fold; the result equals gra_get's bit for bit.
 *   Still GRA_GET_NEEDS_HOST with fold_on_device = 1:
 *     - GRA_MERGE_CONCAT: the join's candidates are unordered, concat is not
 *       folded by gra_multiget;
 *     - any call on a shard that holds host-origin runs (leader writes,
 *       drained arenas): the device fold is switched off for the whole call,
 *       because host runs may hold newer entries of a key; live-merge
 *       queries, including those whose operands straddle device and host
 *       runs, report NEEDS_HOST as with fold_on_device = 0. */
enum { GRA_GET_FOUND = 0, GRA_GET_MISS = 1, GRA_GET_NEEDS_HOST = 2 };
typedef struct {
  uint32_t off, len; /* key slice in keybuf */
} GraKeyRef;
typedef struct {
  uint32_t status; /* GRA_GET_* */
  uint32_t vlen;
} GraGetResult;
int gra_multiget(GraDb *db, uint32_t nq, const GraKeyRef *keys,
                 const uint8_t *keybuf, size_t keybuf_len, uint8_t *valbuf,
                 uint32_t val_stride, GraGetResult *out);

/* Ordered range scan served FROM THE DEVICE STORE ≅ ApplicationDB::NewIterator
 * (rocksdb_admin/application_db.h:55, application_db.cpp:78-83) followed by
 * Seek(lo) and Next() until hi: every stored key k with lo <= k < hi for
 * which gra_get(k) would return GRA_OK, in ascending bytewise order of the
 * STORED key ([cf LE4 | key] for cf != 0 — scan a column family with
 * cf-prefixed bounds; memcmp on the common prefix, then the shorter key
 * first), together with its value. lo_len == 0 scans from the first key,
 * hi == NULL has no upper bound, lo >= hi is an empty result and GRA_OK.
 *
 * Device path: collect the in-range entries of the shard's runs, bitonic-sort
 * them by (key, seq desc), resolve each key from its newest entry and the
 * covering range tombstones, prefix-sum and emit — all on the GPU; only the
 * emitted bytes cross PCIe. Runs are unsorted by key, so the work per call is
 * O(entries in the shard) WHATEVER THE RANGE — with one exception: the sorted
 * run gra_compact leaves as the shard's oldest is entered by a lower-bound
 * search and contributes only its entries inside [lo, hi). Such a call reports
 * served_by = GRA_SCAN_DEVICE_INDEXED; runs appended since are still read
 * whole.
 *
 * Merge operands on the device path (terms as for gra_multiget):
 *   fold_on_device = 0 (default): a key whose newest entry is a live Merge
 *     reports GRA_GET_NEEDS_HOST with the key only; fold it with gra_get.
 *   fold_on_device = 1: the chain is folded on the device — the operands
 *     above max(T, RD) that follow the head in the sorted candidates, over
 *     T's value iff T is a Put above RD — and the entry is GRA_GET_FOUND with
 *     the folded value: 8 little-endian bytes under GRA_MERGE_U64ADD (any
 *     chain length); base and operands, oldest to newest, joined by ','
 *     under GRA_MERGE_CONCAT. Values equal gra_get's bit for bit.
 *   Still GRA_GET_NEEDS_HOST (key only) with fold_on_device = 1: a
 *     GRA_MERGE_CONCAT chain of more than 256 operands.
 * Host path (served_by = GRA_SCAN_HOST; taken when the shard holds host-origin
 * runs — with or without fold_on_device: nothing is folded on the device
 * when host runs could hold newer entries of a key —, when more than 4096
 * range tombstones meet the range, or when device staging cannot be
 * allocated): same result, merges folded with the engine's merge operator, so
 * every entry is GRA_GET_FOUND.
 *
 * Entries are written while n < max_entries and the cumulative bytes fit in
 * cap (an entry costs key_len + val_len, with the FOLDED val_len for a folded
 * entry, and key_len alone for NEEDS_HOST). When
 * the next entry does not fit and n > 0, more = 1 and the call returns
 * GRA_OK; resume with lo = last key + "\x00". GRA_BUF_TOO_SMALL when the very
 * first entry does not fit. Call gra_flush first for linearizable results;
 * scanning recycled ring-store regions is undefined, as for gra_get. */
enum { GRA_SCAN_DEVICE = 0, GRA_SCAN_HOST = 1, GRA_SCAN_DEVICE_INDEXED = 2 };
typedef struct {
  uint32_t key_off, key_len;  /* stored key bytes, in buf */
  uint32_t val_off, val_len;  /* value bytes, in buf (FOUND only; else 0,0) */
  uint32_t status;            /* GRA_GET_FOUND | GRA_GET_NEEDS_HOST */
  uint32_t _pad;
} GraScanEntry;
typedef struct {
  uint32_t n;           /* entries written */
  uint32_t more;        /* 1: stopped at max_entries or cap before the range ended */
  uint32_t served_by;   /* GRA_SCAN_* */
  uint32_t candidates;  /* device path: point entries collected for the sort; host path: 0 */
  uint64_t buf_used;
} GraScanInfo;
int gra_scan(GraDb *db, const void *lo, size_t lo_len, const void *hi,
             size_t hi_len, uint32_t max_entries, GraScanEntry *out,
             uint8_t *buf, size_t cap, GraScanInfo *info);

/* Compact the shard's device runs ≅ AdminHandler::async_tm_compactDB
 * (rocksdb_admin/admin_handler.cpp:2160-2175), which calls
 * ApplicationDB::CompactRange(nullptr, nullptr) (application_db.cpp:138-143):
 * the longest leading stretch of the shard's run list (oldest first) that is
 * device-resident — the prefix — is replaced by ONE run that is sorted by
 * key. Call gra_flush first to include everything submitted; runs appended
 * while the call works stay behind the new run.
 *
 * The new run holds one Put per key gra_get would find looking at the prefix
 * alone, in ascending bytewise order of the stored key (gra_scan's order).
 * A key whose newest entry is a live Put keeps that Put's value and seq; a
 * key with live merge operands is folded with the engine's merge operator,
 * whatever fold_on_device says, exactly as gra_get folds (floor = max(T, RD),
 * the operands above it, over T's value iff T is a Put above RD; chains of
 * any length) and stored as a Put carrying the newest operand's seq.
 * Deletes, SingleDeletes, range tombstones, shadowed versions and dead keys
 * are dropped. Seqs grow along the run list, so everything a tombstone,
 * Delete or Merge of the prefix can act on is in the prefix: no gra_get,
 * gra_multiget or gra_scan result changes, whatever newer runs follow. The
 * shard checksum does change: it sums the records the store holds.
 *
 * The run is laid out exactly as the apply path lays out a tick (headers,
 * then 16-B aligned records), with every header's key fingerprint filled,
 * so all readers work on it unchanged; gra_scan additionally enters it by
 * a lower-bound search (GRA_SCAN_DEVICE_INDEXED).
 *
 * info->status:
 *   GRA_COMPACT_DONE         prefix replaced;
 *   GRA_COMPACT_NOTHING      no device-resident prefix (leader-written,
 *                            drained or empty shard), or the prefix is one
 *                            already-sorted run; store untouched;
 *   GRA_COMPACT_UNSUPPORTED  the prefix holds more than 4096 range
 *                            tombstones or more than 2^30 entries, its
 *                            output payload would reach 4 GiB, or one value
 *                            would reach 0xFFFF0000 bytes; store untouched.
 * Returns GRA_OK with one of these, GRA_ERR on a store_ring engine (it keeps
 * no runs), or GRA_FULL when the arena cannot hold the output; the store is
 * untouched then too. LIMIT: the arena is a bump allocator, so a compaction
 * needs room for its output on top of its input; the space of the replaced
 * runs comes back with the next gra_reclaim (below), not before. bytes_in /
 * bytes_out (header + payload bytes) say what that reclaim will free. */
enum { GRA_COMPACT_DONE = 0, GRA_COMPACT_NOTHING = 1, GRA_COMPACT_UNSUPPORTED = 2 };
typedef struct {
  uint32_t status;               /* GRA_COMPACT_* */
  uint32_t runs_in, runs_after;  /* runs replaced (0 unless DONE); runs the
                                    shard holds after the call */
  uint32_t _pad;
  uint64_t entries_in, entries_out; /* records in the prefix; records written */
  uint64_t bytes_in, bytes_out;  /* header + payload bytes, in and out */
} GraCompactInfo;
int gra_compact(GraDb *db, GraCompactInfo *info);

/* How full the device run arena is. `used` is the bump cursor, read with a
 * stream-ordered copy behind the ticks already enqueued: bytes no tick or
 * compaction can get any more. `live` is what the shards' lists still point
 * at: header + payload bytes of every device-resident run (a truncated run
 * counts its payload's upper bound). used - live is about what gra_reclaim
 * would free (alignment padding stays). The call does not flush: updates
 * staged but not yet ticked are in neither figure. On a store_ring engine
 * `used` is the ring's monotonic cursor and `live` is 0. */
typedef struct {
  uint64_t capacity;  /* opts.store_bytes */
  uint64_t used;      /* the bump cursor */
  uint64_t live;      /* bytes of the device-resident runs the shards list */
} GraStoreUsage;
int gra_store_usage(GraEngine *e, GraStoreUsage *out);

/* Give the arena its dead space back: every live device-resident run of
 * every shard is slid down to the bottom of the arena, in address order, and
 * the bump cursor is reset to the end of the last one, so the apply path and
 * later compactions can use what replaced runs (gra_compact), dropped groups
 * and alignment slack held. A stop-the-world pass: the call flushes first
 * (gra_flush), holds the engine for its whole duration, and excludes
 * gra_compact; reads and ticks issued meanwhile wait. No read result and no
 * shard checksum changes: bytes keep their values, only their place (every
 * segment keeps its offset mod 16, so all readers meet the alignment they met
 * before). Host-origin runs (leader writes, drained arenas of a ring engine)
 * are not in the arena and are left alone; the device runs of a drain_host
 * non-ring engine move like any other, their host spans stay.
 *
 * info->status:
 *   GRA_RECLAIM_DONE     used_after < used_before. bytes_moved may be 0
 *                        (only the tail was dead);
 *   GRA_RECLAIM_NOTHING  empty store, or already dense: store untouched,
 *                        used_after == used_before.
 * Returns GRA_OK with one of these. GRA_ERR on a store_ring engine (it keeps
 * no runs), when the run list is inconsistent (overlapping runs, a run past
 * the cursor) or when staging cannot be allocated: all of that is checked
 * before the first copy is launched, and the store is untouched. A HIP error
 * AFTER the first launch leaves the arena half moved, its contents undefined:
 * the call returns GRA_ERR, gra_last_error says so, and the engine must be
 * destroyed.
 *
 * LIMITS. A compaction still needs room for its output BEFORE the reclaim:
 * compact and reclaim at a high-water mark read from gra_store_usage, not
 * when the arena is full. An arena that is full of live data cannot be
 * helped. Not concurrent with ticks; no ring stores. Everything above the first
 * dead byte moves, every time; behind a hole smaller than a piece it moves
 * through the bounce buffer, at twice the traffic. The copy sizes (bounce
 * buffer 64 MiB, allocated at the first call that needs it; pieces of
 * 16 MiB) can be overridden with GRA_RECLAIM_BOUNCE / GRA_RECLAIM_PIECE,
 * byte counts read at engine creation — for tests. */
enum { GRA_RECLAIM_DONE = 0, GRA_RECLAIM_NOTHING = 1 };
typedef struct {
  uint32_t status;        /* GRA_RECLAIM_* */
  uint32_t runs_moved;    /* runs with at least one segment whose offset changed */
  uint32_t batches;       /* copy batches launched */
  uint32_t _pad;
  uint64_t used_before, used_after; /* cursor before / after */
  uint64_t bytes_moved;   /* bytes of segments whose offset changed */
  uint64_t bytes_bounced; /* of those, moved through the bounce buffer */
} GraReclaimInfo;
int gra_reclaim(GraEngine *e, GraReclaimInfo *info);

/* ---------------- shard images: bootstrap a replica past the log ----------
 * ≅ the data-plane half of AdminHandler::async_tm_backupDB / restoreDB
 * (rocksdb_admin/admin_handler.cpp:865-943): capture a consistent image of a
 * shard, install it in an empty shard, and replication resumes from the
 * image's sequence number instead of replaying a history the retained log
 * (gra_get_updates) may no longer hold. An image built offline is installed
 * the same way (≅ addS3SstFilesToDB, admin_handler.cpp:1635). The image is a
 * byte string; storing and moving it (files, HDFS, S3) is the caller's.
 *
 * FORMAT, version 1, little-endian. A 64-byte header:
 *    0  8 B  magic "GRASHIMG"           32  u64  payload_bytes (multiple of
 *    8  u32  version = 1                         16, < 4 GiB)
 *   12  u32  merge_op (GRA_MERGE_*)     40  u64  content_sum
 *   16  u64  last_seq                   48  u64  reserved, 0
 *   24  u64  n_entries (<= 2^30)        56  u64  header_sum: FNV-1a-64 over
 *                                                bytes 0..55
 * then n_entries record headers of 24 B (u64 seq | u32 kv_off | u32 val_len |
 * u16 key_len | u8 type | u8 flags | u32 kpref), zero-padded to a multiple of
 * 16, then payload_bytes of records: key bytes then value bytes at kv_off,
 * each record padded with zeros to 16 B. image_bytes = 64 + align16(24 n) +
 * payload_bytes. The records are what gra_compact would leave of the whole
 * shard: one Put per live key (merge chains folded with merge_op, carrying
 * the newest operand's seq), strictly ascending in gra_scan's order of the
 * stored key. content_sum is gra_shard_checksum's definition over them;
 * last_seq is the shard's durable seq at capture. Per entry i:
 *   RECORD  type == 1 (Put), flags == 0, 1 <= seq <= last_seq,
 *           val_len < 0xFFFF0000;
 *   LAYOUT  kv_off a multiple of 16 and dense (kv_off[0] == 0, kv_off[i] ==
 *           kv_off[i-1] + align16(key_len[i-1] + val_len[i-1])), the record
 *           inside the payload, the last record ending at payload_bytes;
 *   ORDER   key[i-1] < key[i].
 * kpref (the 32-bit key fingerprint) is written by exporters and recomputed
 * by importers, which ignore the stored value, as they ignore padding.
 *
 * VERDICT (GraImageInfo.reason; one rule for gra_image_check, the device
 * check of gra_import and the tests): the header first — GRA_IMG_BAD_HEADER
 * for fewer than 64 bytes, a wrong magic, version, header_sum, reserved word
 * or unknown merge_op, then GRA_IMG_BAD_SIZE when a limit is exceeded or len
 * is not image_bytes. Otherwise the failing entry with the lowest index
 * decides (bad_index), RECORD before LAYOUT before ORDER. GRA_IMG_BAD_SUM
 * only when every entry passes. */
typedef struct {
  uint32_t version, merge_op;
  uint64_t last_seq, n_entries, payload_bytes, image_bytes, content_sum;
  uint32_t reason;     /* GRA_IMG_* */
  uint32_t served_by;  /* export only: 0 device chain, 1 host path */
  uint64_t bad_index;  /* lowest failing entry, UINT64_MAX if none/header */
} GraImageInfo;
enum { GRA_IMG_OK, GRA_IMG_BAD_HEADER, GRA_IMG_BAD_SIZE, GRA_IMG_BAD_RECORD,
       GRA_IMG_BAD_LAYOUT, GRA_IMG_BAD_ORDER, GRA_IMG_BAD_SUM };

/* Capture ≅ ApplicationDBBackupManager / backupDBHelper's checkpoint
 * (admin_handler.cpp:865-900). The call flushes (gra_flush), then takes the
 * shard's run list and durable seq together; the image is what gra_compact
 * would leave of the WHOLE run list, by its fold rules (chains of any length,
 * the engine's merge operator whatever fold_on_device says). The store is
 * untouched: no run is replaced, no read result or shard checksum changes,
 * gra_store_usage().used is the same after the call.
 *   served_by 0: every run is device-resident. gra_compact's device chain
 *     writes the run into FREE arena space as scratch, it is checked and
 *     summed there, copied to buf, and the cursor is put back. LIMIT, as for
 *     gra_compact: the arena needs room for the output on top of its content;
 *     GRA_FULL otherwise. Excludes gra_compact / gra_reclaim, and ticks wait,
 *     for the duration.
 *   served_by 1: the shard holds host-origin runs (a leader, drained arenas):
 *     the runs are fetched and compacted on the host. Byte-identical to the
 *     device chain's image for the same records.
 * GRA_OK with info filled and info->image_bytes written to buf;
 * GRA_BUF_TOO_SMALL when cap is too small, info->image_bytes exact (nothing
 * written); GRA_FULL (above); GRA_ERR on a store_ring engine (it keeps no
 * runs) and where gra_compact would report GRA_COMPACT_UNSUPPORTED —
 * gra_last_error names the limit. An empty shard exports a valid 64-byte
 * image. */
int gra_export(GraDb *db, uint8_t *buf, size_t cap, GraImageInfo *info);

/* Install ≅ restoreDBHelper (admin_handler.cpp:902-943: restore, reopen,
 * then pull from the restored sequence number). Requires — GRA_ERR otherwise
 * — an engine that is not store_ring, an image whose merge_op is the
 * engine's, and a pristine shard: no runs, latest seq 0, not poisoned,
 * nothing staged, an empty retained log. The header is checked on the host
 * before anything is launched; the body is staged in device memory and
 * proven well-formed THERE (the verdict rule above) before any reader can
 * touch it; then the space is reserved from the store cursor (GRA_FULL when
 * the arena has no room), headers and payload are placed, ONE sorted run is
 * listed (all readers take it unchanged, gra_scan enters it by lower bound:
 * GRA_SCAN_DEVICE_INDEXED) and the shard's durable and latest seq become
 * last_seq, so a pull loop resumes with last_seq as its seq_no. An image
 * without entries lists no run and still sets the seqs.
 * A rejected image returns GRA_CORRUPT with info->reason / bad_index set and
 * leaves shard and arena exactly as they were (used unchanged, no run,
 * seq 0): a later good import into the same shard succeeds. Excludes
 * gra_compact / gra_reclaim, and the shard's other calls wait, for the
 * duration. */
int gra_import(GraDb *db, const uint8_t *img, size_t len, GraImageInfo *info);

/* The verdict rule on the host ≅ BackupEngine::VerifyBackup: no engine, no
 * GPU. GRA_OK or GRA_CORRUPT with info->reason / bad_index. Never reads
 * outside [img, img + len). */
int gra_image_check(const uint8_t *img, size_t len, GraImageInfo *info);

/* Full-store content checksum for any-size parity ("checksum of
 * checksums"): per record FNV-1a over (seq LE8 | type | key_len LE4 |
 * val_len LE4 | key bytes | val bytes), combined per shard by u64
 * ADDITION — order/representation independent, so it can be compared
 * against the oracle's orc_shard_checksum on identically applied streams
 * at ANY size. Computed on-device over the run store (host-origin runs
 * folded on the host). Call gra_flush first. */
int gra_shard_checksum(GraDb *db, uint64_t *out);

/* ---------------- leader update-serving ----------------
 * ≅ ReplicatedDB::handleReplicateRequest batch read-out (replicated_db.cpp:
 * 435-575): serve retained batches with base seq > since_seq, up to
 * max_updates (the reference default is 50, replicated_db.cpp:42-43), as
 * (seq, timestamp, rep bytes) triples — the Update wire triple
 * (replicator.thrift:44-57). Blobs are copied into buf; out[i].off/len
 * index it. Requires opts.retain_log. Returns GRA_OK with *n_out = 0 when
 * caught up; GRA_ERR when since_seq predates the retained log (the
 * reference's WAL-gone case). */
typedef struct {
  uint64_t seq;   /* batch base seq (first record's seq) */
  int64_t ts;     /* timestamp the leader stamped (ms) */
  uint32_t off, len;
} GraServedUpdate;
/* requester_role: 0 = FOLLOWER (the request's seq_no is posted as the
 * confirmed ack), 1 = OBSERVER (no ack — replicated_db.cpp:452-456 ignores
 * observer sequence numbers). */
int gra_get_updates(GraDb *db, uint64_t since_seq, uint32_t max_updates,
                    GraServedUpdate *out, uint32_t *n_out, uint8_t *buf,
                    size_t cap, int requester_role);

/* Per-db counters ≅ the replicator stats hooks' per-db fan-out
 * (rocksdb_replicator/replicator_stats.cpp:33-102: replicator_in_bytes,
 * replicator_out_bytes, replicator_latency_ms, handle-response failures). */
typedef struct {
  uint64_t updates_applied, in_bytes, apply_failures;
  uint64_t updates_served, out_bytes;
  uint64_t latency_ms_sum, latency_samples;
  uint64_t latest_seq;
} GraDbCounters;
int gra_db_counters(GraDb *db, GraDbCounters *out);

/* ≅ MaxNumberBox::wait (max_number_box.h:38-83, .cpp:63) behind the 2-ACK
 * write modes (replicated_db.cpp:147-156): block until the downstream ack
 * reaches seq. confirmed=1 waits for follower-applied progress (mode 2 —
 * the pull request's seq_no, replicated_db.cpp:452-456); confirmed=0 waits
 * for served progress (mode 1, :543-546). GRA_OK, or GRA_NOT_FOUND on
 * timeout. */
int gra_wait_ack(GraDb *db, uint64_t seq, int confirmed, int timeout_ms);

/* ---------------- WriteBatch builder ----------------
 * The reference's callers construct updates with rocksdb::WriteBatch
 * (e.g. examples/counter_service/counter_handler.cpp:152-158); this is the
 * framework-native equivalent producing the identical rep byte layout. */
typedef struct GraBatch GraBatch;
GraBatch *gra_wb_create(void);
void gra_wb_destroy(GraBatch *b);
void gra_wb_clear(GraBatch *b);
void gra_wb_put(GraBatch *b, const void *k, size_t klen, const void *v, size_t vlen);
void gra_wb_delete(GraBatch *b, const void *k, size_t klen);
void gra_wb_single_delete(GraBatch *b, const void *k, size_t klen);
void gra_wb_merge(GraBatch *b, const void *k, size_t klen, const void *v, size_t vlen);
void gra_wb_delete_range(GraBatch *b, const void *bk, size_t bklen,
                         const void *ek, size_t eklen);
/* CF-prefixed record variants (varint cf id before the slices; cf 0 uses
 * the plain forms, as rocksdb does). */
void gra_wb_cf_put(GraBatch *b, uint32_t cf, const void *k, size_t klen,
                   const void *v, size_t vlen);
void gra_wb_cf_delete(GraBatch *b, uint32_t cf, const void *k, size_t klen);
void gra_wb_cf_single_delete(GraBatch *b, uint32_t cf, const void *k,
                             size_t klen);
void gra_wb_cf_merge(GraBatch *b, uint32_t cf, const void *k, size_t klen,
                     const void *v, size_t vlen);
void gra_wb_cf_delete_range(GraBatch *b, uint32_t cf, const void *bk,
                            size_t bklen, const void *ek, size_t eklen);
void gra_wb_put_log_data(GraBatch *b, const void *blob, size_t blen);
void gra_wb_set_seq(GraBatch *b, uint64_t seq);
uint32_t gra_wb_count(const GraBatch *b);
const uint8_t *gra_wb_data(const GraBatch *b, size_t *len);

/* ---------------- replay / measurement harness surface ----------------
 * Re-imagines rocksdb_replicator/performance.cpp:127-167 as a replay
 * harness: pre-encoded update streams are uploaded to HBM once (untimed),
 * then gra_replay_tick runs the apply pipeline with inputs already resident
 * in device memory. */
typedef struct {
  uint32_t shard;
  uint32_t len;    /* rep blob length */
  uint64_t off;    /* offset into the arena */
  int64_t ts;      /* Update.timestamp (ms) */
} GraUpdateDesc;

/* Pinned host allocation (for zero-copy staging by harnesses). */
int gra_pin_alloc(GraEngine *e, size_t bytes, uint8_t **ptr);
void gra_pin_free(GraEngine *e, uint8_t *ptr);

/* Upload a replay stream: arena blobs + descs, H2D once. Descs must be
 * grouped by shard within any tick window that will be replayed. Seqs are
 * assigned per shard at upload (header count field), continuing from the
 * shard's current seq. */
int gra_upload(GraEngine *e, const uint8_t *arena, size_t arena_bytes,
               const GraUpdateDesc *descs, uint64_t ndescs, GraReplay **out);
/* Same, but the blobs already live in device memory (e.g. the output tensor
 * of an RCCL all-to-all shard repartition — BASELINE config #4): zero-copy,
 * caller owns the arena (>=16 B readable slack required) and supplies each
 * batch's header record count (host can't read device headers). */
int gra_upload_dev(GraEngine *e, void *dev_arena, size_t arena_bytes,
                   const GraUpdateDesc *descs, uint64_t ndescs,
                   const uint32_t *counts, GraReplay **out);
/* Config #5: Snappy-compressed Update payloads. descs index the COMPRESSED
 * arena; ulens/counts carry per-update uncompressed size and batch record
 * count. A GPU pre-stage (k_snappy, lane-per-update) decompresses each tick
 * into a scratch arena feeding the normal decode pipeline. */
int gra_upload_snappy(GraEngine *e, const uint8_t *comp_arena,
                      size_t comp_bytes, const GraUpdateDesc *descs,
                      uint64_t ndescs, const uint32_t *ulens,
                      const uint32_t *counts, GraReplay **out);
/* Host-side Snappy codec (transport/leader side + harness). Returns
 * compressed length (0 = dst too small) / uncompressed length (UINT32_MAX =
 * corrupt). */
uint32_t gra_snappy_compress(const uint8_t *src, uint32_t slen, uint8_t *dst,
                             uint32_t dcap);
uint32_t gra_snappy_decompress(const uint8_t *src, uint32_t slen, uint8_t *dst,
                               uint32_t dcap);
void gra_replay_destroy(GraReplay *r);

/* Run one pipeline tick over descs [first, first+n): decode + emit +
 * partition-copy into the device run store. Asynchronous; gra_replay_sync
 * or gra_flush to drain. Updates applied this way are visible to gra_get /
 * gra_latest_seq like streamed ones. */
int gra_replay_tick(GraReplay *r, uint64_t first, uint64_t n);
int gra_replay_sync(GraReplay *r);
/* Pre-build + device-cache the plan for a tick window (group table, sorted
 * snappy task order) so the first tick of the window pays no allocation in
 * a timed region. Optional setup call. */
int gra_replay_prepare(GraReplay *r, uint64_t first, uint64_t n);

/* Streaming-ingest equivalent for PCIe-inclusive measurement: same tick, but
 * blobs start in the (pinned) host arena and are staged H2D inside the tick. */
int gra_replay_tick_h2d(GraReplay *r, uint64_t first, uint64_t n);

/* ---------------- stats / timing (HIP-event-measured, per kernel) -------- */
typedef struct {
  double h2d_ms, snappy_ms, decode_ms, scan_ms, emit_ms, copy_ms, runfix_ms,
      total_ms;
  uint64_t ticks, updates, records, blob_bytes, payload_bytes;
} GraStats;
void gra_stats(GraEngine *e, GraStats *out);
void gra_stats_reset(GraEngine *e);

/* ---------------- synthetic stream generator (harness) ----------------
 * Deterministic xoshiro256** streams, seed 0xR0CK5-style base + shard id
 * (SURVEY §8d). kind: 0 = uniform Put (config #2 shape), 1 = Zipf-0.99 keys
 * (config #3 shape), 2 = mixed Put/Delete/Merge 70/20/10 (config #5 shape).
 * Writes encoded update blobs into arena (cap bytes) and descs (cap n).
 * Returns GRA_OK and the consumed sizes, or GRA_FULL. Each update is one
 * record per batch, ≤50 updates per response window, mirroring
 * performance.cpp:139-142 / replicated_db.cpp:42-43. */
typedef struct {
  uint32_t nshards;
  uint32_t key_len;        /* e.g. 16 */
  uint32_t val_len;        /* e.g. 128 or 1024 */
  uint32_t kind;           /* 0 uniform put, 1 zipf, 2 mixed */
  uint64_t key_space;      /* e.g. 1<<24 */
  double zipf_s;           /* e.g. 0.99 */
  uint64_t seed;
  uint32_t compressible;   /* 1: low-entropy values (Snappy-compressible) */
  uint32_t _pad;
} GraGenOpts;
int gra_gen_stream(const GraGenOpts *g, uint64_t n_updates, uint8_t *arena,
                   size_t arena_cap, size_t *arena_used, GraUpdateDesc *descs,
                   int64_t ts);

#ifdef __cplusplus
}
#endif
#endif /* ROCKSPLICATOR_GPU_H */
