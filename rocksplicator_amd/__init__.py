"""rocksplicator_amd — MI355X-native replication apply path for
pinterest/rocksplicator's follower-side WriteBatch ingest.

The hot path: fbthrift ReplicateResponse payloads (rocksdb
WriteBatch rep blobs, one stream per shard) are staged into HBM and applied
by hand-written CDNA4 HIP kernels — varint record-boundary walk, prefix-sum
placement, partition-copy into per-shard device-resident runs — behind a
C-ABI (include/rocksplicator_gpu.h) that mirrors the reference's
replicator::DbWrapper seam (rocksdb_replicator/db_wrapper.h:6-15).
"""
from .ffi import (  # noqa: F401
    Batch,
    Db,
    Engine,
    Replay,
    gen_stream,
    load,
    GRA_OK,
    GRA_NOT_FOUND,
    GRA_NO_GPU,
    GRA_SCAN_DEVICE,
    GRA_SCAN_HOST,
    GRA_SCAN_DEVICE_INDEXED,
    GRA_COMPACT_DONE,
    GRA_COMPACT_NOTHING,
    GRA_COMPACT_UNSUPPORTED,
    GraCompactInfo,
    GRA_RECLAIM_DONE,
    GRA_RECLAIM_NOTHING,
    GraReclaimInfo,
    GraStoreUsage,
    StoreFullError,
    GRA_IMG_OK,
    GRA_IMG_BAD_HEADER,
    GRA_IMG_BAD_SIZE,
    GRA_IMG_BAD_RECORD,
    GRA_IMG_BAD_LAYOUT,
    GRA_IMG_BAD_ORDER,
    GRA_IMG_BAD_SUM,
    GRA_IMG_NO_INDEX,
    GraImageInfo,
    ImageRejected,
    image_check,
    MERGE_CONCAT,
    MERGE_U64ADD,
)
from .image import pack_image, unpack_image  # noqa: F401

__version__ = "0.1.0"
