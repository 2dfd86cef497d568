/* micro_decode.hip — A/B decode-variant microbench for k_decode's blob walk.
 * Every variant runs the engine's own parser (wb::walk_src from
 * ../rocksplicator_amd/csrc/wb_format.h) lane-per-update over a synthetic
 * blob arena and differs only in where the bytes come from:
 *   global            walk the blob in global memory (the parent's k_decode)
 *   win/wW/pP/u       head of the blob staged into a per-lane LDS row of
 *                     W (+4 if P) bytes by unaligned 16 B loads from the
 *                     blob's first byte; past the window the walk reads
 *                     global memory (wb::WinSrc, the engine's kernel)
 *   win/wW/p1/a       same, chunk loads aligned down to 16 B (one more chunk
 *                     when the blob starts mid-chunk; reads below the blob)
 *   restage/wW        a walk that leaves the window re-stages W bytes at the
 *                     new position instead of falling back to global bytes
 *   win/w48/p1/u rec16
 *                     the win/w48/p1/u parse writing one 16 B wb::EmitRec
 *                     per update (wb::emit_pack, the engine's k_decode) where
 *                     every other row writes WalkTotals + two cached Recs
 * Task mixes: 0 headline (16 B key, 1 KB value), 1 128 B values, 2 30 B
 * deletes, 3 eight records x 100 B, 4 cf-prefixed 1 KB puts, 5 two records
 * x 500 B.
 * Every row checks its WalkTotals and cached Recs against the host walk_f
 * (ok=1); the rec16 row checks every EmitRec against the pack of the host
 * walk and unpacks the one-record ones back to the host's Rec. The block
 * scan k_decode fuses is left out of every variant alike.
 * Args: [updates=819200] [mix=-1 (all)].
 * Build: hipcc --offload-arch=gfx950 -O3 scripts/micro_decode.hip -o build/micro_decode
 */
#include <hip/hip_runtime.h>

#define WB_UNALIGNED_OK 1 /* as engine.hip */

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../rocksplicator_amd/csrc/wb_format.h"

#define CHECK(x)                                                      \
  do {                                                                \
    hipError_t e = (x);                                               \
    if (e != hipSuccess) {                                            \
      printf("ERR %s: %s\n", #x, hipGetErrorString(e));               \
      exit(1);                                                        \
    }                                                                 \
  } while (0)

struct Desc { /* gra::UpdDesc */
  uint64_t off, base_seq;
  uint32_t len, shard;
};
constexpr uint32_t kRecCache = 2;

/* window at an arbitrary byte alignment (the aligned-down variant's row
 * holds the blob from byte `shift` on): byte composition only */
struct ShiftWinSrc {
  const uint8_t *win;
  uint32_t win_len;
  const uint8_t *rep;
  __device__ uint8_t byte(uint32_t pos) const {
    return pos < win_len ? win[pos] : rep[pos];
  }
  __device__ uint32_t u32(uint32_t pos) const {
    return (uint32_t)byte(pos) | ((uint32_t)byte(pos + 1) << 8) |
           ((uint32_t)byte(pos + 2) << 16) | ((uint32_t)byte(pos + 3) << 24);
  }
  __device__ uint64_t u64(uint32_t pos) const {
    return (uint64_t)u32(pos) | ((uint64_t)u32(pos + 4) << 32);
  }
};

/* re-staging window: holds rep[base, base + n); a read outside it loads the
 * W bytes at that position (chunks that start before the blob's end) */
template <int W>
struct RestageSrc {
  uint32_t *row;
  const uint8_t *rep;
  uint32_t len;
  mutable uint32_t base, n;
  __device__ void stage(uint32_t pos) const {
    base = pos;
    n = len - pos < (uint32_t)W ? len - pos : (uint32_t)W;
    const uint32_t nch = (n + 15u) / 16u;
    uint4 c[W / 16];
#pragma unroll
    for (uint32_t k = 0; k < W / 16; k++)
      if (k < nch) c[k] = *(const uint4 *)(rep + pos + 16 * k);
#pragma unroll
    for (uint32_t k = 0; k < W / 16; k++)
      if (k < nch) {
        row[4 * k + 0] = c[k].x;
        row[4 * k + 1] = c[k].y;
        row[4 * k + 2] = c[k].z;
        row[4 * k + 3] = c[k].w;
      }
  }
  __device__ uint8_t byte(uint32_t pos) const {
    if (pos - base >= n) stage(pos);
    return ((const uint8_t *)row)[pos - base];
  }
  __device__ uint32_t u32(uint32_t pos) const {
    return (uint32_t)byte(pos) | ((uint32_t)byte(pos + 1) << 8) |
           ((uint32_t)byte(pos + 2) << 16) | ((uint32_t)byte(pos + 3) << 24);
  }
  __device__ uint64_t u64(uint32_t pos) const {
    return (uint64_t)u32(pos) | ((uint64_t)u32(pos + 4) << 32);
  }
};

enum Mode { kGlobal = 0, kWinUnaligned = 1, kWinAligned = 2, kRestage = 3 };

template <int MODE, int W, int PAD>
__global__ void __launch_bounds__(256) k_dec(const uint8_t *__restrict__ blobs,
                                             const Desc *__restrict__ descs,
                                             uint32_t n,
                                             wb::WalkTotals *__restrict__ totals,
                                             wb::Rec *__restrict__ reccache) {
  /* aligned-down rows hold one more chunk */
  constexpr uint32_t kRow = (W + (MODE == kWinAligned ? 16 : 0) + PAD) / 4;
  __shared__ uint32_t stage[MODE == kGlobal ? 1 : 256 * kRow];
  uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  Desc d = descs[i];
  const uint8_t *rep = blobs + d.off;
  wb::Rec *cache = reccache + (size_t)i * kRecCache;
  auto emit = [&](const wb::Rec &r, uint32_t idx) {
    if (idx < kRecCache) cache[idx] = r;
  };
  uint32_t *row = stage + threadIdx.x * kRow;
  wb::WalkTotals t;
  if (MODE == kGlobal) {
    t = wb::walk_f(rep, d.len, emit);
  } else if (MODE == kWinUnaligned) {
    const uint32_t nch = wb::win_chunks(d.len, W);
    uint4 c[W / 16];
#pragma unroll
    for (uint32_t k = 0; k < W / 16; k++)
      if (k < nch) c[k] = *(const uint4 *)(rep + 16 * k);
#pragma unroll
    for (uint32_t k = 0; k < W / 16; k++)
      if (k < nch) {
        row[4 * k + 0] = c[k].x;
        row[4 * k + 1] = c[k].y;
        row[4 * k + 2] = c[k].z;
        row[4 * k + 3] = c[k].w;
      }
    wb::WinSrc src = {(const uint8_t *)row, wb::win_bytes(d.len, W), rep};
    t = wb::walk_src(src, d.len, emit);
  } else if (MODE == kWinAligned) {
    const uint32_t shift = (uint32_t)((uintptr_t)rep & 15u);
    const uint8_t *abase = rep - shift;
    const uint32_t wl = wb::win_bytes(d.len, W);
    const uint32_t nch = (shift + wl + 15u) / 16u; /* <= W/16 + 1 */
    uint4 c[W / 16 + 1];
#pragma unroll
    for (uint32_t k = 0; k < W / 16 + 1; k++)
      if (k < nch) c[k] = *(const uint4 *)(abase + 16 * k);
#pragma unroll
    for (uint32_t k = 0; k < W / 16 + 1; k++)
      if (k < nch) {
        row[4 * k + 0] = c[k].x;
        row[4 * k + 1] = c[k].y;
        row[4 * k + 2] = c[k].z;
        row[4 * k + 3] = c[k].w;
      }
    ShiftWinSrc src = {(const uint8_t *)row + shift, wl, rep};
    t = wb::walk_src(src, d.len, emit);
  } else {
    RestageSrc<W> src = {row, rep, d.len, 0, 0};
    t = wb::walk_src(src, d.len, emit);
  }
  totals[i] = t;
}

/* The engine's k_decode writer: the window parse of win/wW/p1/u, totals kept
 * in registers, one 16 B wb::EmitRec per update through the shared
 * wb::emit_pack instead of WalkTotals + two cached Recs (80 B). */
template <int W, int PAD>
__global__ void __launch_bounds__(256) k_dec16(const uint8_t *__restrict__ blobs,
                                               const Desc *__restrict__ descs,
                                               uint32_t n,
                                               wb::EmitRec *__restrict__ out) {
  constexpr uint32_t kRow = (W + PAD) / 4;
  __shared__ uint32_t stage[256 * kRow];
  uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  Desc d = descs[i];
  const uint8_t *rep = blobs + d.off;
  uint32_t *row = stage + threadIdx.x * kRow;
  const uint32_t nch = wb::win_chunks(d.len, W);
  uint4 c[W / 16];
#pragma unroll
  for (uint32_t k = 0; k < W / 16; k++)
    if (k < nch) c[k] = *(const uint4 *)(rep + 16 * k);
#pragma unroll
  for (uint32_t k = 0; k < W / 16; k++)
    if (k < nch) {
      row[4 * k + 0] = c[k].x;
      row[4 * k + 1] = c[k].y;
      row[4 * k + 2] = c[k].z;
      row[4 * k + 3] = c[k].w;
    }
  wb::WinSrc src = {(const uint8_t *)row, wb::win_bytes(d.len, W), rep};
  wb::Rec first = {};
  wb::WalkTotals t = wb::walk_src(src, d.len, [&](const wb::Rec &r, uint32_t idx) {
    if (idx == 0) first = r;
  });
  out[i] = wb::emit_pack(t, first);
}

/* ---- host-side blob building ---- */
static void put_varint(std::vector<uint8_t> &b, uint32_t v) {
  while (v >= 0x80) {
    b.push_back((uint8_t)(v | 0x80));
    v >>= 7;
  }
  b.push_back((uint8_t)v);
}
static void put_bytes(std::vector<uint8_t> &b, uint32_t n, uint32_t salt) {
  for (uint32_t i = 0; i < n; i++) b.push_back((uint8_t)(i * 131 + salt * 17 + 7));
}
static void header(std::vector<uint8_t> &b, uint64_t seq, uint32_t count) {
  for (int i = 0; i < 8; i++) b.push_back((uint8_t)(seq >> (8 * i)));
  for (int i = 0; i < 4; i++) b.push_back((uint8_t)(count >> (8 * i)));
}
static void one_blob(std::vector<uint8_t> &b, int mix, uint32_t i) {
  switch (mix) {
    case 0: case 1: { /* one Put, 16 B key, 1 KB / 128 B value */
      header(b, i, 1);
      b.push_back(wb::kValue);
      put_varint(b, 16); put_bytes(b, 16, i);
      uint32_t vl = mix == 0 ? 1024 : 128;
      put_varint(b, vl); put_bytes(b, vl, i);
      break;
    }
    case 2: /* 30 B delete */
      header(b, i, 1);
      b.push_back(wb::kDeletion);
      put_varint(b, 16); put_bytes(b, 16, i);
      break;
    case 3: /* 8 records x 100 B */
      header(b, i, 8);
      for (uint32_t r = 0; r < 8; r++) {
        b.push_back(r % 3 == 2 ? wb::kMerge : wb::kValue);
        put_varint(b, 16); put_bytes(b, 16, i + r);
        put_varint(b, 81); put_bytes(b, 81, i + r);
      }
      break;
    case 4: /* cf-prefixed Put, 1- to 5-byte cf varint */
      header(b, i, 1);
      b.push_back(wb::kCfValue);
      put_varint(b, 1u << (7 * (i % 5)));
      put_varint(b, 16); put_bytes(b, 16, i);
      put_varint(b, 1024); put_bytes(b, 1024, i);
      break;
    default: /* two records per batch, 16 B keys, 500 B values */
      header(b, i, 2);
      for (uint32_t r = 0; r < 2; r++) {
        b.push_back(wb::kValue);
        put_varint(b, 16); put_bytes(b, 16, i + r);
        put_varint(b, 500); put_bytes(b, 500, i + r);
      }
      break;
  }
}

struct HostRef {
  wb::WalkTotals t;
  wb::Rec rec[kRecCache];
};

int main(int argc, char **argv) {
  uint32_t n = argc > 1 ? atoi(argv[1]) : 819200;
  int only = argc > 2 ? atoi(argv[2]) : -1;
  const char *mix_name[6] = {"headline 16B/1KB", "128 B values", "30 B deletes",
                             "8 records x 100 B", "cf-prefixed 1KB",
                             "2 records x 500 B"};
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  for (int mix = 0; mix < 6; mix++) {
    if (only >= 0 && mix != only) continue;
    std::vector<uint8_t> arena;
    std::vector<Desc> descs(n);
    for (uint32_t i = 0; i < n; i++) {
      uint64_t off = arena.size();
      one_blob(arena, mix, i);
      descs[i] = {off, 1 + i, (uint32_t)(arena.size() - off), i & 1023u};
    }
    std::vector<HostRef> ref(n);
    for (uint32_t i = 0; i < n; i++) {
      memset(&ref[i], 0, sizeof(HostRef));
      HostRef *h = &ref[i];
      h->t = wb::walk_f(arena.data() + descs[i].off, descs[i].len,
                        [h](const wb::Rec &r, uint32_t idx) {
                          if (idx < kRecCache) h->rec[idx] = r;
                        });
    }
    uint8_t *d_blobs;
    Desc *d_descs;
    wb::WalkTotals *d_totals;
    wb::Rec *d_cache;
    wb::EmitRec *d_emit;
    CHECK(hipMalloc(&d_emit, (size_t)n * sizeof(wb::EmitRec)));
    CHECK(hipMalloc(&d_blobs, arena.size() + 16));
    CHECK(hipMalloc(&d_descs, (size_t)n * sizeof(Desc)));
    CHECK(hipMalloc(&d_totals, (size_t)n * sizeof(wb::WalkTotals)));
    CHECK(hipMalloc(&d_cache, (size_t)n * kRecCache * sizeof(wb::Rec)));
    CHECK(hipMemcpy(d_blobs, arena.data(), arena.size(), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_descs, descs.data(), (size_t)n * sizeof(Desc),
                    hipMemcpyHostToDevice));
    std::vector<wb::WalkTotals> got_t(n);
    std::vector<wb::Rec> got_r((size_t)n * kRecCache);
    printf("## mix %d: %s, %u updates, %.1f MB arena\n", mix, mix_name[mix], n,
           arena.size() / 1e6);

    auto run = [&](const char *name, auto kern) {
      CHECK(hipMemset(d_totals, 0xEE, (size_t)n * sizeof(wb::WalkTotals)));
      CHECK(hipMemset(d_cache, 0, (size_t)n * kRecCache * sizeof(wb::Rec)));
      kern(); /* warmup + correctness */
      CHECK(hipMemcpy(got_t.data(), d_totals, (size_t)n * sizeof(wb::WalkTotals),
                      hipMemcpyDeviceToHost));
      CHECK(hipMemcpy(got_r.data(), d_cache,
                      (size_t)n * kRecCache * sizeof(wb::Rec),
                      hipMemcpyDeviceToHost));
      bool ok = true;
      for (uint32_t i = 0; i < n && ok; i++) {
        ok = memcmp(&got_t[i], &ref[i].t, sizeof(wb::WalkTotals)) == 0 &&
             memcmp(&got_r[(size_t)i * kRecCache], ref[i].rec,
                    sizeof(ref[i].rec)) == 0;
      }
      CHECK(hipEventRecord(e0));
      for (int i = 0; i < 20; i++) kern();
      CHECK(hipEventRecord(e1));
      CHECK(hipEventSynchronize(e1));
      float ms;
      CHECK(hipEventElapsedTime(&ms, e0, e1));
      printf("%-18s ok=%d  %7.1f us/launch  %6.2f G upd/s\n", name, ok,
             ms * 1000 / 20, n * 20.0 / (ms * 1e-3) / 1e9);
    };
    /* the 16 B writer: every EmitRec equals the pack of the host walk, and
     * a kind-1 record unpacks to the host walk's first Rec */
    std::vector<wb::EmitRec> got_e(n);
    auto run16 = [&](const char *name, auto kern) {
      CHECK(hipMemset(d_emit, 0xEE, (size_t)n * sizeof(wb::EmitRec)));
      kern(); /* warmup + correctness */
      CHECK(hipMemcpy(got_e.data(), d_emit, (size_t)n * sizeof(wb::EmitRec),
                      hipMemcpyDeviceToHost));
      bool ok = true;
      for (uint32_t i = 0; i < n && ok; i++) {
        wb::EmitRec want = wb::emit_pack(ref[i].t, ref[i].rec[0]);
        ok = memcmp(&got_e[i], &want, sizeof want) == 0;
        if (ok && got_e[i].kind == wb::kEmitOne) {
          wb::Rec back = wb::emit_unpack(got_e[i]);
          ok = memcmp(&back, &ref[i].rec[0], sizeof back) == 0;
        }
      }
      CHECK(hipEventRecord(e0));
      for (int i = 0; i < 20; i++) kern();
      CHECK(hipEventRecord(e1));
      CHECK(hipEventSynchronize(e1));
      float ms;
      CHECK(hipEventElapsedTime(&ms, e0, e1));
      printf("%-18s ok=%d  %7.1f us/launch  %6.2f G upd/s\n", name, ok,
             ms * 1000 / 20, n * 20.0 / (ms * 1e-3) / 1e9);
    };
    dim3 grid((n + 255) / 256), blk(256);
#define RUND(NAME, MODE, W, PAD) run(NAME, [&] { \
    hipLaunchKernelGGL((k_dec<MODE, W, PAD>), grid, blk, 0, 0, d_blobs, d_descs, n, d_totals, d_cache); })
    RUND("global", kGlobal, 16, 0);
    RUND("win/w48/p1/u", kWinUnaligned, 48, 4);
    run16("win/w48/p1/u rec16", [&] {
      hipLaunchKernelGGL((k_dec16<48, 4>), grid, blk, 0, 0, d_blobs, d_descs, n,
                         d_emit);
    });
    RUND("win/w48/p1/u", kWinUnaligned, 48, 4); /* again, beside rec16 */
    RUND("win/w64/p1/u", kWinUnaligned, 64, 4);
    RUND("win/w128/p1/u", kWinUnaligned, 128, 4);
    RUND("win/w48/p0/u", kWinUnaligned, 48, 0);
    RUND("win/w64/p0/u", kWinUnaligned, 64, 0);
    RUND("win/w48/p1/a", kWinAligned, 48, 4);
    RUND("win/w64/p1/a", kWinAligned, 64, 4);
    RUND("restage/w48", kRestage, 48, 4);
    RUND("restage/w64", kRestage, 64, 4);
    RUND("global", kGlobal, 16, 0); /* again: drift across the block */
    CHECK(hipFree(d_blobs));
    CHECK(hipFree(d_descs));
    CHECK(hipFree(d_totals));
    CHECK(hipFree(d_cache));
    CHECK(hipFree(d_emit));
  }
  return 0;
}
