/* fold.h — the merge-operand arithmetic shared by the device fold kernels
 * (scan_kernels.h, engine.hip) and a plain C++ host test
 * (scripts/test_fold_host.cpp): both compile these exact lines. The host
 * Get path keeps its own fold_value (host_store.cpp); the two must agree bit
 * for bit, which tests/test_fold_host.py and tests/test_gpu_fold.py check. */
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GRA_FOLD_HD __host__ __device__
#else
#define GRA_FOLD_HD
#endif

namespace gra {
namespace fold {

/* A gra_scan concat chain longer than this reports GRA_GET_NEEDS_HOST: one
 * lane group emits a chain entry by entry, each step behind a dependent
 * candidate load. u64add chains have no bound. */
constexpr uint32_t kFoldMaxConcatOps = 256;

/* A u64add operand or base: the first min(8, len) bytes, little-endian,
 * zero-extended. Byte loads: values sit right after the key at any byte
 * alignment, and nothing past p + len is touched. len == 0 reads nothing. */
GRA_FOLD_HD inline uint64_t load_u64le(const uint8_t *p, uint32_t len) {
  uint32_t n = len < 8 ? len : 8;
  uint64_t v = 0;
  for (uint32_t i = 0; i < n; i++) v |= (uint64_t)p[i] << (8 * i);
  return v;
}

/* the counter add: wraps at 2^64 (unsigned arithmetic) */
GRA_FOLD_HD inline uint64_t add_wrap(uint64_t acc, uint64_t v) {
  return acc + v;
}

/* the 8-byte little-endian result, byte stores (any alignment) */
GRA_FOLD_HD inline void store_u64le(uint8_t *p, uint64_t v, uint32_t n = 8) {
  for (uint32_t i = 0; i < n && i < 8; i++) p[i] = (uint8_t)(v >> (8 * i));
}

/* length of a concat fold: base (if any) and nops operands joined by ','.
 * nops >= 1. */
GRA_FOLD_HD inline uint64_t concat_len(bool have_base, uint32_t base_len,
                                       uint64_t ops_bytes, uint32_t nops) {
  return (have_base ? (uint64_t)base_len + 1 : 0) + ops_bytes + (nops - 1);
}

}  // namespace fold
}  // namespace gra
