/* dev_buf.h — owning staging types of the device read paths (gra_multiget,
 * gra_scan, gra_compact, gra_shard_checksum). Both own only device and
 * pinned memory and free it in their destructors; neither is copyable. */
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

namespace gra {

/* Grow-only device buffer: the pointer and its capacity in bytes. */
template <typename T>
class DevBuf {
public:
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { release(); }

  /* True at once when the capacity suffices. Otherwise the old buffer is
   * freed (its contents are never carried over) and `need` bytes are
   * allocated — `need + need/2 + 64` with `headroom`, so the slack is paid
   * only where a reallocation happens anyway. On failure the buffer is left
   * empty and HIP's last error is cleared: out of memory is the caller's to
   * handle. */
  bool reserve_bytes(size_t need, bool headroom = false) {
    if (cap_ >= need) return true;
    release();
    size_t want = headroom ? need + need / 2 + 64 : need;
    if (hipMalloc(&p_, want) != hipSuccess) {
      (void)hipGetLastError();
      p_ = nullptr;
      return false;
    }
    cap_ = want;
    return true;
  }
  T *get() const { return p_; }
  operator T *() const { return p_; }

private:
  void release() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  T *p_ = nullptr;
  size_t cap_ = 0;
};

/* One T on the device plus its pinned host mirror. */
template <typename T>
struct DevMirror {
  T *d = nullptr, *h = nullptr;
  DevMirror() = default;
  DevMirror(const DevMirror &) = delete;
  DevMirror &operator=(const DevMirror &) = delete;
  ~DevMirror() {
    if (d) (void)hipFree(d);
    if (h) (void)hipHostFree(h);
  }
  /* both or neither */
  bool ensure() {
    if (d) return true;
    if (hipMalloc(&d, sizeof(T)) != hipSuccess) {
      (void)hipGetLastError();
      d = nullptr;
      return false;
    }
    if (hipHostMalloc(&h, sizeof(T)) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(d);
      d = h = nullptr;
      return false;
    }
    return true;
  }
};

} // namespace gra
