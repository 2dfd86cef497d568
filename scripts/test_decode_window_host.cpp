/* test_decode_window_host.cpp — stand-alone driver for the windowed byte
 * source of wb_format.h (wb::WinSrc + wb::walk_src), the host half of
 * k_decode's LDS-staged parse. Plain C++ (g++, no HIP headers), built with
 * -fsanitize=address,undefined by tests/test_decode_window_host.py.
 *
 * Commands on stdin, one per line:
 *   blob <rephex>   walk the blob with plain walk_f, then through a window
 *                   of every length in {0, 1, 11, 12, 13, 14, 31, 32, 33, 48,
 *                   64, 128, len-1, len, len+1}. Each walk gets the blob in
 *                   a heap buffer of exactly len bytes and the window in one
 *                   of exactly min(win, len) bytes, so a read past either is
 *                   an AddressSanitizer report. Prints
 *                   "blob <ok> <n_records> <payload_bytes> <payload16>
 *                   <hdr_count> <hdr_seq> <recs emitted> <windows walked>
 *                   <windows that differ>"
 *   chunks          for len 0..300 and W in {16, 48, 64, 128}: the staged
 *                   chunks must cover min(len, W) bytes, fit the row and end
 *                   at most 15 B past len. Prints "chunks <violations>"
 * "-" is the empty blob. */
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../rocksplicator_amd/csrc/wb_format.h"

static bool unhex(const std::string &s, std::string *out) {
  out->clear();
  if (s == "-") return true;
  if (s.size() % 2) return false;
  auto nib = [](char c) -> int {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    return -1;
  };
  for (size_t i = 0; i < s.size(); i += 2) {
    int h = nib(s[i]), l = nib(s[i + 1]);
    if (h < 0 || l < 0) return false;
    out->push_back((char)(h * 16 + l));
  }
  return true;
}

struct Emitted {
  wb::Rec r;
  uint32_t idx;
};

/* exact-size heap copy; n == 0 still gets its own (zero-length) block */
static std::unique_ptr<uint8_t[]> exact(const uint8_t *p, size_t n) {
  std::unique_ptr<uint8_t[]> b(new uint8_t[n]);
  if (n) memcpy(b.get(), p, n);
  return b;
}

static bool same(const wb::WalkTotals &a, const std::vector<Emitted> &ea,
                 const wb::WalkTotals &b, const std::vector<Emitted> &eb) {
  if (memcmp(&a, &b, sizeof a) != 0 || ea.size() != eb.size()) return false;
  for (size_t i = 0; i < ea.size(); i++)
    if (memcmp(&ea[i].r, &eb[i].r, sizeof(wb::Rec)) != 0 ||
        ea[i].idx != eb[i].idx)
      return false;
  return true;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "blob") {
      std::string hx, raw;
      in >> hx;
      if (!unhex(hx, &raw)) {
        printf("bad hex\n");
        return 2;
      }
      const uint32_t len = (uint32_t)raw.size();
      auto rep = exact((const uint8_t *)raw.data(), len);
      std::vector<Emitted> want_recs;
      auto collect = [](std::vector<Emitted> *v) {
        return [v](const wb::Rec &r, uint32_t i) {
          Emitted e;
          memset(&e, 0, sizeof e);
          e.r = r;
          e.idx = i;
          v->push_back(e);
        };
      };
      wb::WalkTotals want = wb::walk_f(rep.get(), len, collect(&want_recs));
      std::vector<uint32_t> wins = {0, 1, 11, 12, 13, 14, 31, 32, 33, 48, 64,
                                    128, len, len + 1};
      if (len > 0) wins.push_back(len - 1);
      uint32_t differ = 0;
      for (uint32_t w : wins) {
        const uint32_t wl = w < len ? w : len;
        auto rep2 = exact((const uint8_t *)raw.data(), len);
        auto win = exact((const uint8_t *)raw.data(), wl);
        wb::WinSrc src = {win.get(), wl, rep2.get()};
        std::vector<Emitted> got_recs;
        wb::WalkTotals got = wb::walk_src(src, len, collect(&got_recs));
        if (!same(want, want_recs, got, got_recs)) differ++;
      }
      printf("blob %u %u %u %u %u %llu %zu %zu %u\n", want.ok, want.n_records,
             want.payload_bytes, want.payload16, want.hdr_count,
             (unsigned long long)want.hdr_seq, want_recs.size(), wins.size(),
             differ);
    } else if (cmd == "chunks") {
      uint32_t bad = 0;
      for (uint32_t W : {16u, 48u, 64u, 128u})
        for (uint32_t len = 0; len <= 300; len++) {
          const uint32_t staged = 16 * wb::win_chunks(len, W);
          const uint32_t need = len < W ? len : W;
          if (wb::win_bytes(len, W) != need) bad++;
          if (staged < need) bad++;      /* covers min(len, W) */
          if (staged > W) bad++;         /* stays inside the row */
          if (staged > len + 15) bad++;  /* at most 15 B past the blob */
          if (staged >= need + 16) bad++; /* no chunk starts past the end */
        }
      printf("chunks %u\n", bad);
    } else if (!cmd.empty()) {
      printf("unknown command\n");
      return 2;
    }
  }
  return 0;
}
