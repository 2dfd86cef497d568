/* test_snappy_bounds.cpp — stand-alone driver for snp::decompress, meant to
 * be built with g++ -fsanitize=address,undefined (no HIP headers).
 *
 * stdin, one stream per line:  <ulen_meta> <streamhex>   ("-" = empty)
 * Each stream is copied into a heap buffer of exactly its own size and
 * decompressed into a fresh heap buffer of exactly ulen_meta + 16 bytes (the
 * slot plus the slack that the engine gives it), so a read past the stream
 * or a write past the slot is an ASan report, not a silent pass.
 * stdout, one line per stream:  "ok <len> <plainhex>"  or  "bad".
 *
 * This is the host build: the byte loops, not the device's chunked copies.
 * Built and driven by tests/test_snappy_cases_host.py. */
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "../rocksplicator_amd/csrc/snappy.h"

static int nib(char c) {
  if (c >= '0' && c <= '9') return c - '0';
  if (c >= 'a' && c <= 'f') return c - 'a' + 10;
  return -1;
}

int main() {
  std::string line;
  static const char *d = "0123456789abcdef";
  while (std::getline(std::cin, line)) {
    std::istringstream is(line);
    uint32_t ulen;
    std::string hx;
    if (!(is >> ulen >> hx)) return 2;
    if (hx == "-") hx.clear();
    if (hx.size() % 2) return 2;
    uint32_t slen = (uint32_t)(hx.size() / 2);
    uint8_t *src = new uint8_t[slen ? slen : 1];
    for (uint32_t i = 0; i < slen; i++) {
      int h = nib(hx[2 * i]), l = nib(hx[2 * i + 1]);
      if (h < 0 || l < 0) return 2;
      src[i] = (uint8_t)(h * 16 + l);
    }
    uint8_t *dst = new uint8_t[(size_t)ulen + 16];
    std::memset(dst, 0xA5, (size_t)ulen + 16);
    uint32_t r = snp::decompress(src, slen, dst, ulen);
    if (r == UINT32_MAX) {
      std::puts("bad");
    } else {
      std::string out;
      for (uint32_t i = 0; i < r; i++) {
        out.push_back(d[dst[i] >> 4]);
        out.push_back(d[dst[i] & 15]);
      }
      std::printf("ok %u %s\n", r, r ? out.c_str() : "-");
    }
    /* the 16 bytes of slack stay untouched on the host (byte loops) */
    for (uint32_t i = 0; i < 16; i++)
      if (dst[(size_t)ulen + i] != 0xA5) return 3;
    delete[] src;
    delete[] dst;
  }
  return 0;
}
