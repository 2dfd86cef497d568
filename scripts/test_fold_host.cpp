/* test_fold_host.cpp — stand-alone host driver for csrc/fold.h, the
 * merge-operand arithmetic the device fold kernels compile too. Built by
 * tests/test_fold_host.py with g++ -fsanitize=address,undefined and driven
 * over stdin; every operand is placed so that it ends exactly where its heap
 * block does, so a read past p + len is an ASan report.
 *
 *   sizeof                      -> "sizeof <GraEngineOpts> <offsetof fold_on_device>"
 *   loads                       -> "load <len> <mis> <hex u64>" for len 0..12,
 *                                  mis 0..15; operand byte i = 0xA1 + 17 i + mis
 *   add <hex a> <hex b>         -> "add <hex u64>"
 *   fold <mis> <base|*> <op>... -> "fold <16 hex digits: 8 result bytes> <concat_len>"
 *                                  operands oldest to newest, hex, "-" = empty,
 *                                  base "*" = none */
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../include/rocksplicator_gpu.h"
#include "../rocksplicator_amd/csrc/fold.h"

namespace {

/* an operand of `len` bytes at misalignment `mis` (malloc returns 16-B
 * aligned blocks) whose last byte is the block's last byte */
struct Guarded {
  uint8_t *block;
  uint8_t *p;
  Guarded(const std::vector<uint8_t> &bytes, uint32_t mis) {
    block = (uint8_t *)malloc(mis + bytes.size()); /* 0 bytes: all redzone */
    p = block + mis;
    if (!bytes.empty()) memcpy(p, bytes.data(), bytes.size());
  }
  ~Guarded() { free(block); }
  Guarded(const Guarded &) = delete;
};

std::vector<uint8_t> unhex(const std::string &s) {
  std::vector<uint8_t> out;
  if (s == "-") return out;
  for (size_t i = 0; i + 1 < s.size(); i += 2)
    out.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
  return out;
}

}  // namespace

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "sizeof") {
      printf("sizeof %zu %zu\n", sizeof(GraEngineOpts),
             offsetof(GraEngineOpts, fold_on_device));
    } else if (cmd == "loads") {
      for (uint32_t len = 0; len <= 12; len++)
        for (uint32_t mis = 0; mis < 16; mis++) {
          std::vector<uint8_t> b(len);
          for (uint32_t i = 0; i < len; i++)
            b[i] = (uint8_t)(0xA1 + 17 * i + mis);
          Guarded g(b, mis);
          printf("load %u %u %016llx\n", len, mis,
                 (unsigned long long)gra::fold::load_u64le(g.p, len));
        }
    } else if (cmd == "add") {
      std::string a, b;
      in >> a >> b;
      printf("add %016llx\n",
             (unsigned long long)gra::fold::add_wrap(
                 strtoull(a.c_str(), nullptr, 16),
                 strtoull(b.c_str(), nullptr, 16)));
    } else if (cmd == "fold") {
      uint32_t mis;
      std::string base, op;
      in >> mis >> base;
      bool have_base = base != "*";
      uint64_t acc = 0, ops_bytes = 0;
      uint32_t nops = 0, base_len = 0;
      if (have_base) {
        std::vector<uint8_t> b = unhex(base);
        Guarded g(b, mis);
        base_len = (uint32_t)b.size();
        acc = gra::fold::load_u64le(g.p, base_len);
      }
      while (in >> op) {
        std::vector<uint8_t> b = unhex(op);
        Guarded g(b, (mis + nops) & 15);
        acc = gra::fold::add_wrap(
            acc, gra::fold::load_u64le(g.p, (uint32_t)b.size()));
        ops_bytes += b.size();
        nops++;
      }
      /* the result store, at a misaligned guarded destination */
      Guarded out(std::vector<uint8_t>(8, 0), mis);
      gra::fold::store_u64le(out.p, acc);
      printf("fold ");
      for (int i = 0; i < 8; i++) printf("%02x", out.p[i]);
      printf(" %llu\n", (unsigned long long)gra::fold::concat_len(
                            have_base, base_len, ops_bytes, nops));
    } else if (!cmd.empty()) {
      fprintf(stderr, "unknown command: %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
