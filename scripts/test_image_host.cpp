/* test_image_host.cpp — stand-alone driver for the host side of shard
 * images: gra::run_compact -> gra::image_from_run -> gra::check_image. Plain
 * C++ (g++, no HIP headers), built with -fsanitize=address,undefined by
 * tests/test_image_host.py.
 *
 * Commands on stdin, one per line:
 *   run <rephex>          apply a WriteBatch rep as the next run
 *                         (host_build_run, consecutive base seqs)
 *   reset                 drop the runs, seqs start at 1 again
 *   image <merge>         run_compact over all runs, image_from_run with
 *                         last_seq = the last run's; prints
 *                         "image <rc> <hex>" (rc 1: unsupported, hex "-")
 *   check <hex>           check_image over a heap copy of exactly the given
 *                         bytes (so the sanitizer sees any read outside
 *                         them); prints "check <reason> <bad_index> <n>
 *                         <payload_bytes> <image_bytes> <last_seq>
 *                         <content_sum>", bad_index -1 = none
 * Hex fields use "-" for the empty string. */
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "../rocksplicator_amd/csrc/host_store.h"

static bool unhex(const std::string &s, std::string *out) {
  out->clear();
  if (s == "-") return true;
  if (s.size() % 2) return false;
  auto nib = [](char c) -> int {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
  };
  out->reserve(s.size() / 2);
  for (size_t i = 0; i < s.size(); i += 2) {
    int h = nib(s[i]), l = nib(s[i + 1]);
    if (h < 0 || l < 0) return false;
    out->push_back((char)(h * 16 + l));
  }
  return true;
}

static std::string hex(const void *p_, size_t n) {
  if (n == 0) return "-";
  const uint8_t *p = (const uint8_t *)p_;
  static const char *d = "0123456789abcdef";
  std::string s;
  s.reserve(2 * n);
  for (size_t i = 0; i < n; i++) {
    s.push_back(d[p[i] >> 4]);
    s.push_back(d[p[i] & 15]);
  }
  return s;
}

int main() {
  std::vector<std::shared_ptr<gra::Run>> runs;
  uint64_t next_seq = 1;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream is(line);
    std::string cmd;
    if (!(is >> cmd)) continue;
    if (cmd == "run") {
      std::string h, rep;
      if (!(is >> h) || !unhex(h, &rep)) {
        fprintf(stderr, "bad run line\n");
        return 2;
      }
      auto r = std::make_shared<gra::Run>();
      if (!gra::host_build_run((const uint8_t *)rep.data(), rep.size(),
                               next_seq, r.get())) {
        fprintf(stderr, "corrupt rep\n");
        return 2;
      }
      next_seq = r->last_seq + 1;
      runs.push_back(std::move(r));
    } else if (cmd == "reset") {
      runs.clear();
      next_seq = 1;
    } else if (cmd == "image") {
      int merge_op;
      if (!(is >> merge_op)) {
        fprintf(stderr, "bad image line\n");
        return 2;
      }
      gra::Run out;
      int rc = gra::run_compact(runs, merge_op, &out);
      std::vector<uint8_t> img;
      if (rc == 0)
        gra::image_from_run(out, next_seq - 1, (uint32_t)merge_op, &img);
      printf("image %d %s\n", rc, hex(img.data(), img.size()).c_str());
    } else if (cmd == "check") {
      std::string h, bytes;
      if (!(is >> h) || !unhex(h, &bytes)) {
        fprintf(stderr, "bad check line\n");
        return 2;
      }
      /* an exact-size heap block, at an odd address inside it for every
       * second call: the checker may assume no alignment */
      static unsigned calls = 0;
      const size_t shift = calls++ & 1;
      uint8_t *blk = new uint8_t[bytes.size() + shift + (bytes.empty() ? 1 : 0)];
      uint8_t *p = blk + shift;
      memcpy(p, bytes.data(), bytes.size());
      /* with shift == 1 the block ends exactly at the image's end too */
      gra::ImageInfo ii;
      uint32_t reason = gra::check_image(p, bytes.size(), &ii);
      printf("check %u %lld %llu %llu %llu %llu %llu\n", reason,
             ii.bad_index == gra::kImgNoIndex ? -1ll : (long long)ii.bad_index,
             (unsigned long long)ii.n_entries,
             (unsigned long long)ii.payload_bytes,
             (unsigned long long)ii.image_bytes,
             (unsigned long long)ii.last_seq,
             (unsigned long long)ii.content_sum);
      delete[] blk;
    } else {
      fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
