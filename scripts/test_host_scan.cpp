/* test_host_scan.cpp — stand-alone driver for gra::run_scan, the host side
 * of gra_scan. Plain C++ (g++, no HIP headers), so it also serves as the
 * binary to build with -fsanitize=address,undefined.
 *
 * Commands on stdin, one per line:
 *   run <rephex>                        apply a WriteBatch rep as the next run
 *                                       (host_build_run, consecutive base seqs)
 *   scan <lo> <hi> <max> <cap> <merge>  lo/hi are hex; "-" = empty key,
 *                                       hi "*" = no upper bound
 * Every scan prints "rc <rc> n <n> more <0|1>", one "<keyhex> <valhex>" line
 * per entry ("-" = empty) and "end".
 *
 * Built and driven by tests/test_scan_host.py. */
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
  for (size_t i = 0; i < s.size(); i += 2) {
    int h = nib(s[i]), l = nib(s[i + 1]);
    if (h < 0 || l < 0) return false;
    out->push_back((char)(h * 16 + l));
  }
  return true;
}

static std::string hex(const char *p, size_t n) {
  if (n == 0) return "-";
  static const char *d = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; i++) {
    s.push_back(d[(uint8_t)p[i] >> 4]);
    s.push_back(d[(uint8_t)p[i] & 15]);
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
    } else if (cmd == "scan") {
      std::string los, his, lo, hi;
      unsigned long long max_entries, cap;
      int merge_op;
      if (!(is >> los >> his >> max_entries >> cap >> merge_op) ||
          !unhex(los, &lo) || (his != "*" && !unhex(his, &hi))) {
        fprintf(stderr, "bad scan line\n");
        return 2;
      }
      gra::ScanResult res;
      int rc = gra::run_scan(runs, lo.data(), lo.size(),
                             his == "*" ? nullptr : hi.data(), hi.size(),
                             merge_op, (uint32_t)max_entries, (size_t)cap,
                             &res);
      printf("rc %d n %zu more %d\n", rc, res.items.size(), res.more ? 1 : 0);
      for (const auto &it : res.items)
        printf("%s %s\n", hex(res.buf.data() + it.key_off, it.key_len).c_str(),
               hex(res.buf.data() + it.val_off, it.val_len).c_str());
      printf("end\n");
    } else {
      fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
