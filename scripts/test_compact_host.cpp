/* test_compact_host.cpp — stand-alone driver for gra::run_compact, the host
 * restatement of gra_compact. Plain C++ (g++, no HIP headers), built with
 * -fsanitize=address,undefined by tests/test_compact_host.py.
 *
 * Commands on stdin, one per line:
 *   run <rephex>                        apply a WriteBatch rep as the next run
 *                                       (host_build_run, consecutive base seqs)
 *   compact <k> <merge>                 replace the first k runs (0 = all) by
 *                                       run_compact's output; prints
 *                                       "compact <rc> <entries> <payload_bytes>
 *                                       <base_seq> <last_seq> <sorted>"
 *   dump <i>                            the records of run i, one
 *                                       "rec <seq> <type> <flags> <kv_off>
 *                                       <kpref> <keyhex> <valhex>" line each,
 *                                       then "end"
 *   get <keyhex> <merge>                "get <rc> <valhex>"
 *   scan <lo> <hi> <max> <cap> <merge>  as scripts/test_host_scan.cpp
 * Hex fields use "-" for the empty string; scan's hi "*" = no upper bound. */
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

static std::string hex(const void *p_, size_t n) {
  if (n == 0) return "-";
  const uint8_t *p = (const uint8_t *)p_;
  static const char *d = "0123456789abcdef";
  std::string s;
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
    } else if (cmd == "compact") {
      size_t k;
      int merge_op;
      if (!(is >> k >> merge_op) || k > runs.size()) {
        fprintf(stderr, "bad compact line\n");
        return 2;
      }
      if (k == 0) k = runs.size();
      std::vector<std::shared_ptr<gra::Run>> prefix(runs.begin(),
                                                    runs.begin() + k);
      auto out = std::make_shared<gra::Run>();
      int rc = gra::run_compact(prefix, merge_op, out.get());
      printf("compact %d %u %u %llu %llu %d\n", rc, out->n_entries,
             out->payload_bytes, (unsigned long long)out->base_seq,
             (unsigned long long)out->last_seq, out->sorted ? 1 : 0);
      if (rc == 0) {
        runs.erase(runs.begin(), runs.begin() + k);
        runs.insert(runs.begin(), std::move(out));
      }
    } else if (cmd == "dump") {
      size_t i;
      if (!(is >> i) || i >= runs.size()) {
        fprintf(stderr, "bad dump line\n");
        return 2;
      }
      const gra::Run &r = *runs[i];
      const wb::RecHdr *h = (const wb::RecHdr *)r.hdrs_data();
      const uint8_t *pay = r.payload_data();
      for (uint32_t j = 0; j < r.n_entries; j++) {
        if ((uint64_t)h[j].kv_off + h[j].key_len + h[j].val_len >
            r.payload_bytes) {
          fprintf(stderr, "record %u leaves the payload\n", j);
          return 3;
        }
        printf("rec %llu %u %u %u %u %s %s\n", (unsigned long long)h[j].seq,
               h[j].type, h[j].flags, h[j].kv_off, h[j].kpref,
               hex(pay + h[j].kv_off, h[j].key_len).c_str(),
               hex(pay + h[j].kv_off + h[j].key_len, h[j].val_len).c_str());
      }
      printf("end\n");
    } else if (cmd == "get") {
      std::string ks, key, val;
      int merge_op;
      if (!(is >> ks >> merge_op) || !unhex(ks, &key)) {
        fprintf(stderr, "bad get line\n");
        return 2;
      }
      int rc = gra::run_get(runs, key.data(), key.size(), merge_op, &val);
      printf("get %d %s\n", rc, hex(val.data(), rc == 0 ? val.size() : 0).c_str());
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
