/* test_settle_host.cpp — stand-alone driver for gra::settle_group_locked, the
 * ingest rule (what a finished tick leaves of one shard group), and
 * gra::roll_back_locked beneath it. Plain C++ (g++, no HIP headers), built
 * with -fsanitize=address,undefined by tests/test_settle_host.py. The
 * validity bytes and record counts of a group sit in heap arrays of exactly
 * n_upds elements, so a read past either is a sanitizer report.
 *
 * Input on stdin, any number of scenarios:
 *   scenario <nshards>
 *   <durable_seq> <next_seq> <poisoned> <nlog>     per shard, followed by
 *   <base_seq> <count> <rep_bytes>                 its nlog retained batches
 * then operations until the next `scenario` or the end of input:
 *   group <shard> <base_seq> <last_seq> <n_entries> <n_upds> <has_ok>
 *   <count> x n_upds
 *   <ok> x n_upds                                  only when has_ok is 1
 *   submit <shard> <count> <rep_bytes>   a batch accepted at next_seq: what
 *                                        gra_handle_replicate_response does
 *   clear <shard>                        its failure report: poisoned = false
 * Output per operation:
 *   K <n_entries> <last_seq> <whole>     the keep (group only)
 *   S <shard> <durable_seq> <next_seq> <poisoned> <failures> <log entries>
 *     <log_used>                         one line per shard, all shards */
#include <cstdio>
#include <iostream>
#include <memory>
#include <string>

#include "../rocksplicator_amd/csrc/host_store.h"

static int bad(const char *what) {
  fprintf(stderr, "bad %s line\n", what);
  return 2;
}

int main() {
  std::string cmd;
  std::unique_ptr<gra::ShardState[]> shards;
  unsigned long long nshards = 0;
  while (std::cin >> cmd) {
    unsigned long long s = 0, a, b, c, d, e;
    if (cmd == "scenario") {
      if (!(std::cin >> nshards)) return bad("scenario");
      shards.reset(new gra::ShardState[nshards]);
      for (size_t i = 0; i < nshards; i++) {
        if (!(std::cin >> a >> b >> c >> d)) return bad("shard");
        shards[i].durable_seq = a;
        shards[i].next_seq = b;
        shards[i].poisoned = c != 0;
        for (size_t j = 0; j < d; j++) {
          if (!(std::cin >> a >> b >> c)) return bad("log");
          gra::LogEnt ent;
          ent.base_seq = a;
          ent.count = (uint32_t)b;
          ent.rep.resize(c);
          shards[i].log_used += c;
          shards[i].log.push_back(std::move(ent));
        }
      }
      continue;
    }
    if (!(std::cin >> s) || s >= nshards) return bad("shard index");
    gra::ShardState &ss = shards[s];
    if (cmd == "group") {
      if (!(std::cin >> a >> b >> c >> d >> e)) return bad("group");
      std::unique_ptr<uint32_t[]> counts(new uint32_t[d]);
      std::unique_ptr<uint8_t[]> ok(e ? new uint8_t[d] : nullptr);
      for (size_t i = 0; i < d; i++) {
        unsigned long long v;
        if (!(std::cin >> v)) return bad("counts");
        counts[i] = (uint32_t)v;
      }
      for (size_t i = 0; e && i < d; i++) {
        unsigned long long v;
        if (!(std::cin >> v)) return bad("ok");
        ok[i] = (uint8_t)v;
      }
      gra::GroupFacts f = {a, b, (uint32_t)c, ok.get(), counts.get(),
                           (uint32_t)d};
      gra::GroupKeep keep;
      {
        std::lock_guard<std::mutex> lk(ss.mu);
        keep = gra::settle_group_locked(ss, f);
      }
      printf("K %u %llu %d\n", keep.n_entries,
             (unsigned long long)keep.last_seq, keep.whole ? 1 : 0);
    } else if (cmd == "submit") {
      if (!(std::cin >> a >> b)) return bad("submit");
      gra::LogEnt ent;
      ent.base_seq = ss.next_seq;
      ent.count = (uint32_t)a;
      ent.rep.resize(b);
      ss.next_seq += a;
      ss.log_used += b;
      ss.log.push_back(std::move(ent));
    } else if (cmd == "clear") {
      ss.poisoned = false;
    } else {
      return bad("command");
    }
    for (size_t i = 0; i < nshards; i++)
      printf("S %zu %llu %llu %d %llu %zu %llu\n", i,
             (unsigned long long)shards[i].durable_seq,
             (unsigned long long)shards[i].next_seq, shards[i].poisoned ? 1 : 0,
             (unsigned long long)shards[i].cnt_failures.load(),
             shards[i].log.size(), (unsigned long long)shards[i].log_used);
  }
  return 0;
}
