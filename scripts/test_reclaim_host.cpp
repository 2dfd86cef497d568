/* test_reclaim_host.cpp — stand-alone driver for gra::plan_reclaim, the host
 * plan gra_reclaim runs. Plain C++ (g++, no HIP headers), built with
 * -fsanitize=address,undefined by tests/test_reclaim_host.py.
 *
 * Input on stdin, any number of cases:
 *   plan <used> <bounce_bytes> <piece_bytes> <nsegments>
 *   <src> <nbytes>                      one line per segment, in any order
 * Output per case:
 *   err <message>                       the plan was refused, or
 *   ok <new_cursor> <bytes_moved> <bytes_bounced> <nsegs> <npieces> <nbatches>
 *   S <src> <nbytes> <dst> <tag>        per segment, sorted by src; tag = the
 *                                       segment's position in the input
 *   P <seg> <src> <dst> <bnc> <nbytes>  per piece
 *   B <kind> <first> <count> <bytes>    per batch; kind 0 direct, 1 bounce */
#include <cstdio>
#include <iostream>
#include <string>

#include "../rocksplicator_amd/csrc/host_store.h"

int main() {
  std::string cmd;
  while (std::cin >> cmd) {
    unsigned long long used, bounce, piece, nseg;
    if (cmd != "plan" || !(std::cin >> used >> bounce >> piece >> nseg)) {
      fprintf(stderr, "bad plan line\n");
      return 2;
    }
    std::vector<gra::RcSegment> segs(nseg);
    for (size_t i = 0; i < nseg; i++) {
      unsigned long long src, n;
      if (!(std::cin >> src >> n)) {
        fprintf(stderr, "bad segment line\n");
        return 2;
      }
      segs[i].src = src;
      segs[i].nbytes = n;
      segs[i].tag = i;
    }
    gra::RcPlan plan;
    std::string err;
    if (gra::plan_reclaim(segs, used, bounce, piece, &plan, &err) != 0) {
      printf("err %s\n", err.c_str());
      continue;
    }
    printf("ok %llu %llu %llu %zu %zu %zu\n",
           (unsigned long long)plan.new_cursor,
           (unsigned long long)plan.bytes_moved,
           (unsigned long long)plan.bytes_bounced, plan.segs.size(),
           plan.pieces.size(), plan.batches.size());
    for (const auto &s : plan.segs)
      printf("S %llu %llu %llu %llu\n", (unsigned long long)s.src,
             (unsigned long long)s.nbytes, (unsigned long long)s.dst,
             (unsigned long long)s.tag);
    for (const auto &p : plan.pieces)
      printf("P %u %llu %llu %llu %u\n", p.seg, (unsigned long long)p.src,
             (unsigned long long)p.dst, (unsigned long long)p.bnc, p.nbytes);
    for (const auto &b : plan.batches)
      printf("B %u %u %u %llu\n", b.kind, b.first, b.count,
             (unsigned long long)b.bytes);
  }
  return 0;
}
