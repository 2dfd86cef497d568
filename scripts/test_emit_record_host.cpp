/* test_emit_record_host.cpp — stand-alone driver for the packed one-record
 * form of wb_format.h (wb::EmitRec, wb::emit_pack, wb::emit_unpack), what
 * k_decode hands k_emit. Plain C++ (g++, no HIP headers), built with
 * -fsanitize=address,undefined by tests/test_emit_record_host.py.
 *
 * Commands on stdin, one per line:
 *   blob <rephex>   walk the blob (a heap copy of exactly its size) with
 *                   walk_f keeping the first record, pack, and where the
 *                   kind is 1 unpack again. Prints
 *                   "blob <ok> <n_records> <recs emitted>
 *                   <first: key_off key_len val_off val_len tag cf_id>
 *                   <packed: kind key_off key_len val_gap val_len tag cf_id
 *                   pad> <unpack bit-equal to first: 1, 0, or -1 when the
 *                   kind is not 1>"
 *                   The first-record fields are zero when the walk emitted
 *                   none.
 * "-" is the empty blob. */
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

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
  out->reserve(s.size() / 2);
  for (size_t i = 0; i < s.size(); i += 2) {
    int h = nib(s[i]), l = nib(s[i + 1]);
    if (h < 0 || l < 0) return false;
    out->push_back((char)(h * 16 + l));
  }
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
      std::unique_ptr<uint8_t[]> rep(new uint8_t[len]);
      if (len) memcpy(rep.get(), raw.data(), len);
      wb::Rec first;
      memset(&first, 0, sizeof first);
      uint32_t emitted = 0;
      wb::WalkTotals t =
          wb::walk_f(rep.get(), len, [&](const wb::Rec &r, uint32_t idx) {
            if (idx == 0) first = r;
            emitted++;
          });
      wb::EmitRec e = wb::emit_pack(t, first);
      int equal = -1;
      if (e.kind == wb::kEmitOne) {
        wb::Rec back = wb::emit_unpack(e);
        equal = memcmp(&back, &first, sizeof(wb::Rec)) == 0;
      }
      printf("blob %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %d\n",
             t.ok, t.n_records, emitted, first.key_off, first.key_len,
             first.val_off, first.val_len, first.tag, first.cf_id, e.kind,
             e.key_off, e.key_len, e.val_gap, e.val_len, e.tag, e.cf_id,
             e._pad, equal);
    } else if (!cmd.empty()) {
      printf("unknown command\n");
      return 2;
    }
  }
  return 0;
}
