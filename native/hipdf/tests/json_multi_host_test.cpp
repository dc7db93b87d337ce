// Runs the multi-path row scanner of kernels/json_path.h on the host and
// holds it against scan_row() path by path: for every row and every path of
// the group, (state, src_start, src_len, out_len) must be equal. Rows that
// give a value are also written with write_row() and compared with answers
// recorded from the host backend. No HIP: the header compiles as plain C++.
//
// Usage: json_multi_host_test CASEFILE
// Case file: the number of paths; per path the number of steps and one line
// per step ("k HEX" a key with its name in hex, "i N" an index); then one
// line per row: "xDOCHEX" and one answer per path, "xANSWERHEX", "-" where
// the host answers NULL, or "?" where the answer is not to be compared.
// The group runs in every instantiation that holds it (2, 4, 8 slots), as
// the kernel's dead slots do: a slot beyond the group repeats path 0.
// Exit status 1 on any difference.
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "json_path.h"

using jsonpath::RowResult;

static bool unhex(const std::string& h, std::vector<uint8_t>* out) {
  if (h.empty() || h[0] != 'x' || (h.size() - 1) % 2) return false;
  out->clear();
  for (size_t i = 1; i < h.size(); i += 2) {
    int a = jsonpath::hex_val((uint8_t)h[i]);
    int b = jsonpath::hex_val((uint8_t)h[i + 1]);
    if (a < 0 || b < 0) return false;
    out->push_back((uint8_t)(a * 16 + b));
  }
  return true;
}

struct Group {
  std::vector<int32_t> steps;     // every path's triples, one after another
  std::vector<uint8_t> names;
  std::vector<int32_t> step_off;  // in triples
  std::vector<int32_t> step_cnt;
};

template <int K>
static void run_multi(const Group& g, const std::vector<uint8_t>& doc,
                      RowResult* out) {
  jsonpath::PathGroup<K> pg;
  pg.steps = g.steps.data();
  pg.names = g.names.data();
  int npaths = (int)g.step_cnt.size();
  for (int k = 0; k < K; ++k) {
    int q = k < npaths ? k : 0;
    pg.sbase[k] = 3 * g.step_off[q];
    pg.nsteps[k] = g.step_cnt[q];
  }
  jsonpath::scan_row_multi<K>(doc.data(), 0, (int32_t)doc.size(), pg, out);
}

static bool same(const RowResult& a, const RowResult& b) {
  return a.state == b.state && a.src_start == b.src_start &&
         a.src_len == b.src_len && a.out_len == b.out_len;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s CASEFILE\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[1]);
  if (!in) {
    std::fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  int npaths = 0;
  in >> npaths;
  if (npaths < 1 || npaths > jsonpath::kMaxFusedPaths) return 2;
  Group g;
  for (int k = 0; k < npaths; ++k) {
    int nsteps = -1;
    in >> nsteps;
    if (nsteps < 0) return 2;
    g.step_off.push_back((int32_t)(g.steps.size() / 3));
    g.step_cnt.push_back(nsteps);
    for (int i = 0; i < nsteps; ++i) {
      std::string kind, arg;
      in >> kind >> arg;
      if (kind == "k") {
        std::vector<uint8_t> nm;
        if (!unhex(arg, &nm)) return 2;
        g.steps.insert(g.steps.end(),
                       {0, (int32_t)g.names.size(), (int32_t)nm.size()});
        g.names.insert(g.names.end(), nm.begin(), nm.end());
      } else if (kind == "i") {
        g.steps.insert(g.steps.end(), {1, (int32_t)std::stol(arg), 0});
      } else {
        return 2;
      }
    }
  }

  long rows = 0, bad = 0, flagged = 0, values = 0, nulls = 0;
  std::string doc_hex;
  while (in >> doc_hex) {
    // exact-size heap copies, so that a sanitizer sees any read or write
    // outside the row or the output
    std::vector<uint8_t> doc;
    if (!unhex(doc_hex, &doc)) return 2;
    std::vector<std::string> want_hex(npaths);
    for (int k = 0; k < npaths; ++k)
      if (!(in >> want_hex[k])) return 2;
    ++rows;

    std::vector<RowResult> single(npaths);
    for (int k = 0; k < npaths; ++k) {
      jsonpath::Path path{g.steps.data() + 3 * g.step_off[k], g.names.data(),
                          g.step_cnt[k]};
      single[k] = jsonpath::scan_row(doc.data(), 0, (int32_t)doc.size(), path);
    }
    RowResult multi[jsonpath::kMaxFusedPaths];
    const int slots[3] = {2, 4, 8};
    for (int K : slots) {
      if (K < npaths || K > jsonpath::kMaxFusedPaths) continue;
      if (K == 2) run_multi<2>(g, doc, multi);
      else if (K == 4) run_multi<4>(g, doc, multi);
      else run_multi<8>(g, doc, multi);
      for (int k = 0; k < npaths; ++k) {
        if (same(multi[k], single[k])) continue;
        ++bad;
        std::printf("row %ld path %d slots %d: multi (%d,%d,%d,%lld) single "
                    "(%d,%d,%d,%lld): %s\n", rows, k, K, multi[k].state,
                    multi[k].src_start, multi[k].src_len,
                    (long long)multi[k].out_len, single[k].state,
                    single[k].src_start, single[k].src_len,
                    (long long)single[k].out_len, doc_hex.c_str());
      }
    }

    // the last instantiation's results, against the recorded answers
    for (int k = 0; k < npaths; ++k) {
      const RowResult& r = multi[k];
      if (r.state == jsonpath::JP_FLAG) {
        ++flagged;
        continue;
      }
      bool skip = want_hex[k] == "?";
      bool want_null = want_hex[k] == "-";
      std::vector<uint8_t> want;
      if (!skip && !want_null && !unhex(want_hex[k], &want)) return 2;
      if (r.state == jsonpath::JP_NULL) {
        ++nulls;
        if (!skip && !want_null) {
          ++bad;
          std::printf("row %ld path %d: NULL where a value was expected: %s\n",
                      rows, k, doc_hex.c_str());
        }
        continue;
      }
      ++values;
      std::vector<uint8_t> out((size_t)r.out_len);
      jsonpath::write_row(doc.data(), r.src_start, r.src_len, out.data(),
                          r.out_len);
      if (!skip && (want_null || out != want)) {
        ++bad;
        std::printf("row %ld path %d: got '%.*s' expected %s: %s\n", rows, k,
                    (int)out.size(), (const char*)out.data(),
                    want_null ? "NULL" : want_hex[k].c_str(),
                    doc_hex.c_str());
      }
    }
  }
  std::printf("rows %ld values %ld nulls %ld flagged %ld mismatches %ld\n",
              rows, values, nulls, flagged, bad);
  return bad ? 1 : 0;
}
