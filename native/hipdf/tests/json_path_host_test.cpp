// Runs the get_json_object row parser of kernels/json_path.h on the host,
// size pass then write pass per row, against answers recorded from the host
// backend. No HIP: the header compiles as plain C++.
//
// Usage: json_path_host_test CASEFILE
// Case file: first line the number of path steps, then one line per step
// ("k HEX" a key with its name in hex, "i N" an index), then one line per
// row: "xDOCHEX xANSWERHEX", or "xDOCHEX -" where the host answers NULL.
// Exit status 1 on any row where the parser answers a value the host does
// not give, NULL where the host gives a value, or a value where the host
// gives NULL. Rows left to the host (state 2) are counted and printed.
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "json_path.h"

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
  int nsteps = 0;
  in >> nsteps;
  std::vector<int32_t> steps;
  std::vector<uint8_t> names;
  for (int i = 0; i < nsteps; ++i) {
    std::string kind, arg;
    in >> kind >> arg;
    if (kind == "k") {
      std::vector<uint8_t> nm;
      if (!unhex(arg, &nm)) return 2;
      steps.insert(steps.end(),
                   {0, (int32_t)names.size(), (int32_t)nm.size()});
      names.insert(names.end(), nm.begin(), nm.end());
    } else if (kind == "i") {
      steps.insert(steps.end(), {1, (int32_t)std::stol(arg), 0});
    } else {
      return 2;
    }
  }
  jsonpath::Path path{steps.data(), names.data(), nsteps};

  long rows = 0, bad = 0, flagged = 0, values = 0, nulls = 0;
  std::string doc_hex, want_hex;
  while (in >> doc_hex >> want_hex) {
    // exact-size heap copies, so that a sanitizer sees any read or write
    // outside the row or the output
    std::vector<uint8_t> doc, want;
    if (!unhex(doc_hex, &doc)) return 2;
    bool want_null = want_hex == "-";
    if (!want_null && !unhex(want_hex, &want)) return 2;
    ++rows;
    jsonpath::RowResult r =
        jsonpath::scan_row(doc.data(), 0, (int32_t)doc.size(), path);
    if (r.state == jsonpath::JP_FLAG) {
      ++flagged;
      continue;
    }
    if (r.state == jsonpath::JP_NULL) {
      ++nulls;
      if (!want_null) {
        ++bad;
        std::printf("row %ld: NULL where a value was expected: %s\n", rows,
                    doc_hex.c_str());
      }
      continue;
    }
    ++values;
    std::vector<uint8_t> out((size_t)r.out_len);
    jsonpath::write_row(doc.data(), r.src_start, r.src_len, out.data(),
                        r.out_len);
    if (want_null || out != want) {
      ++bad;
      std::printf("row %ld: got '%.*s' expected %s: %s\n", rows,
                  (int)out.size(), (const char*)out.data(),
                  want_null ? "NULL" : want_hex.c_str(), doc_hex.c_str());
    }
  }
  std::printf("rows %ld values %ld nulls %ld flagged %ld mismatches %ld\n",
              rows, values, nulls, flagged, bad);
  return bad ? 1 : 0;
}
