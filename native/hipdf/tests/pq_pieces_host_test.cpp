// Runs the parquet page walker of kernels/pq_pieces.h on the host, under the
// sanitizers. No HIP: the header compiles as plain C++.
//
// Usage: pq_pieces_host_test CASEFILE
// One case per line: CHUNKFILE NUM_VALUES MAX_DEF PHYS_WIDTH MODE [ARGS]
//   ok NPAGES VALUESFILE  the walk must give NPAGES pages whose value bytes,
//                         one after another, are the bytes of VALUESFILE
//   err                   the walk must return a negative code
//   trunc                 the whole chunk must walk, and every proper prefix
//                         of it must return a negative code
// Every walk reads a heap copy of exactly the bytes it is given, so a read
// past the end is an AddressSanitizer error. Exit status 1 on any failure.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "pq_pieces.h"

static bool slurp(const std::string& path, std::vector<uint8_t>* out) {
  std::ifstream f(path, std::ios::binary);
  if (!f) return false;
  out->assign(std::istreambuf_iterator<char>(f),
              std::istreambuf_iterator<char>());
  return true;
}

// the walk over an exact-size heap copy of chunk[0, n)
static int64_t walk_copy(const std::vector<uint8_t>& chunk, size_t n,
                         int64_t num_values, int max_def, int width,
                         std::vector<int64_t>* pages,
                         std::vector<uint8_t>* values) {
  uint8_t* buf = new uint8_t[n ? n : 1];
  if (n) memcpy(buf, chunk.data(), n);
  pages->assign(3 * 64, 0);
  // n == 0 hands the walker a one-byte buffer and a length of zero
  int64_t np = pq_pieces::walk(buf, (int64_t)n, num_values, max_def, width,
                               pages->data(), 64);
  if (np >= 0 && values) {
    values->clear();
    for (int64_t k = 0; k < np; ++k) {
      int64_t off = (*pages)[3 * k], nb = (*pages)[3 * k + 1];
      if (off < 0 || nb < 0 || off + nb > (int64_t)n) {
        np = -1000;  // a piece outside the chunk
        break;
      }
      values->insert(values->end(), buf + off, buf + off + nb);
    }
  }
  delete[] buf;
  return np;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s CASEFILE\n", argv[0]);
    return 2;
  }
  std::ifstream cases(argv[1]);
  std::string line;
  int ncases = 0, failed = 0;
  long prefixes = 0;
  while (std::getline(cases, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string chunk_path, mode;
    int64_t num_values;
    int max_def, width;
    in >> chunk_path >> num_values >> max_def >> width >> mode;
    std::vector<uint8_t> chunk, values, want;
    std::vector<int64_t> pages;
    if (!in || !slurp(chunk_path, &chunk)) {
      fprintf(stderr, "bad case: %s\n", line.c_str());
      return 2;
    }
    ++ncases;
    int64_t np = walk_copy(chunk, chunk.size(), num_values, max_def, width,
                           &pages, &values);
    if (mode == "err") {
      if (np >= 0) {
        printf("FAIL %s: accepted with %lld pages\n", chunk_path.c_str(),
               (long long)np);
        ++failed;
      }
    } else if (mode == "ok") {
      int64_t want_pages;
      std::string values_path;
      in >> want_pages >> values_path;
      if (!in || !slurp(values_path, &want)) {
        fprintf(stderr, "bad case: %s\n", line.c_str());
        return 2;
      }
      int64_t nvals = 0;
      for (int64_t k = 0; k < np; ++k) nvals += pages[3 * k + 2];
      if (np != want_pages || values != want || nvals != num_values) {
        printf("FAIL %s: rc %lld (want %lld pages), %zu value bytes "
               "(want %zu), %lld values\n", chunk_path.c_str(), (long long)np,
               (long long)want_pages, values.size(), want.size(),
               (long long)nvals);
        ++failed;
      }
    } else if (mode == "trunc") {
      if (np < 0) {
        printf("FAIL %s: whole chunk rejected, rc %lld\n",
               chunk_path.c_str(), (long long)np);
        ++failed;
      }
      for (size_t n = 0; n < chunk.size(); ++n) {
        int64_t rc = walk_copy(chunk, n, num_values, max_def, width, &pages,
                               nullptr);
        ++prefixes;
        if (rc >= 0) {
          printf("FAIL %s: prefix of %zu bytes accepted\n",
                 chunk_path.c_str(), n);
          ++failed;
          break;
        }
      }
    } else {
      fprintf(stderr, "bad mode: %s\n", line.c_str());
      return 2;
    }
  }
  printf("cases %d prefixes %ld failed %d\n", ncases, prefixes, failed);
  return failed ? 1 : 0;
}
