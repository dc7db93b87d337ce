// Runs the nullable page walk and the definition-level decoder of
// kernels/pq_levels.h on the host, under the sanitizers. No HIP: the headers
// compile as plain C++.
//
// Usage: pq_levels_host_test CASEFILE
// One case per line:
//   chunk CHUNKFILE NUM_VALUES MAX_DEF PHYS_WIDTH NPAGES VALIDFILE VALUESFILE
//       walk_levels must give NPAGES pages. VALIDFILE holds one byte per row
//       of the chunk (1 = valid). For every page the decoded bits must equal
//       its rows of VALIDFILE, the tile counts their prefix sums, and the
//       valid count times the width the page's value bytes; the pages' value
//       bytes, one after another, are the bytes of VALUESFILE.
//   chunktrunc CHUNKFILE NUM_VALUES MAX_DEF PHYS_WIDTH
//       the whole chunk must walk and decode; every proper prefix of the
//       chunk, and of every page's level stream, must return a negative code
//   stream STREAMFILE N ok VALIDFILE   the stream decodes to VALIDFILE
//   stream STREAMFILE N err            the decode returns a negative code
// Every call reads heap copies of exactly the bytes it is given and writes
// heap buffers of exactly the documented sizes, so a read or write past an
// end is an AddressSanitizer error. Exit status 1 on any failure.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "pq_levels.h"

using namespace pq_pieces;

static bool slurp(const std::string& path, std::vector<uint8_t>* out) {
  std::ifstream f(path, std::ios::binary);
  if (!f) return false;
  out->assign(std::istreambuf_iterator<char>(f),
              std::istreambuf_iterator<char>());
  return true;
}

// decode over exact-size heap copies; on success checks the result against
// want[0, n) (one byte per row) when want is given. Returns the valid count,
// a negative decoder code, or -1000 - k for a mismatch of kind k.
static int64_t decode_copy(const uint8_t* lv, size_t nb, int64_t n,
                           const uint8_t* want) {
  uint8_t* buf = new uint8_t[nb ? nb : 1];
  if (nb) memcpy(buf, lv, nb);
  int64_t mb = mask_bytes(n), te = tile_entries(n);
  uint8_t* mask = new uint8_t[mb ? mb : 1];
  uint32_t* tiles = new uint32_t[te];
  memset(mask, 0xA5, (size_t)(mb ? mb : 1));
  int64_t rc = decode_levels(buf, (int64_t)nb, n, mask, tiles);
  if (rc >= 0 && want) {
    int64_t seen = 0;
    for (int64_t r = 0; r < mb * 8 && rc >= 0; ++r) {
      if (r % kTileRows == 0 && tiles[r / kTileRows] != seen) rc = -1001;
      int bit = (mask[r >> 3] >> (r & 7)) & 1;
      int w = r < n ? want[r] : 0;  // bits at and beyond n are zero
      if (bit != w) rc = -1002;
      seen += bit;
    }
    if (rc >= 0 && (tiles[te - 1] != seen || rc != seen)) rc = -1003;
  }
  delete[] tiles;
  delete[] mask;
  delete[] buf;
  return rc;
}

static int64_t walk_copy(const std::vector<uint8_t>& chunk, size_t n,
                         int64_t num_values, int max_def, int width,
                         std::vector<int64_t>* pages, uint8_t** keep) {
  uint8_t* buf = new uint8_t[n ? n : 1];
  if (n) memcpy(buf, chunk.data(), n);
  pages->assign(kLevelStride * 64, 0);
  int64_t np = walk_levels(buf, (int64_t)n, num_values, max_def, width,
                           pages->data(), 64);
  for (int64_t k = 0; k < np; ++k) {
    const int64_t* pg = &(*pages)[kLevelStride * k];
    if (pg[0] < 0 || pg[1] < 0 || pg[0] + pg[1] > (int64_t)n || pg[3] < 0 ||
        pg[4] < 0 || pg[3] + pg[4] > (int64_t)n) {
      np = -1000;  // a piece outside the chunk
      break;
    }
  }
  if (keep && np >= 0)
    *keep = buf;
  else
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
  long prefixes = 0, npages = 0;
  while (std::getline(cases, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string kind, path;
    in >> kind >> path;
    std::vector<uint8_t> data, valid, want_values;
    if (!in || !slurp(path, &data)) {
      fprintf(stderr, "bad case: %s\n", line.c_str());
      return 2;
    }
    ++ncases;
    if (kind == "stream") {
      int64_t n;
      std::string mode, valid_path;
      in >> n >> mode;
      if (mode == "ok") in >> valid_path;
      if (!in || (mode == "ok" && !slurp(valid_path, &valid)) ||
          (mode == "ok" && (int64_t)valid.size() != n)) {
        fprintf(stderr, "bad case: %s\n", line.c_str());
        return 2;
      }
      int64_t rc = decode_copy(data.data(), data.size(), n,
                               mode == "ok" ? valid.data() : nullptr);
      if ((mode == "ok") != (rc >= 0)) {
        printf("FAIL %s: rc %lld\n", path.c_str(), (long long)rc);
        ++failed;
      }
      continue;
    }
    int64_t num_values;
    int max_def, width;
    in >> num_values >> max_def >> width;
    std::vector<int64_t> pages;
    uint8_t* buf = nullptr;
    int64_t np = walk_copy(data, data.size(), num_values, max_def, width,
                           &pages, &buf);
    if (kind == "chunk") {
      int64_t want_pages;
      std::string valid_path, values_path;
      in >> want_pages >> valid_path >> values_path;
      if (!in || !slurp(valid_path, &valid) ||
          !slurp(values_path, &want_values) ||
          (int64_t)valid.size() != num_values) {
        fprintf(stderr, "bad case: %s\n", line.c_str());
        return 2;
      }
      bool ok = np == want_pages;
      std::vector<uint8_t> values;
      int64_t row = 0;
      for (int64_t k = 0; ok && k < np; ++k) {
        const int64_t* pg = &pages[kLevelStride * k];
        int64_t n = pg[2];
        ok = row + n <= num_values;
        if (!ok) break;
        int64_t nvalid = n;  // max_def 0: no levels, every row valid
        if (max_def > 0)
          nvalid = decode_copy(buf + pg[3], (size_t)pg[4], n,
                               valid.data() + row);
        else
          for (int64_t r = 0; r < n; ++r) ok = ok && valid[row + r] == 1;
        if (nvalid < 0 || nvalid * width != pg[1]) {
          printf("FAIL %s page %lld: %lld valid, %lld value bytes\n",
                 path.c_str(), (long long)k, (long long)nvalid,
                 (long long)pg[1]);
          ok = false;
        }
        values.insert(values.end(), buf + pg[0], buf + pg[0] + pg[1]);
        row += n;
        ++npages;
      }
      if (!ok || row != num_values || values != want_values) {
        printf("FAIL %s: rc %lld (want %lld pages), %lld rows, %zu value "
               "bytes (want %zu)\n", path.c_str(), (long long)np,
               (long long)want_pages, (long long)row, values.size(),
               want_values.size());
        ++failed;
      }
    } else if (kind == "chunktrunc") {
      if (np <= 0) {
        printf("FAIL %s: whole chunk rejected, rc %lld\n", path.c_str(),
               (long long)np);
        ++failed;
      }
      for (int64_t k = 0; k < np; ++k) {
        const int64_t* pg = &pages[kLevelStride * k];
        if (decode_copy(buf + pg[3], (size_t)pg[4], pg[2], nullptr) < 0) {
          printf("FAIL %s page %lld: whole stream rejected\n", path.c_str(),
                 (long long)k);
          ++failed;
        }
        for (int64_t nb = 0; nb < pg[4]; ++nb) {
          ++prefixes;
          if (decode_copy(buf + pg[3], (size_t)nb, pg[2], nullptr) >= 0) {
            printf("FAIL %s page %lld: level prefix of %lld bytes accepted\n",
                   path.c_str(), (long long)k, (long long)nb);
            ++failed;
            break;
          }
        }
      }
      std::vector<int64_t> scratch;
      for (size_t n = 0; n < data.size(); ++n) {
        ++prefixes;
        if (walk_copy(data, n, num_values, max_def, width, &scratch,
                      nullptr) >= 0) {
          printf("FAIL %s: prefix of %zu bytes accepted\n", path.c_str(), n);
          ++failed;
          break;
        }
      }
    } else {
      fprintf(stderr, "bad kind: %s\n", line.c_str());
      return 2;
    }
    delete[] buf;
  }
  printf("cases %d pages %ld prefixes %ld failed %d\n", ncases, npages,
         prefixes, failed);
  return failed ? 1 : 0;
}
