// Host run of the digest cores (kernels/digest.h): the known answers, then
// every algorithm against an expected file (gen_digest_golden.py) for every
// message length 0..260, each message placed at every start alignment 0..15
// in a heap block of exactly the bytes it needs, so that under
// AddressSanitizer a read past the row's end is an error.
//
//   digest_host_test <tests/golden/digest_expected.txt>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "digest.h"

namespace {

constexpr digest::Crc32Table kCrcTable = digest::make_crc32_table();
static_assert(kCrcTable.t[1] == 0x77073096u, "crc table");
static_assert(kCrcTable.t[255] == 0x2d02ef8du, "crc table");

int failures = 0;

std::string run(const std::string& algo, const uint8_t* p, int64_t len) {
  uint8_t hex[129] = {0};
  if (algo == "md5") digest::digest_hex<digest::Md5>(p, len, hex);
  else if (algo == "sha1") digest::digest_hex<digest::Sha1>(p, len, hex);
  else if (algo == "sha224") digest::digest_hex<digest::Sha224>(p, len, hex);
  else if (algo == "sha256") digest::digest_hex<digest::Sha256>(p, len, hex);
  else if (algo == "sha384") digest::digest_hex<digest::Sha384>(p, len, hex);
  else if (algo == "sha512") digest::digest_hex<digest::Sha512>(p, len, hex);
  else if (algo == "crc32") {
    snprintf((char*)hex, sizeof hex, "%08x",
             digest::crc32_row(kCrcTable.t, p, len));
  } else {
    return "?";
  }
  return std::string((const char*)hex);
}

// the message at start alignment `mis` (mod 16), nothing allocated behind it
std::string run_at(const std::string& algo, const uint8_t* msg, int64_t len,
                   int mis) {
  uint8_t* block = (uint8_t*)malloc((size_t)(mis + len) + (mis + len == 0));
  memset(block, 0xAA, (size_t)mis);
  if (len) memcpy(block + mis, msg, (size_t)len);
  std::string got = run(algo, block + mis, len);
  free(block);
  return got;
}

void expect(const std::string& algo, const uint8_t* msg, int64_t len,
            const std::string& want) {
  for (int mis = 0; mis < 16; ++mis) {
    std::string got = run_at(algo, msg, len, mis);
    if (got != want) {
      if (++failures <= 20)
        printf("FAIL %s len %lld mis %d: got %s want %s\n", algo.c_str(),
               (long long)len, mis, got.c_str(), want.c_str());
    }
  }
}

void known(const char* algo, const char* text, const char* want) {
  expect(algo, (const uint8_t*)text, (int64_t)strlen(text), want);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s <expected file>\n", argv[0]);
    return 2;
  }
  known("md5", "", "d41d8cd98f00b204e9800998ecf8427e");
  known("md5", "abc", "900150983cd24fb0d6963f7d28e17f72");
  known("sha1", "abc", "a9993e364706816aba3e25717850c26c9cd0d89d");
  known("sha256", "abc",
        "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad");
  known("crc32", "123456789", "cbf43926");
  int known_failures = failures;

  FILE* f = fopen(argv[1], "r");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  char algo[16], hex[160];
  long long len;
  int cases = 0;
  uint8_t msg[512];
  while (fscanf(f, "%15s %lld %159s", algo, &len, hex) == 3) {
    if (len < 0 || len > (long long)sizeof msg) {
      fprintf(stderr, "bad length %lld\n", len);
      return 2;
    }
    for (long long i = 0; i < len; ++i)
      msg[i] = (uint8_t)((7 * i + 131 * len) & 0xFF);
    expect(algo, msg, len, hex);
    ++cases;
  }
  fclose(f);
  printf("known 5 (failed alignments %d) cases %d alignments 16 "
         "failures %d\n", known_failures, cases, failures);
  return failures == 0 && cases > 0 ? 0 : 1;
}
