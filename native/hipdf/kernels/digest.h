// Message digests of one row's bytes: MD5 (RFC 1321), SHA-1, SHA-224/256 and
// SHA-384/512 (FIPS 180-4), and CRC-32 (zlib / IEEE, reflected).
//
// The same code compiles for the device (under hipcc, called by the kernels
// in digest.hip) and as plain C++ for a host program, so a host test runs
// exactly what the kernel runs. No HIP types appear in the interface.
//
// How a row is read. A row starts at any address. Its bytes come through
// aligned 4-byte loads; the aligned word that holds the row's first byte and
// the one that holds its last are the only ones put together from single
// bytes, and only from bytes inside the row. Two neighbouring aligned words
// shifted by the row's misalignment give one little-endian message word.
//
// How it stays in registers. The state, the 16 message words of a block and
// the rolling 16-word schedule are small arrays that every loop indexes with
// its own counter; every such loop has a constant trip count and is fully
// unrolled, so each index is a compile-time constant and the arrays become
// registers. A runtime index would put them in scratch.
#pragma once

#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define DG_HD __host__ __device__ __forceinline__
#else
#define DG_HD inline
#endif

#if defined(__clang__)
#define DG_UNROLL _Pragma("unroll")
#elif defined(__GNUC__)
#define DG_UNROLL _Pragma("GCC unroll 128")
#else
#define DG_UNROLL
#endif

namespace digest {

DG_HD uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
DG_HD uint32_t rotr32(uint32_t x, int r) { return (x >> r) | (x << (32 - r)); }
DG_HD uint64_t rotr64(uint64_t x, int r) { return (x >> r) | (x << (64 - r)); }
DG_HD uint32_t bswap32(uint32_t x) { return __builtin_bswap32(x); }

// aligned loads out of a byte buffer, as typed accesses so that each is one
// load instruction of its width
typedef uint32_t __attribute__((may_alias)) u32_alias;
typedef uint32_t u32x4_alias __attribute__((vector_size(16), may_alias));

DG_HD uint32_t load_u32(const uint8_t* p) {  // p is 4-byte aligned
  return *reinterpret_cast<const u32_alias*>(p);
}

// ---------------------------------------------------------------------------
// Row bytes as aligned words
// ---------------------------------------------------------------------------

struct RowReader {
  const uint8_t* base;  // row start - mis: a 4-byte aligned address
  int64_t len;
  int mis;  // row start & 3

  DG_HD RowReader(const uint8_t* p, int64_t len_)
      : base(p - ((uintptr_t)p & 3)), len(len_), mis((int)((uintptr_t)p & 3)) {}

  // aligned word j, which the caller knows to lie inside the row
  DG_HD uint32_t load(int64_t j) const {
    return load_u32(base + 4 * j);
  }

  // aligned word j with every byte outside the row read as zero (and not
  // read at all): single-byte loads for the row's first and last word only
  DG_HD uint32_t fetch(int64_t j) const {
    int64_t r = 4 * j - mis;  // row-relative position of the word
    if (r >= 0 && r + 4 <= len) return load(j);
    uint32_t w = 0;
    DG_UNROLL
    for (int t = 0; t < 4; ++t) {
      int64_t q = r + t;
      if (q >= 0 && q < len) w |= (uint32_t)base[4 * j + t] << (8 * t);
    }
    return w;
  }

  // little-endian message word from two neighbouring aligned words
  DG_HD uint32_t join(uint32_t lo, uint32_t hi) const {
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * mis));
  }
};

// ---------------------------------------------------------------------------
// The algorithms: init, one block's compression, and where the digest's
// bytes sit in the state. `w` holds the block's 16 words in the algorithm's
// own byte order and is used up as the rolling schedule.
// ---------------------------------------------------------------------------

struct Md5 {
  typedef uint32_t word;
  static constexpr int kBlockBytes = 64, kState = 4, kOut32 = 4;

  static DG_HD void init(word* s) {
    s[0] = 0x67452301u; s[1] = 0xefcdab89u;
    s[2] = 0x98badcfeu; s[3] = 0x10325476u;
  }

  static DG_HD void pack(word* w, const uint32_t* m, int64_t bits, bool last) {
    DG_UNROLL
    for (int i = 0; i < 16; ++i) w[i] = m[i];
    if (last) {
      w[14] = (uint32_t)bits;
      w[15] = (uint32_t)((uint64_t)bits >> 32);
    }
  }

  static DG_HD void compress(word* s, word* w) {
    constexpr uint32_t K[64] = {
        0xd76aa478u, 0xe8c7b756u, 0x242070dbu, 0xc1bdceeeu, 0xf57c0fafu,
        0x4787c62au, 0xa8304613u, 0xfd469501u, 0x698098d8u, 0x8b44f7afu,
        0xffff5bb1u, 0x895cd7beu, 0x6b901122u, 0xfd987193u, 0xa679438eu,
        0x49b40821u, 0xf61e2562u, 0xc040b340u, 0x265e5a51u, 0xe9b6c7aau,
        0xd62f105du, 0x02441453u, 0xd8a1e681u, 0xe7d3fbc8u, 0x21e1cde6u,
        0xc33707d6u, 0xf4d50d87u, 0x455a14edu, 0xa9e3e905u, 0xfcefa3f8u,
        0x676f02d9u, 0x8d2a4c8au, 0xfffa3942u, 0x8771f681u, 0x6d9d6122u,
        0xfde5380cu, 0xa4beea44u, 0x4bdecfa9u, 0xf6bb4b60u, 0xbebfbc70u,
        0x289b7ec6u, 0xeaa127fau, 0xd4ef3085u, 0x04881d05u, 0xd9d4d039u,
        0xe6db99e5u, 0x1fa27cf8u, 0xc4ac5665u, 0xf4292244u, 0x432aff97u,
        0xab9423a7u, 0xfc93a039u, 0x655b59c3u, 0x8f0ccc92u, 0xffeff47du,
        0x85845dd1u, 0x6fa87e4fu, 0xfe2ce6e0u, 0xa3014314u, 0x4e0811a1u,
        0xf7537e82u, 0xbd3af235u, 0x2ad7d2bbu, 0xeb86d391u};
    constexpr int S[16] = {7, 12, 17, 22, 5, 9,  14, 20,
                           4, 11, 16, 23, 6, 10, 15, 21};
    uint32_t a = s[0], b = s[1], c = s[2], d = s[3];
    DG_UNROLL
    for (int i = 0; i < 64; ++i) {
      uint32_t f;
      int g;
      if (i < 16) {
        f = (b & c) | (~b & d);
        g = i;
      } else if (i < 32) {
        f = (d & b) | (~d & c);
        g = (5 * i + 1) & 15;
      } else if (i < 48) {
        f = b ^ c ^ d;
        g = (3 * i + 5) & 15;
      } else {
        f = c ^ (b | ~d);
        g = (7 * i) & 15;
      }
      uint32_t t = a + f + K[i] + w[g];
      a = d;
      d = c;
      c = b;
      b = b + rotl32(t, S[(i >> 4) * 4 + (i & 3)]);
    }
    s[0] += a; s[1] += b; s[2] += c; s[3] += d;
  }

  // digest bytes 4k .. 4k+3, the first in the low byte
  static DG_HD uint32_t out32(const word* s, int k) { return s[k]; }
};

// the big-endian 32-bit-word family shares its block packing
struct Sha32Base {
  typedef uint32_t word;
  static constexpr int kBlockBytes = 64;

  static DG_HD void pack(word* w, const uint32_t* m, int64_t bits, bool last) {
    DG_UNROLL
    for (int i = 0; i < 16; ++i) w[i] = bswap32(m[i]);
    if (last) {
      w[14] = (uint32_t)((uint64_t)bits >> 32);
      w[15] = (uint32_t)bits;
    }
  }

  static DG_HD uint32_t out32(const word* s, int k) { return bswap32(s[k]); }
};

struct Sha1 : Sha32Base {
  static constexpr int kState = 5, kOut32 = 5;

  static DG_HD void init(word* s) {
    s[0] = 0x67452301u; s[1] = 0xefcdab89u; s[2] = 0x98badcfeu;
    s[3] = 0x10325476u; s[4] = 0xc3d2e1f0u;
  }

  static DG_HD void compress(word* s, word* w) {
    uint32_t a = s[0], b = s[1], c = s[2], d = s[3], e = s[4];
    DG_UNROLL
    for (int i = 0; i < 80; ++i) {
      if (i >= 16)
        w[i & 15] = rotl32(w[(i - 3) & 15] ^ w[(i - 8) & 15] ^
                               w[(i - 14) & 15] ^ w[i & 15], 1);
      uint32_t f, k;
      if (i < 20) {
        f = (b & c) | (~b & d);
        k = 0x5a827999u;
      } else if (i < 40) {
        f = b ^ c ^ d;
        k = 0x6ed9eba1u;
      } else if (i < 60) {
        f = (b & c) | (b & d) | (c & d);
        k = 0x8f1bbcdcu;
      } else {
        f = b ^ c ^ d;
        k = 0xca62c1d6u;
      }
      uint32_t t = rotl32(a, 5) + f + e + k + w[i & 15];
      e = d;
      d = c;
      c = rotl32(b, 30);
      b = a;
      a = t;
    }
    s[0] += a; s[1] += b; s[2] += c; s[3] += d; s[4] += e;
  }
};

struct Sha256 : Sha32Base {
  static constexpr int kState = 8, kOut32 = 8;

  static DG_HD void init(word* s) {
    s[0] = 0x6a09e667u; s[1] = 0xbb67ae85u; s[2] = 0x3c6ef372u;
    s[3] = 0xa54ff53au; s[4] = 0x510e527fu; s[5] = 0x9b05688cu;
    s[6] = 0x1f83d9abu; s[7] = 0x5be0cd19u;
  }

  static DG_HD void compress(word* s, word* w) {
    constexpr uint32_t K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu,
        0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u,
        0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u,
        0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu,
        0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau, 0x983e5152u,
        0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u,
        0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu,
        0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
        0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u,
        0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u,
        0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu,
        0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
        0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    uint32_t a = s[0], b = s[1], c = s[2], d = s[3], e = s[4], f = s[5],
             g = s[6], h = s[7];
    DG_UNROLL
    for (int i = 0; i < 64; ++i) {
      if (i >= 16) {
        uint32_t x = w[(i - 15) & 15], y = w[(i - 2) & 15];
        w[i & 15] += (rotr32(x, 7) ^ rotr32(x, 18) ^ (x >> 3)) +
                     w[(i - 7) & 15] +
                     (rotr32(y, 17) ^ rotr32(y, 19) ^ (y >> 10));
      }
      uint32_t t1 = h + (rotr32(e, 6) ^ rotr32(e, 11) ^ rotr32(e, 25)) +
                    ((e & f) ^ (~e & g)) + K[i] + w[i & 15];
      uint32_t t2 = (rotr32(a, 2) ^ rotr32(a, 13) ^ rotr32(a, 22)) +
                    ((a & b) ^ (a & c) ^ (b & c));
      h = g; g = f; f = e; e = d + t1;
      d = c; c = b; b = a; a = t1 + t2;
    }
    s[0] += a; s[1] += b; s[2] += c; s[3] += d;
    s[4] += e; s[5] += f; s[6] += g; s[7] += h;
  }
};

struct Sha224 : Sha256 {
  static constexpr int kOut32 = 7;

  static DG_HD void init(word* s) {
    s[0] = 0xc1059ed8u; s[1] = 0x367cd507u; s[2] = 0x3070dd17u;
    s[3] = 0xf70e5939u; s[4] = 0xffc00b31u; s[5] = 0x68581511u;
    s[6] = 0x64f98fa7u; s[7] = 0xbefa4fa4u;
  }
};

struct Sha512 {
  typedef uint64_t word;
  static constexpr int kBlockBytes = 128, kState = 8, kOut32 = 16;

  static DG_HD void init(word* s) {
    s[0] = 0x6a09e667f3bcc908ull; s[1] = 0xbb67ae8584caa73bull;
    s[2] = 0x3c6ef372fe94f82bull; s[3] = 0xa54ff53a5f1d36f1ull;
    s[4] = 0x510e527fade682d1ull; s[5] = 0x9b05688c2b3e6c1full;
    s[6] = 0x1f83d9abfb41bd6bull; s[7] = 0x5be0cd19137e2179ull;
  }

  // the 128-bit length field: the high 64 bits are zero for any row
  static DG_HD void pack(word* w, const uint32_t* m, int64_t bits, bool last) {
    DG_UNROLL
    for (int i = 0; i < 16; ++i)
      w[i] = ((uint64_t)bswap32(m[2 * i]) << 32) | bswap32(m[2 * i + 1]);
    if (last) {
      w[14] = 0;
      w[15] = (uint64_t)bits;
    }
  }

  static DG_HD void compress(word* s, word* w) {
    constexpr uint64_t K[80] = {
        0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full,
        0xe9b5dba58189dbbcull, 0x3956c25bf348b538ull, 0x59f111f1b605d019ull,
        0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull, 0xd807aa98a3030242ull,
        0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,
        0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull,
        0xc19bf174cf692694ull, 0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull,
        0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull, 0x2de92c6f592b0275ull,
        0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull,
        0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full,
        0xbf597fc7beef0ee4ull, 0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull,
        0x06ca6351e003826full, 0x142929670a0e6e70ull, 0x27b70a8546d22ffcull,
        0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull,
        0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull,
        0x92722c851482353bull, 0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull,
        0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull, 0xd192e819d6ef5218ull,
        0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull,
        0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull,
        0x34b0bcb5e19b48a8ull, 0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull,
        0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull, 0x748f82ee5defb2fcull,
        0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
        0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull,
        0xc67178f2e372532bull, 0xca273eceea26619cull, 0xd186b8c721c0c207ull,
        0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull, 0x06f067aa72176fbaull,
        0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull,
        0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull,
        0x431d67c49c100d4cull, 0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull,
        0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};
    uint64_t a = s[0], b = s[1], c = s[2], d = s[3], e = s[4], f = s[5],
             g = s[6], h = s[7];
    DG_UNROLL
    for (int i = 0; i < 80; ++i) {
      if (i >= 16) {
        uint64_t x = w[(i - 15) & 15], y = w[(i - 2) & 15];
        w[i & 15] += (rotr64(x, 1) ^ rotr64(x, 8) ^ (x >> 7)) +
                     w[(i - 7) & 15] +
                     (rotr64(y, 19) ^ rotr64(y, 61) ^ (y >> 6));
      }
      uint64_t t1 = h + (rotr64(e, 14) ^ rotr64(e, 18) ^ rotr64(e, 41)) +
                    ((e & f) ^ (~e & g)) + K[i] + w[i & 15];
      uint64_t t2 = (rotr64(a, 28) ^ rotr64(a, 34) ^ rotr64(a, 39)) +
                    ((a & b) ^ (a & c) ^ (b & c));
      h = g; g = f; f = e; e = d + t1;
      d = c; c = b; b = a; a = t1 + t2;
    }
    s[0] += a; s[1] += b; s[2] += c; s[3] += d;
    s[4] += e; s[5] += f; s[6] += g; s[7] += h;
  }

  static DG_HD uint32_t out32(const word* s, int k) {
    return bswap32((uint32_t)(s[k >> 1] >> ((k & 1) ? 0 : 32)));
  }
};

struct Sha384 : Sha512 {
  static constexpr int kOut32 = 12;

  static DG_HD void init(word* s) {
    s[0] = 0xcbbb9d5dc1059ed8ull; s[1] = 0x629a292a367cd507ull;
    s[2] = 0x9159015a3070dd17ull; s[3] = 0x152fecd8f70e5939ull;
    s[4] = 0x67332667ffc00b31ull; s[5] = 0x8eb44a8768581511ull;
    s[6] = 0xdb0c2e0d64f98fa7ull; s[7] = 0x47b5481dbefa4fa4ull;
  }
};

// ---------------------------------------------------------------------------
// One row: whole blocks straight from aligned loads, then the last one or
// two blocks with the 0x80 pad, the zero fill and the bit length. A block is
// a "last" block as soon as the aligned word after it is not wholly inside
// the row; there every word goes through the guarded fetch, which reads
// bytes past the row's end as zero, so the zero fill needs no code of its
// own. When the pad and the length do not fit behind the row's last bytes
// the loop simply runs one block more.
// ---------------------------------------------------------------------------

template <class A>
DG_HD void digest_row(const uint8_t* p, int64_t len, typename A::word* st) {
  constexpr int kBlock = A::kBlockBytes;
  constexpr int kWords = kBlock / 4;      // 32-bit message words per block
  constexpr int kLenBytes = kBlock / 8;   // 8, or 16 for the 128-byte block
  const RowReader rd(p, len);
  const int64_t nblocks = (len + 1 + kLenBytes + kBlock - 1) / kBlock;
  A::init(st);
  uint32_t carry = rd.fetch(0);
  for (int64_t b = 0; b < nblocks; ++b) {
    const int64_t pos = b * kBlock;  // row-relative
    const int64_t j0 = b * kWords;
    uint32_t m[kWords];
    if (pos + kBlock + 4 <= len) {
      DG_UNROLL
      for (int i = 0; i < kWords; ++i) {
        uint32_t next = rd.load(j0 + i + 1);
        m[i] = rd.join(carry, next);
        carry = next;
      }
    } else {
      DG_UNROLL
      for (int i = 0; i < kWords; ++i) {
        uint32_t next = rd.fetch(j0 + i + 1);
        m[i] = rd.join(carry, next);
        carry = next;
        int64_t d = len - (pos + 4 * i);  // where the 0x80 pad byte goes
        if (d >= 0 && d < 4) m[i] |= 0x80u << (8 * (int)d);
      }
    }
    typename A::word w[16];
    A::pack(w, m, len * 8, b == nblocks - 1);
    A::compress(st, w);
  }
}

// ---------------------------------------------------------------------------
// Lowercase hex
// ---------------------------------------------------------------------------

// Four bytes (the first in the low byte of v) as eight lowercase hex digits,
// the first digit in the low byte of the result: store it little-endian.
DG_HD uint64_t hex8(uint32_t v) {
  uint64_t t = v;
  t = (t | (t << 16)) & 0x0000ffff0000ffffull;
  t = (t | (t << 8)) & 0x00ff00ff00ff00ffull;
  // per 16-bit lane: high nibble into the low byte, low nibble above it
  uint64_t n = ((t >> 4) & 0x000f000f000f000full) |
               ((t & 0x000f000f000f000full) << 8);
  // bytes above 9 carry into bit 4 when 6 is added
  uint64_t af = ((n + 0x0606060606060606ull) >> 4) & 0x0101010101010101ull;
  return n + 0x3030303030303030ull + af * 39;  // '0' + n, 'a' - 10 + n
}

template <class A>
constexpr int hex_width() { return A::kOut32 * 8; }

// the row's digest as hex_width<A>() lowercase hex digits, no terminator
template <class A>
DG_HD void digest_hex(const uint8_t* p, int64_t len, uint8_t* out) {
  typename A::word st[A::kState];
  digest_row<A>(p, len, st);
  DG_UNROLL
  for (int k = 0; k < A::kOut32; ++k) {
    uint64_t h = hex8(A::out32(st, k));
    memcpy(out + 8 * k, &h, 8);
  }
}

// ---------------------------------------------------------------------------
// CRC-32, table-driven, one byte per lookup. The table is built at compile
// time; the device kernel stages it into LDS and passes that copy in.
// ---------------------------------------------------------------------------

struct Crc32Table {
  uint32_t t[256];
};

constexpr Crc32Table make_crc32_table() {
  Crc32Table tab{};
  for (uint32_t i = 0; i < 256; ++i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xedb88320u ^ (c >> 1) : c >> 1;
    tab.t[i] = c;
  }
  return tab;
}

DG_HD uint32_t crc32_byte(const uint32_t* tab, uint32_t crc, uint32_t byte) {
  return tab[(crc ^ byte) & 0xff] ^ (crc >> 8);
}

DG_HD uint32_t crc32_word(const uint32_t* tab, uint32_t crc, uint32_t v) {
  crc = crc32_byte(tab, crc, v & 0xff);
  crc = crc32_byte(tab, crc, (v >> 8) & 0xff);
  crc = crc32_byte(tab, crc, (v >> 16) & 0xff);
  return crc32_byte(tab, crc, v >> 24);
}

// Bytes up to the first aligned word, words up to the first 16-byte
// boundary, then 64 bytes at a time as four 16-byte loads issued together
// (with one word per load, a wave whose rows lie far apart touches every
// cache line 32 times and loses it in between), then words, then bytes.
DG_HD uint32_t crc32_row(const uint32_t* tab, const uint8_t* p, int64_t len) {
  uint32_t crc = 0xffffffffu;
  int64_t i = 0;
  for (; i < len && ((uintptr_t)(p + i) & 3); ++i)  // head
    crc = crc32_byte(tab, crc, p[i]);
  for (; i + 4 <= len && ((uintptr_t)(p + i) & 15); i += 4)
    crc = crc32_word(tab, crc, load_u32(p + i));
  for (; i + 64 <= len; i += 64) {
    const u32x4_alias* q = reinterpret_cast<const u32x4_alias*>(p + i);
    u32x4_alias v[4] = {q[0], q[1], q[2], q[3]};
    DG_UNROLL
    for (int k = 0; k < 4; ++k) {
      crc = crc32_word(tab, crc, v[k][0]);
      crc = crc32_word(tab, crc, v[k][1]);
      crc = crc32_word(tab, crc, v[k][2]);
      crc = crc32_word(tab, crc, v[k][3]);
    }
  }
  for (; i + 4 <= len; i += 4) crc = crc32_word(tab, crc, load_u32(p + i));
  for (; i < len; ++i) crc = crc32_byte(tab, crc, p[i]);  // tail
  return ~crc;
}

}  // namespace digest
