// Host-only decode of a parquet data page's definition levels for the native
// scan reader's nullable pieces: the RLE / bit-packed hybrid at bit width 1
// (max_def == 1, no repetition levels) becomes an LSB-first validity bitmask
// plus a table of exclusive valid counts per tile of rows. At bit width 1 a
// bit-packed run already is such a bitmask, so aligned runs are byte copies.
// No HIP calls: builds into tests/pq_levels_host_test.cpp under the
// sanitizers.
//
// Every read of the stream goes through pq_pieces::Cursor: no byte at or
// beyond its end is touched, and a stream that ends before n levels is an
// error.
#ifndef HIPDF_PQ_LEVELS_H
#define HIPDF_PQ_LEVELS_H

#include <stdint.h>
#include <string.h>

#include "pq_pieces.h"

namespace pq_pieces {

constexpr int64_t kErrLevels = -11;  // a level stream parquet does not write

constexpr int kLevelStride = 5;      // int64 entries per page of walk_levels
constexpr int kTileRows = 2048;      // rows per entry of the count table

// As walk(), for chunks that may hold nulls (max_def <= 1): five entries per
// data page, the three of walk() (with the byte length of the DENSE values,
// a multiple of the width and at most n * width) followed by out[5k+3] =
// offset of the page's definition-level stream from the start of the chunk
// (v1: behind its 4-byte length prefix) and out[5k+4] = its byte length
// (0 when max_def == 0).
inline int64_t walk_levels(const uint8_t* chunk, int64_t nbytes,
                           int64_t num_values, int max_def, int phys_width,
                           int64_t* out, int64_t max_out) {
  return walk_impl(chunk, nbytes, num_values, max_def, phys_width, out,
                   max_out, true);
}

// bytes of mask a page of n rows needs: whole tiles, so that a slice of the
// page that starts on a tile starts on a 64-bit word
inline int64_t mask_bytes(int64_t n) {
  return (n + kTileRows - 1) / kTileRows * (kTileRows / 8);
}
inline int64_t tile_entries(int64_t n) {
  return (n + kTileRows - 1) / kTileRows + 1;
}

// set bits [pos, pos + count) of an LSB-first bitmask
inline void fill_ones(uint8_t* mask, int64_t pos, int64_t count) {
  int64_t end = pos + count;
  int64_t b0 = pos >> 3, b1 = end >> 3;
  if (b0 == b1) {
    mask[b0] |= (uint8_t)(((1u << count) - 1u) << (pos & 7));
    return;
  }
  if (pos & 7) {
    mask[b0] |= (uint8_t)(0xFFu << (pos & 7));
    ++b0;
  }
  if (b1 > b0) memset(mask + b0, 0xFF, (size_t)(b1 - b0));
  if (end & 7) mask[b1] |= (uint8_t)((1u << (end & 7)) - 1u);
}

// Decodes n definition levels of bit width 1 from lv[0, nb). mask receives
// mask_bytes(n) bytes (bit r set = row r valid, bits at and beyond n zero);
// tiles receives tile_entries(n) counts, tiles[t] = valid rows before row
// t * kTileRows, the last entry being the total. Returns the number of valid
// rows or a negative kErr* code.
inline int64_t decode_levels(const uint8_t* lv, int64_t nb, int64_t n,
                             uint8_t* mask, uint32_t* tiles) {
  if (nb < 0 || n < 0 || n > INT32_MAX) return kErrMalformed;
  memset(mask, 0, (size_t)mask_bytes(n));
  Cursor c{lv, 0, nb, true};
  int64_t pos = 0;
  while (pos < n) {
    uint64_t h = c.varint();
    if (!c.ok) return kErrTruncated;
    uint64_t count = h >> 1;
    if (count == 0) return kErrLevels;
    if (!(h & 1)) {  // RLE run: one byte of value
      int v = c.byte();
      if (!c.ok) return kErrTruncated;
      if (v != 0 && v != 1) return kErrLevels;
      if (count > (uint64_t)(n - pos)) count = (uint64_t)(n - pos);
      if (v) fill_ones(mask, pos, (int64_t)count);
      pos += (int64_t)count;
      continue;
    }
    // bit-packed run: `count` groups of 8 levels, one byte each; the last
    // group of a page may be padded beyond n, and those bits are dropped
    uint64_t rows = count > (uint64_t)(n - pos + 7) / 8
                        ? (uint64_t)(n - pos)
                        : count * 8;
    if (rows > (uint64_t)(n - pos)) rows = (uint64_t)(n - pos);
    const int64_t bytes = (int64_t)((rows + 7) / 8);
    const int64_t at = c.pos;
    c.advance((uint64_t)bytes);
    if (!c.ok) return kErrTruncated;
    const uint8_t* src = lv + at;
    const int sh = (int)(pos & 7);
    uint8_t* dst = mask + (pos >> 3);
    const int tail = (int)(rows & 7);  // levels in a partial last byte
    if (sh == 0) {
      memcpy(dst, src, (size_t)bytes);
      if (tail) dst[bytes - 1] &= (uint8_t)((1u << tail) - 1u);
    } else {
      for (int64_t i = 0; i < bytes; ++i) {
        unsigned b = src[i];
        if (tail && i == bytes - 1) b &= (1u << tail) - 1u;
        dst[i] |= (uint8_t)(b << sh);
        // the high part is empty whenever it would lie beyond the mask
        if (b >> (8 - sh)) dst[i + 1] |= (uint8_t)(b >> (8 - sh));
      }
    }
    pos += (int64_t)rows;
  }
  // tile counts from the finished mask: one popcount per 64 rows
  const int64_t ntiles = tile_entries(n) - 1;
  uint32_t total = 0;
  for (int64_t t = 0; t < ntiles; ++t) {
    tiles[t] = total;
    const uint8_t* p = mask + t * (kTileRows / 8);
    for (int w = 0; w < kTileRows / 64; ++w) {
      uint64_t word;
      memcpy(&word, p + 8 * w, 8);
      total += (uint32_t)__builtin_popcountll(word);
    }
  }
  tiles[ntiles] = total;
  return (int64_t)total;
}

}  // namespace pq_pieces

#endif  // HIPDF_PQ_LEVELS_H
