// Host-side description of one sort key column for hipdf_sort_order
// (sort.hip); shared with the pybind module, which fills it from python.
#pragma once

#include <stdint.h>

enum HipdfSortKind : int32_t {
  SORT_KEY_FIXED = 0,       // one u64 key per row from an HType column
  SORT_KEY_STRING = 1,      // nchunks 8-byte big-endian chunks, last first
  SORT_KEY_DECIMAL128 = 2,  // interleaved (lo, hi) int64 pairs: lo then hi
};

struct HipdfSortKey {
  int32_t kind;         // HipdfSortKind
  int32_t htype;        // HType of data (fixed keys only)
  const void* data;     // values; string bytes for SORT_KEY_STRING
  const void* valid;    // validity bitmask, or null
  const void* offsets;  // int32 string offsets (SORT_KEY_STRING only)
  int32_t desc;
  int32_t nulls_last;
  int32_t has_valid;    // the column carries a validity mask
  int32_t nchunks;      // ceil(max string length / 8), at least 1
};
