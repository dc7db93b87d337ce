// Host-only walk of one parquet column chunk's page headers for the native
// scan reader: is the chunk nothing but PLAIN fixed-width values, and where
// do each page's values lie? No HIP calls, so the walker also builds into a
// plain host program (tests/pq_pieces_host_test.cpp) under the sanitizers.
//
// Every read goes through Cursor, which never touches a byte at or beyond
// `end`; a header that runs off the chunk is an error, not a fault.
#ifndef HIPDF_PQ_PIECES_H
#define HIPDF_PQ_PIECES_H

#include <stdint.h>

namespace pq_pieces {

// error codes of walk() (all negative)
constexpr int64_t kErrTruncated = -1;    // a header or page runs past nbytes
constexpr int64_t kErrDictionary = -2;   // dictionary page
constexpr int64_t kErrEncoding = -3;     // a data page that is not PLAIN
constexpr int64_t kErrCompressed = -4;   // compressed, or sizes disagree
constexpr int64_t kErrWidth = -5;        // physical width is not 4 or 8
constexpr int64_t kErrNulls = -6;        // def levels are not all-valid
constexpr int64_t kErrNested = -7;       // repetition levels present
constexpr int64_t kErrMalformed = -8;    // thrift that parquet does not write
constexpr int64_t kErrCapacity = -9;     // more pages than max_out
constexpr int64_t kErrCount = -10;       // pages do not add up to num_values

struct Cursor {
  const uint8_t* p;
  int64_t pos;
  int64_t end;
  bool ok;

  int byte() {
    if (pos >= end) {
      ok = false;
      return 0;
    }
    return p[pos++];
  }
  uint64_t varint() {
    uint64_t out = 0;
    for (int shift = 0; shift < 64; shift += 7) {
      int b = byte();
      if (!ok) return 0;
      out |= (uint64_t)(b & 0x7F) << shift;
      if (!(b & 0x80)) return out;
    }
    ok = false;  // longer than any i64
    return 0;
  }
  int64_t zigzag() {
    uint64_t v = varint();
    return (int64_t)(v >> 1) ^ -(int64_t)(v & 1);
  }
  void advance(uint64_t n) {
    if (n > (uint64_t)(end - pos)) {
      ok = false;
      return;
    }
    pos += (int64_t)n;
  }
};

enum { CT_STOP = 0, CT_TRUE = 1, CT_FALSE = 2, CT_BYTE = 3, CT_I16 = 4,
       CT_I32 = 5, CT_I64 = 6, CT_DOUBLE = 7, CT_BINARY = 8, CT_LIST = 9,
       CT_SET = 10, CT_MAP = 11, CT_STRUCT = 12 };

inline void skip_struct(Cursor& c, int depth);

inline void skip_value(Cursor& c, int ctype, int depth) {
  if (!c.ok) return;
  switch (ctype) {
    case CT_TRUE:
    case CT_FALSE:
      return;
    case CT_BYTE:
      c.advance(1);
      return;
    case CT_I16:
    case CT_I32:
    case CT_I64:
      c.varint();
      return;
    case CT_DOUBLE:
      c.advance(8);
      return;
    case CT_BINARY:
      c.advance(c.varint());
      return;
    case CT_STRUCT:
      skip_struct(c, depth + 1);
      return;
    case CT_LIST:
    case CT_SET: {
      int h = c.byte();
      uint64_t size = (uint64_t)(h >> 4);
      int et = h & 0x0F;
      if (size == 15) size = c.varint();
      // booleans in a list take a byte each, unlike struct fields
      if (et == CT_TRUE || et == CT_FALSE) {
        c.advance(size);
        return;
      }
      for (uint64_t i = 0; i < size && c.ok; ++i) skip_value(c, et, depth);
      return;
    }
    default:
      c.ok = false;  // maps do not occur in a page header
  }
}

// iterate the fields of a compact struct: returns the field id (> 0) and
// its type, or 0 at the stop byte / on error
struct Fields {
  Cursor& c;
  int last = 0;
  explicit Fields(Cursor& cur) : c(cur) {}
  int next(int* ctype) {
    int b = c.byte();
    if (!c.ok || b == CT_STOP) return 0;
    int delta = b >> 4;
    *ctype = b & 0x0F;
    if (delta == 0)
      last = (int)c.zigzag();
    else
      last += delta;
    if (!c.ok || last <= 0) {
      c.ok = false;
      return 0;
    }
    return last;
  }
};

inline void skip_struct(Cursor& c, int depth) {
  if (depth > 8) {
    c.ok = false;
    return;
  }
  Fields f(c);
  int t;
  while (f.next(&t)) skip_value(c, t, depth);
}

// the def-level stream of a page holds n copies of max_def as plain RLE runs
// (what the python reader's _rle_all_valid accepts)
inline bool rle_all_valid(const uint8_t* lv, int64_t nb, int64_t n,
                          int max_def) {
  Cursor c{lv, 0, nb, true};
  int64_t seen = 0;
  while (seen < n) {
    uint64_t h = c.varint();
    if (!c.ok) return false;
    if (h & 1) return false;  // bit-packed run: a mix of levels
    uint64_t count = h >> 1;
    int v = c.byte();
    if (!c.ok || v != max_def || count == 0) return false;
    if (count > (uint64_t)(n - seen)) count = (uint64_t)(n - seen);
    seen += (int64_t)count;
  }
  return true;
}

// The walk behind walk() and walk_levels(). with_levels = false: three
// entries per page and every page all-valid. with_levels = true: five entries
// per page (kLevelStride), pages with nulls accepted for max_def <= 1.
inline int64_t walk_impl(const uint8_t* chunk, int64_t nbytes,
                         int64_t num_values, int max_def, int phys_width,
                         int64_t* out, int64_t max_out, bool with_levels) {
  const int stride = with_levels ? 5 : 3;
  if (phys_width != 4 && phys_width != 8) return kErrWidth;
  if (nbytes < 0 || num_values < 0 || max_def < 0 || max_def > 127)
    return kErrMalformed;
  if (with_levels && max_def > 1) return kErrNulls;
  Cursor c{chunk, 0, nbytes, true};
  int64_t decoded = 0, npages = 0;
  while (decoded < num_values && c.pos < nbytes) {
    int64_t type = -1, usize = -1, csize = -1;
    // v1 / v2 data page header fields
    int64_t n = -1, enc = -1, nulls = 0, def_len = 0, rep_len = 0;
    bool v2 = false, have_dp = false, v2_compressed = true;
    Fields f(c);
    int t;
    int fid;
    while ((fid = f.next(&t)) != 0) {
      if (fid == 1 && t == CT_I32) {
        type = c.zigzag();
      } else if (fid == 2 && t == CT_I32) {
        usize = c.zigzag();
      } else if (fid == 3 && t == CT_I32) {
        csize = c.zigzag();
      } else if (fid == 5 && t == CT_STRUCT) {
        have_dp = true;
        Fields g(c);
        int t2, f2;
        while ((f2 = g.next(&t2)) != 0) {
          if (f2 == 1 && t2 == CT_I32)
            n = c.zigzag();
          else if (f2 == 2 && t2 == CT_I32)
            enc = c.zigzag();
          else
            skip_value(c, t2, 1);
        }
      } else if (fid == 7 && t == CT_STRUCT) {
        return kErrDictionary;
      } else if (fid == 8 && t == CT_STRUCT) {
        have_dp = v2 = true;
        Fields g(c);
        int t2, f2;
        while ((f2 = g.next(&t2)) != 0) {
          if (f2 == 1 && t2 == CT_I32)
            n = c.zigzag();
          else if (f2 == 2 && t2 == CT_I32)
            nulls = c.zigzag();
          else if (f2 == 4 && t2 == CT_I32)
            enc = c.zigzag();
          else if (f2 == 5 && t2 == CT_I32)
            def_len = c.zigzag();
          else if (f2 == 6 && t2 == CT_I32)
            rep_len = c.zigzag();
          else if (f2 == 7 && (t2 == CT_TRUE || t2 == CT_FALSE))
            v2_compressed = t2 == CT_TRUE;
          else
            skip_value(c, t2, 1);
        }
      } else {
        skip_value(c, t, 0);
      }
      if (!c.ok) return kErrTruncated;
    }
    if (!c.ok) return kErrTruncated;
    if (type == 2) return kErrDictionary;
    if ((type != 0 && type != 3) || !have_dp || (type == 3) != v2)
      return kErrMalformed;
    if (usize < 0 || csize < 0 || n < 0) return kErrMalformed;
    if (csize > nbytes - c.pos) return kErrTruncated;
    if (enc != 0) return kErrEncoding;
    if (csize != usize) return kErrCompressed;
    const int64_t page = c.pos;  // first payload byte
    int64_t vpos = 0;            // values start, relative to the payload
    int64_t lpos = 0, llen = 0;  // def-level stream, relative to the payload
    if (!v2) {
      if (max_def > 0) {
        if (csize < 4) return kErrTruncated;
        uint32_t len = (uint32_t)chunk[page] | (uint32_t)chunk[page + 1] << 8 |
                       (uint32_t)chunk[page + 2] << 16 |
                       (uint32_t)chunk[page + 3] << 24;
        if ((int64_t)len > csize - 4) return kErrTruncated;
        if (!with_levels &&
            !rle_all_valid(chunk + page + 4, (int64_t)len, n, max_def))
          return kErrNulls;
        lpos = 4;
        llen = (int64_t)len;
        vpos = 4 + (int64_t)len;
      }
    } else {
      if (rep_len != 0) return kErrNested;
      if (def_len < 0 || def_len > csize) return kErrMalformed;
      if (max_def > 0) {
        if (!with_levels) {
          if (nulls != 0) return kErrNulls;
          if (!rle_all_valid(chunk + page, def_len, n, max_def))
            return kErrNulls;
        }
        llen = def_len;
      } else if (def_len != 0) {
        return kErrMalformed;
      }
      // an uncompressed chunk may still say is_compressed; what counts is
      // that the value bytes below are exactly n fixed-width values
      (void)v2_compressed;
      vpos = def_len;
    }
    // n * width cannot overflow: n is an i32
    const int64_t vbytes = csize - vpos;
    if (with_levels && max_def > 0) {
      // the values are dense: how many there are is known only once the
      // levels are decoded, and checked there
      if (vbytes % phys_width != 0 || vbytes > n * (int64_t)phys_width)
        return kErrCompressed;
    } else if (vbytes != n * (int64_t)phys_width) {
      return kErrCompressed;
    }
    if (n > num_values - decoded) return kErrCount;
    if (npages >= max_out) return kErrCapacity;
    out[stride * npages] = page + vpos;
    out[stride * npages + 1] = vbytes;
    out[stride * npages + 2] = n;
    if (with_levels) {
      out[stride * npages + 3] = page + lpos;
      out[stride * npages + 4] = llen;
    }
    ++npages;
    decoded += n;
    c.pos = page + csize;
  }
  if (decoded != num_values) return decoded < num_values ? kErrTruncated
                                                         : kErrCount;
  return npages;
}

// One entry per data page: out[3k] = offset of the page's values from the
// start of the chunk, out[3k+1] = their byte length, out[3k+2] = number of
// values. Returns the number of pages or a negative kErr* code.
inline int64_t walk(const uint8_t* chunk, int64_t nbytes, int64_t num_values,
                    int max_def, int phys_width, int64_t* out,
                    int64_t max_out) {
  return walk_impl(chunk, nbytes, num_values, max_def, phys_width, out,
                   max_out, false);
}

}  // namespace pq_pieces

#endif  // HIPDF_PQ_PIECES_H
