// get_json_object row parser: a validating JSON tokenizer with a path
// matcher (size pass) and a normalising writer (write pass).
//
// The same code compiles for the device (under hipcc, called by the kernels
// in json.hip) and as plain C++ for a host program, so a host test runs
// exactly what the kernel runs. No HIP types appear in the interface.
//
// scan_row() walks one whole row, because validity is a property of the whole
// document, and answers what Python's json.loads + a path walk + json.dumps
// would answer: NULL (JP_NULL), a value whose rendering the writer reproduces
// byte for byte (JP_VALUE), or "ask the host" (JP_FLAG) where the host's
// rendering cannot be reproduced cheaply (non-canonical floats, escapes
// inside a container result, ...). write_row() re-reads only the matched
// span and emits the normalised bytes.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define JP_HD __host__ __device__ __forceinline__
#else
#define JP_HD inline
#endif

namespace jsonpath {

enum : uint8_t { JP_NULL = 0, JP_VALUE = 1, JP_FLAG = 2 };

constexpr int kMaxDepth = 64;         // one bit per level in the stack word
constexpr int kMaxIntDigits = 1000;   // longer integers go to the host
constexpr int kMaxFloatDigits = 15;   // digits that round-trip through repr

// Encoded path: int32 triples [kind, a, b] per step. kind 0 = key whose name
// is names[a .. a+b), kind 1 = array index a.
struct Path {
  const int32_t* steps;
  const uint8_t* names;
  int nsteps;
};

struct RowResult {
  int64_t out_len;    // bytes the writer emits (JP_VALUE only)
  int32_t src_start;  // matched value's span in the source bytes
  int32_t src_len;
  uint8_t state;
};

// Source bytes come through aligned 8-byte words held in a register: a row
// is read front to back, so one load serves eight positions. The word that
// holds a row's first or last byte may reach outside the row; an aligned
// word never crosses a page, so the device reads it whole. The host build
// assembles the word from the bytes inside [lo, hi) only.
struct ByteReader {
  const uint8_t* base;  // data - misalignment: an 8-byte aligned address
  int64_t mis;
  int64_t cur;          // index of the word held, -1 for none
  uint64_t word;
  int64_t lo, hi;       // readable positions (host build)

  JP_HD ByteReader(const uint8_t* data, int64_t lo_, int64_t hi_)
      : base(data - ((uintptr_t)data & 7)), mis((int64_t)((uintptr_t)data & 7)),
        cur(-1), word(0), lo(lo_), hi(hi_) {}

  JP_HD uint8_t at(int64_t p) {
    int64_t q = p + mis;
    int64_t wi = q >> 3;
    if (wi != cur) {
      cur = wi;
#if defined(__HIP_DEVICE_COMPILE__)
      word = *reinterpret_cast<const uint64_t*>(base + wi * 8);
#else
      word = 0;
      for (int k = 0; k < 8; ++k) {
        int64_t pos = wi * 8 + k - mis;
        if (pos >= lo && pos < hi)
          word |= (uint64_t)base[wi * 8 + k] << (8 * k);
      }
#endif
    }
    return (uint8_t)(word >> ((q & 7) * 8));
  }
};

JP_HD bool is_ws(uint8_t c) {
  return c == ' ' || c == '\t' || c == '\n' || c == '\r';
}

JP_HD int hex_val(uint8_t c) {
  if (c >= '0' && c <= '9') return c - '0';
  c |= 0x20;
  if (c >= 'a' && c <= 'f') return c - 'a' + 10;
  return -1;
}

JP_HD bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }

// One row's parser state. Everything is a scalar so that it stays in
// registers; there is no per-level array. The container stack is one 64-bit
// word (bit = object), and path matching needs only the depth of the
// innermost container that lies on the path (`on`): its parents lie on the
// path too, an array parent can match its index only once, and an object
// parent needs no counter.
//
// MultiRowScanner below is this scanner with the matcher state held once per
// path: its tokenizer and validator (scan_string, scan_number, scan_literal,
// close_container, run) repeat the ones here, and its contract is to answer
// what this one answers. A change to either goes into both;
// native/hipdf/tests/json_multi_host_test.cpp holds them against each other.
struct RowScanner {
  ByteReader rd;
  Path path;
  int32_t p, re;
  uint64_t stack;
  int depth;
  int on;            // depth of the innermost open on-path container, 0 = none
  int32_t elem;      // element counter of that container when it is an array
  bool pending;      // the next value is the one the current step selects
  bool in_target;    // inside a container that is the result
  int target_depth;
  int32_t nws, nws0;  // whitespace bytes seen outside strings / at target start
  bool tflag;        // the container result holds something to flag
  bool hard_flag;    // flag whatever the result is
  RowResult res;

  JP_HD RowScanner(const uint8_t* data, int32_t rs, int32_t re_, Path path_)
      : rd(data, rs, re_), path(path_), p(rs), re(re_), stack(0), depth(0),
        on(0), elem(0), pending(true), in_target(false), target_depth(0),
        nws(0), nws0(0), tflag(false), hard_flag(false) {
    res.out_len = 0;
    res.src_start = 0;
    res.src_len = 0;
    res.state = JP_NULL;
  }

  JP_HD void set_result(int32_t start, int32_t len, int64_t out_len,
                        bool flag) {
    res.src_start = start;
    res.src_len = len;
    res.out_len = out_len;
    res.state = flag ? JP_FLAG : JP_VALUE;
  }

  // p is at the opening quote. vmode: 0 validate only, 1 the string is the
  // result, 2 inside a container result. match_key: compare the raw bytes
  // with the current key step's name. Leaves p behind the closing quote.
  JP_HD bool scan_string(int vmode, bool match_key, bool* key_hit) {
    int32_t start = p;
    int32_t name_at = 0, name_len = 0, k = 0;
    if (match_key) {
      name_at = path.steps[(on - 1) * 3 + 1];
      name_len = path.steps[(on - 1) * 3 + 2];
    }
    bool same = true, has_bs = false, has_hi = false;
    bool hi_pending = false, lone = false;
    int64_t declen = 0;
    ++p;
    for (;;) {
      if (p >= re) return false;  // unterminated
      uint8_t c = rd.at(p);
      if (c == '"') break;
      if (c < 0x20) return false;
      if (c == '\\') {
        has_bs = true;
        if (++p >= re) return false;
        uint8_t e = rd.at(p);
        if (e == 'u') {
          if (p + 4 >= re) return false;
          int cp = 0;
          for (int j = 1; j <= 4; ++j) {
            int h = hex_val(rd.at(p + j));
            if (h < 0) return false;
            cp = cp * 16 + h;
          }
          p += 5;
          if (cp >= 0xDC00 && cp <= 0xDFFF) {
            if (hi_pending) declen += 4; else lone = true;
            hi_pending = false;
            continue;
          }
          if (hi_pending) lone = true;
          hi_pending = cp >= 0xD800 && cp <= 0xDBFF;
          if (!hi_pending) declen += cp < 0x80 ? 1 : cp < 0x800 ? 2 : 3;
          continue;
        }
        if (!(e == '"' || e == '\\' || e == '/' || e == 'b' || e == 'f' ||
              e == 'n' || e == 'r' || e == 't'))
          return false;
        if (hi_pending) { lone = true; hi_pending = false; }
        ++declen;
        ++p;
        continue;
      }
      if (hi_pending) { lone = true; hi_pending = false; }
      if (c >= 0x80) has_hi = true;
      if (match_key) {
        if (k < name_len && path.names[name_at + k] == c) ++k;
        else same = false;
      }
      ++declen;
      ++p;
    }
    ++p;  // closing quote
    if (hi_pending) lone = true;
    if (match_key) {
      // an escaped key might decode to the name: the host decides
      if (has_bs) hard_flag = true;
      else *key_hit = same && k == name_len;
    }
    if (vmode == 1) set_result(start, p - start, declen, lone);
    else if (vmode == 2 && (has_bs || has_hi)) tflag = true;
    return true;
  }

  // p is at '-' or a digit. Leaves p behind the number.
  JP_HD bool scan_number(int vmode) {
    int32_t start = p;
    bool neg = rd.at(p) == '-';
    if (neg && ++p >= re) return false;
    uint8_t c = rd.at(p);
    if (neg && c == 'I') return scan_literal(vmode, start);
    int intd = 0, fracd = 0, lead_zeros = 0;
    bool zero_int = c == '0', is_float = false, has_exp = false;
    bool seen_nonzero = false;
    uint8_t last_frac = 0;
    if (zero_int) {
      ++p;
      intd = 1;
    } else if (is_digit(c)) {
      while (p < re && is_digit(rd.at(p))) { ++p; ++intd; }
    } else {
      return false;
    }
    if (p < re && rd.at(p) == '.') {
      is_float = true;
      ++p;
      while (p < re && is_digit(c = rd.at(p))) {
        if (c != '0') seen_nonzero = true;
        else if (!seen_nonzero) ++lead_zeros;
        last_frac = c;
        ++fracd;
        ++p;
      }
      if (fracd == 0) return false;
    }
    if (p < re && (rd.at(p) | 0x20) == 'e') {
      is_float = has_exp = true;
      ++p;
      if (p < re && (rd.at(p) == '+' || rd.at(p) == '-')) ++p;
      int expd = 0;
      while (p < re && is_digit(rd.at(p))) { ++p; ++expd; }
      if (expd == 0) return false;
    }
    if (vmode == 0) return true;
    bool flag;
    if (!is_float) {
      flag = (neg && zero_int) || intd > kMaxIntDigits;
    } else {
      // verbatim only where Python's repr of the parsed double is the text
      flag = has_exp || intd + fracd > kMaxFloatDigits ||
             (last_frac == '0' && fracd > 1) || (zero_int && lead_zeros >= 4);
    }
    if (vmode == 1) set_result(start, p - start, p - start, flag);
    else if (flag) tflag = true;
    return true;
  }

  JP_HD bool word_is(int32_t at, const char* w, int n) {
    if (at + n > re) return false;
    for (int j = 0; j < n; ++j)
      if (rd.at(at + j) != (uint8_t)w[j]) return false;
    return true;
  }

  // true, false, null, and the literals only Python reads: NaN, Infinity,
  // -Infinity (start is then at the '-').
  JP_HD bool scan_literal(int vmode, int32_t start) {
    uint8_t c = rd.at(p);
    int n;
    if (c == 't' && word_is(p, "true", 4)) n = 4;
    else if (c == 'f' && word_is(p, "false", 5)) n = 5;
    else if (c == 'n' && word_is(p, "null", 4)) n = 4;
    else if (c == 'N' && word_is(p, "NaN", 3)) { n = 3; hard_flag = true; }
    else if (c == 'I' && word_is(p, "Infinity", 8)) { n = 8; hard_flag = true; }
    else return false;
    p += n;
    // a null result stays NULL
    if (vmode == 1 && c != 'n') set_result(start, p - start, p - start, false);
    return true;
  }

  JP_HD void close_container() {
    if (depth == on) {
      // back in the parent, which lies on the path as well; an array parent
      // has had its one match
      on = depth - 1;
      if (on > 0 && !((stack >> 1) & 1)) elem = INT32_MIN;
    }
    stack >>= 1;
    --depth;
    ++p;
    if (in_target && depth == target_depth) {
      in_target = false;
      int32_t len = p - res.src_start;
      set_result(res.src_start, len, len - (nws - nws0), tflag);
    }
  }

  JP_HD RowResult run() {
    enum { ST_VALUE, ST_ARR_FIRST, ST_OBJ_FIRST, ST_KEY, ST_COLON, ST_AFTER };
    int st = ST_VALUE;
    bool ok = true;
    while (ok) {
      uint8_t c = 0;
      while (p < re && is_ws(c = rd.at(p))) { ++p; ++nws; }
      if (p >= re) break;
      if (st == ST_AFTER) {
        if (depth == 0) { ok = false; break; }  // trailing text
        bool obj = stack & 1;
        if (c == ',') {
          st = obj ? ST_KEY : ST_VALUE;
          ++p;
        } else if (c == (obj ? '}' : ']')) {
          close_container();
        } else {
          ok = false;
        }
        continue;
      }
      if (st == ST_COLON) {
        ok = c == ':';
        st = ST_VALUE;
        ++p;
        continue;
      }
      if (st == ST_OBJ_FIRST || st == ST_KEY) {
        if (c == '}' && st == ST_OBJ_FIRST) {
          close_container();
          st = ST_AFTER;
          continue;
        }
        if (c != '"') { ok = false; break; }
        bool match_key = depth == on && path.steps[(on - 1) * 3] == 0;
        bool hit = false;
        ok = scan_string(in_target ? 2 : 0, match_key, &hit);
        if (hit) pending = true;
        st = ST_COLON;
        continue;
      }
      if (st == ST_ARR_FIRST && c == ']') {
        close_container();
        st = ST_AFTER;
        continue;
      }
      // a value starts here
      bool sel = pending;
      pending = false;
      if (depth == on && depth > 0 && !(stack & 1)) {
        sel = path.steps[(on - 1) * 3] == 1 &&
              elem == path.steps[(on - 1) * 3 + 1];
        ++elem;
      }
      // a later duplicate of a matched key replaces what the earlier one gave
      if (sel) res.state = JP_NULL;
      bool is_target = sel && depth == path.nsteps;
      int vmode = is_target ? 1 : in_target ? 2 : 0;
      st = ST_AFTER;
      if (c == '{' || c == '[') {
        if (depth == kMaxDepth) {
          res.state = JP_FLAG;
          return res;
        }
        if (is_target) {
          in_target = true;
          target_depth = depth;
          res.src_start = p;
          nws0 = nws;
          tflag = false;
        } else if (sel) {
          on = depth + 1;
          elem = 0;
        }
        stack = (stack << 1) | (c == '{' ? 1u : 0u);
        ++depth;
        ++p;
        st = c == '{' ? ST_OBJ_FIRST : ST_ARR_FIRST;
      } else if (c == '"') {
        bool hit;
        ok = scan_string(vmode, false, &hit);
      } else if (c == '-' || is_digit(c)) {
        ok = scan_number(vmode);
      } else {
        ok = scan_literal(vmode, p);
      }
    }
    if (!ok || st != ST_AFTER || depth != 0) {
      res.state = JP_NULL;
    } else if (hard_flag) {
      res.state = JP_FLAG;
    }
    if (res.state != JP_VALUE) res.out_len = 0;
    return res;
  }
};

// Size pass for one row [rs, re) of `data`.
JP_HD RowResult scan_row(const uint8_t* data, int32_t rs, int32_t re,
                         Path path) {
  RowScanner sc(data, rs, re, path);
  return sc.run();
}

// ---- several paths over one row, one parse ---------------------------------
//
// MultiRowScanner walks a row once and answers K paths. The tokenizer and
// validator state (position, reader, container stack, depth, whitespace
// count) is shared; the matcher state of RowScanner exists once per path.
// For every path the result equals scan_row()'s for that path alone, field
// by field, including the span fields of a row that ends NULL or flagged.
//
// K is a template parameter and every per-path loop is fully unrolled, so the
// per-path arrays are indexed by constants only and stay in registers. The
// per-path booleans are bit j of one mask word each.

constexpr int kMaxFusedPaths = 8;

#if defined(__HIPCC__)
#define JP_UNROLL _Pragma("unroll")
#else
#define JP_UNROLL
#endif

// K encoded paths that share one steps array and one names blob: path j's
// triples start at steps[sbase[j]] and there are nsteps[j] of them.
template <int K>
struct PathGroup {
  const int32_t* steps;
  const uint8_t* names;
  int32_t sbase[K];
  int32_t nsteps[K];
};

template <int K>
struct MultiRowScanner {
  static_assert(K >= 1 && K <= kMaxFusedPaths, "group size");
  ByteReader rd;
  const PathGroup<K>& g;
  int32_t p, re;
  uint64_t stack;
  int depth;
  int32_t nws;
  bool doc_flag;       // NaN / Infinity somewhere: every path is flagged
  uint32_t pending;    // bit j: the next value is the one path j selects
  uint32_t in_target;  // bit j: inside the container that is path j's result
  uint32_t tflag;      // bit j: that container holds something to flag
  uint32_t pflag;      // bit j: flag path j whatever its result is
  // per path: `on` in bits 0-7, target_depth in bits 8-15 (both at most 64),
  // the result state in bits 16-17
  uint32_t meta[K];
  int32_t elem[K];
  int32_t nws0[K];
  int32_t src_start[K], src_len[K];
  int32_t out_len[K];  // never more than the row's bytes

  JP_HD MultiRowScanner(const uint8_t* data, int32_t rs, int32_t re_,
                        const PathGroup<K>& group)
      : rd(data, rs, re_), g(group), p(rs), re(re_), stack(0), depth(0),
        nws(0), doc_flag(false), pending((1u << K) - 1), in_target(0),
        tflag(0), pflag(0) {
    JP_UNROLL
    for (int j = 0; j < K; ++j) {
      meta[j] = 0;  // on 0, target_depth 0, JP_NULL
      elem[j] = 0;
      nws0[j] = 0;
      src_start[j] = 0;
      src_len[j] = 0;
      out_len[j] = 0;
    }
  }

  JP_HD int on(int j) const { return (int)(meta[j] & 0xFF); }
  JP_HD int target_depth(int j) const { return (int)((meta[j] >> 8) & 0xFF); }
  JP_HD uint8_t state(int j) const { return (uint8_t)((meta[j] >> 16) & 3); }
  JP_HD void set_on(int j, int v) {
    meta[j] = (meta[j] & ~0xFFu) | (uint32_t)v;
  }
  JP_HD void set_target_depth(int j, int v) {
    meta[j] = (meta[j] & ~0xFF00u) | ((uint32_t)v << 8);
  }
  JP_HD void set_state(int j, uint8_t v) {
    meta[j] = (meta[j] & ~0x30000u) | ((uint32_t)v << 16);
  }
  // word t (0 kind, 1 a, 2 b) of the step that path j's innermost on-path
  // container waits for
  JP_HD int32_t step(int j, int t) const {
    return g.steps[g.sbase[j] + (on(j) - 1) * 3 + t];
  }

  JP_HD void set_results(uint32_t mask, int32_t start, int32_t len,
                         int32_t olen, bool flag) {
    JP_UNROLL
    for (int j = 0; j < K; ++j) {
      if (!((mask >> j) & 1)) continue;
      src_start[j] = start;
      src_len[j] = len;
      out_len[j] = olen;
      set_state(j, flag ? JP_FLAG : JP_VALUE);
    }
  }

  // As RowScanner::scan_string. result: the paths whose result this string
  // is; inside: the paths whose container result holds it; keys: the paths
  // that listen for a key here. A key's raw bytes are compared with every
  // listening path's name at once: `same` keeps bit j while the k bytes read
  // so far are the first k of path j's name.
  JP_HD bool scan_string(uint32_t result, uint32_t inside, uint32_t keys,
                         uint32_t* hits) {
    int32_t start = p;
    int32_t k = 0;
    uint32_t same = keys;
    bool has_bs = false, has_hi = false;
    bool hi_pending = false, lone = false;
    int32_t declen = 0;
    ++p;
    for (;;) {
      if (p >= re) return false;  // unterminated
      uint8_t c = rd.at(p);
      if (c == '"') break;
      if (c < 0x20) return false;
      if (c == '\\') {
        has_bs = true;
        if (++p >= re) return false;
        uint8_t e = rd.at(p);
        if (e == 'u') {
          if (p + 4 >= re) return false;
          int cp = 0;
          for (int j = 1; j <= 4; ++j) {
            int h = hex_val(rd.at(p + j));
            if (h < 0) return false;
            cp = cp * 16 + h;
          }
          p += 5;
          if (cp >= 0xDC00 && cp <= 0xDFFF) {
            if (hi_pending) declen += 4; else lone = true;
            hi_pending = false;
            continue;
          }
          if (hi_pending) lone = true;
          hi_pending = cp >= 0xD800 && cp <= 0xDBFF;
          if (!hi_pending) declen += cp < 0x80 ? 1 : cp < 0x800 ? 2 : 3;
          continue;
        }
        if (!(e == '"' || e == '\\' || e == '/' || e == 'b' || e == 'f' ||
              e == 'n' || e == 'r' || e == 't'))
          return false;
        if (hi_pending) { lone = true; hi_pending = false; }
        ++declen;
        ++p;
        continue;
      }
      if (hi_pending) { lone = true; hi_pending = false; }
      if (c >= 0x80) has_hi = true;
      if (same) {
        JP_UNROLL
        for (int j = 0; j < K; ++j) {
          // the name's place is read again per byte: few keys stay equal
          // beyond their first byte, and two more registers per path cost
          // every row occupancy
          if (((same >> j) & 1) &&
              !(k < step(j, 2) && g.names[step(j, 1) + k] == c))
            same &= ~(1u << j);
        }
        ++k;
      }
      ++declen;
      ++p;
    }
    ++p;  // closing quote
    if (hi_pending) lone = true;
    if (keys) {
      // an escaped key might decode to the name: the host decides
      if (has_bs) {
        pflag |= keys;
      } else {
        JP_UNROLL
        for (int j = 0; j < K; ++j)
          if (((same >> j) & 1) && k != step(j, 2)) same &= ~(1u << j);
        *hits = same;
      }
    }
    set_results(result, start, p - start, declen, lone);
    if (has_bs || has_hi) tflag |= inside;
    return true;
  }

  JP_HD bool scan_number(uint32_t result, uint32_t inside) {
    int32_t start = p;
    bool neg = rd.at(p) == '-';
    if (neg && ++p >= re) return false;
    uint8_t c = rd.at(p);
    if (neg && c == 'I') return scan_literal(result, start);
    int intd = 0, fracd = 0, lead_zeros = 0;
    bool zero_int = c == '0', is_float = false, has_exp = false;
    bool seen_nonzero = false;
    uint8_t last_frac = 0;
    if (zero_int) {
      ++p;
      intd = 1;
    } else if (is_digit(c)) {
      while (p < re && is_digit(rd.at(p))) { ++p; ++intd; }
    } else {
      return false;
    }
    if (p < re && rd.at(p) == '.') {
      is_float = true;
      ++p;
      while (p < re && is_digit(c = rd.at(p))) {
        if (c != '0') seen_nonzero = true;
        else if (!seen_nonzero) ++lead_zeros;
        last_frac = c;
        ++fracd;
        ++p;
      }
      if (fracd == 0) return false;
    }
    if (p < re && (rd.at(p) | 0x20) == 'e') {
      is_float = has_exp = true;
      ++p;
      if (p < re && (rd.at(p) == '+' || rd.at(p) == '-')) ++p;
      int expd = 0;
      while (p < re && is_digit(rd.at(p))) { ++p; ++expd; }
      if (expd == 0) return false;
    }
    if (!(result | inside)) return true;
    bool flag;
    if (!is_float) {
      flag = (neg && zero_int) || intd > kMaxIntDigits;
    } else {
      flag = has_exp || intd + fracd > kMaxFloatDigits ||
             (last_frac == '0' && fracd > 1) || (zero_int && lead_zeros >= 4);
    }
    set_results(result, start, p - start, p - start, flag);
    if (flag) tflag |= inside;
    return true;
  }

  JP_HD bool word_is(int32_t at, const char* w, int n) {
    if (at + n > re) return false;
    for (int j = 0; j < n; ++j)
      if (rd.at(at + j) != (uint8_t)w[j]) return false;
    return true;
  }

  JP_HD bool scan_literal(uint32_t result, int32_t start) {
    uint8_t c = rd.at(p);
    int n;
    if (c == 't' && word_is(p, "true", 4)) n = 4;
    else if (c == 'f' && word_is(p, "false", 5)) n = 5;
    else if (c == 'n' && word_is(p, "null", 4)) n = 4;
    else if (c == 'N' && word_is(p, "NaN", 3)) { n = 3; doc_flag = true; }
    else if (c == 'I' && word_is(p, "Infinity", 8)) { n = 8; doc_flag = true; }
    else return false;
    p += n;
    // a null result stays NULL
    if (c != 'n') set_results(result, start, p - start, p - start, false);
    return true;
  }

  JP_HD void close_container() {
    bool parent_is_array = !((stack >> 1) & 1);
    JP_UNROLL
    for (int j = 0; j < K; ++j) {
      if (depth == on(j)) {
        set_on(j, depth - 1);
        if (depth > 1 && parent_is_array) elem[j] = INT32_MIN;
      }
    }
    stack >>= 1;
    --depth;
    ++p;
    if (in_target) {
      JP_UNROLL
      for (int j = 0; j < K; ++j) {
        if (((in_target >> j) & 1) && depth == target_depth(j)) {
          in_target &= ~(1u << j);
          int32_t len = p - src_start[j];
          src_len[j] = len;
          out_len[j] = len - (nws - nws0[j]);
          set_state(j, ((tflag >> j) & 1) ? JP_FLAG : JP_VALUE);
        }
      }
    }
  }

  JP_HD void emit(RowResult* out) {
    JP_UNROLL
    for (int j = 0; j < K; ++j) {
      out[j].out_len = out_len[j];
      out[j].src_start = src_start[j];
      out[j].src_len = src_len[j];
      out[j].state = state(j);
    }
  }

  JP_HD void run(RowResult* out) {
    enum { ST_VALUE, ST_ARR_FIRST, ST_OBJ_FIRST, ST_KEY, ST_COLON, ST_AFTER };
    int st = ST_VALUE;
    bool ok = true;
    while (ok) {
      uint8_t c = 0;
      while (p < re && is_ws(c = rd.at(p))) { ++p; ++nws; }
      if (p >= re) break;
      if (st == ST_AFTER) {
        if (depth == 0) { ok = false; break; }  // trailing text
        bool obj = stack & 1;
        if (c == ',') {
          st = obj ? ST_KEY : ST_VALUE;
          ++p;
        } else if (c == (obj ? '}' : ']')) {
          close_container();
        } else {
          ok = false;
        }
        continue;
      }
      if (st == ST_COLON) {
        ok = c == ':';
        st = ST_VALUE;
        ++p;
        continue;
      }
      if (st == ST_OBJ_FIRST || st == ST_KEY) {
        if (c == '}' && st == ST_OBJ_FIRST) {
          close_container();
          st = ST_AFTER;
          continue;
        }
        if (c != '"') { ok = false; break; }
        uint32_t keys = 0;
        JP_UNROLL
        for (int j = 0; j < K; ++j)
          if (depth == on(j) && step(j, 0) == 0) keys |= 1u << j;
        uint32_t hits = 0;
        ok = scan_string(0, in_target, keys, &hits);
        pending |= hits;
        st = ST_COLON;
        continue;
      }
      if (st == ST_ARR_FIRST && c == ']') {
        close_container();
        st = ST_AFTER;
        continue;
      }
      // a value starts here
      uint32_t sel = pending;
      pending = 0;
      if (depth > 0 && !(stack & 1)) {
        JP_UNROLL
        for (int j = 0; j < K; ++j) {
          if (depth != on(j)) continue;
          bool m = step(j, 0) == 1 && elem[j] == step(j, 1);
          sel = m ? sel | (1u << j) : sel & ~(1u << j);
          ++elem[j];
        }
      }
      // a later duplicate of a matched key replaces what the earlier one gave
      uint32_t target = 0;
      JP_UNROLL
      for (int j = 0; j < K; ++j) {
        if (!((sel >> j) & 1)) continue;
        set_state(j, JP_NULL);
        if (depth == g.nsteps[j]) target |= 1u << j;
      }
      st = ST_AFTER;
      if (c == '{' || c == '[') {
        if (depth == kMaxDepth) {
          JP_UNROLL
          for (int j = 0; j < K; ++j) set_state(j, JP_FLAG);
          emit(out);
          return;
        }
        if (sel) {
          JP_UNROLL
          for (int j = 0; j < K; ++j) {
            if ((target >> j) & 1) {
              in_target |= 1u << j;
              set_target_depth(j, depth);
              src_start[j] = p;
              nws0[j] = nws;
              tflag &= ~(1u << j);
            } else if ((sel >> j) & 1) {
              set_on(j, depth + 1);
              elem[j] = 0;
            }
          }
        }
        stack = (stack << 1) | (c == '{' ? 1u : 0u);
        ++depth;
        ++p;
        st = c == '{' ? ST_OBJ_FIRST : ST_ARR_FIRST;
      } else if (c == '"') {
        uint32_t hits;
        ok = scan_string(target, in_target, 0, &hits);
      } else if (c == '-' || is_digit(c)) {
        ok = scan_number(target, in_target);
      } else {
        ok = scan_literal(target, p);
      }
    }
    bool invalid = !ok || st != ST_AFTER || depth != 0;
    JP_UNROLL
    for (int j = 0; j < K; ++j) {
      if (invalid) set_state(j, JP_NULL);
      else if (doc_flag || ((pflag >> j) & 1)) set_state(j, JP_FLAG);
      if (state(j) != JP_VALUE) out_len[j] = 0;
    }
    emit(out);
  }
};

// Size pass for one row [rs, re) of `data` and K paths: out[j] is what
// scan_row() gives for path j of the group alone.
template <int K>
JP_HD void scan_row_multi(const uint8_t* data, int32_t rs, int32_t re,
                          const PathGroup<K>& group, RowResult* out) {
  MultiRowScanner<K> sc(data, rs, re, group);
  sc.run(out);
}

JP_HD int64_t put_utf8(uint8_t* out, int64_t o, int64_t cap, int cp) {
  uint8_t b[4];
  int n;
  if (cp < 0x80) {
    b[0] = (uint8_t)cp; n = 1;
  } else if (cp < 0x800) {
    b[0] = (uint8_t)(0xC0 | (cp >> 6));
    b[1] = (uint8_t)(0x80 | (cp & 0x3F)); n = 2;
  } else if (cp < 0x10000) {
    b[0] = (uint8_t)(0xE0 | (cp >> 12));
    b[1] = (uint8_t)(0x80 | ((cp >> 6) & 0x3F));
    b[2] = (uint8_t)(0x80 | (cp & 0x3F)); n = 3;
  } else {
    b[0] = (uint8_t)(0xF0 | (cp >> 18));
    b[1] = (uint8_t)(0x80 | ((cp >> 12) & 0x3F));
    b[2] = (uint8_t)(0x80 | ((cp >> 6) & 0x3F));
    b[3] = (uint8_t)(0x80 | (cp & 0x3F)); n = 4;
  }
  if (n > 0 && o < cap) out[o] = b[0];
  if (n > 1 && o + 1 < cap) out[o + 1] = b[1];
  if (n > 2 && o + 2 < cap) out[o + 2] = b[2];
  if (n > 3 && o + 3 < cap) out[o + 3] = b[3];
  return o + n;
}

// Write pass for one JP_VALUE row: re-reads the span [ss, ss + sl) that the
// size pass validated and writes out_len normalised bytes to `out`. A string
// has its escapes resolved, a container loses the whitespace outside its
// strings, everything else is copied. No store goes beyond out_len.
JP_HD void write_row(const uint8_t* data, int32_t ss, int32_t sl,
                     uint8_t* out, int64_t out_len) {
  if (sl <= 0) return;
  ByteReader rd(data, ss, (int64_t)ss + sl);
  int32_t p = ss, end = ss + sl;
  int64_t o = 0;
  uint8_t first = rd.at(p);
  if (first == '"') {
    ++p;
    --end;  // the quotes
    int hi = 0;
    while (p < end) {
      uint8_t c = rd.at(p++);
      if (c != '\\') {
        if (o < out_len) out[o] = c;
        ++o;
        continue;
      }
      if (p >= end) break;
      uint8_t e = rd.at(p++);
      if (e == 'u') {
        int cp = 0;
        for (int j = 0; j < 4 && p < end; ++j) {
          int h = hex_val(rd.at(p++));
          cp = cp * 16 + (h < 0 ? 0 : h);
        }
        if (cp >= 0xD800 && cp <= 0xDBFF) {
          hi = cp;
          continue;
        }
        if (cp >= 0xDC00 && cp <= 0xDFFF)
          cp = 0x10000 + ((hi - 0xD800) << 10) + (cp - 0xDC00);
        o = put_utf8(out, o, out_len, cp);
        continue;
      }
      uint8_t d = e == 'b' ? '\b' : e == 'f' ? '\f' : e == 'n' ? '\n'
                : e == 'r' ? '\r' : e == 't' ? '\t' : e;
      if (o < out_len) out[o] = d;
      ++o;
    }
  } else if (first == '{' || first == '[') {
    bool in_str = false;
    while (p < end) {
      uint8_t c = rd.at(p++);
      if (in_str) {
        if (c == '"') in_str = false;
      } else if (c == '"') {
        in_str = true;
      } else if (is_ws(c)) {
        continue;
      }
      if (o < out_len) out[o] = c;
      ++o;
    }
  } else {
    while (p < end) {
      uint8_t c = rd.at(p++);
      if (o < out_len) out[o] = c;
      ++o;
    }
  }
}

}  // namespace jsonpath
