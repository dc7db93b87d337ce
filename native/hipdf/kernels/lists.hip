// Segmented operations inside the rows of a LIST column (reference analogue:
// GpuSortArray / GpuArraySort / GpuArrayDistinct / GpuArrayMin / GpuArrayMax
// in collectionOperations.scala, reached there through cudf segmented sort),
// the two-list set operations built on the sorted order, and what the
// higher-order functions need around a lambda body (both further down).
//
// Inputs are always the LIST offsets (int32[n+1], offsets[0] need not be 0),
// the child's values and the child's validity bitmask. The sort produces an
// int32 permutation of GLOBAL child indices, written at position
// (p - offsets[0]) for child position p, which the caller applies with the
// ordinary gather (validity and string bytes follow for free).
//
// Ordering inside one list is (null rank, key, original index): key is the
// radix sort's order-preserving transform (sort_keys.h), descending inverts
// the key but never the index tie-break, so the result is that of a stable
// sort. Strings use an 8-byte big-endian prefix as the key and compare the
// remaining bytes on a tie (shorter string first on a common prefix).
//
// Tiers by list length:
//   <= 64    W lanes (8/16/32/64) own one list, one element per lane,
//            bitonic network over __shfl_xor — no LDS, up to 8 lists/wave
//   <= 2048  one 256-thread block per list, bitonic in LDS over
//            (u64 key, u32 rank|local index) = 24 KB at the cap
//   longer   host routes those rows through the global radix sort
#include "hipdf.h"
#include "hipdf_common.h"
#include "sort_keys.h"

#define LIST_BLOCK 256
#define LIST_BLOCK_CAP 2048
#define LT_STR 7        // element type id for strings (after HT_F64)
#define RANK_PAD 2u     // padding sentinel: sorts after real nulls

// ---- element sources -----------------------------------------------------

template <typename T>
struct FixedSrc {
  const T* data;
  static FixedSrc of(const void* data, const void*) {
    return FixedSrc{(const T*)data};
  }
  __device__ __forceinline__ uint64_t key(int32_t i) const {
    return sort_key_of<T>(data[i]);
  }
  __device__ __forceinline__ int tie(int32_t, int32_t) const { return 0; }
  __device__ __forceinline__ int tie(int32_t, const FixedSrc&,
                                     int32_t) const {
    return 0;
  }
};

struct StrSrc {
  const int32_t* offs;
  const uint8_t* bytes;
  static StrSrc of(const void* data, const void* eoffs) {
    return StrSrc{(const int32_t*)eoffs, (const uint8_t*)data};
  }
  __device__ __forceinline__ uint64_t key(int32_t i) const {
    int32_t a = offs[i], b = offs[i + 1];
    uint64_t k = 0;
    for (int j = 0; j < 8; ++j) {
      uint8_t c = (a + j < b) ? bytes[a + j] : 0;
      k = (k << 8) | c;
    }
    return k;
  }
  // byte order of two strings whose prefix keys are equal: -1 / 0 / 1.
  // Equal keys mean the first min(8, la, lb) bytes agree, so start there.
  __device__ int tie(int32_t x, int32_t y) const {
    int32_t ax = offs[x], ay = offs[y];
    int32_t lx = offs[x + 1] - ax, ly = offs[y + 1] - ay;
    int32_t m = lx < ly ? lx : ly;
    for (int32_t j = m < 8 ? m : 8; j < m; ++j) {
      uint8_t cx = bytes[ax + j], cy = bytes[ay + j];
      if (cx != cy) return cx < cy ? -1 : 1;
    }
    return lx == ly ? 0 : (lx < ly ? -1 : 1);
  }
  // the same between element x here and element y of another child
  __device__ int tie(int32_t x, const StrSrc& o, int32_t y) const {
    int32_t ax = offs[x], ay = o.offs[y];
    int32_t lx = offs[x + 1] - ax, ly = o.offs[y + 1] - ay;
    int32_t m = lx < ly ? lx : ly;
    for (int32_t j = m < 8 ? m : 8; j < m; ++j) {
      uint8_t cx = bytes[ax + j], cy = o.bytes[ay + j];
      if (cx != cy) return cx < cy ? -1 : 1;
    }
    return lx == ly ? 0 : (lx < ly ? -1 : 1);
  }
};

struct Elem {
  uint64_t key;
  int32_t idx;    // global child index (-1 for padding)
  uint32_t rank;  // null rank; RANK_PAD for padding
};

// vrank = rank of a valid element (1 under NULLS FIRST, 0 under NULLS LAST);
// nulls take the other one and key 0
template <typename Src>
__device__ __forceinline__ Elem load_elem(const Src& src,
                                          const uint64_t* cvalid, int32_t gi,
                                          uint32_t vrank, int desc) {
  Elem e;
  e.idx = gi;
  if (valid_bit(cvalid, gi)) {
    uint64_t k = src.key(gi);
    e.key = desc ? ~k : k;
    e.rank = vrank;
  } else {
    e.key = 0;
    e.rank = 1u - vrank;
  }
  return e;
}

template <typename Src>
__device__ __forceinline__ bool elem_less(const Src& src, uint32_t ra,
                                          uint64_t ka, int32_t ia,
                                          uint32_t rb, uint64_t kb,
                                          int32_t ib, uint32_t vrank,
                                          int desc) {
  if (ra != rb) return ra < rb;
  if (ka != kb) return ka < kb;
  if (ra == vrank) {
    int c = src.tie(ia, ib);
    if (c) return desc ? c > 0 : c < 0;
  }
  return ia < ib;
}

// ---- sub-wave tier: W lanes per list, bitonic over shuffles --------------

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int m, int w) {
  uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, w);
  uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, w);
  return ((uint64_t)hi << 32) | lo;
}

template <typename Src, int W>
__global__ __launch_bounds__(HIPDF_BLOCK) void k_list_sort_wave(
    Src src, const int32_t* __restrict__ offsets,
    const uint64_t* __restrict__ cvalid, uint32_t vrank, int desc,
    int32_t* __restrict__ perm, int64_t n) {
  constexpr int L = WAVE / W;  // lists per wave
  int lane = lane_id();
  int sub = lane / W, sl = lane & (W - 1);
  int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  int64_t nwaves = (int64_t)gridDim.x * blockDim.x / WAVE;
  int32_t off0 = offsets[0];
  // loop bounds are wave-uniform: every lane reaches every shuffle
  for (int64_t base = wave * L; base < n; base += nwaves * L) {
    int64_t row = base + sub;
    int32_t start = 0, len = 0;
    if (row < n) {
      start = offsets[row];
      len = offsets[row + 1] - start;
    }
    if (len > W) len = 0;  // longer rows belong to another tier
    Elem e;
    e.key = (uint64_t)sl;  // distinct keys keep the order strict among pads
    e.idx = -1;
    e.rank = RANK_PAD;
    if (sl < len) e = load_elem(src, cvalid, start + sl, vrank, desc);
#pragma unroll
    for (int k = 2; k <= W; k <<= 1) {
#pragma unroll
      for (int j = k >> 1; j > 0; j >>= 1) {
        Elem o;
        o.key = shfl_xor_u64(e.key, j, W);
        o.idx = __shfl_xor(e.idx, j, W);
        o.rank = (uint32_t)__shfl_xor((int)e.rank, j, W);
        bool keep_min = ((sl & j) == 0) == ((sl & k) == 0);
        bool o_less = elem_less(src, o.rank, o.key, o.idx, e.rank, e.key,
                                e.idx, vrank, desc);
        if (keep_min == o_less) e = o;
      }
    }
    if (sl < len) perm[start - off0 + sl] = e.idx;
  }
}

// ---- block tier: one block per list, bitonic in LDS ----------------------

template <typename Src>
__global__ __launch_bounds__(LIST_BLOCK) void k_list_sort_block(
    Src src, const int32_t* __restrict__ offsets,
    const uint64_t* __restrict__ cvalid, const int32_t* __restrict__ rows,
    int64_t nrows, uint32_t vrank, int desc, int32_t* __restrict__ perm) {
  __shared__ uint64_t skey[LIST_BLOCK_CAP];
  __shared__ uint32_t spk[LIST_BLOCK_CAP];  // rank << 16 | local index
  int tid = threadIdx.x;
  int32_t off0 = offsets[0];
  for (int64_t r = blockIdx.x; r < nrows; r += gridDim.x) {
    int32_t row = rows[r];
    int32_t start = offsets[row];
    int32_t len = offsets[row + 1] - start;
    if (len < 1 || len > LIST_BLOCK_CAP) continue;  // block-uniform
    int P = 2;
    while (P < len) P <<= 1;
    for (int i = tid; i < P; i += LIST_BLOCK) {
      if (i < len) {
        Elem e = load_elem(src, cvalid, start + i, vrank, desc);
        skey[i] = e.key;
        spk[i] = (e.rank << 16) | (uint32_t)i;
      } else {
        skey[i] = 0;
        spk[i] = (RANK_PAD << 16) | (uint32_t)i;
      }
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = tid; i < (P >> 1); i += LIST_BLOCK) {
          int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1));
          int hi = lo | j;
          bool up = (lo & k) == 0;
          uint64_t ka = skey[lo], kb = skey[hi];
          uint32_t pa = spk[lo], pb = spk[hi];
          bool b_less = elem_less(src, pb >> 16, kb,
                                  start + (int32_t)(pb & 0xffffu), pa >> 16,
                                  ka, start + (int32_t)(pa & 0xffffu), vrank,
                                  desc);
          if (b_less == up) {
            skey[lo] = kb; skey[hi] = ka;
            spk[lo] = pb; spk[hi] = pa;
          }
        }
        __syncthreads();
      }
    }
    for (int i = tid; i < len; i += LIST_BLOCK)
      perm[start - off0 + i] = start + (int32_t)(spk[i] & 0xffffu);
    __syncthreads();  // LDS is reused by the next row
  }
}

// ---- distinct flags from an ascending sorted permutation -----------------
// keep[orig - off0] = 0 when the element's predecessor in its own list (in
// sorted order) has the same null rank and key; index tie-break in the sort
// makes the survivor of each run the first occurrence.

template <typename Src>
__global__ void k_list_distinct_flags(Src src,
                                      const int32_t* __restrict__ offsets,
                                      int64_t n,
                                      const uint64_t* __restrict__ cvalid,
                                      const int32_t* __restrict__ perm,
                                      uint8_t* __restrict__ keep,
                                      int64_t total) {
  int32_t off0 = offsets[0];
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total;
       p += (int64_t)gridDim.x * blockDim.x) {
    int32_t pos = off0 + (int32_t)p;
    // last row r in [0, n) with offsets[r] <= pos (pos < offsets[n])
    int64_t lo = 0, hi = n;
    while (hi - lo > 1) {
      int64_t mid = (lo + hi) >> 1;
      if (offsets[mid] <= pos) lo = mid; else hi = mid;
    }
    int32_t gi = perm[p];
    bool dup = false;
    if (pos != offsets[lo]) {
      int32_t gj = perm[p - 1];
      bool vi = valid_bit(cvalid, gi), vj = valid_bit(cvalid, gj);
      if (vi != vj) dup = false;
      else if (!vi) dup = true;
      else dup = src.key(gi) == src.key(gj) && src.tie(gi, gj) == 0;
    }
    keep[gi - off0] = dup ? 0 : 1;
  }
}

// ---- segmented arg-min / arg-max ignoring nulls --------------------------
// W lanes stride over one list, then an xor-shuffle reduction. Result is the
// global child index of the first least (greatest) element, or -1 for a
// null / empty / all-null list.

template <typename Src>
__device__ __forceinline__ bool cand_better(const Src& src, uint64_t ka,
                                            int32_t ia, uint64_t kb,
                                            int32_t ib, int is_max) {
  if (ka != kb) return ka < kb;  // key already inverted for max
  int c = src.tie(ia, ib);
  if (c) return is_max ? c > 0 : c < 0;
  return ia < ib;
}

template <typename Src, int W>
__global__ __launch_bounds__(HIPDF_BLOCK) void k_list_argminmax(
    Src src, const int32_t* __restrict__ offsets,
    const uint64_t* __restrict__ cvalid, const uint64_t* __restrict__ rvalid,
    int is_max, int32_t* __restrict__ out, int64_t n) {
  constexpr int L = WAVE / W;
  int lane = lane_id();
  int sub = lane / W, sl = lane & (W - 1);
  int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  int64_t nwaves = (int64_t)gridDim.x * blockDim.x / WAVE;
  for (int64_t base = wave * L; base < n; base += nwaves * L) {
    int64_t row = base + sub;
    int32_t start = 0, len = 0;
    if (row < n && valid_bit(rvalid, row)) {
      start = offsets[row];
      len = offsets[row + 1] - start;
    }
    uint64_t bk = 0;
    int32_t bi = -1;
    for (int32_t i = sl; i < len; i += W) {
      int32_t gi = start + i;
      if (!valid_bit(cvalid, gi)) continue;
      uint64_t k = src.key(gi);
      if (is_max) k = ~k;
      if (bi < 0 || cand_better(src, k, gi, bk, bi, is_max)) {
        bk = k;
        bi = gi;
      }
    }
#pragma unroll
    for (int j = W >> 1; j > 0; j >>= 1) {
      uint64_t ok = shfl_xor_u64(bk, j, W);
      int32_t oi = __shfl_xor(bi, j, W);
      if (oi >= 0 && (bi < 0 || cand_better(src, ok, oi, bk, bi, is_max))) {
        bk = ok;
        bi = oi;
      }
    }
    if (sl == 0 && row < n) out[row] = bi;
  }
}

// ---- two-list set operations ---------------------------------------------
// array_union / array_intersect / array_except / arrays_overlap (reference
// analogue: GpuArrayUnion, GpuArrayIntersect, GpuArrayExcept,
// GpuArraysOverlap). Side a is probed against side b, row by row. The two
// sides have their own children, validity masks and first offsets; b comes
// with its ascending, nulls-first sorted permutation.

// last row r in [0, n) with offsets[r] <= pos; needs n >= 1 and
// offsets[0] <= pos < offsets[n]
__device__ __forceinline__ int64_t row_of(const int32_t* __restrict__ offsets,
                                          int64_t n, int32_t pos) {
  int64_t lo = 0, hi = n;
  while (hi - lo > 1) {
    int64_t mid = (lo + hi) >> 1;
    if (offsets[mid] <= pos) lo = mid; else hi = mid;
  }
  return lo;
}

// member[p] = 1 when element (aoffsets[0] + p) of a has an equal element in
// the same row of b. A null element of a is a member exactly when b's sorted
// row starts with a null; otherwise a lower-bound style binary search over
// b's sorted row on (prefix key, byte tie-break), nulls of b sorting first.
template <typename Src>
__global__ void k_list_member_flags(Src a, const int32_t* __restrict__ aoffs,
                                    const uint64_t* __restrict__ avalid,
                                    Src b, const int32_t* __restrict__ boffs,
                                    const uint64_t* __restrict__ bvalid,
                                    const int32_t* __restrict__ bperm,
                                    int64_t n, uint8_t* __restrict__ member,
                                    int64_t total) {
  int32_t aoff0 = aoffs[0], boff0 = boffs[0];
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total;
       p += (int64_t)gridDim.x * blockDim.x) {
    int32_t gi = aoff0 + (int32_t)p;
    int64_t row = row_of(aoffs, n, gi);
    // positions inside bperm, rebased by b's own first offset
    int32_t lo = boffs[row] - boff0, hi = boffs[row + 1] - boff0;
    bool hit = false;
    if (lo < hi) {
      if (!valid_bit(avalid, gi)) {
        hit = !valid_bit(bvalid, bperm[lo]);
      } else {
        uint64_t ka = a.key(gi);
        while (lo < hi) {
          int32_t mid = lo + ((hi - lo) >> 1);
          int32_t gj = bperm[mid];
          int c;  // order of b's element against the probe
          if (!valid_bit(bvalid, gj)) {
            c = -1;
          } else {
            uint64_t kb = b.key(gj);
            c = kb < ka ? -1 : (kb > ka ? 1 : b.tie(gj, a, gi));
          }
          if (c == 0) { hit = true; break; }
          if (c < 0) lo = mid + 1; else hi = mid;
        }
      }
    }
    member[p] = hit ? 1 : 0;
  }
}

// arrays_overlap per row from a's member flags: 1 when a non-null element of
// a is a member; else NULL when both rows are non-empty and either holds a
// null (b's is its first sorted element); else 0. A row that is null on
// either side is NULL. One wave owns a stripe of 64 rows, W lanes per row and
// WAVE / W rows at a time, so it writes the stripe's validity word whole.
template <int W>
__global__ __launch_bounds__(HIPDF_BLOCK) void k_list_overlap(
    const uint8_t* __restrict__ member, const int32_t* __restrict__ aoffs,
    const uint64_t* __restrict__ avalid, const uint64_t* __restrict__ arvalid,
    const int32_t* __restrict__ boffs, const uint64_t* __restrict__ bvalid,
    const uint64_t* __restrict__ brvalid, const int32_t* __restrict__ bperm,
    uint8_t* __restrict__ out, uint64_t* __restrict__ vout, int64_t n) {
  constexpr int L = WAVE / W;  // rows per step
  int lane = lane_id();
  int sub = lane / W, sl = lane & (W - 1);
  int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  int64_t nwaves = (int64_t)gridDim.x * blockDim.x / WAVE;
  int64_t nstripes = (n + WAVE - 1) / WAVE;
  int32_t aoff0 = aoffs[0], boff0 = boffs[0];
  // loop bounds are wave-uniform: every lane reaches every shuffle / ballot
  for (int64_t stripe = wave; stripe < nstripes; stripe += nwaves) {
    uint64_t word = 0;
    for (int step = 0; step < W; ++step) {
      int64_t row = stripe * WAVE + step * L + sub;
      bool rv = row < n && valid_bit(arvalid, row) && valid_bit(brvalid, row);
      int32_t astart = 0, alen = 0, bstart = 0, blen = 0;
      if (rv) {
        astart = aoffs[row];
        alen = aoffs[row + 1] - astart;
        bstart = boffs[row];
        blen = boffs[row + 1] - bstart;
      }
      int hit = 0, anull = 0;
      for (int32_t i = sl; i < alen; i += W) {
        int32_t gi = astart + i;
        if (valid_bit(avalid, gi)) hit |= member[gi - aoff0];
        else anull = 1;
      }
      int st = hit | (anull << 1);
#pragma unroll
      for (int j = W >> 1; j > 0; j >>= 1) st |= __shfl_xor(st, j, W);
      bool bnull = blen > 0 && !valid_bit(bvalid, bperm[bstart - boff0]);
      bool any = (st & 1) != 0;
      bool unknown = !any && alen > 0 && blen > 0 && ((st & 2) || bnull);
      bool valid = rv && !unknown;
      uint64_t bal = __ballot(valid && sl == 0);  // bit sub * W = row's bit
#pragma unroll
      for (int g = 0; g < L; ++g)
        word |= ((bal >> (g * W)) & 1ull) << (step * L + g);
      if (sl == 0 && row < n) out[row] = (valid && any) ? 1 : 0;
    }
    if (lane == 0) vout[stripe] = word;
  }
}

// array_union's layout: row r of the result is a's kept elements followed by
// b's. ascan / bscan are exclusive scans of the kept flags with one extra
// slot for the total. One flat index space covers the n + 1 new offsets, a's
// elements and b's elements; idx points into concat(a.child, b.child), where
// b's child starts at row bbase.
__global__ void k_list_union_map(const int64_t* __restrict__ ascan,
                                 const int32_t* __restrict__ aoffs,
                                 int64_t atotal,
                                 const int64_t* __restrict__ bscan,
                                 const int32_t* __restrict__ boffs,
                                 int64_t btotal, int64_t n, int32_t bbase,
                                 int32_t* __restrict__ new_offs,
                                 int32_t* __restrict__ idx) {
  int32_t aoff0 = aoffs[0], boff0 = boffs[0];
  int64_t work = n + 1 + atotal + btotal;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < work;
       t += (int64_t)gridDim.x * blockDim.x) {
    if (t <= n) {
      new_offs[t] = (int32_t)(ascan[aoffs[t] - aoff0] +
                              bscan[boffs[t] - boff0]);
    } else if (t < n + 1 + atotal) {
      int64_t p = t - (n + 1);
      if (ascan[p + 1] == ascan[p]) continue;
      int32_t gi = aoff0 + (int32_t)p;
      int64_t row = row_of(aoffs, n, gi);
      idx[ascan[p] + bscan[boffs[row] - boff0]] = gi;
    } else {
      int64_t q = t - (n + 1 + atotal);
      if (bscan[q + 1] == bscan[q]) continue;
      int32_t gj = boff0 + (int32_t)q;
      int64_t row = row_of(boffs, n, gj);
      idx[bscan[q] + ascan[aoffs[row + 1] - aoff0]] = bbase + gj;
    }
  }
}

// ---- higher-order functions ----------------------------------------------
// transform / filter / exists / forall evaluate a lambda body as ordinary
// column kernels over the flattened child (reference analogue:
// GpuArrayTransform, GpuArrayFilter, GpuArrayExists in
// higherOrderFunctions.scala). What they need from here is the element to
// row map, for outer columns and the position variable, and the per-row
// three-valued reduction of the predicate column.

// rowid[p] = row owning element (offsets[0] + p); pos[p] = its 0-based place
// in that row (pos may be null). One thread per element: short rows keep
// every lane busy, and both outputs are indexed from 0.
__global__ void k_list_elem_rows(const int32_t* __restrict__ offsets,
                                 int64_t n, int32_t* __restrict__ rowid,
                                 int32_t* __restrict__ pos, int64_t total) {
  int32_t off0 = offsets[0];
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total;
       p += (int64_t)gridDim.x * blockDim.x) {
    int32_t gi = off0 + (int32_t)p;
    int64_t row = row_of(offsets, n, gi);
    rowid[p] = (int32_t)row;
    if (pos) pos[p] = gi - offsets[row];
  }
}

// exists (decide = 1) / forall (decide = 0) per row over a predicate column
// that has one entry per element from offsets[0]: the row is `decide` when a
// non-null predicate equals it, else NULL when a predicate is null, else
// !decide (so an empty row is false for exists, true for forall). A null row
// is NULL whatever range it owns. Stripes, W and the word write are
// k_list_overlap's; rows longer than W are covered by the stride.
template <int W>
__global__ __launch_bounds__(HIPDF_BLOCK) void k_list_bool_reduce(
    const uint8_t* __restrict__ pred, const uint64_t* __restrict__ pvalid,
    const int32_t* __restrict__ offsets, const uint64_t* __restrict__ rvalid,
    int decide, uint8_t* __restrict__ out, uint64_t* __restrict__ vout,
    int64_t n) {
  constexpr int L = WAVE / W;  // rows per step
  int lane = lane_id();
  int sub = lane / W, sl = lane & (W - 1);
  int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  int64_t nwaves = (int64_t)gridDim.x * blockDim.x / WAVE;
  int64_t nstripes = (n + WAVE - 1) / WAVE;
  int32_t off0 = offsets[0];
  // loop bounds are wave-uniform: every lane reaches every shuffle / ballot
  for (int64_t stripe = wave; stripe < nstripes; stripe += nwaves) {
    uint64_t word = 0;
    for (int step = 0; step < W; ++step) {
      int64_t row = stripe * WAVE + step * L + sub;
      bool rv = row < n && valid_bit(rvalid, row);
      int32_t start = 0, len = 0;
      if (rv) {
        start = offsets[row];
        len = offsets[row + 1] - start;
      }
      int hit = 0, unknown = 0;
      for (int32_t i = sl; i < len; i += W) {
        int64_t p = (int64_t)(start + i) - off0;
        if (!valid_bit(pvalid, p)) unknown = 1;
        else if ((pred[p] != 0) == (decide != 0)) hit = 1;
      }
      int st = hit | (unknown << 1);
#pragma unroll
      for (int j = W >> 1; j > 0; j >>= 1) st |= __shfl_xor(st, j, W);
      bool any = (st & 1) != 0;
      bool valid = rv && (any || !(st & 2));
      uint64_t bal = __ballot(valid && sl == 0);  // bit sub * W = row's bit
#pragma unroll
      for (int g = 0; g < L; ++g)
        word |= ((bal >> (g * W)) & 1ull) << (step * L + g);
      if (sl == 0 && row < n)
        out[row] = (valid && any == (decide != 0)) ? 1 : 0;
    }
    if (lane == 0) vout[stripe] = word;
  }
}

// ---- search, slice -------------------------------------------------------
// array_position / array_remove / slice (reference analogue:
// GpuArrayPosition, GpuArrayRemove, GpuSlice in collectionOperations.scala).
// Next to the list each row has a scalar operand: the needle, or the start
// and the length.

// Per-row search for the row's needle (entry `row` of a second source of the
// same kind). An element matches when it is non-null and equal to the needle
// under k_list_member_flags's equality: equal key() and a zero tie(). A row
// is live when it and its needle are non-null; only live rows are read
// through. match (one entry per element from offsets[0]) is 0 all over a row
// that is not live; first is the 1-based place of the first match, 0 for
// none. Any of the three outputs may be null. Stripes, W and the word write
// are k_list_bool_reduce's; rows longer than W are covered by the stride.
template <typename Src, int W>
__global__ __launch_bounds__(HIPDF_BLOCK) void k_list_find(
    Src src, const uint64_t* __restrict__ cvalid,
    const int32_t* __restrict__ offsets, const uint64_t* __restrict__ rvalid,
    Src needle, const uint64_t* __restrict__ nvalid,
    uint8_t* __restrict__ match, int64_t* __restrict__ first,
    uint64_t* __restrict__ vout, int64_t n) {
  constexpr int L = WAVE / W;  // rows per step
  constexpr int32_t NONE = 0x7fffffff;
  int lane = lane_id();
  int sub = lane / W, sl = lane & (W - 1);
  int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  int64_t nwaves = (int64_t)gridDim.x * blockDim.x / WAVE;
  int64_t nstripes = (n + WAVE - 1) / WAVE;
  int32_t off0 = offsets[0];
  // loop bounds are wave-uniform: every lane reaches every shuffle / ballot
  for (int64_t stripe = wave; stripe < nstripes; stripe += nwaves) {
    uint64_t word = 0;
    for (int step = 0; step < W; ++step) {
      int64_t row = stripe * WAVE + step * L + sub;
      bool live = row < n && valid_bit(rvalid, row) && valid_bit(nvalid, row);
      int32_t start = 0, len = 0;
      if (row < n && (live || match)) {
        start = offsets[row];
        len = offsets[row + 1] - start;
      }
      uint64_t nk = live ? needle.key((int32_t)row) : 0;
      int32_t best = NONE;
      // the element loop has no shuffle in it, so its bounds may differ
      for (int32_t i = sl; i < len; i += W) {
        int32_t gi = start + i;
        bool hit = live && valid_bit(cvalid, gi) && src.key(gi) == nk &&
                   src.tie(gi, needle, (int32_t)row) == 0;
        if (match) match[gi - off0] = hit ? 1 : 0;
        if (hit && best == NONE) {
          best = i;
          if (!match) break;  // later elements of this lane come after it
        }
      }
#pragma unroll
      for (int j = W >> 1; j > 0; j >>= 1) {
        int32_t o = __shfl_xor(best, j, W);
        best = o < best ? o : best;
      }
      uint64_t bal = __ballot(live && sl == 0);  // bit sub * W = row's bit
#pragma unroll
      for (int g = 0; g < L; ++g)
        word |= ((bal >> (g * W)) & 1ull) << (step * L + g);
      if (first && sl == 0 && row < n)
        first[row] = best == NONE ? 0 : (int64_t)best + 1;
    }
    if (vout && lane == 0) vout[stripe] = word;
  }
}

// slice(a, start, length) per row, one lane per row and one wave per 64-row
// stripe. A row is live when it, its start and its length are non-null.
// start is 1-based, negative counts from the end; everything is 64-bit, so
// start + length cannot wrap. src_start: global child index of the first
// element taken; out_len: elements taken, 0 for a row that is not live, is
// empty or is in error, and entry n is 0 so that the array scans into n + 1
// offsets. err[0] counts live rows with start == 0, err[1] those with
// length < 0 (the host zeroes err and raises).
__global__ __launch_bounds__(HIPDF_BLOCK) void k_list_slice_ranges(
    const int32_t* __restrict__ offsets, const uint64_t* __restrict__ rvalid,
    const int32_t* __restrict__ start, const uint64_t* __restrict__ svalid,
    const int32_t* __restrict__ length, const uint64_t* __restrict__ lvalid,
    int32_t* __restrict__ src_start, int64_t* __restrict__ out_len,
    uint64_t* __restrict__ vout, unsigned long long* __restrict__ err,
    int64_t n) {
  int lane = lane_id();
  int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  int64_t nwaves = (int64_t)gridDim.x * blockDim.x / WAVE;
  // rows 0..n: the last stripe also holds the closing entry of out_len
  int64_t nstripes = (n + 1 + WAVE - 1) / WAVE;
  for (int64_t stripe = wave; stripe < nstripes; stripe += nwaves) {
    int64_t row = stripe * WAVE + lane;
    bool live = row < n && valid_bit(rvalid, row) && valid_bit(svalid, row) &&
                valid_bit(lvalid, row);
    int32_t s0 = 0;
    int64_t taken = 0;
    bool bad_start = false, bad_len = false;
    if (live) {
      int64_t st = start[row], ln = length[row];
      int32_t b = offsets[row];
      int64_t len = (int64_t)offsets[row + 1] - b;
      bad_start = st == 0;
      bad_len = ln < 0;
      if (!bad_start && !bad_len) {
        int64_t f = st > 0 ? st - 1 : len + st;
        if (f >= 0 && f < len) {
          int64_t e = f + ln < len ? f + ln : len;
          s0 = b + (int32_t)f;
          taken = e - f;
        }
      }
    }
    if (row < n) src_start[row] = s0;
    if (row <= n) out_len[row] = taken;
    uint64_t bal = __ballot(live);
    uint64_t bs = __ballot(bad_start), bl = __ballot(bad_len);
    if (lane == 0) {
      if (stripe * WAVE < n) vout[stripe] = bal;
      if (bs) atomicAdd(&err[0], (unsigned long long)__popcll(bs));
      if (bl) atomicAdd(&err[1], (unsigned long long)__popcll(bl));
    }
  }
}

// gather map of slice: idx[p] = src_start[row] + (p - new_offs[row]) for the
// row that owns output element p; new_offs are the result's offsets, from 0.
__global__ void k_list_slice_map(const int32_t* __restrict__ new_offs,
                                 const int32_t* __restrict__ src_start,
                                 int64_t n, int32_t* __restrict__ idx,
                                 int64_t total) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total;
       p += (int64_t)gridDim.x * blockDim.x) {
    int64_t row = row_of(new_offs, n, (int32_t)p);
    idx[p] = src_start[row] + ((int32_t)p - new_offs[row]);
  }
}

// ---- builders ------------------------------------------------------------
// array() / concat / flatten / sequence / array_join (reference analogue:
// GpuCreateArray in complexTypeCreator.scala, GpuConcat, GpuFlatten,
// GpuSequence and GpuArrayJoin in collectionOperations.scala). These make
// arrays, or a string per array, out of per-row operands. A launch takes up
// to HIPDF_LIST_MAX_OPERANDS operands by value in a HipdfListOperands; its
// pointers are picked with an unrolled compare, never by a run-time index,
// so the struct stays in kernel-argument registers.

constexpr int LIST_OPS = HIPDF_LIST_MAX_OPERANDS;

template <typename P>
__device__ __forceinline__ P pick_operand(const void* const (&a)[LIST_OPS],
                                          int j) {
  const void* p = a[0];
#pragma unroll
  for (int q = 1; q < LIST_OPS; ++q)
    if (j == q) p = a[q];
  return (P)p;
}

// array(c_0 .. c_{k-1}) over fixed-width operands: out[i * k + j] = c_j[i].
// This launch holds operands j0 .. j0 + kk - 1. One thread per output
// element of the whole result, so neighbouring lanes store neighbouring
// elements; an element of another launch's operand is left alone. A wave
// owns the 64 outputs of one validity word. With every operand in one launch
// (shared == 0) it stores the word whole from its ballot; otherwise the
// caller has zeroed the mask and the wave ORs its bits in. vout may be null
// when no operand has a validity mask. new_offs (may be null): the result's
// offsets, new_offs[i] = i * k for i in 0..n.
template <typename T>
__global__ __launch_bounds__(HIPDF_BLOCK) void k_list_interleave(
    HipdfListOperands ops, int k, int j0, int kk, int shared,
    T* __restrict__ out, uint64_t* __restrict__ vout,
    int32_t* __restrict__ new_offs, int64_t n) {
  int lane = lane_id();
  int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  int64_t total = n * k;  // <= INT32_MAX, the caller checks
  if (new_offs)
    for (int64_t i = tid; i <= n; i += nthreads) new_offs[i] = (int32_t)(i * k);
  // wave-uniform bounds: every lane reaches the ballot
  for (int64_t base = tid - lane; base < total; base += nthreads) {
    int64_t p = base + lane;
    bool bit = false;
    if (p < total) {
      uint32_t i = (uint32_t)p / (uint32_t)k;
      int j = (int)((uint32_t)p - i * (uint32_t)k) - j0;
      if (j >= 0 && j < kk) {
        out[p] = pick_operand<const T*>(ops.a, j)[i];
        bit = valid_bit(pick_operand<const uint64_t*>(ops.valid, j), i);
      }
    }
    uint64_t bal = __ballot(bit);
    if (vout && lane == 0) {
      if (!shared) vout[base >> 6] = bal;
      else if (bal) atomicOr((unsigned long long*)&vout[base >> 6],
                             (unsigned long long)bal);
    }
  }
}

// The same layout as a gather map, for operands that move through the
// gather (strings, decimal128): idx[i * k + j] = j * n + i indexes the
// concatenation of the k operand columns.
__global__ void k_list_interleave_map(int k, int32_t* __restrict__ idx,
                                      int32_t* __restrict__ new_offs,
                                      int64_t n) {
  int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  int64_t total = n * k;
  for (int64_t i = tid; i <= n; i += nthreads) new_offs[i] = (int32_t)(i * k);
  for (int64_t p = tid; p < total; p += nthreads) {
    uint32_t i = (uint32_t)p / (uint32_t)k;
    uint32_t j = (uint32_t)p - i * (uint32_t)k;
    idx[p] = (int32_t)((int64_t)j * n + i);
  }
}

// concat(a_0 .. a_{k-1}) per-row lengths, operands j0.. of this launch in
// ops (a = int32 offsets[n + 1], valid = row validity). One lane per row and
// one wave per 64-row stripe, rows 0..n (entry n of out_len is 0). The first
// launch starts the running length and the validity word, a later one reads
// what the launches before it left; prefix (may be null) receives the
// running length BEFORE this launch's operands, which is where they start
// inside the result row. The last launch zeroes the length of a row that is
// null in any operand, so that out_len scans into the offsets.
__global__ __launch_bounds__(HIPDF_BLOCK) void k_list_concat_lens(
    HipdfListOperands ops, int kk, int first, int last,
    int64_t* __restrict__ out_len, int32_t* __restrict__ prefix,
    uint64_t* __restrict__ vout, int64_t n) {
  int lane = lane_id();
  int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  int64_t nwaves = (int64_t)gridDim.x * blockDim.x / WAVE;
  int64_t nstripes = (n + 1 + WAVE - 1) / WAVE;
  for (int64_t stripe = wave; stripe < nstripes; stripe += nwaves) {
    int64_t row = stripe * WAVE + lane;
    bool live = row < n;
    int64_t sum = 0;
    if (row < n) {
#pragma unroll
      for (int j = 0; j < LIST_OPS; ++j) {
        if (j >= kk) continue;
        const int32_t* o = (const int32_t*)ops.a[j];
        sum += (int64_t)o[row + 1] - o[row];
        live = live && valid_bit((const uint64_t*)ops.valid[j], row);
      }
    }
    bool has_word = stripe * WAVE < n;  // the closing entry may stand alone
    uint64_t word = __ballot(live);
    if (!first && has_word) word &= vout[stripe];
    int64_t prev = (first || row >= n) ? 0 : out_len[row];
    if (prefix && row < n) prefix[row] = (int32_t)prev;
    int64_t tot = prev + sum;
    if (last && !((word >> lane) & 1ull)) tot = 0;
    if (row <= n) out_len[row] = row < n ? tot : 0;
    if (lane == 0 && has_word) vout[stripe] = word;
  }
}

// gather map of concat, one thread per output element p: new_offs are the
// result's offsets (from 0), prefix[row] (null = 0) the place in the result
// row where this launch's operands begin, cbase.a[j] (an integer carried in
// the pointer slot) the row of the concatenated children at which operand
// j's child starts. An element that belongs to another launch's operands is
// left alone.
struct ListBases { int64_t b[LIST_OPS]; };

__global__ void k_list_concat_map(HipdfListOperands ops, ListBases cbase,
                                  int kk, const int32_t* __restrict__ new_offs,
                                  const int32_t* __restrict__ prefix,
                                  int64_t n, int32_t* __restrict__ idx,
                                  int64_t total) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total;
       p += (int64_t)gridDim.x * blockDim.x) {
    int64_t row = row_of(new_offs, n, (int32_t)p);
    int32_t r = (int32_t)p - new_offs[row] - (prefix ? prefix[row] : 0);
    if (r < 0) continue;
#pragma unroll
    for (int j = 0; j < LIST_OPS; ++j) {
      if (j >= kk || r < 0) continue;
      const int32_t* o = (const int32_t*)ops.a[j];
      int32_t b = o[row], len = o[row + 1] - b;
      if (r < len) {
        idx[p] = (int32_t)(cbase.b[j] + b + r);
        r = -1;  // placed
      } else {
        r -= len;
      }
    }
  }
}

// flatten(LIST<LIST<T>>): the new offsets index the innermost child,
// new_offs[i] = inner[outer[i]] - inner[outer[0]] for i in 0..n. A row is
// valid when the outer row is and none of its inner arrays is null. W lanes
// stride over a row's inner arrays; stripes and the word write are
// k_list_bool_reduce's. span[0] / span[1] receive the first and the closing
// innermost index, which the host needs to cut the child.
template <int W>
__global__ __launch_bounds__(HIPDF_BLOCK) void k_list_flatten(
    const int32_t* __restrict__ outer, const uint64_t* __restrict__ rvalid,
    const int32_t* __restrict__ inner, const uint64_t* __restrict__ ivalid,
    int32_t* __restrict__ new_offs, uint64_t* __restrict__ vout,
    int64_t* __restrict__ span, int64_t n) {
  constexpr int L = WAVE / W;  // rows per step
  int lane = lane_id();
  int sub = lane / W, sl = lane & (W - 1);
  int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t wave = tid / WAVE;
  int64_t nwaves = (int64_t)gridDim.x * blockDim.x / WAVE;
  int64_t nstripes = (n + WAVE - 1) / WAVE;
  int32_t base = inner[outer[0]];
  if (tid == 0) {
    span[0] = base;
    span[1] = inner[outer[n]];
    new_offs[n] = inner[outer[n]] - base;
  }
  // loop bounds are wave-uniform: every lane reaches every shuffle / ballot
  for (int64_t stripe = wave; stripe < nstripes; stripe += nwaves) {
    uint64_t word = 0;
    for (int step = 0; step < W; ++step) {
      int64_t row = stripe * WAVE + step * L + sub;
      bool rv = row < n && valid_bit(rvalid, row);
      int32_t start = 0, len = 0;
      if (row < n) {
        start = outer[row];
        if (sl == 0) new_offs[row] = inner[start] - base;
        if (rv && ivalid) len = outer[row + 1] - start;
      }
      int bad = 0;
      for (int32_t i = sl; i < len; i += W)
        if (!valid_bit(ivalid, start + i)) bad = 1;
#pragma unroll
      for (int j = W >> 1; j > 0; j >>= 1) bad |= __shfl_xor(bad, j, W);
      uint64_t bal = __ballot(rv && !bad && sl == 0);
#pragma unroll
      for (int g = 0; g < L; ++g)
        word |= ((bal >> (g * W)) & 1ull) << (step * L + g);
    }
    if (lane == 0) vout[stripe] = word;
  }
}

// sequence(start, stop[, step]) per row: lengths, validity and the error
// record. T is int32_t or int64_t, U its unsigned twin; step == null means
// 1 when start <= stop, else -1. A row is live when every operand is
// non-null. start == stop has one element whatever the step; otherwise a
// zero step, or one that points away from stop, is an error. The distance
// and the step's magnitude are taken in U, where stop - start cannot
// overflow, and the length is capped at 2^31 so that n of them cannot
// overflow the int64 scan (anything above INT32_MAX is refused by the host
// anyway). out_len: int64[n + 1], 0 for a row that is not live or is in
// error, entry n is 0. err[0] (preset to INT64_MAX by the caller) becomes
// the least row index in error.
template <typename T, typename U>
__global__ __launch_bounds__(HIPDF_BLOCK) void k_sequence_ranges(
    const T* __restrict__ start, const uint64_t* __restrict__ avalid,
    const T* __restrict__ stop, const uint64_t* __restrict__ bvalid,
    const T* __restrict__ step, const uint64_t* __restrict__ svalid,
    int64_t* __restrict__ out_len, uint64_t* __restrict__ vout,
    long long* __restrict__ err, int64_t n) {
  int lane = lane_id();
  int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  int64_t nwaves = (int64_t)gridDim.x * blockDim.x / WAVE;
  int64_t nstripes = (n + 1 + WAVE - 1) / WAVE;
  for (int64_t stripe = wave; stripe < nstripes; stripe += nwaves) {
    int64_t row = stripe * WAVE + lane;
    bool live = row < n && valid_bit(avalid, row) && valid_bit(bvalid, row) &&
                (!step || valid_bit(svalid, row));
    int64_t len = 0;
    bool bad = false;
    if (live) {
      T a = start[row], b = stop[row];
      T st = step ? step[row] : (a <= b ? (T)1 : (T)-1);
      if (a == b) {
        len = 1;
      } else if (st == 0 || (b > a) != (st > 0)) {
        bad = true;
      } else {
        U dist = b > a ? (U)b - (U)a : (U)a - (U)b;
        U mag = st > 0 ? (U)st : (U)0 - (U)st;
        U q = dist / mag;
        len = q >= (U)0x7fffffff ? (int64_t)1 << 31 : (int64_t)q + 1;
      }
    }
    if (row <= n) out_len[row] = len;
    uint64_t bal = __ballot(live);
    uint64_t bb = __ballot(bad);
    if (lane == 0) {
      if (stripe * WAVE < n) vout[stripe] = bal;
      if (bb) atomicMin(&err[0], (long long)(stripe * WAVE + __ffsll((unsigned long long)bb) - 1));
    }
  }
}

// completes the error record after k_sequence_ranges (same stream): err[1..3]
// = start, stop and step of row err[0], when there is one
template <typename T>
__global__ void k_sequence_err_values(const T* __restrict__ start,
                                      const T* __restrict__ stop,
                                      const T* __restrict__ step,
                                      long long* __restrict__ err, int64_t n) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  long long row = err[0];
  if (row < 0 || row >= n) return;
  T a = start[row], b = stop[row];
  err[1] = a;
  err[2] = b;
  err[3] = step ? step[row] : (a <= b ? (T)1 : (T)-1);
}

// out[p] = start[row] + (p - offs[row]) * step[row] for the row that owns
// element p; offs from 0. The product is formed in U: it may pass through
// values T cannot hold, the sum never leaves T's range.
template <typename T, typename U>
__global__ void k_sequence_fill(const int32_t* __restrict__ offs,
                                const T* __restrict__ start,
                                const T* __restrict__ stop,
                                const T* __restrict__ step, int64_t n,
                                T* __restrict__ out, int64_t total) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total;
       p += (int64_t)gridDim.x * blockDim.x) {
    int64_t row = row_of(offs, n, (int32_t)p);
    T a = start[row];
    T st = step ? step[row] : (a <= stop[row] ? (T)1 : (T)-1);
    out[p] = (T)((U)a + (U)((int32_t)p - offs[row]) * (U)st);
  }
}

// array_join(LIST<STRING>, delimiter[, replacement]), element-parallel.
// Sizes: contrib[p] for element (offsets[0] + p) is its byte length (the
// replacement's for a null element when there is one) plus the delimiter's,
// 0 for a skipped null and all over a null row; entry `total` is 0. After
// the exclusive scan S of contrib, a row over elements [a, b) holds
// S[b] - S[a] bytes less one delimiter (when that is not 0), and an element
// is the row's first emitted one exactly when S[p] == S[a]: if an emitted
// element before it contributed nothing, the delimiter is empty and the
// difference is nothing to write.
__global__ void k_array_join_sizes(const int32_t* __restrict__ offsets,
                                   const uint64_t* __restrict__ rvalid,
                                   const int32_t* __restrict__ eoffs,
                                   const uint64_t* __restrict__ cvalid,
                                   int32_t dlen, int32_t rlen, int64_t n,
                                   int64_t* __restrict__ contrib,
                                   int64_t total) {
  int32_t off0 = offsets[0];
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p <= total;
       p += (int64_t)gridDim.x * blockDim.x) {
    int64_t c = 0;
    if (p < total) {
      int32_t gi = off0 + (int32_t)p;
      int64_t row = row_of(offsets, n, gi);
      if (valid_bit(rvalid, row)) {
        if (valid_bit(cvalid, gi)) c = (int64_t)(eoffs[gi + 1] - eoffs[gi]) + dlen;
        else if (rlen >= 0) c = (int64_t)rlen + dlen;
      }
    }
    contrib[p] = c;
  }
}

// row byte lengths from the scan S (int64[total + 1]); entry n is 0
__global__ void k_array_join_rows(const int32_t* __restrict__ offsets,
                                  const int64_t* __restrict__ S, int32_t dlen,
                                  int64_t n, int64_t* __restrict__ out_len) {
  int32_t off0 = offsets[0];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t len = 0;
    if (i < n) {
      len = S[offsets[i + 1] - off0] - S[offsets[i] - off0];
      if (len > 0) len -= dlen;
    }
    out_len[i] = len;
  }
}

// write pass, one thread per element: the delimiter unless the element is
// the first emitted one of its row, then the element's (or replacement's)
// bytes. out_off: int64 byte offset of every row in out.
__global__ void k_array_join_write(const int32_t* __restrict__ offsets,
                                   const uint64_t* __restrict__ rvalid,
                                   const int32_t* __restrict__ eoffs,
                                   const uint8_t* __restrict__ bytes,
                                   const uint64_t* __restrict__ cvalid,
                                   const uint8_t* __restrict__ delim,
                                   int32_t dlen,
                                   const uint8_t* __restrict__ repl,
                                   int32_t rlen, const int64_t* __restrict__ S,
                                   const int64_t* __restrict__ out_off,
                                   int64_t n, uint8_t* __restrict__ out,
                                   int64_t total) {
  int32_t off0 = offsets[0];
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total;
       p += (int64_t)gridDim.x * blockDim.x) {
    if (S[p + 1] == S[p] && dlen > 0) continue;  // nothing emitted here
    int32_t gi = off0 + (int32_t)p;
    int64_t row = row_of(offsets, n, gi);
    if (!valid_bit(rvalid, row)) continue;
    const uint8_t* src;
    int32_t len;
    if (valid_bit(cvalid, gi)) {
      src = bytes + eoffs[gi];
      len = eoffs[gi + 1] - eoffs[gi];
    } else if (rlen >= 0) {
      src = repl;
      len = rlen;
    } else {
      continue;
    }
    int64_t within = S[p] - S[offsets[row] - off0];
    uint8_t* dst = out + out_off[row] + within;
    if (within > 0)
      for (int32_t b = 0; b < dlen; ++b) dst[b - dlen] = delim[b];
    for (int32_t b = 0; b < len; ++b) dst[b] = src[b];
  }
}

// ---- host side -----------------------------------------------------------

template <typename F>
static inline void dispatch_src(int t, const void* data, const void* eoffs,
                                F&& f) {
  if (t == LT_STR) {
    f(StrSrc::of(data, eoffs));
  } else {
    dispatch_type(t, [&]<typename T>() { f(FixedSrc<T>::of(data, eoffs)); });
  }
}

template <typename F>
static inline void dispatch_width(int w, F&& f) {
  switch (w) {
    case 8: f.template operator()<8>(); break;
    case 16: f.template operator()<16>(); break;
    case 32: f.template operator()<32>(); break;
    case 64: f.template operator()<64>(); break;
    default: throw std::runtime_error("hipdf: list group width not 8/16/32/64");
  }
}

// one W-lane group per row, HIPDF_BLOCK threads per block, grid capped
static inline dim3 group_grid(int64_t n, int w) {
  int64_t per_block = (int64_t)HIPDF_BLOCK / w;
  int64_t blocks = (n + per_block - 1) / per_block;
  if (blocks > HIPDF_MAX_BLOCKS) blocks = HIPDF_MAX_BLOCKS;
  if (blocks < 1) blocks = 1;
  return dim3((uint32_t)blocks);
}

extern "C" {

int hipdf_list_block_cap() { return LIST_BLOCK_CAP; }

void hipdf_list_sort_wave(int t, const void* data, const void* eoffs,
                          const void* cvalid, const void* offsets, int w,
                          int nulls_first, int desc, void* perm, int64_t n,
                          hipStream_t stream) {
  if (n <= 0) return;
  dispatch_src(t, data, eoffs, [&](auto src) {
    using Src = decltype(src);
    dispatch_width(w, [&]<int W>() {
      hipLaunchKernelGGL((k_list_sort_wave<Src, W>), group_grid(n, W),
                         dim3(HIPDF_BLOCK), 0, stream, src,
                         (const int32_t*)offsets, (const uint64_t*)cvalid,
                         (uint32_t)(nulls_first ? 1 : 0), desc,
                         (int32_t*)perm, n);
    });
  });
}

void hipdf_list_sort_block(int t, const void* data, const void* eoffs,
                           const void* cvalid, const void* offsets,
                           const void* rows, int64_t nrows, int nulls_first,
                           int desc, void* perm, hipStream_t stream) {
  if (nrows <= 0) return;
  int64_t blocks = nrows < HIPDF_MAX_BLOCKS ? nrows : HIPDF_MAX_BLOCKS;
  dispatch_src(t, data, eoffs, [&](auto src) {
    using Src = decltype(src);
    hipLaunchKernelGGL((k_list_sort_block<Src>), dim3((uint32_t)blocks),
                       dim3(LIST_BLOCK), 0, stream, src,
                       (const int32_t*)offsets, (const uint64_t*)cvalid,
                       (const int32_t*)rows, nrows,
                       (uint32_t)(nulls_first ? 1 : 0), desc, (int32_t*)perm);
  });
}

void hipdf_list_distinct_flags(int t, const void* data, const void* eoffs,
                               const void* cvalid, const void* offsets,
                               int64_t n, const void* perm, void* keep,
                               int64_t total, hipStream_t stream) {
  if (n <= 0 || total <= 0) return;
  dispatch_src(t, data, eoffs, [&](auto src) {
    using Src = decltype(src);
    hipLaunchKernelGGL((k_list_distinct_flags<Src>), flat_grid(total),
                       dim3(HIPDF_BLOCK), 0, stream, src,
                       (const int32_t*)offsets, n, (const uint64_t*)cvalid,
                       (const int32_t*)perm, (uint8_t*)keep, total);
  });
}

void hipdf_list_argminmax(int t, const void* data, const void* eoffs,
                          const void* cvalid, const void* offsets,
                          const void* rvalid, int w, int is_max, void* out,
                          int64_t n, hipStream_t stream) {
  if (n <= 0) return;
  dispatch_src(t, data, eoffs, [&](auto src) {
    using Src = decltype(src);
    dispatch_width(w, [&]<int W>() {
      hipLaunchKernelGGL((k_list_argminmax<Src, W>), group_grid(n, W),
                         dim3(HIPDF_BLOCK), 0, stream, src,
                         (const int32_t*)offsets, (const uint64_t*)cvalid,
                         (const uint64_t*)rvalid, is_max, (int32_t*)out, n);
    });
  });
}

void hipdf_list_member_flags(int t, const void* adata, const void* aeoffs,
                             const void* acvalid, const void* aoffsets,
                             const void* bdata, const void* beoffs,
                             const void* bcvalid, const void* boffsets,
                             const void* bperm, int64_t n, void* member,
                             int64_t total, hipStream_t stream) {
  if (n <= 0 || total <= 0) return;
  dispatch_src(t, adata, aeoffs, [&](auto a) {
    using Src = decltype(a);
    hipLaunchKernelGGL((k_list_member_flags<Src>), flat_grid(total),
                       dim3(HIPDF_BLOCK), 0, stream, a,
                       (const int32_t*)aoffsets, (const uint64_t*)acvalid,
                       Src::of(bdata, beoffs), (const int32_t*)boffsets,
                       (const uint64_t*)bcvalid, (const int32_t*)bperm, n,
                       (uint8_t*)member, total);
  });
}

void hipdf_list_overlap(const void* member, const void* aoffsets,
                        const void* acvalid, const void* arvalid,
                        const void* boffsets, const void* bcvalid,
                        const void* brvalid, const void* bperm, int w,
                        void* out, void* vout, int64_t n,
                        hipStream_t stream) {
  if (n <= 0) return;
  int64_t waves = (n + WAVE - 1) / WAVE;  // one wave per 64-row stripe
  dispatch_width(w, [&]<int W>() {
    hipLaunchKernelGGL((k_list_overlap<W>), flat_grid(waves * WAVE),
                       dim3(HIPDF_BLOCK), 0, stream, (const uint8_t*)member,
                       (const int32_t*)aoffsets, (const uint64_t*)acvalid,
                       (const uint64_t*)arvalid, (const int32_t*)boffsets,
                       (const uint64_t*)bcvalid, (const uint64_t*)brvalid,
                       (const int32_t*)bperm, (uint8_t*)out, (uint64_t*)vout,
                       n);
  });
}

void hipdf_list_union_map(const void* ascan, const void* aoffsets,
                          int64_t atotal, const void* bscan,
                          const void* boffsets, int64_t btotal, int64_t n,
                          int64_t bbase, void* new_offs, void* idx,
                          hipStream_t stream) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_list_union_map, flat_grid(n + 1 + atotal + btotal),
                     dim3(HIPDF_BLOCK), 0, stream, (const int64_t*)ascan,
                     (const int32_t*)aoffsets, atotal, (const int64_t*)bscan,
                     (const int32_t*)boffsets, btotal, n, (int32_t)bbase,
                     (int32_t*)new_offs, (int32_t*)idx);
}

void hipdf_list_elem_rows(const void* offsets, int64_t n, void* rowid,
                          void* pos, int64_t total, hipStream_t stream) {
  if (n <= 0 || total <= 0) return;
  hipLaunchKernelGGL(k_list_elem_rows, flat_grid(total), dim3(HIPDF_BLOCK), 0,
                     stream, (const int32_t*)offsets, n, (int32_t*)rowid,
                     (int32_t*)pos, total);
}

void hipdf_list_bool_reduce(const void* pred, const void* pvalid,
                            const void* offsets, const void* rvalid, int w,
                            int mode, void* out, void* vout, int64_t n,
                            hipStream_t stream) {
  if (n <= 0) return;
  int64_t waves = (n + WAVE - 1) / WAVE;  // one wave per 64-row stripe
  dispatch_width(w, [&]<int W>() {
    hipLaunchKernelGGL((k_list_bool_reduce<W>), flat_grid(waves * WAVE),
                       dim3(HIPDF_BLOCK), 0, stream, (const uint8_t*)pred,
                       (const uint64_t*)pvalid, (const int32_t*)offsets,
                       (const uint64_t*)rvalid, mode == 0 ? 1 : 0,
                       (uint8_t*)out, (uint64_t*)vout, n);
  });
}

void hipdf_list_find(int t, const void* data, const void* eoffs,
                     const void* cvalid, const void* offsets,
                     const void* rvalid, const void* ndata,
                     const void* neoffs, const void* nvalid, int w,
                     void* match, void* first, void* vout, int64_t n,
                     hipStream_t stream) {
  if (n <= 0) return;
  int64_t waves = (n + WAVE - 1) / WAVE;  // one wave per 64-row stripe
  dispatch_src(t, data, eoffs, [&](auto src) {
    using Src = decltype(src);
    dispatch_width(w, [&]<int W>() {
      hipLaunchKernelGGL((k_list_find<Src, W>), flat_grid(waves * WAVE),
                         dim3(HIPDF_BLOCK), 0, stream, src,
                         (const uint64_t*)cvalid, (const int32_t*)offsets,
                         (const uint64_t*)rvalid, Src::of(ndata, neoffs),
                         (const uint64_t*)nvalid, (uint8_t*)match,
                         (int64_t*)first, (uint64_t*)vout, n);
    });
  });
}

void hipdf_list_slice_ranges(const void* offsets, const void* rvalid,
                             const void* start, const void* svalid,
                             const void* length, const void* lvalid,
                             void* src_start, void* out_len, void* vout,
                             void* err, int64_t n, hipStream_t stream) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_list_slice_ranges, stripe_grid(n + 1),
                     dim3(HIPDF_BLOCK), 0, stream, (const int32_t*)offsets,
                     (const uint64_t*)rvalid, (const int32_t*)start,
                     (const uint64_t*)svalid, (const int32_t*)length,
                     (const uint64_t*)lvalid, (int32_t*)src_start,
                     (int64_t*)out_len, (uint64_t*)vout,
                     (unsigned long long*)err, n);
}

void hipdf_list_slice_map(const void* new_offs, const void* src_start,
                          int64_t n, void* idx, int64_t total,
                          hipStream_t stream) {
  if (n <= 0 || total <= 0) return;
  hipLaunchKernelGGL(k_list_slice_map, flat_grid(total), dim3(HIPDF_BLOCK), 0,
                     stream, (const int32_t*)new_offs,
                     (const int32_t*)src_start, n, (int32_t*)idx, total);
}

static inline int list_operand_count(int kk) {
  if (kk < 1 || kk > LIST_OPS)
    throw std::runtime_error("hipdf: 1 to 8 list operands per launch");
  return kk;
}

void hipdf_list_interleave(int esize, const void* ops, int k, int j0, int kk,
                           int shared, void* out, void* vout, void* new_offs,
                           int64_t n, hipStream_t stream) {
  if (n <= 0) return;
  list_operand_count(kk);
  if (k < 1 || j0 < 0 || j0 + kk > k || n * (int64_t)k > INT32_MAX)
    throw std::runtime_error("hipdf: list_interleave operand range");
  HipdfListOperands o = *(const HipdfListOperands*)ops;  // host memory
  auto launch = [&]<typename T>() {
    hipLaunchKernelGGL((k_list_interleave<T>), flat_grid(n * k),
                       dim3(HIPDF_BLOCK), 0, stream, o, k, j0, kk, shared,
                       (T*)out, (uint64_t*)vout, (int32_t*)new_offs, n);
  };
  switch (esize) {
    case 1: launch.template operator()<uint8_t>(); break;
    case 2: launch.template operator()<uint16_t>(); break;
    case 4: launch.template operator()<uint32_t>(); break;
    case 8: launch.template operator()<uint64_t>(); break;
    default: throw std::runtime_error("hipdf: list_interleave element size");
  }
}

void hipdf_list_interleave_map(int k, void* idx, void* new_offs, int64_t n,
                               hipStream_t stream) {
  if (n <= 0) return;
  if (k < 1 || n * (int64_t)k > INT32_MAX)
    throw std::runtime_error("hipdf: list_interleave_map operand count");
  hipLaunchKernelGGL(k_list_interleave_map, flat_grid(n * k),
                     dim3(HIPDF_BLOCK), 0, stream, k, (int32_t*)idx,
                     (int32_t*)new_offs, n);
}

void hipdf_list_concat_lens(const void* ops, int kk, int first, int last,
                            void* out_len, void* prefix, void* vout,
                            int64_t n, hipStream_t stream) {
  if (n <= 0) return;
  list_operand_count(kk);
  HipdfListOperands o = *(const HipdfListOperands*)ops;  // host memory
  hipLaunchKernelGGL(k_list_concat_lens, stripe_grid(n + 1),
                     dim3(HIPDF_BLOCK), 0, stream, o, kk, first, last,
                     (int64_t*)out_len, (int32_t*)prefix, (uint64_t*)vout, n);
}

void hipdf_list_concat_map(const void* ops, const void* cbase, int kk,
                           const void* new_offs, const void* prefix,
                           int64_t n, void* idx, int64_t total,
                           hipStream_t stream) {
  if (n <= 0 || total <= 0) return;
  list_operand_count(kk);
  HipdfListOperands o = *(const HipdfListOperands*)ops;  // host memory
  ListBases b{};
  for (int j = 0; j < kk; ++j) b.b[j] = ((const int64_t*)cbase)[j];
  hipLaunchKernelGGL(k_list_concat_map, flat_grid(total), dim3(HIPDF_BLOCK),
                     0, stream, o, b, kk, (const int32_t*)new_offs,
                     (const int32_t*)prefix, n, (int32_t*)idx, total);
}

void hipdf_list_flatten(const void* outer, const void* rvalid,
                        const void* inner, const void* ivalid, int w,
                        void* new_offs, void* vout, void* span, int64_t n,
                        hipStream_t stream) {
  if (n <= 0) return;
  int64_t waves = (n + WAVE - 1) / WAVE;  // one wave per 64-row stripe
  dispatch_width(w, [&]<int W>() {
    hipLaunchKernelGGL((k_list_flatten<W>), flat_grid(waves * WAVE),
                       dim3(HIPDF_BLOCK), 0, stream, (const int32_t*)outer,
                       (const uint64_t*)rvalid, (const int32_t*)inner,
                       (const uint64_t*)ivalid, (int32_t*)new_offs,
                       (uint64_t*)vout, (int64_t*)span, n);
  });
}

void hipdf_sequence_ranges(int t, const void* start, const void* avalid,
                           const void* stop, const void* bvalid,
                           const void* step, const void* svalid,
                           void* out_len, void* vout, void* err, int64_t n,
                           hipStream_t stream) {
  if (n <= 0) return;
  auto launch = [&]<typename T, typename U>() {
    hipLaunchKernelGGL((k_sequence_ranges<T, U>), stripe_grid(n + 1),
                       dim3(HIPDF_BLOCK), 0, stream, (const T*)start,
                       (const uint64_t*)avalid, (const T*)stop,
                       (const uint64_t*)bvalid, (const T*)step,
                       (const uint64_t*)svalid, (int64_t*)out_len,
                       (uint64_t*)vout, (long long*)err, n);
    hipLaunchKernelGGL((k_sequence_err_values<T>), dim3(1), dim3(WAVE), 0,
                       stream, (const T*)start, (const T*)stop,
                       (const T*)step, (long long*)err, n);
  };
  if (t == HT_I32) launch.template operator()<int32_t, uint32_t>();
  else if (t == HT_I64) launch.template operator()<int64_t, uint64_t>();
  else throw std::runtime_error("hipdf: sequence needs int32 or int64");
}

void hipdf_sequence_fill(int t, const void* offs, const void* start,
                         const void* stop, const void* step, int64_t n,
                         void* out, int64_t total, hipStream_t stream) {
  if (n <= 0 || total <= 0) return;
  auto launch = [&]<typename T, typename U>() {
    hipLaunchKernelGGL((k_sequence_fill<T, U>), flat_grid(total),
                       dim3(HIPDF_BLOCK), 0, stream, (const int32_t*)offs,
                       (const T*)start, (const T*)stop, (const T*)step, n,
                       (T*)out, total);
  };
  if (t == HT_I32) launch.template operator()<int32_t, uint32_t>();
  else if (t == HT_I64) launch.template operator()<int64_t, uint64_t>();
  else throw std::runtime_error("hipdf: sequence needs int32 or int64");
}

void hipdf_array_join_sizes(const void* offsets, const void* rvalid,
                            const void* eoffs, const void* cvalid, int dlen,
                            int rlen, int64_t n, void* contrib, int64_t total,
                            hipStream_t stream) {
  if (n <= 0 || total < 0) return;
  hipLaunchKernelGGL(k_array_join_sizes, flat_grid(total + 1),
                     dim3(HIPDF_BLOCK), 0, stream, (const int32_t*)offsets,
                     (const uint64_t*)rvalid, (const int32_t*)eoffs,
                     (const uint64_t*)cvalid, (int32_t)dlen, (int32_t)rlen, n,
                     (int64_t*)contrib, total);
}

void hipdf_array_join_rows(const void* offsets, const void* scanned, int dlen,
                           int64_t n, void* out_len, hipStream_t stream) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_array_join_rows, flat_grid(n + 1), dim3(HIPDF_BLOCK),
                     0, stream, (const int32_t*)offsets,
                     (const int64_t*)scanned, (int32_t)dlen, n,
                     (int64_t*)out_len);
}

void hipdf_array_join_write(const void* offsets, const void* rvalid,
                            const void* eoffs, const void* bytes,
                            const void* cvalid, const void* delim, int dlen,
                            const void* repl, int rlen, const void* scanned,
                            const void* out_off, int64_t n, void* out,
                            int64_t total, hipStream_t stream) {
  if (n <= 0 || total <= 0) return;
  hipLaunchKernelGGL(k_array_join_write, flat_grid(total), dim3(HIPDF_BLOCK),
                     0, stream, (const int32_t*)offsets,
                     (const uint64_t*)rvalid, (const int32_t*)eoffs,
                     (const uint8_t*)bytes, (const uint64_t*)cvalid,
                     (const uint8_t*)delim, (int32_t)dlen,
                     (const uint8_t*)repl, (int32_t)rlen,
                     (const int64_t*)scanned, (const int64_t*)out_off, n,
                     (uint8_t*)out, total);
}

}  // extern "C"
