// Stable LSD radix sort producing a permutation (sort_order), multi-key via
// least-significant-key-first passes (reference analogue: cudf sortOrder /
// orderBy reached from GpuSortExec — SURVEY.md §2.8A).
//
// Per key column: an order-preserving u64 key transform (sign-flip ints,
// IEEE flip floats with Spark NaN/-0.0 normalization, descending = bit
// inversion, null byte above the value bytes encoding NULLS FIRST/LAST),
// then 8-bit-digit passes. Each pass: per-block 256-bin LDS histogram
// (digit-major global layout so one flat exclusive scan yields
// [digit][block] offsets), then a stable scatter where the within-block
// rank comes from a wave-level multi-split (8 ballots) + per-bin cross-wave
// scan in LDS — rows keep their relative order, which LSD correctness
// requires.
//
// hipdf_sort_order runs all of that for every key in one host call: it takes
// a host array of key descriptors and caller-owned scratch, and enqueues the
// key-builds and passes back to back with no allocation and no synchronise.
// Each key-build also ORs key[i] ^ key[0] over the rows into one device u64;
// a pass whose byte of that word is zero (a constant digit) skips its count
// and scan and copies keys and perm through, so the host's buffer ping-pong
// never depends on device state. The per-kernel entries remain for callers
// that drive single steps (range_key, tests).
#include "hipdf.h"
#include "hipdf_common.h"
#include "sort_keys.h"

#define SORT_BLOCK 256
#define RADIX_BINS 256
#define SORT_ITEMS 16  // rows per thread per pass (tile = 4096 rows/block)

// ---- key transform -------------------------------------------------------

// sort_key_of<T>: shared with the segmented list sort (sort_keys.h)

// key width in value bytes per type
static inline int sort_key_width(int t) {
  switch (t) {
    case HT_U8: case HT_I8: return 1;
    case HT_I16: return 2;
    case HT_I32: case HT_F32: return 4;
    default: return 8;
  }
}

// Varying bits of a key column: OR over the rows of key[i] ^ key[0]. Every
// thread passes the bits it saw; one atomicOr per wave lands them in *diff
// (cleared on the stream before the key-build). A digit whose byte of *diff
// is zero is the same in every row, so its radix pass permutes nothing.
__device__ __forceinline__ void publish_key_diff(uint64_t acc,
                                                 uint64_t* diff) {
  if (!diff) return;
  for (int off = WAVE / 2; off > 0; off >>= 1)
    acc |= (uint64_t)__shfl_xor((unsigned long long)acc, off);
  if (lane_id() == 0 && acc) atomicOr((unsigned long long*)diff,
                                      (unsigned long long)acc);
}

__device__ __forceinline__ bool radix_pass_skipped(const uint64_t* diff,
                                                   int shift) {
  return diff && ((*diff >> shift) & 255ull) == 0;
}

template <typename T>
__device__ __forceinline__ uint64_t fixed_key_at(
    const T* __restrict__ data, const uint64_t* __restrict__ valid,
    const int32_t* __restrict__ perm, int desc, int width_bytes,
    int null_byte_null, int null_only, int64_t i) {
  // width 8 leaves no room for the null byte in 64 bits: value-only keys
  // here, and the caller runs one extra null_only pass afterwards.
  uint64_t vmask = width_bytes >= 8 ? ~0ull : ((1ull << (8 * width_bytes)) - 1);
  bool embed_null = width_bytes < 8;
  int32_t r = perm ? perm[i] : (int32_t)i;
  bool ok = valid_bit(valid, r);
  uint64_t nb = ok ? (uint64_t)(1 - null_byte_null) : (uint64_t)null_byte_null;
  if (null_only) return nb;
  uint64_t k = 0;
  if (ok) {
    k = sort_key_of<T>(data[r]) & vmask;
    if (desc) k = (~k) & vmask;
  }
  return embed_null ? (k | (nb << (8 * width_bytes))) : k;
}

// build u64 keys for rows in permutation order: key[i] = transform(col[perm[i]])
template <typename T>
__global__ void k_make_sort_keys(const T* __restrict__ data,
                                 const uint64_t* __restrict__ valid,
                                 const int32_t* __restrict__ perm, int desc,
                                 int width_bytes, int null_byte_null,
                                 int null_only, uint64_t* __restrict__ keys,
                                 int64_t n, uint64_t* __restrict__ diff) {
  uint64_t k0 = 0, acc = 0;
  if (diff && n > 0)
    k0 = fixed_key_at<T>(data, valid, perm, desc, width_bytes, null_byte_null,
                         null_only, 0);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint64_t k = fixed_key_at<T>(data, valid, perm, desc, width_bytes,
                                 null_byte_null, null_only, i);
    keys[i] = k;
    acc |= k ^ k0;
  }
  publish_key_diff(acc, diff);
}

// string sort keys: big-endian 8-byte chunk `chunk` of each string
// (short strings pad with 0x00, which orders prefixes first like byte
// comparison). The host loops chunks last-to-first through the stable
// radix, LSD-style over chunks; the null-order pass reuses null_only.
__device__ __forceinline__ uint64_t str_key_at(
    const int32_t* __restrict__ offsets, const uint8_t* __restrict__ bytes,
    const uint64_t* __restrict__ valid, const int32_t* __restrict__ perm,
    int desc, int chunk, int64_t i) {
  int32_t r = perm ? perm[i] : (int32_t)i;
  uint64_t k = 0;
  if (valid_bit(valid, r)) {
    int32_t a = offsets[r] + 8 * chunk, b = offsets[r + 1];
    for (int j = 0; j < 8; ++j) {
      uint8_t c = (a + j < b && a + j >= offsets[r]) ? bytes[a + j] : 0;
      k = (k << 8) | c;
    }
    if (desc) k = ~k;
  }
  return k;
}

__global__ void k_make_sort_keys_str(const int32_t* __restrict__ offsets,
                                     const uint8_t* __restrict__ bytes,
                                     const uint64_t* __restrict__ valid,
                                     const int32_t* __restrict__ perm,
                                     int desc, int chunk,
                                     uint64_t* __restrict__ keys,
                                     int64_t n, uint64_t* __restrict__ diff) {
  uint64_t k0 = 0, acc = 0;
  if (diff && n > 0)
    k0 = str_key_at(offsets, bytes, valid, perm, desc, chunk, 0);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint64_t k = str_key_at(offsets, bytes, valid, perm, desc, chunk, i);
    keys[i] = k;
    acc |= k ^ k0;
  }
  publish_key_diff(acc, diff);
}

// decimal128 sort keys: word `word` (0 = lo unsigned-biased, 1 = hi
// signed-biased) of the interleaved pairs; host runs lo then hi.
__device__ __forceinline__ uint64_t i128_key_at(
    const int64_t* __restrict__ data, const uint64_t* __restrict__ valid,
    const int32_t* __restrict__ perm, int desc, int word, int64_t i) {
  int32_t r = perm ? perm[i] : (int32_t)i;
  uint64_t k = 0;
  if (valid_bit(valid, r)) {
    if (word == 0) {
      k = (uint64_t)data[2 * r];  // lo is unsigned: raw order
    } else {
      k = (uint64_t)data[2 * r + 1] ^ 0x8000000000000000ull;  // sign bias
    }
    if (desc) k = ~k;
  }
  return k;
}

__global__ void k_make_sort_keys_i128(const int64_t* __restrict__ data,
                                      const uint64_t* __restrict__ valid,
                                      const int32_t* __restrict__ perm,
                                      int desc, int word,
                                      uint64_t* __restrict__ keys,
                                      int64_t n, uint64_t* __restrict__ diff) {
  uint64_t k0 = 0, acc = 0;
  if (diff && n > 0) k0 = i128_key_at(data, valid, perm, desc, word, 0);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint64_t k = i128_key_at(data, valid, perm, desc, word, i);
    keys[i] = k;
    acc |= k ^ k0;
  }
  publish_key_diff(acc, diff);
}

// ---- radix pass ----------------------------------------------------------

__global__ void k_radix_count(const uint64_t* __restrict__ keys, int shift,
                              int64_t* __restrict__ counts, int64_t nblocks,
                              int64_t n, const uint64_t* __restrict__ diff) {
  if (radix_pass_skipped(diff, shift)) return;  // counts are not read
  __shared__ int lcnt[RADIX_BINS];
  for (int b = threadIdx.x; b < RADIX_BINS; b += blockDim.x) lcnt[b] = 0;
  __syncthreads();
  int64_t base = (int64_t)blockIdx.x * SORT_BLOCK * SORT_ITEMS;
#pragma unroll 4
  for (int it = 0; it < SORT_ITEMS; ++it) {
    int64_t i = base + (int64_t)it * SORT_BLOCK + threadIdx.x;
    if (i < n) {
      int digit = (int)((keys[i] >> shift) & 255);
      atomicAdd(&lcnt[digit], 1);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < RADIX_BINS; b += blockDim.x)
    counts[(int64_t)b * nblocks + blockIdx.x] = lcnt[b];
}

// Stable multi-round scatter: each round handles 256 rows in row order,
// maintaining a running per-digit offset in LDS across rounds so relative
// order is preserved within the block (LSD stability requirement).
__global__ void k_radix_scatter(const uint64_t* __restrict__ keys_in,
                                const int32_t* __restrict__ perm_in,
                                int shift,
                                const int64_t* __restrict__ offsets,
                                int64_t nblocks,
                                uint64_t* __restrict__ keys_out,
                                int32_t* __restrict__ perm_out, int64_t n,
                                const uint64_t* __restrict__ diff) {
  __shared__ int wave_bin[SORT_BLOCK / WAVE][RADIX_BINS];
  __shared__ int running[RADIX_BINS];
  int tid = threadIdx.x;
  int wid = tid / WAVE;
  int lane = tid & (WAVE - 1);
  int64_t base0 = (int64_t)blockIdx.x * SORT_BLOCK * SORT_ITEMS;
  if (radix_pass_skipped(diff, shift)) {
    // constant digit: the stable scatter is the identity, so copy the tile
    // through and the host's buffer ping-pong stays unconditional
    for (int it = 0; it < SORT_ITEMS; ++it) {
      int64_t i = base0 + (int64_t)it * SORT_BLOCK + tid;
      if (i < n) {
        keys_out[i] = keys_in[i];
        perm_out[i] = perm_in ? perm_in[i] : (int32_t)i;
      }
    }
    return;
  }
  for (int b = tid; b < RADIX_BINS; b += blockDim.x) running[b] = 0;

  for (int it = 0; it < SORT_ITEMS; ++it) {
    int64_t i = base0 + (int64_t)it * SORT_BLOCK + tid;
    bool active = i < n;
    uint64_t key = active ? keys_in[i] : 0;
    int digit = (int)((key >> shift) & 255);

    uint64_t active_mask = __ballot(active);
    uint64_t peers = active_mask;
    for (int b = 0; b < 8; ++b) {
      uint64_t m = __ballot((digit >> b) & 1);
      peers &= ((digit >> b) & 1) ? m : ~m;
    }
    uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    int rank_in_wave = __popcll(peers & lt);

    for (int w = 0; w < SORT_BLOCK / WAVE; ++w)
      for (int b = tid; b < RADIX_BINS; b += blockDim.x) wave_bin[w][b] = 0;
    __syncthreads();
    if (active && rank_in_wave == 0) wave_bin[wid][digit] = __popcll(peers);
    __syncthreads();
    // per-bin exclusive scan across the 4 waves, on top of `running`
    for (int b = tid; b < RADIX_BINS; b += blockDim.x) {
      int acc = running[b];
      for (int w = 0; w < SORT_BLOCK / WAVE; ++w) {
        int c = wave_bin[w][b];
        wave_bin[w][b] = acc;
        acc += c;
      }
      running[b] = acc;
    }
    __syncthreads();
    if (active) {
      int64_t base = offsets[(int64_t)digit * nblocks + blockIdx.x];
      int64_t pos = base + wave_bin[wid][digit] + rank_in_wave;
      keys_out[pos] = key;
      perm_out[pos] = perm_in ? perm_in[i] : (int32_t)i;
    }
    __syncthreads();
  }
}

extern "C" {

int64_t sort_num_blocks(int64_t n) {
  int64_t per = (int64_t)SORT_BLOCK * SORT_ITEMS;
  int64_t nb = (n + per - 1) / per;
  return nb < 1 ? 1 : nb;
}

int hipdf_sort_key_width(int t) { return sort_key_width(t); }

void hipdf_make_sort_keys_str(const void* offsets, const void* bytes,
                              const void* valid, const void* perm, int desc,
                              int chunk, void* keys, int64_t n,
                              hipStream_t stream) {
  hipLaunchKernelGGL(k_make_sort_keys_str, flat_grid(n), dim3(HIPDF_BLOCK),
                     0, stream, (const int32_t*)offsets,
                     (const uint8_t*)bytes, (const uint64_t*)valid,
                     (const int32_t*)perm, desc, chunk, (uint64_t*)keys, n,
                     (uint64_t*)nullptr);
}

void hipdf_make_sort_keys_i128(const void* data, const void* valid,
                               const void* perm, int desc, int word,
                               void* keys, int64_t n, hipStream_t stream) {
  hipLaunchKernelGGL(k_make_sort_keys_i128, flat_grid(n), dim3(HIPDF_BLOCK),
                     0, stream, (const int64_t*)data, (const uint64_t*)valid,
                     (const int32_t*)perm, desc, word, (uint64_t*)keys, n,
                     (uint64_t*)nullptr);
}

void hipdf_make_sort_keys(int t, const void* data, const void* valid,
                          const void* perm, int desc, int nulls_last,
                          int null_only, void* keys, int64_t n,
                          hipStream_t stream) {
  int w = sort_key_width(t);
  // null byte: NULLS LAST -> null rows get 1 (sort after valid rows);
  // NULLS FIRST -> null rows get 0 and valid rows 1
  int null_byte_null = nulls_last ? 1 : 0;
  dispatch_type(t, [&]<typename T>() {
    hipLaunchKernelGGL((k_make_sort_keys<T>), flat_grid(n), dim3(HIPDF_BLOCK),
                       0, stream, (const T*)data, (const uint64_t*)valid,
                       (const int32_t*)perm, desc, w, null_byte_null,
                       null_only, (uint64_t*)keys, n, (uint64_t*)nullptr);
  });
}

void hipdf_radix_count(const void* keys, int shift, void* counts, int64_t n,
                       hipStream_t stream) {
  int64_t nb = sort_num_blocks(n);
  hipLaunchKernelGGL(k_radix_count, dim3((uint32_t)nb), dim3(SORT_BLOCK), 0,
                     stream, (const uint64_t*)keys, shift, (int64_t*)counts,
                     nb, n, (const uint64_t*)nullptr);
}

void hipdf_radix_scatter(const void* keys_in, const void* perm_in, int shift,
                         const void* offsets, void* keys_out, void* perm_out,
                         int64_t n, hipStream_t stream) {
  int64_t nb = sort_num_blocks(n);
  hipLaunchKernelGGL(k_radix_scatter, dim3((uint32_t)nb), dim3(SORT_BLOCK), 0,
                     stream, (const uint64_t*)keys_in, (const int32_t*)perm_in,
                     shift, (const int64_t*)offsets, nb, (uint64_t*)keys_out,
                     (int32_t*)perm_out, n, (const uint64_t*)nullptr);
}

// The whole multi-key sort, enqueued on `stream` with no allocation and no
// synchronise: for each key, least significant first, build the u64 keys
// (and their varying-bits word), then run the digit passes. Caller-owned
// scratch: keys_a/keys_b u64[n], perm_a/perm_b i32[n], counts and scanned
// i64[256 * sort_num_blocks(n)], scan_scratch i64[scan_scratch_elems of
// that], diff u64[1]. out_perm i32[n] receives the final permutation.
void hipdf_sort_order(const HipdfSortKey* sort_keys, int nkeys, int64_t n,
                      void* keys_a, void* keys_b, void* perm_a, void* perm_b,
                      void* counts, void* scanned, void* scan_scratch,
                      void* diff_word, void* out_perm, hipStream_t stream) {
  if (n <= 0) return;
  uint64_t* keys[2] = {(uint64_t*)keys_a, (uint64_t*)keys_b};
  int32_t* perms[2] = {(int32_t*)perm_a, (int32_t*)perm_b};
  uint64_t* diff = (uint64_t*)diff_word;
  int64_t nb = sort_num_blocks(n);
  int kc = 0;                         // keys[kc] holds the current keys
  int pa = 0;                         // perms[pa] is the next pass's output
  const int32_t* cur_perm = nullptr;  // null = identity, nothing sorted yet

  auto passes = [&](int npasses) {
    for (int p = 0; p < npasses; ++p) {
      int sh = 8 * p;
      hipLaunchKernelGGL(k_radix_count, dim3((uint32_t)nb), dim3(SORT_BLOCK),
                         0, stream, (const uint64_t*)keys[kc], sh,
                         (int64_t*)counts, nb, n, (const uint64_t*)diff);
      hipdf_exclusive_scan_i64_skip(counts, scanned, scan_scratch,
                                    RADIX_BINS * nb, diff, sh, stream);
      hipLaunchKernelGGL(k_radix_scatter, dim3((uint32_t)nb),
                         dim3(SORT_BLOCK), 0, stream,
                         (const uint64_t*)keys[kc], cur_perm, sh,
                         (const int64_t*)scanned, nb, keys[1 - kc], perms[pa],
                         n, (const uint64_t*)diff);
      kc = 1 - kc;
      cur_perm = perms[pa];
      pa = 1 - pa;
    }
  };
  auto make_fixed = [&](int t, const HipdfSortKey& k, int null_only) {
    (void)hipMemsetAsync(diff, 0, sizeof(uint64_t), stream);
    int w = sort_key_width(t);
    int null_byte_null = k.nulls_last ? 1 : 0;
    dispatch_type(t, [&]<typename T>() {
      hipLaunchKernelGGL((k_make_sort_keys<T>), flat_grid(n),
                         dim3(HIPDF_BLOCK), 0, stream, (const T*)k.data,
                         (const uint64_t*)k.valid, cur_perm, k.desc, w,
                         null_byte_null, null_only, keys[kc], n, diff);
    });
  };

  // least-significant key first: stability carries earlier orders forward
  for (int ki = nkeys - 1; ki >= 0; --ki) {
    const HipdfSortKey& k = sort_keys[ki];
    bool wide = k.kind != SORT_KEY_FIXED;
    if (k.kind == SORT_KEY_STRING) {
      for (int chunk = k.nchunks - 1; chunk >= 0; --chunk) {
        (void)hipMemsetAsync(diff, 0, sizeof(uint64_t), stream);
        hipLaunchKernelGGL(k_make_sort_keys_str, flat_grid(n),
                           dim3(HIPDF_BLOCK), 0, stream,
                           (const int32_t*)k.offsets, (const uint8_t*)k.data,
                           (const uint64_t*)k.valid, cur_perm, k.desc, chunk,
                           keys[kc], n, diff);
        passes(8);
      }
    } else if (k.kind == SORT_KEY_DECIMAL128) {
      for (int word = 0; word < 2; ++word) {  // lo (unsigned) then hi
        (void)hipMemsetAsync(diff, 0, sizeof(uint64_t), stream);
        hipLaunchKernelGGL(k_make_sort_keys_i128, flat_grid(n),
                           dim3(HIPDF_BLOCK), 0, stream,
                           (const int64_t*)k.data, (const uint64_t*)k.valid,
                           cur_perm, k.desc, word, keys[kc], n, diff);
        passes(8);
      }
    } else {
      int vwidth = sort_key_width(k.htype);
      bool embedded_null = vwidth < 8;  // null byte fits above the value
      make_fixed(k.htype, k, 0);
      passes(vwidth + ((k.has_valid && embedded_null) ? 1 : 0));
      wide = !embedded_null;
    }
    if (k.has_valid && wide) {
      // no embedded null byte: one extra null-ordering pass
      make_fixed(HT_I64, k, 1);
      passes(1);
    }
  }
  if (cur_perm) {
    (void)hipMemcpyAsync(out_perm, cur_perm, (size_t)n * sizeof(int32_t),
                         hipMemcpyDeviceToDevice, stream);
  } else {
    hipdf_iota_i32(out_perm, n, stream);
  }
}

}  // extern "C"
