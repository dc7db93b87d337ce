// Hash equi-join gather maps: build chained hash table on the build side,
// probe from the stream side, emit (left_map, right_map) row indices
// (reference analogue: cudf innerJoinGatherMaps / leftJoinGatherMaps /
// leftSemi/AntiJoinGatherMap reached from GpuHashJoin — SURVEY.md §2.8A).
// Null join keys never match (Spark equi-join semantics): they are neither
// inserted nor probed.
//
// Chained table: head[slot] -> newest row, next[row] -> older row in bucket.
// Duplicates and collisions live on the chain; equality filters on probe.
#include "hipdf.h"
#include "hipdf_common.h"
#include "keys.h"
#include "murmur3.h"

enum JoinHow : int { J_INNER = 0, J_LEFT, J_SEMI, J_ANTI, J_FULL };

__global__ void k_join_build(const int32_t* __restrict__ hashes,
                             const KeyCol* __restrict__ keys, int nkeys,
                             int32_t* __restrict__ head,
                             int32_t* __restrict__ next, uint32_t slot_mask,
                             int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (row_has_null_key(keys, nkeys, i)) continue;
    uint32_t slot = slot_of((uint32_t)hashes[i], slot_mask);
    next[i] = atomicExch(&head[slot], (int32_t)i);
  }
}

// pass 1: per-probe-row output count
__global__ void k_join_count(int how, const int32_t* __restrict__ lhashes,
                             const KeyCol* __restrict__ lkeys,
                             const KeyCol* __restrict__ rkeys, int nkeys,
                             const int32_t* __restrict__ head,
                             const int32_t* __restrict__ next,
                             uint32_t slot_mask, int64_t* __restrict__ counts,
                             int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t matches = 0;
    if (!row_has_null_key(lkeys, nkeys, i)) {
      uint32_t slot = slot_of((uint32_t)lhashes[i], slot_mask);
      for (int32_t r = head[slot]; r != -1; r = next[r]) {
        if (rows_equal(lkeys, rkeys, nkeys, i, r)) {
          ++matches;
          if (how == J_SEMI || how == J_ANTI) break;
        }
      }
    }
    int64_t c;
    switch (how) {
      case J_INNER: c = matches; break;
      case J_LEFT: case J_FULL: c = matches ? matches : 1; break;
      case J_SEMI: c = matches ? 1 : 0; break;
      default: c = matches ? 0 : 1; break;  // anti
    }
    counts[i] = c;
  }
}

// pass 2: fill gather maps at scanned offsets
__global__ void k_join_fill(int how, const int32_t* __restrict__ lhashes,
                            const KeyCol* __restrict__ lkeys,
                            const KeyCol* __restrict__ rkeys, int nkeys,
                            const int32_t* __restrict__ head,
                            const int32_t* __restrict__ next,
                            uint32_t slot_mask,
                            const int64_t* __restrict__ offsets,
                            int32_t* __restrict__ lmap,
                            int32_t* __restrict__ rmap,
                            uint8_t* __restrict__ right_matched, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t off = offsets[i];
    int64_t matches = 0;
    if (!row_has_null_key(lkeys, nkeys, i)) {
      uint32_t slot = slot_of((uint32_t)lhashes[i], slot_mask);
      for (int32_t r = head[slot]; r != -1; r = next[r]) {
        if (rows_equal(lkeys, rkeys, nkeys, i, r)) {
          ++matches;
          if (how == J_INNER || how == J_LEFT || how == J_FULL) {
            lmap[off] = (int32_t)i;
            rmap[off] = r;
            if (right_matched) right_matched[r] = 1;
            ++off;
          } else {
            break;
          }
        }
      }
    }
    if ((how == J_LEFT || how == J_FULL) && matches == 0) {
      lmap[off] = (int32_t)i;
      rmap[off] = -1;  // null right row
    } else if (how == J_SEMI && matches) {
      lmap[off] = (int32_t)i;
    } else if (how == J_ANTI && matches == 0) {
      lmap[off] = (int32_t)i;
    }
  }
}

// ---- unique build side --------------------------------------------------
// When no two build rows share a key every probe row has 0 or 1 matches,
// so the per-row count, the row-level scan and the second chain walk of the
// general path are not needed. The probe is the 3-phase stream compaction
// of selection.hip (k_mask_count / k_mask_scatter): one chain walk writes
// match[row] and per-block emit counts, the block counts are scanned, and a
// compaction pass writes the maps in ascending left-row order.

#define JOIN_ITEMS 4  // probe rows per thread per block
#define JOIN_SEED 42u  // seed of the build-side row hash (gpu_backend.py)
#define JOIN_WAVES (HIPDF_BLOCK / WAVE)

// after k_join_build: a non-null build row whose key also sits further
// down its own chain (an older row) is a duplicate
__global__ void k_join_check_unique(const KeyCol* __restrict__ keys, int nkeys,
                                    const int32_t* __restrict__ next,
                                    int32_t* __restrict__ dup_flag,
                                    int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (row_has_null_key(keys, nkeys, i)) continue;
    for (int32_t r = next[i]; r != -1; r = next[r]) {
      if (rows_equal(keys, keys, nkeys, i, r)) {
        atomicOr(dup_flag, 1);
        break;
      }
    }
  }
}

// does a probe row with match index r (-1 = none) emit an output row
__device__ __forceinline__ bool join_emits(int how, int32_t r) {
  return how == J_ANTI ? r < 0 : (how == J_LEFT || how == J_FULL || r >= 0);
}

// inline murmur3 of one integer key: bit-identical to k_murmur3_col with
// HK_INT (value widened to int32) / HK_LONG and the same seed
template <typename T>
__device__ __forceinline__ uint32_t join_key_hash(T v) {
  if constexpr (sizeof(T) == 8)
    return hash_long((uint64_t)(int64_t)v, JOIN_SEED);
  else
    return hash_int((uint32_t)(int32_t)v, JOIN_SEED);
}

// block-wide sum of `count`, written by thread 0 (block_counts may be null:
// left/full joins emit every probe row and need no counts)
__device__ __forceinline__ void join_block_count(
    int count, int64_t* __restrict__ block_counts) {
  if (!block_counts) return;
  for (int off = WAVE / 2; off > 0; off >>= 1)
    count += __shfl_down(count, off);
  __shared__ int wave_sums[JOIN_WAVES];
  if (lane_id() == 0) wave_sums[threadIdx.x / WAVE] = count;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
    for (int w = 0; w < JOIN_WAVES; ++w) total += wave_sums[w];
    block_counts[blockIdx.x] = total;
  }
}

// phase 1, single integer key: hash computed inline from the key, build key
// compared directly (chain rows are never null: nulls are not inserted)
template <typename T>
__global__ void __launch_bounds__(HIPDF_BLOCK)
k_join_probe_unique_key(int how, const T* __restrict__ lkey,
                        const uint64_t* __restrict__ lvalid,
                        const T* __restrict__ rkey,
                        const int32_t* __restrict__ head,
                        const int32_t* __restrict__ next, uint32_t slot_mask,
                        int32_t* __restrict__ match,
                        uint8_t* __restrict__ right_matched,
                        int64_t* __restrict__ block_counts, int64_t n) {
  int64_t base = (int64_t)blockIdx.x * HIPDF_BLOCK * JOIN_ITEMS;
  T v[JOIN_ITEMS];
  int32_t cur[JOIN_ITEMS];
  // issue the key and chain-head loads of all items before walking any
#pragma unroll
  for (int it = 0; it < JOIN_ITEMS; ++it) {
    int64_t row = base + it * HIPDF_BLOCK + threadIdx.x;
    cur[it] = -1;
    v[it] = T{};
    if (row < n && valid_bit(lvalid, row)) {
      v[it] = lkey[row];
      cur[it] = head[slot_of(join_key_hash<T>(v[it]), slot_mask)];
    }
  }
  int count = 0;
#pragma unroll
  for (int it = 0; it < JOIN_ITEMS; ++it) {
    int64_t row = base + it * HIPDF_BLOCK + threadIdx.x;
    if (row >= n) continue;
    int32_t r = cur[it];
    while (r != -1 && rkey[r] != v[it]) r = next[r];
    match[row] = r;
    if (r >= 0 && right_matched) right_matched[r] = 1;
    count += join_emits(how, r) ? 1 : 0;
  }
  join_block_count(count, block_counts);
}

// phase 1, any key shape (strings, floats, decimal128, several columns):
// precomputed row hashes, generic row equality
__global__ void __launch_bounds__(HIPDF_BLOCK)
k_join_probe_unique(int how, const int32_t* __restrict__ lhashes,
                    const KeyCol* __restrict__ lkeys,
                    const KeyCol* __restrict__ rkeys, int nkeys,
                    const int32_t* __restrict__ head,
                    const int32_t* __restrict__ next, uint32_t slot_mask,
                    int32_t* __restrict__ match,
                    uint8_t* __restrict__ right_matched,
                    int64_t* __restrict__ block_counts, int64_t n) {
  int64_t base = (int64_t)blockIdx.x * HIPDF_BLOCK * JOIN_ITEMS;
  int count = 0;
  for (int it = 0; it < JOIN_ITEMS; ++it) {
    int64_t row = base + it * HIPDF_BLOCK + threadIdx.x;
    if (row >= n) continue;
    int32_t r = -1;
    if (!row_has_null_key(lkeys, nkeys, row)) {
      r = head[slot_of((uint32_t)lhashes[row], slot_mask)];
      while (r != -1 && !rows_equal(lkeys, rkeys, nkeys, row, r)) r = next[r];
    }
    match[row] = r;
    if (r >= 0 && right_matched) right_matched[r] = 1;
    count += join_emits(how, r) ? 1 : 0;
  }
  join_block_count(count, block_counts);
}

// phase 3: compact emitting rows into the gather maps at the scanned block
// offsets. Rows are visited in the order of phase 1 (item, wave, lane), which
// is ascending row order, so lmap comes out ascending.
__global__ void __launch_bounds__(HIPDF_BLOCK)
k_join_compact_unique(int how, const int32_t* __restrict__ match,
                      const int64_t* __restrict__ block_offsets,
                      int32_t* __restrict__ lmap, int32_t* __restrict__ rmap,
                      int64_t n) {
  __shared__ int wave_counts[JOIN_ITEMS * JOIN_WAVES];
  int64_t base = (int64_t)blockIdx.x * HIPDF_BLOCK * JOIN_ITEMS;
  int wid = threadIdx.x / WAVE;
  int lane = lane_id();
  uint64_t below = (1ull << lane) - 1;
  int32_t r[JOIN_ITEMS];
  bool emit[JOIN_ITEMS];
  int prefix[JOIN_ITEMS];
#pragma unroll
  for (int it = 0; it < JOIN_ITEMS; ++it) {
    int64_t row = base + it * HIPDF_BLOCK + threadIdx.x;
    r[it] = row < n ? match[row] : -1;
    emit[it] = row < n && join_emits(how, r[it]);
    uint64_t ballot = __ballot(emit[it]);
    prefix[it] = __popcll(ballot & below);
    if (lane == 0) wave_counts[it * JOIN_WAVES + wid] = __popcll(ballot);
  }
  __syncthreads();
  int64_t pos = block_offsets[blockIdx.x];
  int slot = 0;
#pragma unroll
  for (int it = 0; it < JOIN_ITEMS; ++it) {
    // emitting rows of earlier (item, wave) pairs come first
    for (int w = 0; w < JOIN_WAVES; ++w, ++slot) {
      if (w == wid && emit[it]) {
        int64_t row = base + it * HIPDF_BLOCK + threadIdx.x;
        lmap[pos + prefix[it]] = (int32_t)row;
        if (rmap) rmap[pos + prefix[it]] = r[it];
      }
      pos += wave_counts[slot];
    }
  }
}

extern "C" {

int64_t join_probe_num_blocks(int64_t n) {
  return (n + (int64_t)HIPDF_BLOCK * JOIN_ITEMS - 1) /
         ((int64_t)HIPDF_BLOCK * JOIN_ITEMS);
}

void hipdf_join_check_unique(const void* keys, int nkeys, const void* next,
                             void* dup_flag, int64_t n, hipStream_t stream) {
  hipLaunchKernelGGL(k_join_check_unique, flat_grid(n), dim3(HIPDF_BLOCK), 0,
                     stream, (const KeyCol*)keys, nkeys, (const int32_t*)next,
                     (int32_t*)dup_flag, n);
}

// key_type >= 0: single integer key column of that HType, hashed inline
// (lkey / lvalid / rkey are its buffers; lhashes, lkeys, rkeys unused);
// key_type < 0: precomputed lhashes + KeyCol descriptors
void hipdf_join_probe_unique(int how, int key_type, const void* lkey,
                             const void* lvalid, const void* rkey,
                             const void* lhashes, const void* lkeys,
                             const void* rkeys, int nkeys, const void* head,
                             const void* next, int64_t cap, void* match,
                             void* right_matched, void* block_counts,
                             int64_t n, hipStream_t stream) {
  if (n <= 0) return;
  dim3 grid((uint32_t)join_probe_num_blocks(n));
  uint32_t slot_mask = (uint32_t)(cap - 1);
  if (key_type < 0) {
    hipLaunchKernelGGL(k_join_probe_unique, grid, dim3(HIPDF_BLOCK), 0, stream,
                       how, (const int32_t*)lhashes, (const KeyCol*)lkeys,
                       (const KeyCol*)rkeys, nkeys, (const int32_t*)head,
                       (const int32_t*)next, slot_mask, (int32_t*)match,
                       (uint8_t*)right_matched, (int64_t*)block_counts, n);
    return;
  }
  if (key_type > HT_I64)
    throw std::runtime_error("hipdf: join inline hash needs an integer key");
  dispatch_type(key_type, [&]<typename T>() {
    if constexpr (std::is_integral_v<T>) {
      hipLaunchKernelGGL((k_join_probe_unique_key<T>), grid,
                         dim3(HIPDF_BLOCK), 0, stream, how, (const T*)lkey,
                         (const uint64_t*)lvalid, (const T*)rkey,
                         (const int32_t*)head, (const int32_t*)next, slot_mask,
                         (int32_t*)match, (uint8_t*)right_matched,
                         (int64_t*)block_counts, n);
    }
  });
}

void hipdf_join_compact_unique(int how, const void* match,
                               const void* block_offsets, void* lmap,
                               void* rmap, int64_t n, hipStream_t stream) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_join_compact_unique,
                     dim3((uint32_t)join_probe_num_blocks(n)),
                     dim3(HIPDF_BLOCK), 0, stream, how, (const int32_t*)match,
                     (const int64_t*)block_offsets, (int32_t*)lmap,
                     (int32_t*)rmap, n);
}

void hipdf_join_build(const void* hashes, const void* keys, int nkeys,
                      void* head, void* next, int64_t cap, int64_t n,
                      hipStream_t stream) {
  hipLaunchKernelGGL(k_join_build, flat_grid(n), dim3(HIPDF_BLOCK), 0, stream,
                     (const int32_t*)hashes, (const KeyCol*)keys, nkeys,
                     (int32_t*)head, (int32_t*)next, (uint32_t)(cap - 1), n);
}

void hipdf_join_count(int how, const void* lhashes, const void* lkeys,
                      const void* rkeys, int nkeys, const void* head,
                      const void* next, int64_t cap, void* counts, int64_t n,
                      hipStream_t stream) {
  hipLaunchKernelGGL(k_join_count, flat_grid(n), dim3(HIPDF_BLOCK), 0, stream,
                     how, (const int32_t*)lhashes, (const KeyCol*)lkeys,
                     (const KeyCol*)rkeys, nkeys, (const int32_t*)head,
                     (const int32_t*)next, (uint32_t)(cap - 1),
                     (int64_t*)counts, n);
}

void hipdf_join_fill(int how, const void* lhashes, const void* lkeys,
                     const void* rkeys, int nkeys, const void* head,
                     const void* next, int64_t cap, const void* offsets,
                     void* lmap, void* rmap, void* right_matched, int64_t n,
                     hipStream_t stream) {
  hipLaunchKernelGGL(k_join_fill, flat_grid(n), dim3(HIPDF_BLOCK), 0, stream,
                     how, (const int32_t*)lhashes, (const KeyCol*)lkeys,
                     (const KeyCol*)rkeys, nkeys, (const int32_t*)head,
                     (const int32_t*)next, (uint32_t)(cap - 1),
                     (const int64_t*)offsets, (int32_t*)lmap, (int32_t*)rmap,
                     (uint8_t*)right_matched, n);
}

}  // extern "C"
