// get_json_object on the device: one thread per row runs the validating
// parser of json_path.h over the whole row (size pass), then re-reads only
// the matched span and writes the normalised bytes (write pass). Rows are
// independent and of uneven length, so both kernels are thread-per-row and
// grid-strided; the parser's state is a 64-bit container stack plus scalars
// and stays in registers.
#include "hipdf.h"
#include "hipdf_common.h"
#include "json_path.h"

__global__ void k_json_path_size(const int32_t* __restrict__ offsets,
                                 const uint8_t* __restrict__ data,
                                 const uint64_t* __restrict__ valid,
                                 const int32_t* __restrict__ steps,
                                 const uint8_t* __restrict__ names,
                                 int nsteps, int64_t* __restrict__ out_len,
                                 int32_t* __restrict__ src_start,
                                 int32_t* __restrict__ src_len,
                                 uint8_t* __restrict__ state, int64_t n) {
  jsonpath::Path path{steps, names, nsteps};
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    jsonpath::RowResult r{0, 0, 0, jsonpath::JP_NULL};
    if (valid_bit(valid, i))
      r = jsonpath::scan_row(data, offsets[i], offsets[i + 1], path);
    out_len[i] = r.out_len;
    src_start[i] = r.src_start;
    src_len[i] = r.src_len;
    state[i] = r.state;
  }
}

// Size pass for npaths <= K paths in one parse per row. Path k's steps are
// steps[3 * step_off[k] ..) and step_cnt[k] of them; key names index the one
// names blob. Results are path-major: entry k * n + i is row i of path k, so
// each path's arrays are contiguous and the write kernel serves all of them
// as one array of npaths * n entries. A path slot beyond npaths repeats path
// 0 and is not stored.
template <int K>
__global__ void __launch_bounds__(HIPDF_BLOCK) k_json_path_multi_size(
    const int32_t* __restrict__ offsets, const uint8_t* __restrict__ data,
    const uint64_t* __restrict__ valid, const int32_t* __restrict__ steps,
    const int32_t* __restrict__ step_off,
    const int32_t* __restrict__ step_cnt, const uint8_t* __restrict__ names,
    int npaths, int64_t* __restrict__ out_len,
    int32_t* __restrict__ src_start, int32_t* __restrict__ src_len,
    uint8_t* __restrict__ state, int64_t n) {
  jsonpath::PathGroup<K> group;
  group.steps = steps;
  group.names = names;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    int q = k < npaths ? k : 0;
    group.sbase[k] = 3 * step_off[q];
    group.nsteps[k] = step_cnt[q];
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    jsonpath::RowResult r[K];
    // a NULL row is scanned as an empty one: NULL and zeros for every path
    int32_t rs = offsets[i];
    int32_t re = valid_bit(valid, i) ? offsets[i + 1] : rs;
    jsonpath::scan_row_multi<K>(data, rs, re, group, r);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (k >= npaths) continue;
      int64_t at = (int64_t)k * n + i;
      out_len[at] = r[k].out_len;
      src_start[at] = r[k].src_start;
      src_len[at] = r[k].src_len;
      state[at] = r[k].state;
    }
  }
}

__global__ void k_json_path_write(const uint8_t* __restrict__ data,
                                  const int32_t* __restrict__ src_start,
                                  const int32_t* __restrict__ src_len,
                                  const uint8_t* __restrict__ state,
                                  const int64_t* __restrict__ out_off,
                                  const int64_t* __restrict__ out_len,
                                  uint8_t* __restrict__ out_bytes,
                                  int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (state[i] != jsonpath::JP_VALUE) continue;
    jsonpath::write_row(data, src_start[i], src_len[i],
                        out_bytes + out_off[i], out_len[i]);
  }
}

extern "C" {

void hipdf_json_path(const void* offsets, const void* bytes,
                     const void* valid, const void* steps, const void* names,
                     int nsteps, const void* out_off, void* out_len,
                     void* src_start, void* src_len, void* state,
                     void* out_bytes, int mode, int64_t n,
                     hipStream_t stream) {
  if (mode == 0) {
    hipLaunchKernelGGL(k_json_path_size, flat_grid(n), dim3(HIPDF_BLOCK), 0,
                       stream, (const int32_t*)offsets, (const uint8_t*)bytes,
                       (const uint64_t*)valid, (const int32_t*)steps,
                       (const uint8_t*)names, nsteps, (int64_t*)out_len,
                       (int32_t*)src_start, (int32_t*)src_len,
                       (uint8_t*)state, n);
  } else {
    hipLaunchKernelGGL(k_json_path_write, flat_grid(n), dim3(HIPDF_BLOCK), 0,
                       stream, (const uint8_t*)bytes,
                       (const int32_t*)src_start, (const int32_t*)src_len,
                       (const uint8_t*)state, (const int64_t*)out_off,
                       (const int64_t*)out_len, (uint8_t*)out_bytes, n);
  }
}

void hipdf_json_path_multi(const void* offsets, const void* bytes,
                           const void* valid, const void* steps,
                           const void* step_off, const void* step_cnt,
                           const void* names, int npaths, void* out_len,
                           void* src_start, void* src_len, void* state,
                           int64_t n, hipStream_t stream) {
  if (npaths < 1 || npaths > jsonpath::kMaxFusedPaths || n <= 0) return;
#define HIPDF_JSON_MULTI(K)                                                  \
  hipLaunchKernelGGL(k_json_path_multi_size<K>, flat_grid(n),                \
                     dim3(HIPDF_BLOCK), 0, stream, (const int32_t*)offsets,  \
                     (const uint8_t*)bytes, (const uint64_t*)valid,          \
                     (const int32_t*)steps, (const int32_t*)step_off,        \
                     (const int32_t*)step_cnt, (const uint8_t*)names,        \
                     npaths, (int64_t*)out_len, (int32_t*)src_start,         \
                     (int32_t*)src_len, (uint8_t*)state, n)
  if (npaths <= 2) HIPDF_JSON_MULTI(2);
  else if (npaths <= 4) HIPDF_JSON_MULTI(4);
  else HIPDF_JSON_MULTI(8);
#undef HIPDF_JSON_MULTI
}

}  // extern "C"
