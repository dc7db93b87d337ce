// Order-preserving u64 key transforms shared by the global radix sort
// (sort.hip) and the segmented list sort (lists.hip): sign-flipped ints,
// IEEE-flipped floats with Spark's NaN (canonical, greatest) and -0.0
// (== 0.0) normalization. Unsigned comparison of the keys is the engine's
// ascending value order.
#pragma once

#include "hipdf_common.h"

template <typename T>
__device__ __forceinline__ uint64_t sort_key_of(T v);

template <> __device__ __forceinline__ uint64_t sort_key_of<uint8_t>(uint8_t v) {
  return v;
}
template <> __device__ __forceinline__ uint64_t sort_key_of<int8_t>(int8_t v) {
  return (uint8_t)(v ^ (int8_t)0x80);
}
template <> __device__ __forceinline__ uint64_t sort_key_of<int16_t>(int16_t v) {
  return (uint16_t)(v ^ (int16_t)0x8000);
}
template <> __device__ __forceinline__ uint64_t sort_key_of<int32_t>(int32_t v) {
  return (uint32_t)(v ^ (int32_t)0x80000000);
}
template <> __device__ __forceinline__ uint64_t sort_key_of<int64_t>(int64_t v) {
  return (uint64_t)v ^ 0x8000000000000000ull;
}
template <> __device__ __forceinline__ uint64_t sort_key_of<float>(float v) {
  if (isnan(v)) v = __uint_as_float(0x7FC00000u);  // canonical, greatest
  if (v == 0.0f) v = 0.0f;                          // -0.0 -> 0.0
  uint32_t b = __float_as_uint(v);
  b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return b;
}
template <> __device__ __forceinline__ uint64_t sort_key_of<double>(double v) {
  if (isnan(v)) v = __longlong_as_double(0x7FF8000000000000ll);
  if (v == 0.0) v = 0.0;
  uint64_t b = (uint64_t)__double_as_longlong(v);
  return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
}
