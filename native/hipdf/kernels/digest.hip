// md5 / sha1 / sha2 as lowercase hex strings and crc32 over a STRING column's
// UTF-8 bytes (reference analogue: GpuMd5, GpuSha1, GpuSha2, GpuCrc32 over
// spark-rapids-jni Hash). The digests themselves are in digest.h, which a
// host program runs too.
//
// Thread per row, grid-stride: one message's digest is serial, so the
// parallelism is across rows (and thread-per-row beat wave-per-row by about
// 6x at short keys for the string hashes in hash.hip). Every row's result
// has the same width W, so row i is written at out + i * W with no size pass
// and no scan; the caller's offsets are i * W.
#include "hipdf.h"
#include "hipdf_common.h"
#include "digest.h"

namespace {

typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

// W bytes at o, which is 8-byte aligned, 16-byte when W is a multiple of 16
template <int W>
__device__ __forceinline__ void store_hex(uint8_t* o, const uint64_t* h) {
  if constexpr (W % 16 == 0) {
#pragma unroll
    for (int k = 0; k < W / 16; ++k) {
      u64x2 v = {h[2 * k], h[2 * k + 1]};
      *reinterpret_cast<u64x2*>(o + 16 * k) = v;
    }
  } else {
#pragma unroll
    for (int k = 0; k < W / 8; ++k)
      *reinterpret_cast<uint64_t*>(o + 8 * k) = h[k];
  }
}

template <class A>
__global__ void __launch_bounds__(HIPDF_BLOCK)
k_digest_hex(const int32_t* __restrict__ offsets,
             const uint8_t* __restrict__ bytes,
             const uint64_t* __restrict__ av, uint8_t* __restrict__ out,
             int64_t n) {
  constexpr int W = digest::hex_width<A>();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint64_t h[W / 8];
    if (valid_bit(av, i)) {
      typename A::word st[A::kState];
      int32_t s = offsets[i];
      digest::digest_row<A>(bytes + s, (int64_t)offsets[i + 1] - s, st);
#pragma unroll
      for (int k = 0; k < W / 8; ++k) h[k] = digest::hex8(A::out32(st, k));
    } else {
      // a null row's bytes are defined too: '0' digits
#pragma unroll
      for (int k = 0; k < W / 8; ++k) h[k] = 0x3030303030303030ull;
    }
    store_hex<W>(out + i * W, h);
  }
}

__constant__ digest::Crc32Table d_crc32_table = digest::make_crc32_table();

__global__ void __launch_bounds__(HIPDF_BLOCK)
k_crc32_str(const int32_t* __restrict__ offsets,
            const uint8_t* __restrict__ bytes,
            const uint64_t* __restrict__ av, int64_t* __restrict__ out,
            int64_t n) {
  __shared__ uint32_t tab[256];
  for (int t = threadIdx.x; t < 256; t += blockDim.x)
    tab[t] = d_crc32_table.t[t];
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t v = 0;
    if (valid_bit(av, i)) {
      int32_t s = offsets[i];
      v = (int64_t)digest::crc32_row(tab, bytes + s,
                                     (int64_t)offsets[i + 1] - s);
    }
    out[i] = v;
  }
}

template <class A>
void launch_digest(const void* offsets, const void* bytes, const void* av,
                   void* out, int64_t n, hipStream_t stream) {
  hipLaunchKernelGGL((k_digest_hex<A>), flat_grid(n), dim3(HIPDF_BLOCK), 0,
                     stream, (const int32_t*)offsets, (const uint8_t*)bytes,
                     (const uint64_t*)av, (uint8_t*)out, n);
}

}  // namespace

extern "C" {

void hipdf_digest_hex(int algo, const void* offsets, const void* bytes,
                      const void* av, void* out_bytes, int64_t n,
                      hipStream_t stream) {
  if (algo < 0 || algo > 5) throw std::runtime_error("hipdf: bad digest algo");
  if (n <= 0) return;
  if ((uintptr_t)out_bytes & 15)
    throw std::runtime_error("hipdf: digest output must be 16-byte aligned");
  switch (algo) {
    case 0: launch_digest<digest::Md5>(offsets, bytes, av, out_bytes, n, stream); break;
    case 1: launch_digest<digest::Sha1>(offsets, bytes, av, out_bytes, n, stream); break;
    case 2: launch_digest<digest::Sha224>(offsets, bytes, av, out_bytes, n, stream); break;
    case 3: launch_digest<digest::Sha256>(offsets, bytes, av, out_bytes, n, stream); break;
    case 4: launch_digest<digest::Sha384>(offsets, bytes, av, out_bytes, n, stream); break;
    default: launch_digest<digest::Sha512>(offsets, bytes, av, out_bytes, n, stream); break;
  }
}

void hipdf_crc32_str(const void* offsets, const void* bytes, const void* av,
                     void* out_i64, int64_t n, hipStream_t stream) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_crc32_str, flat_grid(n), dim3(HIPDF_BLOCK), 0, stream,
                     (const int32_t*)offsets, (const uint8_t*)bytes,
                     (const uint64_t*)av, (int64_t*)out_i64, n);
}

}  // extern "C"
