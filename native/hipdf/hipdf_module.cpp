// pybind11 bindings for the hipdf CDNA4 kernel library.
// Python (spark_rapids_amd/ops/gpu_backend.py) passes torch tensor
// data_ptr()s, sizes and the current torch HIP stream; all device buffers are
// allocated by the PyTorch-ROCm caching allocator (the RMM-style pool on
// 288 GB HBM3E) so hipdf itself never calls hipMalloc.
//
// The C surface is declared once, in include/hipdf.h; nothing is re-declared
// here. A pass-through entry point is bound with BIND(name), which derives
// the python signature from the declaration.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "hipdf.h"

namespace py = pybind11;

static void check_async() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    throw std::runtime_error(std::string("hipdf kernel launch: ") +
                             hipGetErrorString(e));
}

// ---- generic binder -------------------------------------------------------
// bound<&hipdf_f>::call has hipdf_f's parameter list with every const void*,
// void* and hipStream_t taken as an int64 (a data_ptr() or the stream
// handle) and every other type unchanged, in the same order. It calls
// hipdf_f with the GIL held, then check_async(), so a failed launch raises
// at the call that made it.
template <class T>
inline constexpr bool is_handle = std::is_same_v<T, const void*> ||
                                  std::is_same_v<T, void*> ||
                                  std::is_same_v<T, hipStream_t>;
template <class T>
using py_arg = std::conditional_t<is_handle<T>, int64_t, T>;

template <class T>
static T to_c(py_arg<T> v) {
  if constexpr (is_handle<T>)
    return reinterpret_cast<T>(v);
  else
    return v;
}

template <auto F>
struct bound;
template <class... A, void (*F)(A...)>
struct bound<F> {
  static void call(py_arg<A>... a) {
    F(to_c<A>(a)...);
    check_async();
  }
};

#define BIND(name) m.def(#name, &bound<&hipdf_##name>::call)

// heap-allocated and intentionally leaked: a static py::object would run
// its destructor at .so unload AFTER Py_Finalize and crash the exit
static py::object* g_spill_cb = nullptr;

static int spill_cb_trampoline(size_t needed, int retry) {
  if (!g_spill_cb || !Py_IsInitialized()) return 0;
  py::gil_scoped_acquire gil;
  try {
    return (*g_spill_cb)((size_t)needed, retry).cast<int>();
  } catch (const std::exception& e) {
    fprintf(stderr, "[hipdf pool] spill callback raised: %s\n", e.what());
    PyErr_Clear();
    return 0;
  } catch (...) {
    PyErr_Clear();
    return 0;
  }
}

// Host-side walk of an RLE/bit-packed hybrid stream's RUN HEADERS: one
// varint per run (cheap), emitting [kind, src_off_abs, out_off, count]
// int64 records for the fully parallel k_rle_expand kernel. Returns the
// number of runs, or -1 when max_runs would overflow / stream malformed.
static int64_t rle_walk(const uint8_t* data, int64_t nbytes, int bit_width,
                        int64_t n_values, int64_t src_base, int64_t out_base,
                        int64_t* runs, int64_t max_runs) {
  int64_t pos = 0, emitted = 0, nruns = 0;
  int byte_per_val = (bit_width + 7) / 8;
  while (emitted < n_values) {
    if (pos >= nbytes) return -1;
    uint64_t h = 0;
    int shift = 0;
    while (pos < nbytes) {
      uint8_t b = data[pos++];
      h |= (uint64_t)(b & 0x7F) << shift;
      if (!(b & 0x80)) break;
      shift += 7;
    }
    if (nruns >= max_runs) return -1;
    int64_t* r = runs + 4 * nruns;
    if ((h & 1) == 0) {
      int64_t cnt = (int64_t)(h >> 1);
      if (cnt <= 0) return -1;
      r[0] = (int64_t)bit_width << 1;  // kind 0 | bw
      r[1] = src_base + pos;
      r[2] = out_base + emitted;
      r[3] = cnt;
      pos += byte_per_val;
      emitted += cnt;
    } else {
      int64_t groups = (int64_t)(h >> 1);
      if (groups <= 0) return -1;
      r[0] = ((int64_t)bit_width << 1) | 1;  // kind 1 | bw
      r[1] = src_base + pos;
      r[2] = out_base + emitted;
      r[3] = groups * 8;
      pos += groups * bit_width;
      emitted += groups * 8;
    }
    ++nruns;
  }
  return nruns;
}

// Host-side walk of parquet length-prefixed BYTE_ARRAY records. The chain
// pos -> len -> pos is inherently serial, so it runs on the CPU (one
// dependent L1 load per record, ~2ns) instead of a single GPU thread
// (~70ns per dependent global load); the GIL is released so the
// multi-file prefetch pool overlaps walks across column chunks.
static int64_t byte_array_offsets_walk(const uint8_t* p, int64_t nbytes,
                                       int64_t count, int32_t* starts,
                                       int64_t* lens) {
  int64_t pos = 0, total = 0;
  for (int64_t i = 0; i < count; ++i) {
    if (pos + 4 > nbytes) return -1;
    uint32_t l = (uint32_t)p[pos] | ((uint32_t)p[pos + 1] << 8) |
                 ((uint32_t)p[pos + 2] << 16) | ((uint32_t)p[pos + 3] << 24);
    pos += 4;
    if (pos + (int64_t)l > nbytes) return -1;
    starts[i] = (int32_t)pos;
    lens[i] = l;
    total += l;
    pos += l;
  }
  return total;
}

// Host decode of a parquet DELTA_BINARY_PACKED stream (header varints +
// per-block zigzag min_delta + bit-packed miniblocks). The format is a
// serial chain of varints, so like the walks above it runs on the CPU;
// the decoded ints are only per-page length vectors (DELTA_LENGTH_/
// DELTA_BYTE_ARRAY string pages), never bulk column data. Returns bytes
// consumed (so the caller can locate the payload that follows) or -1.
static int64_t pq_delta_walk(const uint8_t* p, int64_t nbytes, int64_t* out,
                             int64_t n) {
  int64_t pos = 0;
  auto varint = [&](uint64_t* v) -> bool {
    uint64_t r = 0;
    int shift = 0;
    while (pos < nbytes && shift < 64) {
      uint8_t b = p[pos++];
      r |= (uint64_t)(b & 0x7F) << shift;
      if (!(b & 0x80)) {
        *v = r;
        return true;
      }
      shift += 7;
    }
    return false;
  };
  auto zigzag = [&](int64_t* v) -> bool {
    uint64_t u;
    if (!varint(&u)) return false;
    *v = (int64_t)(u >> 1) ^ -(int64_t)(u & 1);
    return true;
  };
  uint64_t block_size, mb_per_block, total_count;
  int64_t first;
  if (!varint(&block_size) || !varint(&mb_per_block) ||
      !varint(&total_count) || !zigzag(&first))
    return -1;
  if (mb_per_block == 0 || block_size == 0 ||
      block_size % mb_per_block != 0)
    return -1;
  int64_t per_mb = (int64_t)(block_size / mb_per_block);
  if (per_mb % 8 != 0) return -1;
  int64_t want = (int64_t)total_count < n ? (int64_t)total_count : n;
  int64_t emitted = 0;
  int64_t cur = first;
  if (want > 0) out[emitted++] = cur;
  while (emitted < want) {
    int64_t min_delta;
    if (!zigzag(&min_delta)) return -1;
    if (pos + (int64_t)mb_per_block > nbytes) return -1;
    const uint8_t* bws = p + pos;
    pos += mb_per_block;
    for (uint64_t mb = 0; mb < mb_per_block; ++mb) {
      if (emitted >= want) break;  // trailing miniblocks are omitted
      int bw = bws[mb];
      if (bw > 64) return -1;
      int64_t mb_bytes = per_mb * bw / 8;
      if (pos + mb_bytes > nbytes) return -1;
      const uint8_t* src = p + pos;
      for (int64_t i = 0; i < per_mb && emitted < want; ++i) {
        uint64_t v = 0;
        if (bw > 0) {
          int64_t bit = i * bw;
          // miniblock is zero-padded to a full 8-byte-safe read window?
          // no: read byte-by-byte to stay in bounds
          for (int b = 0; b < bw; ++b) {
            int64_t bb = bit + b;
            if (src[bb >> 3] & (1 << (bb & 7))) v |= (uint64_t)1 << b;
          }
        }
        cur += min_delta + (int64_t)v;
        out[emitted++] = cur;
      }
      pos += mb_bytes;  // full (padded) miniblock is always present
    }
  }
  return pos;
}

// Host reconstruction of DELTA_BYTE_ARRAY strings: each value is
// prefix_len bytes of the PREVIOUS value + its suffix — a serial chain,
// so it runs on the CPU in one memcpy pass; the result uploads as a
// dense string column. Returns 0 or -1.
static int64_t delta_ba_concat(const int64_t* pre, const int64_t* suf,
                               const uint8_t* sufbytes, int64_t suf_nbytes,
                               int64_t n, uint8_t* out,
                               const int64_t* out_offs) {
  int64_t spos = 0;
  for (int64_t i = 0; i < n; ++i) {
    int64_t plen = pre[i], slen = suf[i];
    if (plen < 0 || slen < 0 || spos + slen > suf_nbytes) return -1;
    if (i == 0 ? plen != 0
               : plen > out_offs[i] - out_offs[i - 1])
      return -1;
    uint8_t* dst = out + out_offs[i];
    if (plen) memcpy(dst, out + out_offs[i - 1], (size_t)plen);
    if (slen) memcpy(dst + plen, sufbytes + spos, (size_t)slen);
    spos += slen;
  }
  return 0;
}

PYBIND11_MODULE(hipdf, m) {
  m.doc() = "hand-written CDNA4 (gfx950) columnar kernels for MI355X";

  m.def("build_arch", []() { return std::string("gfx950"); });
  m.def("device_count", []() {
    int n = 0;
    hipGetDeviceCount(&n);
    return n;
  });
  m.def("synchronize", []() {
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess)
      throw std::runtime_error(hipGetErrorString(e));
  });

  // ---- device memory pool ------------------------------------------------
  m.def("pool_init", &hipdf_pool_init);
  m.def("pool_active", []() { return hipdf_pool_active() != 0; });
  m.def("pool_used", &hipdf_pool_used);
  m.def("pool_reserved", &hipdf_pool_reserved);
  m.def("pool_high_watermark", &hipdf_pool_high_watermark);
  m.def("pool_overflow", &hipdf_pool_overflow);
  m.def("pool_selftest", &hipdf_pool_selftest);
  m.def("pool_set_spill_cb", [](py::object f) {
    if (!g_spill_cb) g_spill_cb = new py::object();
    *g_spill_cb = f;
    hipdf_pool_set_failure_cb(f.is_none() ? nullptr : &spill_cb_trampoline);
  });

  // ---- host memory and host-side stream walks ----------------------------
  m.def("host_register", [](int64_t ptr, int64_t nbytes) -> int {
    // pin an existing host range (the parquet file mmap) so H2D copies
    // from it are direct DMA instead of a staged bounce
    return (int)hipHostRegister((void*)ptr, (size_t)nbytes,
                                hipHostRegisterDefault);
  });
  m.def("host_unregister", [](int64_t ptr) {
    hipHostUnregister((void*)ptr);
  });
  // GIL released: from pageable memory (the parquet file mapping) this
  // returns only after the runtime has staged the whole source, and the
  // reader's prefetch threads and the kernel-launching thread must not
  // queue behind one another for that long
  m.def("memcpy_h2d", [](int64_t dst, int64_t src, int64_t nbytes,
                         int64_t stream) -> int {
    return (int)hipMemcpyAsync((void*)dst, (const void*)src,
                               (size_t)nbytes, hipMemcpyHostToDevice,
                               to_c<hipStream_t>(stream));
  }, py::call_guard<py::gil_scoped_release>());
  m.def("rle_walk_host",
        [](int64_t data, int64_t nbytes, int bw, int64_t n_values,
           int64_t src_base, int64_t out_base, int64_t runs,
           int64_t max_runs) -> int64_t {
          return rle_walk((const uint8_t*)data, nbytes, bw, n_values,
                          src_base, out_base, (int64_t*)runs, max_runs);
        },
        py::call_guard<py::gil_scoped_release>());
  m.def("pq_delta_walk_host",
        [](int64_t data, int64_t nbytes, int64_t out,
           int64_t n) -> int64_t {
          return pq_delta_walk((const uint8_t*)data, nbytes, (int64_t*)out,
                               n);
        },
        py::call_guard<py::gil_scoped_release>());
  m.def("delta_ba_concat_host",
        [](int64_t pre, int64_t suf, int64_t sufbytes, int64_t suf_nbytes,
           int64_t n, int64_t out, int64_t out_offs) -> int64_t {
          return delta_ba_concat((const int64_t*)pre, (const int64_t*)suf,
                                 (const uint8_t*)sufbytes, suf_nbytes, n,
                                 (uint8_t*)out, (const int64_t*)out_offs);
        },
        py::call_guard<py::gil_scoped_release>());
  m.def("byte_array_offsets_host",
        [](int64_t data, int64_t nbytes, int64_t count, int64_t starts,
           int64_t lens) -> int64_t {
          return byte_array_offsets_walk((const uint8_t*)data, nbytes, count,
                                         (int32_t*)starts, (int64_t*)lens);
        },
        py::call_guard<py::gil_scoped_release>());

  // ---- native in-order scan reader ---------------------------------------
  // handles and tickets are plain integers; every call that can block
  // (thread start, page walk, waiting for a group, draining) releases the GIL
  m.def("pq_plain_pieces",
        [](int64_t chunk, int64_t nbytes, int64_t num_values, int max_def,
           int phys_width, int64_t out, int64_t max_out) -> int64_t {
          return hipdf_pq_plain_pieces((const void*)chunk, nbytes, num_values,
                                       max_def, phys_width, (int64_t*)out,
                                       max_out);
        },
        py::call_guard<py::gil_scoped_release>());
  m.def("scan_open",
        [](int n_threads, int n_streams, int64_t piece_bytes) -> int64_t {
          return (int64_t)hipdf_scan_open(n_threads, n_streams, piece_bytes);
        },
        py::call_guard<py::gil_scoped_release>());
  m.def("scan_submit",
        [](int64_t reader, int64_t chunks, int64_t n_chunks, int n_groups,
           int64_t consumer) -> int64_t {
          return hipdf_scan_submit((HipdfScanReader*)reader,
                                   (const HipdfScanChunk*)chunks, n_chunks,
                                   n_groups, to_c<hipStream_t>(consumer));
        },
        py::call_guard<py::gil_scoped_release>());
  m.def("scan_wait_group",
        [](int64_t reader, int64_t ticket, int group,
           int64_t consumer) -> int {
          return hipdf_scan_wait_group((HipdfScanReader*)reader, ticket,
                                       group, to_c<hipStream_t>(consumer));
        },
        py::call_guard<py::gil_scoped_release>());
  m.def("scan_cancel",
        [](int64_t reader, int64_t ticket) {
          hipdf_scan_cancel((HipdfScanReader*)reader, ticket);
        },
        py::call_guard<py::gil_scoped_release>());
  m.def("scan_close",
        [](int64_t reader) { hipdf_scan_close((HipdfScanReader*)reader); },
        py::call_guard<py::gil_scoped_release>());

  // ---- elementwise -------------------------------------------------------
  BIND(binary_arith);
  BIND(binary_cmp);
  BIND(binary_bool);
  BIND(unary);
  BIND(cast);
  BIND(f64_to_i64_rint);
  BIND(decimal_rescale);
  BIND(if_else);
  BIND(mask_expand);

  // ---- selection ---------------------------------------------------------
  m.def("sel_num_blocks", &sel_num_blocks);
  BIND(expand_rows);
  BIND(mask_count);
  BIND(mask_scatter);
  BIND(gather_fixed);
  BIND(gather_codes);
  BIND(gather_table);
  BIND(gather_validity);
  BIND(gather_str_lens);
  BIND(gather_str_bytes);
  BIND(narrow_i64_i32);
  BIND(copy_valid_range);

  // ---- scan / reduce -----------------------------------------------------
  m.def("scan_num_blocks", &scan_num_blocks);
  m.def("scan_scratch_elems", &scan_scratch_elems);
  BIND(scan_block);
  BIND(scan_add_offsets);
  // every level of the scan in one call; the total lands in scratch[-1]
  BIND(exclusive_scan_i64);
  BIND(reduce);

  // ---- hashing -----------------------------------------------------------
  BIND(murmur3_col);
  BIND(murmur3_str);
  BIND(xxhash64_col);
  BIND(xxhash64_str);
  BIND(pmod_part);
  BIND(digest_hex);
  BIND(crc32_str);

  // ---- group-by ----------------------------------------------------------
  BIND(gb_build);
  BIND(gb_number);
  BIND(gb_rowgid);
  BIND(dense_gid);
  BIND(dense_null_slot);
  BIND(gb_acc_init);
  BIND(gb_agg);
  BIND(gb_agg_multi);
  BIND(gb_reduce_reps);
  BIND(mask_from_nonzero);
  BIND(gb_hll);
  BIND(gb_percentile);
  BIND(gb_collect_count);
  BIND(gb_collect_fill);

  // ---- hash join ---------------------------------------------------------
  m.def("join_probe_num_blocks", &join_probe_num_blocks);
  BIND(join_build);
  BIND(join_count);
  BIND(join_fill);
  BIND(join_check_unique);
  BIND(join_probe_unique);
  BIND(join_compact_unique);

  // ---- partition ---------------------------------------------------------
  m.def("part_num_blocks", &part_num_blocks);
  BIND(part_hist);
  BIND(part_scatter);

  // ---- sort --------------------------------------------------------------
  m.def("sort_num_blocks", &sort_num_blocks);
  m.def("sort_key_width", &hipdf_sort_key_width);
  BIND(make_sort_keys);
  BIND(make_sort_keys_str);
  BIND(make_sort_keys_i128);
  BIND(radix_count);
  BIND(radix_scatter);
  // keys: one tuple per sort key, most significant first:
  // (kind, htype, data, valid, offsets, desc, nulls_last, has_valid, nchunks)
  m.def("sort_order", [](const std::vector<py::tuple>& keys, int64_t n,
                         int64_t keys_a, int64_t keys_b, int64_t perm_a,
                         int64_t perm_b, int64_t counts, int64_t scanned,
                         int64_t scan_scratch, int64_t diff, int64_t out_perm,
                         int64_t stream) {
    std::vector<HipdfSortKey> ks;
    ks.reserve(keys.size());
    for (const py::tuple& t : keys) {
      if (t.size() != 9) throw std::runtime_error("hipdf: bad sort key");
      HipdfSortKey k;
      k.kind = t[0].cast<int32_t>();
      k.htype = t[1].cast<int32_t>();
      k.data = to_c<const void*>(t[2].cast<int64_t>());
      k.valid = to_c<const void*>(t[3].cast<int64_t>());
      k.offsets = to_c<const void*>(t[4].cast<int64_t>());
      k.desc = t[5].cast<bool>();
      k.nulls_last = t[6].cast<bool>();
      k.has_valid = t[7].cast<bool>();
      k.nchunks = t[8].cast<int32_t>();
      if (k.kind < SORT_KEY_FIXED || k.kind > SORT_KEY_DECIMAL128 ||
          (k.kind == SORT_KEY_STRING && k.nchunks < 1))
        throw std::runtime_error("hipdf: bad sort key");
      ks.push_back(k);
    }
    {
      py::gil_scoped_release nogil;
      hipdf_sort_order(ks.data(), (int)ks.size(), n, to_c<void*>(keys_a),
                       to_c<void*>(keys_b), to_c<void*>(perm_a),
                       to_c<void*>(perm_b), to_c<void*>(counts),
                       to_c<void*>(scanned), to_c<void*>(scan_scratch),
                       to_c<void*>(diff), to_c<void*>(out_perm),
                       to_c<hipStream_t>(stream));
    }
    check_async();
  });

  // ---- file-format decode ------------------------------------------------
  BIND(pq_delta_i64);
  BIND(orc_bool_rle);
  BIND(orc_rle_v2);
  BIND(str_plain_encode);
  BIND(str_plain_offsets);
  BIND(rle_hybrid_decode);
  BIND(rle_expand);
  BIND(rle_hybrid_batch);
  BIND(scatter_fixed);
  BIND(levels_to_mask);

  // ---- CSV / JSON --------------------------------------------------------
  BIND(json_field);
  BIND(byte_eq);
  BIND(csv_parse);
  BIND(json_path);
  BIND(json_path_multi);

  // ---- strings -----------------------------------------------------------
  BIND(str_cmp);
  BIND(str_cmp_scalar);
  BIND(str_find);
  BIND(str_like);
  BIND(str_pad);
  BIND(str_locate);
  BIND(str_length);
  BIND(str_case);
  BIND(i64_to_str);
  BIND(str_concat_ws);
  BIND(str_initcap);
  BIND(str_reverse);
  BIND(str_split_count);
  BIND(str_split_fill);
  BIND(str_trim_ranges);
  BIND(str_concat2);
  BIND(substr_ranges);
  BIND(substr_copy);

  // ---- window ------------------------------------------------------------
  BIND(win_minmax);
  BIND(range_bounds);
  BIND(change_flags);
  BIND(iota_i32);
  BIND(scan_block_f64);
  BIND(scan_add_offsets_f64);

  // ---- decimal128 --------------------------------------------------------
  BIND(dec_mul_div_wide);
  BIND(i128_rescale);
  BIND(dec64_mul_div);
  BIND(i128_arith);
  BIND(i128_cmp);
  BIND(i64_to_i128);
  BIND(i128_to_f64);
  BIND(gb_sum_i128_lds);
  BIND(gb_sum_i64_to_i128);
  BIND(gb_sum_i128);

  // ---- regex -------------------------------------------------------------
  BIND(regex_extract);
  BIND(regex_extract_all);
  BIND(regex_replace);
  BIND(regex_match);

  // ---- string <-> decimal casts, datetime --------------------------------
  BIND(str_to_dec);
  BIND(dec_to_str);
  BIND(tz_convert);
  BIND(date_format);
  BIND(ts_parse);

  // ---- lists -------------------------------------------------------------
  m.def("list_block_cap", &hipdf_list_block_cap);
  BIND(list_sort_wave);
  BIND(list_sort_block);
  BIND(list_distinct_flags);
  BIND(list_argminmax);
  BIND(list_member_flags);
  BIND(list_overlap);
  BIND(list_union_map);
  BIND(list_elem_rows);
  BIND(list_bool_reduce);
  BIND(list_find);
  BIND(list_slice_ranges);
  BIND(list_slice_map);
  BIND(list_interleave);
  BIND(list_interleave_map);
  BIND(list_concat_lens);
  BIND(list_concat_map);
  BIND(list_flatten);
  BIND(sequence_ranges);
  BIND(sequence_fill);
  BIND(array_join_sizes);
  BIND(array_join_rows);
  BIND(array_join_write);
}
