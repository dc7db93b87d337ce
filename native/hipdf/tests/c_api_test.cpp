// Non-python consumer of the hipdf C ABI: links
// against libhipdf.so and runs filter -> gather -> hash group-by, then a
// two-key sort, on device, verifying results on the host. Build:
//   hipcc -I native/hipdf/include c_api_test.cpp -L. -lhipdf -o c_api_test
#include <hipdf.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(x)                                                        \
  do {                                                                  \
    if (!(x)) {                                                         \
      fprintf(stderr, "FAILED at %s:%d: %s\n", __FILE__, __LINE__, #x); \
      return 1;                                                         \
    }                                                                   \
  } while (0)

#define HIP_OK(x) CHECK((x) == hipSuccess)

template <typename T>
T* dev(const std::vector<T>& h) {
  void* p;
  if (hipMalloc(&p, h.size() * sizeof(T) + 8) != hipSuccess) return nullptr;
  hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
  return (T*)p;
}

int main() {
  const int64_t N = 100000;
  std::vector<int64_t> vals(N);
  std::vector<int32_t> keys(N);
  std::vector<uint8_t> mask(N);
  for (int64_t i = 0; i < N; ++i) {
    vals[i] = i % 1000;
    keys[i] = (int32_t)(i % 37);
    mask[i] = (i % 3) != 0;  // keep 2/3 of rows
  }
  int64_t* d_vals = dev(vals);
  int32_t* d_keys = dev(keys);
  uint8_t* d_mask = dev(mask);
  CHECK(d_vals && d_keys && d_mask);
  hipStream_t s = 0;

  // ---- filter: mask -> selected indices --------------------------------
  int64_t nb = sel_num_blocks(N);
  std::vector<int64_t> h_counts(nb);
  int64_t* d_counts = dev(h_counts);
  hipdf_mask_count(d_mask, nullptr, d_counts, N, s);
  HIP_OK(hipMemcpy(h_counts.data(), d_counts, nb * 8,
                   hipMemcpyDeviceToHost));
  int64_t n_sel = 0;
  std::vector<int64_t> h_offs(nb);
  for (int64_t b = 0; b < nb; ++b) {
    h_offs[b] = n_sel;
    n_sel += h_counts[b];
  }
  int64_t exp_sel = 0;
  for (int64_t i = 0; i < N; ++i) exp_sel += mask[i] ? 1 : 0;
  CHECK(n_sel == exp_sel);
  int64_t* d_offs = dev(h_offs);
  void* d_idx;
  HIP_OK(hipMalloc(&d_idx, n_sel * 4));
  hipdf_mask_scatter(d_mask, nullptr, d_offs, d_idx, N, s);

  // ---- gather the selected rows ---------------------------------------
  void* d_gvals;
  void* d_gkeys;
  HIP_OK(hipMalloc(&d_gvals, n_sel * 8));
  HIP_OK(hipMalloc(&d_gkeys, n_sel * 4));
  hipdf_gather_fixed(8, d_vals, d_idx, d_gvals, n_sel, s);
  hipdf_gather_fixed(4, d_keys, d_idx, d_gkeys, n_sel, s);

  // ---- elementwise: doubled = gvals + gvals ----------------------------
  void* d_doubled;
  HIP_OK(hipMalloc(&d_doubled, n_sel * 8));
  hipdf_binary_arith(/*add*/ 0, HIPDF_I64, d_gvals, d_gvals, 0.0, 0, 0,
                     nullptr, nullptr, d_doubled, nullptr, n_sel, s);

  // ---- hash group-by: sum(doubled) by key ------------------------------
  std::vector<int32_t> seeds(n_sel, 42);
  int32_t* d_seeds = dev(seeds);
  hipdf_murmur3_col(/*int kind*/ 0, HIPDF_I32, d_gkeys, nullptr, nullptr,
                    d_seeds, n_sel, s);
  int64_t cap = 1;
  while (cap < 2 * n_sel) cap <<= 1;
  std::vector<int32_t> slot_init(cap, -1);
  int32_t* d_slot_row = dev(slot_init);
  void *d_row_slot, *d_claimed, *d_ngroups, *d_slot_gid, *d_leaders;
  HIP_OK(hipMalloc(&d_row_slot, n_sel * 4));
  HIP_OK(hipMalloc(&d_claimed, n_sel * 4));
  HIP_OK(hipMalloc(&d_ngroups, 4));
  HIP_OK(hipMemset(d_ngroups, 0, 4));
  HIP_OK(hipMalloc(&d_slot_gid, cap * 4));
  HIP_OK(hipMalloc(&d_leaders, n_sel * 4));
  HipdfKeyCol kc = {HIPDF_I32, 0, d_gkeys, nullptr, nullptr};
  HipdfKeyCol* d_kc;
  HIP_OK(hipMalloc((void**)&d_kc, sizeof(kc)));
  HIP_OK(hipMemcpy(d_kc, &kc, sizeof(kc), hipMemcpyHostToDevice));
  hipdf_gb_build(d_seeds, d_kc, 1, nullptr, d_slot_row, d_row_slot,
                 d_claimed, d_ngroups, cap, n_sel, s);
  int32_t ngroups = 0;
  HIP_OK(hipMemcpy(&ngroups, d_ngroups, 4, hipMemcpyDeviceToHost));
  CHECK(ngroups == 37);
  hipdf_gb_number(d_claimed, d_slot_row, d_slot_gid, d_ngroups, d_leaders,
                  n_sel, s);
  void* d_rowgid;
  HIP_OK(hipMalloc(&d_rowgid, n_sel * 4));
  hipdf_gb_rowgid(d_row_slot, d_slot_gid, d_rowgid, n_sel, s);
  void *d_acc, *d_cnt;
  HIP_OK(hipMalloc(&d_acc, ngroups * 8));
  HIP_OK(hipMalloc(&d_cnt, ngroups * 8));
  HIP_OK(hipMemset(d_cnt, 0, ngroups * 8));
  hipdf_gb_acc_init(/*sum*/ 0, d_acc, 0, ngroups, s);
  hipdf_gb_agg(/*sum*/ 0, HIPDF_I64, d_doubled, nullptr, d_rowgid, d_acc,
               d_cnt, 0, ngroups, n_sel, s);
  HIP_OK(hipDeviceSynchronize());

  // ---- verify against a host reference ---------------------------------
  std::vector<int32_t> h_leaders(ngroups);
  HIP_OK(hipMemcpy(h_leaders.data(), d_leaders, ngroups * 4,
                   hipMemcpyDeviceToHost));
  std::vector<int64_t> h_acc(ngroups);
  HIP_OK(hipMemcpy(h_acc.data(), d_acc, ngroups * 8,
                   hipMemcpyDeviceToHost));
  std::vector<int32_t> h_gkeys(n_sel);
  HIP_OK(hipMemcpy(h_gkeys.data(), d_gkeys, n_sel * 4,
                   hipMemcpyDeviceToHost));
  // host reference sums
  std::vector<int64_t> ref(37, 0);
  for (int64_t i = 0; i < N; ++i)
    if (mask[i]) ref[keys[i]] += 2 * vals[i];
  for (int32_t g = 0; g < ngroups; ++g) {
    int32_t leader_row = h_leaders[g];
    int32_t key = h_gkeys[leader_row];
    CHECK(key >= 0 && key < 37);
    if (h_acc[g] != ref[key]) {
      fprintf(stderr, "group key %d: got %lld want %lld\n", key,
              (long long)h_acc[g], (long long)ref[key]);
      return 1;
    }
  }

  // ---- multi-key sort through HipdfSortKey -----------------------------
  // key 0: int32, 7 distinct values, ascending; key 1: int64 descending,
  // row 0 null, NULLS LAST. Scratch sized as gpu_backend.py sizes it.
  const int64_t NS = 1000;
  std::vector<int32_t> sk0(NS);
  std::vector<int64_t> sk1(NS);
  std::vector<uint64_t> sv1((NS + 63) / 64, ~0ull);
  for (int64_t i = 0; i < NS; ++i) {
    sk0[i] = (int32_t)((i * 5 + 3) % 7);
    sk1[i] = (i * 7919) % 101 - 50;  // repeats, so ties test stability
  }
  sv1[0] &= ~1ull;
  int32_t* d_sk0 = dev(sk0);
  int64_t* d_sk1 = dev(sk1);
  uint64_t* d_sv1 = dev(sv1);
  CHECK(d_sk0 && d_sk1 && d_sv1);
  HipdfSortKey sort_keys[2] = {
      {SORT_KEY_FIXED, HIPDF_I32, d_sk0, nullptr, nullptr, 0, 0, 0, 0},
      {SORT_KEY_FIXED, HIPDF_I64, d_sk1, d_sv1, nullptr, 1, 1, 1, 0},
  };
  int64_t ncounts = 256 * sort_num_blocks(NS);
  int64_t nscan = scan_scratch_elems(ncounts);
  void *d_ka, *d_kb, *d_pa, *d_pb, *d_cnts, *d_scanned, *d_sscratch, *d_diff,
      *d_perm;
  HIP_OK(hipMalloc(&d_ka, NS * 8));
  HIP_OK(hipMalloc(&d_kb, NS * 8));
  HIP_OK(hipMalloc(&d_pa, NS * 4));
  HIP_OK(hipMalloc(&d_pb, NS * 4));
  HIP_OK(hipMalloc(&d_cnts, ncounts * 8));
  HIP_OK(hipMalloc(&d_scanned, ncounts * 8));
  HIP_OK(hipMalloc(&d_sscratch, nscan * 8));
  HIP_OK(hipMalloc(&d_diff, 8));
  HIP_OK(hipMalloc(&d_perm, NS * 4));
  hipdf_sort_order(sort_keys, 2, NS, d_ka, d_kb, d_pa, d_pb, d_cnts,
                   d_scanned, d_sscratch, d_diff, d_perm, s);
  HIP_OK(hipDeviceSynchronize());
  std::vector<int32_t> h_perm(NS), ref_perm(NS);
  HIP_OK(hipMemcpy(h_perm.data(), d_perm, NS * 4, hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < NS; ++i) ref_perm[i] = (int32_t)i;
  std::stable_sort(ref_perm.begin(), ref_perm.end(),
                   [&](int32_t a, int32_t b) {
                     if (sk0[a] != sk0[b]) return sk0[a] < sk0[b];
                     bool null_a = a == 0, null_b = b == 0;  // row 0
                     if (null_a != null_b) return null_b;    // nulls last
                     if (null_a) return false;
                     return sk1[a] > sk1[b];  // descending
                   });
  for (int64_t i = 0; i < NS; ++i) {
    if (h_perm[i] != ref_perm[i]) {
      fprintf(stderr, "sort perm[%lld]: got %d want %d\n", (long long)i,
              h_perm[i], ref_perm[i]);
      return 1;
    }
  }

  printf("C_API_OK filter=%lld/%lld groups=%d\n", (long long)n_sel,
         (long long)N, ngroups);
  return 0;
}
