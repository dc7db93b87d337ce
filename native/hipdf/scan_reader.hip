// Native in-order scan reader: uploads the PLAIN fixed-width column chunks
// of several parquet files straight into caller-owned destination columns,
// file by file, so that file 0 is complete on the device while files 1..n
// are still on the wire.
//
// A submit is a table of column-chunk descriptors, each tagged with a group
// (the file's index). The chunks are walked (kernels/pq_pieces.h) and cut
// into pieces of at most piece_bytes; the worker threads claim the pieces
// strictly in group-major order, so every worker pulls the earliest
// unfinished file first. A piece is one pageable hipMemcpyAsync on the
// worker's stream: same-width values land in the destination column at the
// file's row offset, INT32 values of an int64-backed column land in the
// worker's scratch buffer and one widen kernel on the same stream writes
// them in place. The file mapping is never hipHostRegister'ed.
//
// A chunk that comes with a validity buffer may hold nulls (max_def 1). Its
// piece is a whole data page: the worker that claims it decodes the page's
// definition levels on the host (kernels/pq_levels.h) into a bitmask and a
// table of valid counts per tile of rows, checks that the page holds exactly
// that many dense values, and cuts the page into slices of whole tiles whose
// dense values fit piece_bytes. A slice is three copies into the worker's
// scratch (dense values, mask words, tile counts) and one k_place_nullable
// launch on the worker's stream: it writes the values to their rows, zero
// at null rows (widening INT32 to int64 where asked), and the validity bits
// at the chunk's bit offset in the destination mask.
//
// MEMORY RULE. The device pool (pool.hip) ignores streams: a freed block is
// reusable at once, ordered only by the consumer stream that the engine's
// kernels run on. Therefore
//   - every destination buffer of a submit is allocated by the caller BEFORE
//     the submit, and the submit records one event on the consumer stream;
//     every copy stream waits on that event before its first write, so no
//     copy lands in memory that earlier consumer-stream work still reads;
//   - a group is handed over by events recorded on each stream that carried
//     one of its pieces; wait_group makes the consumer stream wait on them
//     (hipStreamWaitEvent, no host synchronise), so whatever later reuses the
//     destination is ordered behind the copies;
//   - a submit that is dropped before all its groups were waited for is
//     drained with a host synchronise of the copy streams before cancel
//     returns, because then nothing orders the consumer stream behind them;
//   - the host memory a nullable piece decodes its levels into belongs to the
//     submit, is written once by the worker that claimed the piece, is not
//     reused within the submit, and is released in hipdf_scan_cancel after
//     that drain: the rule the caller's file mapping follows, which it keeps
//     alive until cancel returns. The destination validity buffers arrive
//     zeroed by work on the consumer stream before the submit's event.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "hipdf.h"
#include "pq_levels.h"
#include "pq_pieces.h"

namespace {

constexpr int kTile = pq_pieces::kTileRows;

__global__ void k_widen_i32_i64(const int32_t* __restrict__ in,
                                int64_t* __restrict__ out, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) out[i] = (int64_t)in[i];
}

// One thread per bit of the destination mask, starting at the 64-bit word
// that holds the slice's first row: a wave's ballot is one whole word of the
// destination, whatever bit offset the slice starts at. Row r of the slice
// is valid when bit r of `mask` is set; its value is src[rank], rank being
// the valid rows before it: the host's count for its tile (relative to the
// slice's first tile) plus the set bits of the tile's mask words before r.
// Words that lie wholly in the slice are plain stores; a first or last word
// shared with a neighbouring slice, page or file is merged with atomicOr
// (the mask arrives zeroed).
template <typename SrcT, typename DstT>
__global__ void k_place_nullable(const SrcT* __restrict__ src,
                                 const uint64_t* __restrict__ mask,
                                 const uint32_t* __restrict__ tiles,
                                 DstT* __restrict__ dst,
                                 uint32_t* __restrict__ valid, int64_t bit0,
                                 int64_t n) {
  const int64_t d = (bit0 & ~(int64_t)63) + (int64_t)blockIdx.x * blockDim.x +
                    threadIdx.x;
  const int64_t r = d - bit0;
  const bool in = r >= 0 && r < n;
  bool v = false;
  if (in) {
    const int64_t wi = r >> 6;
    const uint64_t word = mask[wi];
    v = (word >> (r & 63)) & 1;
    DstT out = (DstT)0;
    if (v) {
      const int64_t tile = r / kTile;
      uint32_t rank = tiles[tile] - tiles[0];
      for (int64_t w = tile * (kTile / 64); w < wi; ++w)
        rank += (uint32_t)__popcll(mask[w]);
      rank += (uint32_t)__popcll(word & (((uint64_t)1 << (r & 63)) - 1));
      out = (DstT)src[rank];
    }
    dst[r] = out;
  }
  const uint64_t bits = __ballot(v);
  const uint64_t rows = __ballot(in);
  if ((threadIdx.x & 63) == 0 && rows) {
    uint32_t* w32 = valid + (d >> 6) * 2;  // d is a multiple of 64 here
    const uint32_t lo = (uint32_t)bits, hi = (uint32_t)(bits >> 32);
    if (rows == ~(uint64_t)0) {
      w32[0] = lo;
      w32[1] = hi;
    } else {
      if (lo) atomicOr(&w32[0], lo);
      if (hi) atomicOr(&w32[1], hi);
    }
  }
}

struct Piece {
  const uint8_t* src;
  uint8_t* dst;
  int64_t nbytes;  // source bytes
  int32_t widen;   // 1: int32 source values into int64 destination
  int32_t group;
  // a page that may hold nulls (valid != nullptr): src / nbytes are its
  // dense values, dst its first row
  uint32_t* valid = nullptr;     // destination mask
  int64_t bit0 = 0;              // bit of the page's first row in it
  int64_t rows = 0;
  const uint8_t* levels = nullptr;
  int64_t level_bytes = 0;
  int32_t phys_width = 0;
  uint8_t* host = nullptr;  // decoded mask + tile counts, owned by the submit
};

struct Group {
  int64_t total = 0;     // pieces of the group
  int64_t enqueued = 0;  // pieces whose copy is on a stream
  int open_workers = 0;  // workers that touched it and owe an event
  std::vector<hipEvent_t> events;
  bool waited = false;
};

struct Submit {
  int64_t ticket = 0;
  std::vector<Piece> pieces;  // group-major
  size_t next = 0;            // next piece to claim
  std::vector<Group> groups;
  hipEvent_t start = nullptr;  // recorded on the consumer stream
  int in_flight = 0;           // workers between claim and enqueue
  bool cancelled = false;
  int error = 0;
  std::vector<char> stream_used;  // per worker

  bool group_ready(int g) const {
    const Group& gr = groups[(size_t)g];
    return gr.enqueued == gr.total && gr.open_workers == 0;
  }
  bool exhausted() const { return cancelled || next >= pieces.size(); }
  void release_host() {
    for (Piece& p : pieces) {
      delete[] p.host;
      p.host = nullptr;
    }
  }
  ~Submit() { release_host(); }
};

}  // namespace

struct HipdfScanReader {
  int device = 0;
  int64_t piece_bytes = 0;
  std::vector<std::thread> threads;
  std::vector<hipStream_t> streams;  // one per worker slot (may repeat)
  std::vector<hipStream_t> owned_streams;
  // per worker: value_cap bytes of values, then (nullable slices) mask_cap
  // bytes of mask words and the tile counts
  std::vector<void*> scratch;
  int64_t value_cap = 0;
  int64_t mask_cap = 0;
  int64_t tiles_cap = 0;
  std::mutex mu;
  std::condition_variable work_cv;  // workers: new work or stop
  std::condition_variable done_cv;  // callers: a group or a drain finished
  std::deque<std::shared_ptr<Submit>> queue;  // submits with pieces left
  std::vector<std::shared_ptr<Submit>> live;  // until cancel releases them
  int64_t next_ticket = 1;
  bool stop = false;

  std::shared_ptr<Submit> find(int64_t ticket) {
    for (auto& s : live)
      if (s->ticket == ticket) return s;
    return nullptr;
  }

  // a worker leaves group g of submit s: its stream's event joins the group
  void leave_group(Submit& s, int g, int w) {
    hipEvent_t ev = nullptr;
    hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(ev, streams[(size_t)w]);
    std::lock_guard<std::mutex> lk(mu);
    if (e != hipSuccess && !s.error) s.error = (int)e;
    if (ev) s.groups[(size_t)g].events.push_back(ev);
    --s.groups[(size_t)g].open_workers;
    done_cv.notify_all();
  }

  // rows per slice of a nullable page: whole tiles whose values fit
  // piece_bytes, one tile at the least
  int64_t slice_rows(int width) const {
    return std::max<int64_t>(kTile, piece_bytes / width / kTile * kTile);
  }

  // A nullable page: decode its levels, check them against its dense values,
  // and enqueue its slices on stream st. 0, a hipError_t, or a negative
  // pq_pieces code.
  int nullable_piece(Piece& p, int w, hipStream_t st) {
    using namespace pq_pieces;
    const int64_t n = p.rows;
    if (n == 0) return p.nbytes == 0 ? 0 : (int)kErrCount;
    const int64_t mb = mask_bytes(n), te = tile_entries(n);
    p.host = new (std::nothrow) uint8_t[(size_t)(mb + te * 4)];
    if (!p.host) return (int)hipErrorOutOfMemory;
    uint32_t* tiles = (uint32_t*)(p.host + mb);  // mb is a multiple of 256
    int64_t nvalid = decode_levels(p.levels, p.level_bytes, n, p.host, tiles);
    if (nvalid < 0) return (int)nvalid;
    if (nvalid * p.phys_width != p.nbytes) return (int)kErrCount;
    uint8_t* vals = (uint8_t*)scratch[(size_t)w];
    uint8_t* dmask = vals + value_cap;
    uint8_t* dtiles = dmask + mask_cap;
    const int dst_width = p.widen ? 8 : p.phys_width;
    const int64_t step = slice_rows(p.phys_width);
    for (int64_t r0 = 0; r0 < n; r0 += step) {
      const int64_t rows = std::min(step, n - r0);
      const int64_t t0 = r0 / kTile, t1 = t0 + (rows + kTile - 1) / kTile;
      const int64_t v0 = tiles[t0], v1 = tiles[t1];
      hipError_t e = hipSuccess;
      if (v1 > v0)
        e = hipMemcpyAsync(vals, p.src + v0 * p.phys_width,
                           (size_t)((v1 - v0) * p.phys_width),
                           hipMemcpyHostToDevice, st);
      if (e == hipSuccess)
        e = hipMemcpyAsync(dmask, p.host + t0 * (kTile / 8),
                           (size_t)((rows + 63) / 64 * 8),
                           hipMemcpyHostToDevice, st);
      if (e == hipSuccess)
        e = hipMemcpyAsync(dtiles, tiles + t0, (size_t)((t1 - t0 + 1) * 4),
                           hipMemcpyHostToDevice, st);
      if (e != hipSuccess) return (int)e;
      const int64_t bit0 = p.bit0 + r0;
      const int64_t span = (bit0 & 63) + rows;
      dim3 grid((unsigned)((span + 255) / 256)), block(256);
      uint8_t* dst = p.dst + r0 * dst_width;
      if (p.widen)
        hipLaunchKernelGGL((k_place_nullable<int32_t, int64_t>), grid, block,
                           0, st, (const int32_t*)vals,
                           (const uint64_t*)dmask, (const uint32_t*)dtiles,
                           (int64_t*)dst, p.valid, bit0, rows);
      else if (p.phys_width == 4)
        hipLaunchKernelGGL((k_place_nullable<uint32_t, uint32_t>), grid,
                           block, 0, st, (const uint32_t*)vals,
                           (const uint64_t*)dmask, (const uint32_t*)dtiles,
                           (uint32_t*)dst, p.valid, bit0, rows);
      else
        hipLaunchKernelGGL((k_place_nullable<uint64_t, uint64_t>), grid,
                           block, 0, st, (const uint64_t*)vals,
                           (const uint64_t*)dmask, (const uint32_t*)dtiles,
                           (uint64_t*)dst, p.valid, bit0, rows);
      e = hipGetLastError();
      if (e != hipSuccess) return (int)e;
    }
    return 0;
  }

  void worker(int w) {
    (void)hipSetDevice(device);
    std::shared_ptr<Submit> cur;  // submit of the group this worker is in
    int cur_group = -1;
    for (;;) {
      std::shared_ptr<Submit> s;
      size_t idx = 0;
      {
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
          while (!queue.empty() && queue.front()->exhausted())
            queue.pop_front();
          if (stop || !queue.empty()) break;
          if (cur) break;  // owe an event before sleeping
          work_cv.wait(lk);
        }
        if (!stop && !queue.empty()) {
          s = queue.front();
          idx = s->next++;
          int g = s->pieces[idx].group;
          if (s != cur || g != cur_group) ++s->groups[(size_t)g].open_workers;
          ++s->in_flight;
        }
      }
      if (cur && (!s || s != cur || s->pieces[idx].group != cur_group)) {
        leave_group(*cur, cur_group, w);
        cur.reset();
        cur_group = -1;
      }
      if (!s) {
        std::lock_guard<std::mutex> lk(mu);
        if (stop) return;
        continue;
      }
      Piece& p = s->pieces[idx];  // claimed: this worker's alone
      hipStream_t st = streams[(size_t)w];
      int e = hipSuccess;
      if (!s->stream_used[(size_t)w]) {
        // MEMORY RULE: no write before the consumer stream reached the submit
        e = hipStreamWaitEvent(st, s->start, 0);
        s->stream_used[(size_t)w] = 1;
      }
      if (e == hipSuccess) {
        if (p.valid) {
          e = nullable_piece(p, w, st);
        } else if (!p.widen) {
          e = hipMemcpyAsync(p.dst, p.src, (size_t)p.nbytes,
                             hipMemcpyHostToDevice, st);
        } else {
          e = hipMemcpyAsync(scratch[(size_t)w], p.src, (size_t)p.nbytes,
                             hipMemcpyHostToDevice, st);
          if (e == hipSuccess) {
            int64_t n = p.nbytes / 4;
            int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
            hipLaunchKernelGGL(k_widen_i32_i64, dim3((unsigned)blocks),
                               dim3(256), 0, st,
                               (const int32_t*)scratch[(size_t)w],
                               (int64_t*)p.dst, n);
            e = hipGetLastError();
          }
        }
      }
      cur = s;
      cur_group = p.group;
      {
        std::lock_guard<std::mutex> lk(mu);
        if (e != hipSuccess && !s->error) s->error = e;
        ++s->groups[(size_t)p.group].enqueued;
        --s->in_flight;
        done_cv.notify_all();
      }
    }
  }
};

extern "C" {

int64_t hipdf_pq_plain_pieces(const void* chunk, int64_t nbytes,
                              int64_t num_values, int max_def, int phys_width,
                              int64_t* out, int64_t max_out) {
  return pq_pieces::walk((const uint8_t*)chunk, nbytes, num_values, max_def,
                         phys_width, out, max_out);
}

HipdfScanReader* hipdf_scan_open(int n_threads, int n_streams,
                                 int64_t piece_bytes) {
  n_threads = std::max(1, std::min(n_threads, 8));
  n_streams = std::max(1, std::min(n_streams, n_threads));
  piece_bytes = std::max<int64_t>(piece_bytes, 64) / 8 * 8;
  auto* r = new HipdfScanReader();
  r->piece_bytes = piece_bytes;
  // a nullable slice holds at least one tile of 8-byte values; its mask and
  // counts are sized for the most rows a slice can have, those of 4-byte
  // values
  r->value_cap = std::max<int64_t>(piece_bytes, kTile * 8);
  r->mask_cap = r->slice_rows(4) / 8;
  r->tiles_cap = (r->slice_rows(4) / kTile + 1) * 4;
  if (hipGetDevice(&r->device) != hipSuccess) {
    delete r;
    return nullptr;
  }
  bool ok = true;
  for (int i = 0; i < n_streams && ok; ++i) {
    hipStream_t st = nullptr;
    ok = hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess;
    if (ok) r->owned_streams.push_back(st);
  }
  for (int w = 0; w < n_threads && ok; ++w) {
    void* p = nullptr;
    ok = hipMalloc(&p, (size_t)(r->value_cap + r->mask_cap +
                                r->tiles_cap)) == hipSuccess;
    if (ok) r->scratch.push_back(p);
  }
  if (!ok) {
    for (void* p : r->scratch) (void)hipFree(p);
    for (hipStream_t st : r->owned_streams) (void)hipStreamDestroy(st);
    delete r;
    return nullptr;
  }
  // two workers never share a stream's scratch: the scratch is per worker,
  // and one worker's copy -> widen -> copy sequence is in stream order
  for (int w = 0; w < n_threads; ++w)
    r->streams.push_back(r->owned_streams[(size_t)(w % n_streams)]);
  for (int w = 0; w < n_threads; ++w)
    r->threads.emplace_back([r, w] { r->worker(w); });
  return r;
}

int64_t hipdf_scan_submit(HipdfScanReader* r, const HipdfScanChunk* chunks,
                          int64_t n_chunks, int n_groups,
                          hipStream_t consumer) {
  if (!r || n_chunks < 0 || n_groups < 0) return -100;
  auto s = std::make_shared<Submit>();
  s->groups.resize((size_t)n_groups);
  s->stream_used.assign(r->threads.size(), 0);
  std::vector<int64_t> pages;
  for (int64_t i = 0; i < n_chunks; ++i) {
    const HipdfScanChunk& c = chunks[i];
    if (c.group < 0 || c.group >= n_groups) return -100;
    bool widen = c.phys_width == 4 && c.dst_width == 8;
    if (!widen && c.dst_width != c.phys_width) return pq_pieces::kErrWidth;
    if (pages.empty()) pages.resize(3 * 256);
    int64_t np;
    if (c.valid) {
      // may hold nulls: one piece per data page, decoded by its worker
      if (c.max_def != 1 || c.valid_bit0 < 0) return -100;
      const int ls = pq_pieces::kLevelStride;
      for (;;) {
        np = pq_pieces::walk_levels((const uint8_t*)c.src, c.nbytes,
                                    c.num_values, c.max_def, c.phys_width,
                                    pages.data(), (int64_t)pages.size() / ls);
        if (np != pq_pieces::kErrCapacity || pages.size() >= (3u << 22))
          break;
        pages.resize(pages.size() * 4);
      }
      if (np < 0) return np;
      int64_t row = 0;
      for (int64_t k = 0; k < np; ++k) {
        const int64_t* pg = &pages[(size_t)(ls * k)];
        Piece p;
        p.src = (const uint8_t*)c.src + pg[0];
        p.dst = (uint8_t*)c.dst + row * (int64_t)c.dst_width;
        p.nbytes = pg[1];
        p.widen = widen ? 1 : 0;
        p.group = c.group;
        p.valid = (uint32_t*)c.valid;
        p.bit0 = c.valid_bit0 + row;
        p.rows = pg[2];
        p.levels = (const uint8_t*)c.src + pg[3];
        p.level_bytes = pg[4];
        p.phys_width = c.phys_width;
        s->pieces.push_back(p);
        row += pg[2];
      }
      continue;
    }
    for (;;) {
      np = pq_pieces::walk((const uint8_t*)c.src, c.nbytes, c.num_values,
                           c.max_def, c.phys_width, pages.data(),
                           (int64_t)pages.size() / 3);
      if (np != pq_pieces::kErrCapacity || pages.size() >= (3u << 22)) break;
      pages.resize(pages.size() * 4);
    }
    if (np < 0) return np;
    int64_t row = 0;
    for (int64_t k = 0; k < np; ++k) {
      int64_t off = pages[(size_t)(3 * k)], nb = pages[(size_t)(3 * k + 1)];
      for (int64_t done = 0; done < nb; done += r->piece_bytes) {
        int64_t take = std::min(r->piece_bytes, nb - done);
        Piece p;
        p.src = (const uint8_t*)c.src + off + done;
        p.dst = (uint8_t*)c.dst +
                (row + done / c.phys_width) * (int64_t)c.dst_width;
        p.nbytes = take;
        p.widen = widen ? 1 : 0;
        p.group = c.group;
        s->pieces.push_back(p);
      }
      row += pages[(size_t)(3 * k + 2)];
    }
  }
  std::stable_sort(s->pieces.begin(), s->pieces.end(),
                   [](const Piece& a, const Piece& b) {
                     return a.group < b.group;
                   });
  for (const Piece& p : s->pieces) ++s->groups[(size_t)p.group].total;
  if (hipEventCreateWithFlags(&s->start, hipEventDisableTiming) != hipSuccess)
    return -101;
  if (hipEventRecord(s->start, consumer) != hipSuccess) {
    (void)hipEventDestroy(s->start);
    return -101;
  }
  std::lock_guard<std::mutex> lk(r->mu);
  s->ticket = r->next_ticket++;
  r->live.push_back(s);
  if (!s->pieces.empty()) r->queue.push_back(s);
  r->work_cv.notify_all();
  return s->ticket;
}

int hipdf_scan_wait_group(HipdfScanReader* r, int64_t ticket, int group,
                          hipStream_t consumer) {
  if (!r) return -100;
  std::unique_lock<std::mutex> lk(r->mu);
  std::shared_ptr<Submit> s = r->find(ticket);
  if (!s || group < 0 || group >= (int)s->groups.size()) return -100;
  r->done_cv.wait(lk, [&] {
    return s->group_ready(group) || s->cancelled || s->error || r->stop;
  });
  if (s->error) return -102;
  if (!s->group_ready(group)) return -103;  // cancelled or closing
  Group& g = s->groups[(size_t)group];
  for (hipEvent_t ev : g.events)
    if (hipStreamWaitEvent(consumer, ev, 0) != hipSuccess) return -102;
  g.waited = true;
  return 0;
}

void hipdf_scan_cancel(HipdfScanReader* r, int64_t ticket) {
  if (!r) return;
  std::shared_ptr<Submit> s;
  bool drain = false;
  {
    std::unique_lock<std::mutex> lk(r->mu);
    s = r->find(ticket);
    if (!s) return;
    s->cancelled = true;  // no further piece is claimed
    r->work_cv.notify_all();
    r->done_cv.notify_all();
    // what is claimed gets enqueued, and every worker hands in its event
    r->done_cv.wait(lk, [&] {
      if (s->in_flight) return false;
      for (const Group& g : s->groups)
        if (g.open_workers) return false;
      return true;
    });
    for (const Group& g : s->groups)
      if (!g.waited && g.enqueued) drain = true;
    r->live.erase(std::find(r->live.begin(), r->live.end(), s));
  }
  if (drain)  // MEMORY RULE: nothing else orders the consumer behind these
    for (size_t w = 0; w < s->stream_used.size(); ++w)
      if (s->stream_used[w]) (void)hipStreamSynchronize(r->streams[w]);
  for (Group& g : s->groups)
    for (hipEvent_t ev : g.events) (void)hipEventDestroy(ev);
  (void)hipEventDestroy(s->start);
  s->release_host();  // MEMORY RULE: no worker is inside the submit any more
}

void hipdf_scan_close(HipdfScanReader* r) {
  if (!r) return;
  std::vector<int64_t> tickets;
  {
    std::lock_guard<std::mutex> lk(r->mu);
    for (auto& s : r->live) tickets.push_back(s->ticket);
  }
  for (int64_t t : tickets) hipdf_scan_cancel(r, t);
  {
    std::lock_guard<std::mutex> lk(r->mu);
    r->stop = true;
    r->work_cv.notify_all();
    r->done_cv.notify_all();
  }
  for (std::thread& t : r->threads) t.join();
  for (hipStream_t st : r->owned_streams) {
    (void)hipStreamSynchronize(st);
    (void)hipStreamDestroy(st);
  }
  for (void* p : r->scratch) (void)hipFree(p);
  delete r;
}

}  // extern "C"
