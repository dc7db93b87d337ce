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
//     returns, because then nothing orders the consumer stream behind them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "hipdf.h"
#include "pq_pieces.h"

namespace {

__global__ void k_widen_i32_i64(const int32_t* __restrict__ in,
                                int64_t* __restrict__ out, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) out[i] = (int64_t)in[i];
}

struct Piece {
  const uint8_t* src;
  uint8_t* dst;
  int64_t nbytes;  // source bytes
  int32_t widen;   // 1: int32 source values into int64 destination
  int32_t group;
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
};

}  // namespace

struct HipdfScanReader {
  int device = 0;
  int64_t piece_bytes = 0;
  std::vector<std::thread> threads;
  std::vector<hipStream_t> streams;  // one per worker slot (may repeat)
  std::vector<hipStream_t> owned_streams;
  std::vector<void*> scratch;  // per worker, piece_bytes each
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
      const Piece& p = s->pieces[idx];
      hipStream_t st = streams[(size_t)w];
      hipError_t e = hipSuccess;
      if (!s->stream_used[(size_t)w]) {
        // MEMORY RULE: no write before the consumer stream reached the submit
        e = hipStreamWaitEvent(st, s->start, 0);
        s->stream_used[(size_t)w] = 1;
      }
      if (e == hipSuccess) {
        if (!p.widen) {
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
        if (e != hipSuccess && !s->error) s->error = (int)e;
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
    ok = hipMalloc(&p, (size_t)piece_bytes) == hipSuccess;
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
