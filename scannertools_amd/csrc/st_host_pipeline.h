// The host pipeline of the batch decoders (st_jpeg.hip's host path, st_png.hip): streams are filled into two slots on a pool
// of threads while the calling thread issues the sub-batches in order.  DESIGN.md 4.12.
//
// Only the C++17 standard library: no HIP header, so scripts/host_pipeline_check.cpp drives it on a CPU under the sanitizers.
#ifndef ST_HOST_PIPELINE_H_
#define ST_HOST_PIPELINE_H_

#include <algorithm>
#include <atomic>
#include <climits>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

// Threads for a call of n streams: min(16, the machine's), or what the environment variable `env` says (read at each call),
// within 1 .. min(64, n).
inline int st_pipe_threads(const char* env, int n) {
  int t = (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
  if (const char* e = getenv(env)) t = atoi(e);
  return std::max(1, std::min(std::min(t, 64), n));
}

// The plan of a call is a vector of these (or of structs derived from it), consecutive and in stream order: sub-batch k is
// filled into slot k & 1.
struct StPipeSubBatch { int first, count; };

// status 0: every sub-batch was issued.  stream >= 0: the fill of that stream failed with this status and message; stream -1:
// issue or release returned the status (and has said why itself).
struct StPipeResult {
  int status = 0, stream = -1;
  char message[160] = {0};
};

// T worker threads take the streams in order and call fill(i, k, slot, msg, msg_len) -> status for stream i of sub-batch k,
// once sub-batch k is allowed: the first two are at the start.  The calling thread calls issue(k, slot) -> status for each
// sub-batch in order once all its fills are done, and, when there is a sub-batch k + 2, release(slot) -> status, after which
// that one is allowed: a slot is refilled only when its reader says it is done with it.  A failing fill ends the call before
// the next issue, fills that have not begun are then skipped, and of the failures recorded the lowest stream is reported; so
// does an error from issue or release.  Every thread is joined before this returns.
template <class SB, class Fill, class Issue, class Release>
StPipeResult st_pipe_run(const std::vector<SB>& plan, int T, Fill&& fill, Issue&& issue, Release&& release) {
  const int nsb = (int)plan.size();
  const int n = nsb ? plan.back().first + plan.back().count : 0;
  std::vector<int> sb_of((size_t)n);
  struct Shared {
    std::mutex mu;
    std::condition_variable cv;
    int allowed = 2;
    std::vector<int> remaining;
    bool failed = false;
    StPipeResult fail;
  } sh;
  sh.remaining.resize((size_t)nsb);
  for (int k = 0; k < nsb; ++k) {
    sh.remaining[k] = plan[k].count;
    for (int i = plan[k].first; i < plan[k].first + plan[k].count; ++i) sb_of[i] = k;
  }
  std::atomic<int> next{0};
  auto work = [&]() {
    for (;;) {
      const int i = next.fetch_add(1);
      if (i >= n) return;
      const int k = sb_of[i];
      bool skip;
      {
        std::unique_lock<std::mutex> lk(sh.mu);
        sh.cv.wait(lk, [&] { return sh.allowed > k; });
        skip = sh.failed;
      }
      StPipeResult r;
      if (!skip) r.status = fill(i, k, k & 1, r.message, sizeof r.message);
      std::lock_guard<std::mutex> lk(sh.mu);
      if (r.status != 0 && (!sh.failed || i < sh.fail.stream)) {
        sh.failed = true;
        sh.fail = r;
        sh.fail.stream = i;
      }
      --sh.remaining[k];
      sh.cv.notify_all();
    }
  };
  std::vector<std::thread> pool;
  pool.reserve((size_t)T);
  for (int t = 0; t < T; ++t) pool.emplace_back(work);

  StPipeResult res;
  for (int k = 0; k < nsb && res.status == 0; ++k) {
    {
      std::unique_lock<std::mutex> lk(sh.mu);
      sh.cv.wait(lk, [&] { return sh.remaining[k] == 0; });
      if (sh.failed) { res = sh.fail; break; }
    }
    res.status = issue(k, k & 1);
    if (res.status == 0 && k + 2 < nsb && (res.status = release(k & 1)) == 0) {
      std::lock_guard<std::mutex> lk(sh.mu);
      sh.allowed = k + 3;
      sh.cv.notify_all();
    }
  }
  {
    // on an error the workers run out of streams without filling them
    std::lock_guard<std::mutex> lk(sh.mu);
    if (res.status != 0) sh.failed = true;
    sh.allowed = INT_MAX;
    sh.cv.notify_all();
  }
  for (std::thread& t : pool) t.join();
  return res;
}

#endif  // ST_HOST_PIPELINE_H_
