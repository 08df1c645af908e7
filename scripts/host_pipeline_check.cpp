// Drives st_pipe_run (scannertools_amd/csrc/st_host_pipeline.h), the sub-batch pipeline of the JPEG host path and the PNG
// decoder, with callbacks over ordinary memory: the slots are plain int arrays, so a build with -fsanitize=thread reports a
// slot that is refilled while its sub-batch is still being read, and the program's own checks report everything else.
// Stand-alone (no HIP, no GPU):
//   c++ -std=c++17 -g -O1 -fsanitize=thread -pthread -Iscannertools_amd/csrc scripts/host_pipeline_check.cpp -o host_pipeline_check
//   ./host_pipeline_check
// Only outcomes the pipeline's rules make certain are checked: which of two failures in different sub-batches that are in
// flight together is reported depends on timing, and is not.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "st_host_pipeline.h"

namespace {
int failures = 0, runs = 0;
std::atomic<int> fill_failures{0};   // checks that fail on a worker thread

#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      printf("line %d: ", __LINE__);     \
      printf(__VA_ARGS__);               \
      printf("\n");                      \
      ++failures;                        \
    }                                    \
  } while (0)

enum { FILL_FAILED = 7, ISSUE_FAILED = 98, RELEASE_FAILED = 99 };

struct Case {
  int n, T, cut;
  int fail_a = -1, fail_b = -1;   // streams whose fill fails; with both set they are in one sub-batch and fail together
  int issue_fails_at = -1, release_fails_at = -1;   // sub-batches
};

std::vector<StPipeSubBatch> plan_of(int n, int cut) {
  std::vector<StPipeSubBatch> plan;
  for (int i = 0; i < n; ++i) {
    if (plan.empty() || plan.back().count >= cut) plan.push_back(StPipeSubBatch{i, 0});
    plan.back().count++;
  }
  return plan;
}

void run_case(const Case& c) {
  ++runs;
  const std::vector<StPipeSubBatch> plan = plan_of(c.n, c.cut);
  const int nsb = (int)plan.size();
  std::vector<int> sb_of((size_t)c.n);
  for (int k = 0; k < nsb; ++k)
    for (int i = plan[k].first; i < plan[k].first + plan[k].count; ++i) sb_of[i] = k;
  std::vector<int> slot[2];   // the id of the sub-batch each place was last filled for: plain memory on purpose
  for (int s = 0; s < 2; ++s) slot[s].assign((size_t)c.cut, -1);
  std::vector<std::atomic<int>> filled((size_t)c.n);
  for (auto& f : filled) f = 0;
  std::atomic<int> may_fill{2};   // sub-batches below this may be filled: moved on as the last thing release does
  std::atomic<int> inside{0}, together{0};
  const std::thread::id caller = std::this_thread::get_id();
  std::atomic<int> issued{0};   // written by the calling thread
  int released = 0;             // touched by the calling thread only

  auto fill = [&](int i, int k, int s, char* msg, size_t msg_len) -> int {
    ++inside;
    bool ok = k == sb_of[i] && s == (k & 1) && std::this_thread::get_id() != caller && msg_len == sizeof(StPipeResult().message);
    ok = ok && k < may_fill.load();   // no fill of sub-batch k + 2 before release of sub-batch k has returned
    ok = ok && filled[(size_t)i].fetch_add(1) == 0;
    if (!ok) ++fill_failures;
    for (int spin = (i * 7) % 5; spin > 0; --spin) std::this_thread::yield();
    slot[s][(size_t)(i - plan[k].first)] = k;
    int st = 0;
    if (i == c.fail_a || i == c.fail_b) {
      if (c.fail_a >= 0 && c.fail_b >= 0 && c.T > 1) {
        // Both are running before either fails: a fill that begins after a failure was recorded would be skipped.  And the
        // sub-batch before theirs was issued: until then the calling thread may see the first failure before the second.
        ++together;
        const auto t0 = std::chrono::steady_clock::now();
        auto met = [&] { return together.load() == 2 && issued.load() >= k; };
        while (!met() && std::chrono::steady_clock::now() - t0 < std::chrono::seconds(20)) std::this_thread::yield();
        if (!met()) ++fill_failures;
      }
      st = FILL_FAILED + i;
      snprintf(msg, msg_len, "stream %d is broken", i);
    }
    --inside;
    return st;
  };
  auto issue = [&](int k, int s) -> int {
    CHECK(std::this_thread::get_id() == caller, "issue off the calling thread");
    const int nth = issued.fetch_add(1);
    CHECK(k == nth && s == (k & 1), "issue(%d, %d) as number %d", k, s, nth);
    for (int j = 0; j < plan[k].count; ++j) CHECK(slot[s][(size_t)j] == k, "sub-batch %d: place %d of its slot holds %d", k, j, slot[s][(size_t)j]);
    for (int i = plan[k].first; i < plan[k].first + plan[k].count; ++i) CHECK(filled[(size_t)i].load() == 1, "stream %d filled %d times at its issue", i, filled[(size_t)i].load());
    return k == c.issue_fails_at ? (int)ISSUE_FAILED : 0;
  };
  auto release = [&](int s) -> int {
    const int k = issued.load() - 1;
    CHECK(std::this_thread::get_id() == caller, "release off the calling thread");
    CHECK(k + 2 < nsb && s == (k & 1) && released == k, "release(%d) behind sub-batch %d of %d, %d released", s, k, nsb, released);
    ++released;
    if (k == c.release_fails_at) return RELEASE_FAILED;
    for (int j = 0; j < plan[k].count; ++j) CHECK(slot[s][(size_t)j] == k, "sub-batch %d: its slot was refilled before its release", k);
    may_fill = k + 3;
    return 0;
  };
  const StPipeResult r = st_pipe_run(plan, c.T, fill, issue, release);
  const int issued_n = issued.load();

  CHECK(inside.load() == 0, "%d fills still running", inside.load());
  const int fail = c.fail_a >= 0 && c.fail_b >= 0 ? std::min(c.fail_a, c.fail_b) : std::max(c.fail_a, c.fail_b);
  if (fail >= 0) {
    char want[64];
    snprintf(want, sizeof want, "stream %d is broken", fail);
    CHECK(r.status == FILL_FAILED + fail && r.stream == fail && strcmp(r.message, want) == 0, "n %d T %d cut %d, fill of %d (and %d) fails: %d, %d, '%s'", c.n,
          c.T, c.cut, c.fail_a, c.fail_b, r.status, r.stream, r.message);
    CHECK(issued_n <= sb_of[fail], "sub-batch %d was issued with a failed stream, %d issued", sb_of[fail], issued_n);
    for (int i = 0; i < c.n; ++i) CHECK(filled[(size_t)i].load() <= 1, "stream %d filled %d times", i, filled[(size_t)i].load());
  } else if (c.issue_fails_at >= 0 || c.release_fails_at >= 0) {
    const int k = std::max(c.issue_fails_at, c.release_fails_at);
    CHECK(r.status == (c.issue_fails_at >= 0 ? ISSUE_FAILED : RELEASE_FAILED) && r.stream == -1, "n %d T %d cut %d: error at sub-batch %d comes back as %d, %d", c.n,
          c.T, c.cut, k, r.status, r.stream);
    CHECK(issued_n == k + 1, "%d issued with an error at sub-batch %d", issued_n, k);
  } else {
    CHECK(r.status == 0 && r.stream == -1 && r.message[0] == 0, "n %d T %d cut %d: %d, %d, '%s'", c.n, c.T, c.cut, r.status, r.stream, r.message);
    CHECK(issued_n == nsb && released == std::max(0, nsb - 2), "%d of %d issued, %d released", issued_n, nsb, released);
    for (int i = 0; i < c.n; ++i) CHECK(filled[(size_t)i].load() == 1, "stream %d filled %d times", i, filled[(size_t)i].load());
  }
}
}  // namespace

int main() {
  CHECK(st_pipe_threads("ST_NO_SUCH_VARIABLE", 1) == 1 && st_pipe_threads("ST_NO_SUCH_VARIABLE", 1000) <= 16, "default thread count");
  setenv("ST_PIPE_CHECK_THREADS", "200", 1);
  CHECK(st_pipe_threads("ST_PIPE_CHECK_THREADS", 1000) == 64 && st_pipe_threads("ST_PIPE_CHECK_THREADS", 5) == 5, "thread count above its range");
  setenv("ST_PIPE_CHECK_THREADS", "-3", 1);
  CHECK(st_pipe_threads("ST_PIPE_CHECK_THREADS", 9) == 1, "thread count below its range");
  CHECK(st_pipe_run(std::vector<StPipeSubBatch>(), 1, [](int, int, int, char*, size_t) { return 1; }, [](int, int) { return 1; }, [](int) { return 1; }).status == 0,
        "an empty plan");
  for (int n : {1, 2, 17, 70})
    for (int T : {1, 4, 16})
      for (int cut : {T, 3}) {
        const std::vector<StPipeSubBatch> plan = plan_of(n, cut);
        const int nsb = (int)plan.size();
        Case c{n, std::min(T, n), cut};   // (the callers never ask for more threads than streams)
        run_case(c);
        for (int f : {0, n / 2, n - 1}) {
          Case one = c;
          one.fail_a = f;
          run_case(one);
        }
        for (const StPipeSubBatch& sb : {plan.front(), plan[(size_t)nsb / 2], plan.back()}) {
          if (sb.count < 2) continue;
          Case two = c;
          two.fail_a = sb.first + 1;   // the higher stream first in the case: the lower one is what comes back
          two.fail_b = sb.first;
          run_case(two);
        }
        for (int k : {0, nsb / 2, nsb - 1}) {
          Case e = c;
          e.issue_fails_at = k;
          run_case(e);
          if (k + 2 < nsb) {
            e = c;
            e.release_fails_at = k;
            run_case(e);
          }
        }
      }
  failures += fill_failures.load();
  printf("host_pipeline_check: %d runs, %d failures\n", runs, failures);
  return failures ? 1 : 0;
}
