// net_wgrad.h — the weight-gradient helper thread of the layer-program executor's backward pass (net.hip, which alone includes
// this file): a self-contained thread protocol.  The pass publishes WgradJobs; the worker issues their launches on the second stream.
#pragma once
#include <unistd.h>
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "gpn_common.h"
namespace {
// partials of the layers whose slice sums are batched into one launch: at most this much (they are written and read back
// within a few launches - the bound keeps them inside the 256 MB memory-side cache)
constexpr size_t kWgradBatchBytes = (size_t)96 << 20;

// The weight-gradient launches of a backward pass are issued by a helper thread: they go to the second stream, nothing
// on the main chain waits for them, and a HIP launch costs the issuing thread ~2 us - taking them (and their stream
// waits) off the thread that issues the dgrad / BatchNorm chain shortens the host side of the pass by about a third.
// Protocol: the caller publishes jobs (plain structs) through an atomic counter while the pass runs; the worker spins
// on the counter during a pass and sleeps on a condition variable between passes.
// layers per weight-gradient contraction launch (1 ... gpn::kWgradSets; gpn_net_wgrad_group()).  1 = only
// the two networks of a paired pass share a launch (what every measurement of round 3 ran: the knob was unreadable, see the
// note at env_bn_fusion).  First measurement, round 4 (tools/wgrad_group_ab.sh, profiles/r04_wgrad_group_ab.txt): the grouped
// path is bit-equal (48 executor / paired-pass / golden tests at 4), 90 -> 67 launches per step on the weight-gradient stream,
// step time 8.79 / 8.78 / 8.72 ms mean of three interleaved runs at 1 / 2 / 4 - inside the noise, fewer launches for the helper
// thread to issue: default 4.
std::atomic<int> g_wgrad_group{4};

constexpr int64_t g_wgrad_group_rows = 16384;  // only layers with fewer rows than this share a launch

struct WgradJob {
  const float* in;
  const float* dout;
  const int32_t *pair_src, *pair_dst, *tile_off;
  int K;
  int64_t n_dst;
  gpn::DevRows rows;  // n_dst is a bound and the live count of destination rows a device counter (or {nullptr, 0})
  int cin, cout;
  float* dW;
  hipEvent_t after;  // recorded on the caller's stream once dout is final
  // the same layer of the second network of a paired pass (one launch contracts both), or nulls
  const float* in2;
  const float* dout2;
  float* dW2;
};

class WgradWorker {
 public:
  // start a pass: jobs will be issued to `side` of device `dev` with workspace `ws`
  void begin(int dev, hipStream_t side, void* ws, size_t ws_bytes, size_t max_jobs) {
    ensure_thread();
    jobs_.resize(max_jobs);
    dev_ = dev, side_ = side, ws_ = ws, ws_bytes_ = ws_bytes;
    published_.store(0, std::memory_order_relaxed);
    closed_.store(false, std::memory_order_relaxed);
    finished_.store(false, std::memory_order_relaxed);
    rc_ = GPN_OK;
    {
      std::lock_guard<std::mutex> lk(mu_);
      active_ = true;
    }
    cv_.notify_one();
  }
  void push(const WgradJob& j) {
    const size_t i = published_.load(std::memory_order_relaxed);
    jobs_[i] = j;
    published_.store(i + 1, std::memory_order_release);
  }
  // end of pass: wait until every published job has been issued; returns the first error (message in `err`)
  int finish(std::string& err) {
    closed_.store(true, std::memory_order_release);
    while (!finished_.load(std::memory_order_acquire)) std::this_thread::yield();
    err = err_;
    return rc_;
  }

 private:
  void ensure_thread() {
    const pid_t pid = getpid();
    if (started_ && pid_ == pid) return;
    started_ = true;  // (after a fork the child starts its own worker; the parent's thread does not exist there)
    pid_ = pid;
    std::thread([this] { run(); }).detach();
  }
  void run() {
    for (;;) {
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [this] { return active_; });
        active_ = false;
      }
      (void)hipSetDevice(dev_);
      size_t done = 0;
      // slice sums are deferred: every contraction gets its own piece of the workspace, and the sums of a batch of layers
      // (up to kWgradReduceJobs of them / kWgradBatchBytes of partials) run as ONE launch (gpn::wgrad_reduce_many)
      gpn::WgradReduceJob pending[gpn::kWgradReduceJobs];
      int n_pending = 0;
      size_t used = 0;
      const size_t room = std::min(ws_bytes_, kWgradBatchBytes);
      auto fail = [this](int rc) {
        if (rc_ == GPN_OK) {
          rc_ = rc;
          err_ = gpn_last_error();
        }
      };
      auto flush = [&] {
        if (n_pending && rc_ == GPN_OK) {
          const int rc = gpn::wgrad_reduce_many(pending, n_pending, side_);
          if (rc != GPN_OK) fail(rc);
        }
        n_pending = 0;
        used = 0;
      };
      // consecutive jobs of one shape (the convs of a level's residual blocks; the two networks of a paired pass) are
      // contracted by ONE launch of up to kWgradSets layers: held back until a job of another shape arrives or the pass ends
      // (on the deep levels a contraction is a 15-40 us latency chain over a few hundred workgroups: together they overlap)
      WgradJob group[gpn::kWgradSets];
      int n_group = 0, group_sets = 0;
      auto same_shape = [](const WgradJob& a, const WgradJob& b) {
        return a.K == b.K && a.n_dst == b.n_dst && a.cin == b.cin && a.cout == b.cout && a.rows.dev == b.rows.dev;
      };
      auto launch_group = [&]() -> int {
        if (!n_group) return GPN_OK;
        const WgradJob& j0 = group[0];
        const int n = n_group, n_sets = group_sets;
        n_group = 0, group_sets = 0;
        // the events were recorded in job order on one stream: the last one covers the others
        if (hipStreamWaitEvent(side_, group[n - 1].after, 0) != hipSuccess) {
          gpn::set_error("gpn_net_backward: hipStreamWaitEvent failed on the weight-gradient stream");
          return GPN_ERR_HIP;
        }
        const size_t elems = (size_t)j0.K * j0.cin * j0.cout;
        if (j0.n_dst == 0) {
          for (int g = 0; g < n; ++g) {
            GPN_CHECK_HIP(hipMemsetAsync(group[g].dW, 0, sizeof(float) * elems, side_));
            if (group[g].dW2) GPN_CHECK_HIP(hipMemsetAsync(group[g].dW2, 0, sizeof(float) * elems, side_));
          }
          return GPN_OK;
        }
        const int S = gpn::wgrad_slices(j0.K, j0.cin, j0.cout, gpn::plan_rows(j0.n_dst, j0.rows));
        const size_t bytes = gpn::align_up((size_t)S * elems * sizeof(float));
        if (used + n_sets * bytes > room || n_pending + n_sets > gpn::kWgradReduceJobs) flush();
        if (n_sets * bytes > ws_bytes_ || !ws_) {
          gpn::set_error("gpn_net_backward: weight-gradient workspace too small");
          return GPN_ERR_WS;
        }
        gpn::WgradSets sets;
        float* dW_of[gpn::kWgradSets];
        for (int g = 0; g < n; ++g) {
          const WgradJob& j = group[g];
          float* partial = reinterpret_cast<float*>(static_cast<char*>(ws_) + used + sets.n * bytes);
          dW_of[sets.n] = j.dW;
          sets.s[sets.n++] = gpn::WgradSet{j.in, j.dout, j.pair_src, j.pair_dst, j.tile_off, partial};
          if (j.dW2) {
            partial = reinterpret_cast<float*>(static_cast<char*>(ws_) + used + sets.n * bytes);
            dW_of[sets.n] = j.dW2;
            sets.s[sets.n++] = gpn::WgradSet{j.in2, j.dout2, j.pair_src, j.pair_dst, j.tile_off, partial};
          }
        }
        const int rc = gpn::wgrad_contract(sets, j0.K, j0.n_dst, j0.cin, j0.cout, S, side_, j0.rows.dev);
        if (rc != GPN_OK) return rc;
        for (int q = 0; q < sets.n; ++q)
          pending[n_pending++] = gpn::wgrad_reduce_job(sets.s[q].partial, S, j0.K, j0.cin, j0.cout, GPN_LAYOUT_OKI, dW_of[q]);
        used += sets.n * bytes;
        return GPN_OK;
      };
      auto issue = [&](const WgradJob& j) -> int {
        const int n_sets = j.dW2 ? 2 : 1;
        // (a layer with many rows fills the chip on its own: holding it back only delays it)
        const int limit = gpn::plan_rows(j.n_dst, j.rows) < g_wgrad_group_rows ? g_wgrad_group.load(std::memory_order_relaxed) : 1;
        if (n_group && (!same_shape(group[0], j) || group_sets + n_sets > limit)) {
          const int rc = launch_group();
          if (rc != GPN_OK) return rc;
        }
        group[n_group++] = j;
        group_sets += n_sets;
        if (group_sets >= limit) return launch_group();
        return GPN_OK;
      };
      for (;;) {
        const size_t avail = published_.load(std::memory_order_acquire);
        if (done < avail) {
          const WgradJob& j = jobs_[done++];
          if (rc_ != GPN_OK) continue;  // drain after an error
          const int rc = issue(j);
          if (rc != GPN_OK) fail(rc);
        } else if (closed_.load(std::memory_order_acquire) && done == published_.load(std::memory_order_acquire)) {
          break;
        } else {
          std::this_thread::yield();  // nothing published yet: give the core away (8 ranks share the host's cores)
        }
      }
      if (rc_ == GPN_OK) {
        const int rc = launch_group();
        if (rc != GPN_OK) fail(rc);
      }
      flush();
      finished_.store(true, std::memory_order_release);
    }
  }

  std::mutex mu_;
  std::condition_variable cv_;
  bool active_ = false, started_ = false;
  pid_t pid_ = 0;
  std::vector<WgradJob> jobs_;
  std::atomic<size_t> published_{0};
  std::atomic<bool> closed_{false}, finished_{false};
  int dev_ = 0;
  hipStream_t side_ = nullptr;
  void* ws_ = nullptr;
  size_t ws_bytes_ = 0;
  int rc_ = GPN_OK;
  std::string err_;
};

// one worker (thread + pass lock) per device: passes on different devices of one process do not serialise, and nothing
// here is keyed by "the" device of the process
struct DeviceWorker {
  std::mutex pass_mu;  // one backward pass at a time per device (a worker serves a single pass)
  WgradWorker worker;
};

DeviceWorker& device_worker(int dev) {
  static std::mutex mu;
  static DeviceWorker* per_device[gpn::kMaxDevices] = {};  // leaked on purpose: detached threads may outlive static destructors
  std::lock_guard<std::mutex> lk(mu);
  if (!per_device[dev]) per_device[dev] = new DeviceWorker();
  return *per_device[dev];
}
}  // namespace
