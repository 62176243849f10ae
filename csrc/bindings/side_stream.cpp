// Side-stream fork of the native executors (block_ops.cpp, head_ops.cpp): one event pool,
// one fork helper, and the stash that keeps the side stream's operands alive until the join
// (ops/streams.py join -> side_stash_release).
#include "conv_internal.h"
#include "ops_decl.h"

#include <c10/hip/HIPStream.h>

#include <mutex>

namespace sdx_bind {

std::vector<torch::Tensor>& side_stash() {
  static std::vector<torch::Tensor> v;
  return v;
}

namespace {
// event pool for fork / join points
hipEvent_t next_event() {
  static std::mutex mu;
  static std::vector<hipEvent_t> pool;
  static size_t next = 0;
  std::lock_guard<std::mutex> lk(mu);
  if (pool.empty()) {
    // The pool only orders the two streams of one device (record on one, hipStreamWaitEvent
    // on the other); the kernels' own dispatch fences publish their writes device-wide. A
    // record's default system-scope release (L2 writeback + invalidate) is for host / peer
    // visibility, which nothing here needs: without it the main stream's bubble at each fork
    // point drops from ~7.0 to ~5.0 us (48 forks per step) and the step by 0.11 ms (3/3
    // same-box rounds, profiles/event_fence_r6.txt). SDX_EV_FENCE: 0 = the default fence,
    // 1 = hipEventDisableSystemFence (default), 2 = hipEventReleaseToDevice (-0.03 ms)
    const int fm = (int)sdx_plan::env_int("SDX_EV_FENCE", 1);
    const unsigned fl = hipEventDisableTiming | (fm == 1 ? hipEventDisableSystemFence : 0u) |
                        (fm == 2 ? hipEventReleaseToDevice : 0u);
    pool.resize(512);
    for (auto& e : pool) check_hip(hipEventCreateWithFlags(&e, fl), "hipEventCreate");
  }
  hipEvent_t e = pool[next];
  next = (next + 1) % pool.size();
  return e;
}
}  // namespace

hipEvent_t stream_mark() {
  hipEvent_t ev = next_event();
  check_hip(hipEventRecord(ev, cur_stream()), "hipEventRecord");
  return ev;
}

void stream_wait(hipEvent_t ev) { check_hip(hipStreamWaitEvent(cur_stream(), ev, 0), "hipStreamWaitEvent"); }

c10::hip::HIPStreamGuard side_fork(int64_t side, const torch::Device& dev, std::initializer_list<torch::Tensor> keep) {
  hipStream_t ss = reinterpret_cast<hipStream_t>(side);
  check_hip(hipStreamWaitEvent(ss, stream_mark(), 0), "hipStreamWaitEvent");
  for (const auto& t : keep) side_stash().push_back(t);
  return c10::hip::HIPStreamGuard(c10::hip::getStreamFromExternal(ss, dev.index()));
}

}  // namespace sdx_bind
