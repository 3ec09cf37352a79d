// CycleGraph: "capture once, instantiate, keep, replay" for the cycles that replay a graph (solver.cpp).
// A header of its own so that tests/sanitize/capture_once_asan.cpp can drive every failure path on the
// host, against stand-ins for the seven HIP calls below.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/amg_hip.h"

namespace amg_hip {
amg_hip_status fail_status(amg_hip_status st, const std::string& msg);  // solver.cpp: sets amg_hip_last_error

// Owns the captured graph of one enqueue and its executable form; empty until the first capture.
// Whoever owns the stream destroys (or resets) its CycleGraphs before the stream.
class CycleGraph {
 public:
  CycleGraph() = default;
  CycleGraph(const CycleGraph&) = delete;
  CycleGraph& operator=(const CycleGraph&) = delete;
  ~CycleGraph() { reset(); }

  void reset() {
    if (exec_) (void)hipGraphExecDestroy(exec_);
    if (graph_) (void)hipGraphDestroy(graph_);
    exec_ = nullptr;
    graph_ = nullptr;
  }
  bool captured() const { return exec_ != nullptr; }

  // Captures what enqueue() puts on `st` (thread-local mode) and instantiates it; nothing when already
  // captured.  enqueue returns an amg_hip_status, and one that is not AMG_HIP_OK is returned as it is,
  // after the capture has been ended.  On any failure what was made is destroyed and the holder stays
  // empty, so the next call starts again from nothing.
  template <typename F>
  amg_hip_status capture(hipStream_t st, F&& enqueue) {
    if (exec_) return AMG_HIP_OK;
    hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) return hip_fail("hipStreamBeginCapture(s->stream, hipStreamCaptureModeThreadLocal)", e);
    const amg_hip_status r = enqueue();
    hipGraph_t g = nullptr;
    e = hipStreamEndCapture(st, &g);  // also after a failed enqueue: the stream must leave capture mode
    hipGraphExec_t x = nullptr;
    if (r == AMG_HIP_OK && e == hipSuccess) {
      e = hipGraphInstantiate(&x, g, nullptr, nullptr, 0);
      if (e == hipSuccess) {
        graph_ = g;
        exec_ = x;
        return AMG_HIP_OK;
      }
      (void)hipGraphDestroy(g);
      return hip_fail("hipGraphInstantiate", e);
    }
    if (g) (void)hipGraphDestroy(g);
    return r != AMG_HIP_OK ? r : fail_status(AMG_HIP_EHIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
  }

  // n launches of the graph on `st`, captured from enqueue() at the first use
  template <typename F>
  amg_hip_status replay(hipStream_t st, F&& enqueue, int n = 1) {
    const amg_hip_status r = capture(st, enqueue);
    if (r != AMG_HIP_OK) return r;
    for (int i = 0; i < n; ++i) {
      const hipError_t e = hipGraphLaunch(exec_, st);
      if (e != hipSuccess) return hip_fail("hipGraphLaunch", e);
    }
    return AMG_HIP_OK;
  }

 private:
  static amg_hip_status hip_fail(const char* call, hipError_t e) {
    return fail_status(e == hipErrorOutOfMemory ? AMG_HIP_ENOMEM : AMG_HIP_EHIP,
                       std::string(call) + ": " + hipGetErrorString(e));
  }
  hipGraph_t graph_ = nullptr;
  hipGraphExec_t exec_ = nullptr;
};

// n times the enqueue on `st`: replays of its captured graph G, or (use_graph = 0) the enqueue itself
template <typename F>
amg_hip_status replay_or_enqueue(bool use_graph, CycleGraph& G, hipStream_t st, F&& enqueue, int n = 1) {
  if (use_graph) return G.replay(st, enqueue, n);
  for (int i = 0; i < n; ++i) {
    const amg_hip_status r = enqueue();
    if (r != AMG_HIP_OK) return r;
  }
  return AMG_HIP_OK;
}
}  // namespace amg_hip
