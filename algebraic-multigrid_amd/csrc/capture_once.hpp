// capture_once: "capture once, instantiate, keep" for the cycles that replay a graph (solver.cpp).
// A header of its own so that tests/sanitize/capture_once_asan.cpp can drive every failure path on the
// host, against stand-ins for the six HIP calls below.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/amg_hip.h"

namespace amg_hip {
amg_hip_status fail_status(amg_hip_status st, const std::string& msg);  // solver.cpp: sets amg_hip_last_error

// Captures what enqueue() puts on `st` (thread-local mode) into *graph and instantiates it into *exec;
// both are null on entry.  enqueue returns an amg_hip_status, and one that is not AMG_HIP_OK is returned
// as it is, after the capture has been ended.  On any failure what was made is destroyed and both
// handles stay null, so the next call starts again from nothing.
template <typename F>
amg_hip_status capture_once(hipStream_t st, F&& enqueue, hipGraph_t* graph, hipGraphExec_t* exec) {
  auto hip_fail = [](const char* call, hipError_t e) {
    return fail_status(e == hipErrorOutOfMemory ? AMG_HIP_ENOMEM : AMG_HIP_EHIP,
                       std::string(call) + ": " + hipGetErrorString(e));
  };
  hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
  if (e != hipSuccess) return hip_fail("hipStreamBeginCapture(s->stream, hipStreamCaptureModeThreadLocal)", e);
  const amg_hip_status r = enqueue();
  hipGraph_t g = nullptr;
  e = hipStreamEndCapture(st, &g);  // also after a failed enqueue: the stream must leave capture mode
  hipGraphExec_t x = nullptr;
  if (r == AMG_HIP_OK && e == hipSuccess) {
    e = hipGraphInstantiate(&x, g, nullptr, nullptr, 0);
    if (e == hipSuccess) {
      *graph = g;
      *exec = x;
      return AMG_HIP_OK;
    }
    (void)hipGraphDestroy(g);
    return hip_fail("hipGraphInstantiate", e);
  }
  if (g) (void)hipGraphDestroy(g);
  return r != AMG_HIP_OK ? r : fail_status(AMG_HIP_EHIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
}
}  // namespace amg_hip
