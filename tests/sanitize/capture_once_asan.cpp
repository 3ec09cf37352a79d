// TEST INFRASTRUCTURE: drives capture_once (csrc/capture_once.hpp) through its success path and its
// four failure paths on the HOST, under AddressSanitizer + UndefinedBehaviorSanitizer.  No GPU and no
// HIP runtime: the six HIP calls the helper makes are the stand-ins below, which count what they
// create and destroy and fail on request.  Not part of the test suite (make capture_once_asan).
// After every failure both handles must be null, the capture ended, and nothing created left alive.
#include <cstdio>
#include <string>

#include "../../algebraic-multigrid_amd/csrc/capture_once.hpp"

namespace {
int g_graphs = 0, g_execs = 0;  // alive
bool g_capturing = false;
hipError_t g_begin = hipSuccess, g_end = hipSuccess, g_inst = hipSuccess;
bool g_end_gives_graph = true;  // a failed hipStreamEndCapture may or may not hand out a graph
std::string g_msg;
}  // namespace

extern "C" {
hipError_t hipStreamBeginCapture(hipStream_t, hipStreamCaptureMode mode) {
  if (mode != hipStreamCaptureModeThreadLocal || g_capturing) return hipErrorInvalidValue;
  if (g_begin != hipSuccess) return g_begin;
  g_capturing = true;
  return hipSuccess;
}
hipError_t hipStreamEndCapture(hipStream_t, hipGraph_t* g) {
  if (!g_capturing) return hipErrorInvalidValue;
  g_capturing = false;
  *g = nullptr;
  if (g_end == hipSuccess || g_end_gives_graph) {
    *g = reinterpret_cast<hipGraph_t>(new int(1));
    ++g_graphs;
  }
  return g_end;
}
hipError_t hipGraphInstantiate(hipGraphExec_t* x, hipGraph_t g, hipGraphNode_t*, char*, size_t) {
  if (!g) return hipErrorInvalidValue;
  if (g_inst != hipSuccess) return g_inst;
  *x = reinterpret_cast<hipGraphExec_t>(new int(2));
  ++g_execs;
  return hipSuccess;
}
hipError_t hipGraphDestroy(hipGraph_t g) {
  delete reinterpret_cast<int*>(g);
  --g_graphs;
  return hipSuccess;
}
hipError_t hipGraphExecDestroy(hipGraphExec_t x) {
  delete reinterpret_cast<int*>(x);
  --g_execs;
  return hipSuccess;
}
const char* hipGetErrorString(hipError_t) { return "stub error"; }
}

namespace amg_hip {
amg_hip_status fail_status(amg_hip_status st, const std::string& msg) {
  g_msg = msg;
  return st;
}
}  // namespace amg_hip

#define CHECK(c)                                                                       \
  do {                                                                                 \
    if (!(c)) {                                                                        \
      std::fprintf(stderr, "capture_once_asan: %s failed (line %d)\n", #c, __LINE__);  \
      return 1;                                                                        \
    }                                                                                  \
  } while (0)

// one call with the given faults; then: the expected status, handles null, nothing alive, not capturing
static int failing(hipError_t begin, amg_hip_status enq, hipError_t end, bool end_gives_graph, hipError_t inst,
                   amg_hip_status want, const char* text) {
  g_begin = begin;
  g_end = end;
  g_end_gives_graph = end_gives_graph;
  g_inst = inst;
  g_msg.clear();
  int calls = 0;
  hipGraph_t g = nullptr;
  hipGraphExec_t x = nullptr;
  const amg_hip_status r = amg_hip::capture_once(
      nullptr,
      [&] {
        ++calls;
        return enq;
      },
      &g, &x);
  CHECK(r == want);
  CHECK(g == nullptr && x == nullptr);
  CHECK(g_graphs == 0 && g_execs == 0 && !g_capturing);
  CHECK(calls == (begin == hipSuccess ? 1 : 0));
  CHECK(g_msg.find(text) == 0);
  return 0;
}

int main() {
  const hipError_t ok = hipSuccess, bad = hipErrorUnknown;
  if (failing(bad, AMG_HIP_OK, ok, true, ok, AMG_HIP_EHIP, "hipStreamBeginCapture(")) return 1;
  if (failing(hipErrorOutOfMemory, AMG_HIP_OK, ok, true, ok, AMG_HIP_ENOMEM, "hipStreamBeginCapture(")) return 1;
  // the enqueue's own status comes back (its message is the enqueue's business), with and without a graph
  if (failing(ok, AMG_HIP_EINVAL, ok, true, ok, AMG_HIP_EINVAL, "")) return 1;
  if (failing(ok, AMG_HIP_EINVAL, bad, false, ok, AMG_HIP_EINVAL, "")) return 1;
  if (failing(ok, AMG_HIP_OK, bad, false, ok, AMG_HIP_EHIP, "hipStreamEndCapture: ")) return 1;
  if (failing(ok, AMG_HIP_OK, bad, true, ok, AMG_HIP_EHIP, "hipStreamEndCapture: ")) return 1;
  if (failing(ok, AMG_HIP_OK, ok, true, bad, AMG_HIP_EHIP, "hipGraphInstantiate: ")) return 1;
  if (failing(ok, AMG_HIP_OK, ok, true, hipErrorOutOfMemory, AMG_HIP_ENOMEM, "hipGraphInstantiate: ")) return 1;
  // success after the failures: both handles set, one of each alive, and they are the caller's to destroy
  g_begin = g_end = g_inst = hipSuccess;
  hipGraph_t g = nullptr;
  hipGraphExec_t x = nullptr;
  CHECK(amg_hip::capture_once(nullptr, [] { return AMG_HIP_OK; }, &g, &x) == AMG_HIP_OK);
  CHECK(g && x && g_graphs == 1 && g_execs == 1 && !g_capturing);
  (void)hipGraphExecDestroy(x);
  (void)hipGraphDestroy(g);
  CHECK(g_graphs == 0 && g_execs == 0);
  std::puts("capture_once_asan ok");
  return 0;
}
