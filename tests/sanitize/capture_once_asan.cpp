// TEST INFRASTRUCTURE: drives CycleGraph (csrc/capture_once.hpp) through its success paths and its
// four failure paths on the HOST, under AddressSanitizer + UndefinedBehaviorSanitizer.  No GPU and no
// HIP runtime: the seven HIP calls the type makes are the stand-ins below, which count what they
// create, destroy and launch and fail on request (make capture_once_asan; tests/test_capture_once_asan.py).
// After every failure the holder must be empty, the capture ended, and nothing created left alive.
#include <cstdio>
#include <string>

#include "../../algebraic-multigrid_amd/csrc/capture_once.hpp"

namespace {
int g_graphs = 0, g_execs = 0;  // alive
int g_launches = 0;
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
hipError_t hipGraphLaunch(hipGraphExec_t x, hipStream_t) {
  if (!x || *reinterpret_cast<int*>(x) != 2 || g_capturing) return hipErrorInvalidValue;
  ++g_launches;
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

// one capture (or replay) with the given faults; then: the expected status, the holder empty, nothing
// alive, not capturing, nothing launched; and a replay without faults on the same holder succeeds
static int failing(bool by_replay, hipError_t begin, amg_hip_status enq, hipError_t end, bool end_gives_graph,
                   hipError_t inst, amg_hip_status want, const char* text) {
  g_begin = begin;
  g_end = end;
  g_end_gives_graph = end_gives_graph;
  g_inst = inst;
  g_msg.clear();
  g_launches = 0;
  int calls = 0;
  amg_hip::CycleGraph G;
  auto enqueue = [&] {
    ++calls;
    return enq;
  };
  const amg_hip_status r = by_replay ? G.replay(nullptr, enqueue) : G.capture(nullptr, enqueue);
  CHECK(r == want);
  CHECK(!G.captured());
  CHECK(g_graphs == 0 && g_execs == 0 && !g_capturing && g_launches == 0);
  CHECK(calls == (begin == hipSuccess ? 1 : 0));
  CHECK(g_msg.find(text) == 0);
  g_begin = g_end = g_inst = hipSuccess;
  CHECK(G.replay(nullptr, [] { return AMG_HIP_OK; }) == AMG_HIP_OK);
  CHECK(G.captured() && g_graphs == 1 && g_execs == 1 && !g_capturing && g_launches == 1);
  G.reset();
  CHECK(!G.captured() && g_graphs == 0 && g_execs == 0);
  return 0;
}

int main() {
  const hipError_t ok = hipSuccess, bad = hipErrorUnknown;
  for (const bool by_replay : {false, true}) {
    if (failing(by_replay, bad, AMG_HIP_OK, ok, true, ok, AMG_HIP_EHIP, "hipStreamBeginCapture(")) return 1;
    if (failing(by_replay, hipErrorOutOfMemory, AMG_HIP_OK, ok, true, ok, AMG_HIP_ENOMEM, "hipStreamBeginCapture("))
      return 1;
    // the enqueue's own status comes back (its message is the enqueue's business), with and without a graph
    if (failing(by_replay, ok, AMG_HIP_EINVAL, ok, true, ok, AMG_HIP_EINVAL, "")) return 1;
    if (failing(by_replay, ok, AMG_HIP_EINVAL, bad, false, ok, AMG_HIP_EINVAL, "")) return 1;
    if (failing(by_replay, ok, AMG_HIP_OK, bad, false, ok, AMG_HIP_EHIP, "hipStreamEndCapture: ")) return 1;
    if (failing(by_replay, ok, AMG_HIP_OK, bad, true, ok, AMG_HIP_EHIP, "hipStreamEndCapture: ")) return 1;
    if (failing(by_replay, ok, AMG_HIP_OK, ok, true, bad, AMG_HIP_EHIP, "hipGraphInstantiate: ")) return 1;
    if (failing(by_replay, ok, AMG_HIP_OK, ok, true, hipErrorOutOfMemory, AMG_HIP_ENOMEM, "hipGraphInstantiate: "))
      return 1;
  }
  g_begin = g_end = g_inst = hipSuccess;
  g_launches = 0;
  int calls = 0;
  auto enqueue = [&] {
    ++calls;
    return AMG_HIP_OK;
  };
  {
    amg_hip::CycleGraph G;
    // capture without replay launches nothing; a second capture is a no-op
    CHECK(G.capture(nullptr, enqueue) == AMG_HIP_OK && G.capture(nullptr, enqueue) == AMG_HIP_OK);
    CHECK(G.captured() && calls == 1 && g_graphs == 1 && g_execs == 1 && !g_capturing && g_launches == 0);
    // replay on the captured holder only launches
    CHECK(G.replay(nullptr, enqueue) == AMG_HIP_OK);
    CHECK(calls == 1 && g_launches == 1);
    // reset destroys both, and the holder starts again from nothing
    G.reset();
    CHECK(!G.captured() && g_graphs == 0 && g_execs == 0);
    // replay twice captures once and launches twice
    g_launches = 0;
    CHECK(G.replay(nullptr, enqueue) == AMG_HIP_OK && G.replay(nullptr, enqueue) == AMG_HIP_OK);
    CHECK(calls == 2 && g_graphs == 1 && g_execs == 1 && g_launches == 2);
    // n launches in one call
    CHECK(G.replay(nullptr, enqueue, 3) == AMG_HIP_OK);
    CHECK(calls == 2 && g_launches == 5);
  }
  // a holder that goes out of scope destroys both
  CHECK(g_graphs == 0 && g_execs == 0);
  // replay_or_enqueue: the eager side runs the enqueue n times and touches no graph
  {
    amg_hip::CycleGraph G;
    g_launches = 0;
    CHECK(amg_hip::replay_or_enqueue(false, G, nullptr, enqueue, 2) == AMG_HIP_OK);
    CHECK(calls == 4 && !G.captured() && g_graphs == 0 && g_launches == 0);
    CHECK(amg_hip::replay_or_enqueue(true, G, nullptr, enqueue, 2) == AMG_HIP_OK);
    CHECK(calls == 5 && G.captured() && g_launches == 2);
  }
  CHECK(g_graphs == 0 && g_execs == 0);
  std::puts("capture_once_asan ok");
  return 0;
}
