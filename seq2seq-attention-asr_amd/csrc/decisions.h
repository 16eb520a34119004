// Host-side record of dispatch decisions (test infrastructure; not part of include/s2s_hip.h).
//
// The library picks a kernel path from exact dimensions and process-wide knobs.  A test written for one path,
// or comparing two paths as A/B arms, must be able to prove which path ran.  Each decision site calls
// decide(name, value) where its launch is issued, with the variable that steers the launch -- the probe never
// recomputes a plan.  The record is off by default (a site then costs one relaxed atomic load);
// s2s_debug_decisions(1) turns it on, s2s_debug_decision(name, &value, &count) reads name -> (last value, count)
// and s2s_debug_decisions_clear() empties the table (capi_debug.cpp).  Host code only: it records at issue time,
// so it also works while a stream is being captured (ProfScope's events do not).
#pragma once
#include <atomic>

namespace s2s {

extern std::atomic<int> g_decisions_on;
void decision_store(const char* name, long value);  // mutex-guarded table (capi_debug.cpp)

inline void decide(const char* name, long value) {
  if (g_decisions_on.load(std::memory_order_relaxed)) decision_store(name, value);
}

}  // namespace s2s
