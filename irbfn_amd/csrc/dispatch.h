// Run-time value -> compile-time constant, the one way a launcher turns a net's DC / OP / basis class into a kernel
// instance.  No HIP header: tests/test_dispatch_cpu.py compiles it with the host compiler alone.
#pragma once

#include <type_traits>
#include <utility>

#include "irbfn_hip.h"

namespace irbfn {

// f(std::integral_constant<int, V>{}) for the V of the list that equals v, and f's status unchanged; IRBFN_ERR_UNSUPPORTED,
// and no call, if none does.  Each launcher spells out its own list: the list is what gets compiled.
template <int... Vs, class F>
int dispatch(int v, F&& f) {
  int rc = IRBFN_ERR_UNSUPPORTED;
  (void)(... || (v == Vs && ((rc = f(std::integral_constant<int, Vs>{})), true)));
  return rc;
}

}  // namespace irbfn
