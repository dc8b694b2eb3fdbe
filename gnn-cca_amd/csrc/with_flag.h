#pragma once
// A template bool of a launch chosen at run time: f(std::true_type{}) or f(std::false_type{}), so a kernel<A, B> ladder is two nested
// calls instead of four written-out launches (graph_build.hip, mpn_forward.hip).
#include <type_traits>

namespace gnncca {

template <class F>
static void with_flag(bool flag, F&& f) { flag ? f(std::true_type{}) : f(std::false_type{}); }

}  // namespace gnncca
