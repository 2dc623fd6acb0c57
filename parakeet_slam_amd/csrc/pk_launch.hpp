// Host-side helpers of the observe launchers: what every kernel argument struct shares is filled here, once.  The argument structs
// themselves live beside their kernels (FastArgs, SweepArgs, PubArgs, AssocArgs, ...); they share member NAMES, not a base, so
// these are templates over the argument type.  Everything is inline or a template: the one-call builds see every source at once.
#pragma once
#include <cassert>
#include <type_traits>
#include <utility>

#include "pk_kernels.hpp"
#include "pk_math.hpp"

namespace pk {

template <class A, class = void>
struct has_heading : std::false_type {};
template <class A>
struct has_heading<A, std::void_t<decltype(std::declval<A&>().h)>> : std::true_type {};

// What a kernel READS of the live generation: where the particles' slots are, their poses (the heading where the struct has one)
// and the map's dimensions.
template <class A>
inline auto fill_particles(A& a, const DeviceState& d) -> decltype((void)a.ss) {
  a.ss = slot_source(d);
  a.count_off = d.lay.count_off;
  a.src = d.src[d.cur];
  a.x = d.x[d.cur];
  a.y = d.y[d.cur];
  if constexpr (has_heading<A>::value) a.h = d.h[d.cur];
  a.L = d.lay.L;
  a.Lp = d.lay.Lp;
}
// ... and what an observe kernel WRITES: the other map buffer and the log-weights
template <class A>
inline auto fill_state(A& a, const DeviceState& d) -> decltype((void)a.ss) {
  fill_particles(a, d);
  a.map_dst = d.map[d.mcur ^ 1];
  a.logw = d.logw[d.cur];
  a.immutable = d.immutable;
}
// FusedArgs, RegsArgs: a FastArgs `f` (which has no heading) with the heading beside it
template <class A>
inline auto fill_state(A& a, const DeviceState& d) -> decltype((void)a.f) {
  fill_state(a.f, d);
  a.h = d.h[d.cur];
}

inline Noise<double> device_noise(const NoiseD& q) { return make_noise(q.q00, q.rr, q.rg, q.rb, q.gg, q.gb, q.bb); }

// The scan of a maximum-likelihood observe kernel and the launch's options
template <class A>
inline auto fill_scan(A& a, const ScanTables& scan, const ObserveExtras& ex, const NoiseD& qt) -> decltype((void)a.exact) {
  a.exact = scan.exact;
  a.order = scan.order;
  a.B = scan.B;
  a.reset = ex.reset ? 1 : 0;
  a.gmax_key = ex.gmax_key;
  a.qt = device_noise(qt);
}
template <class A>
inline auto fill_scan(A& a, const ScanTables& scan, const ObserveExtras& ex, const NoiseD& qt) -> decltype((void)a.f) {
  fill_scan(a.f, scan, ex, qt);
}

// The kernels may ask for `bytes` of dynamic LDS: once per device (`done`: the launcher's own flags), errors swallowed -- a kernel
// that is refused fails at its launch, and no sticky error is left behind for other users of the runtime.
template <class... K>
inline void allow_dynamic_lds(bool (&done)[kMaxDevices], size_t bytes, K*... kernels) {
  if (!first_time_on_this_device(done)) return;
  for (const void* fn : {reinterpret_cast<const void*>(kernels)...})
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) (void)hipGetLastError();
}

}  // namespace pk
