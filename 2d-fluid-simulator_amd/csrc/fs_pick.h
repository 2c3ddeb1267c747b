// fs_pick.h - from a run-time value to a compile-time one: the one way a launch site chooses a template instantiation.  Standard library only (the
// CPU tests compile it with the host compiler: fs_tiles_host.cpp).
//
//   pick<2, 4>(rt, [&](auto RT) { klaunch(k_foo<RT, T>, ...); })        calls the callable with Int<2>{} or Int<4>{} and returns true; returns false
//                                                                      - nothing called - for an `rt` that is not listed
//   pick_bool(flag, [&](auto FLAG) { ... k_foo<FLAG> ... })             the same for a flag: Bool<true>{} / Bool<false>{}
//   with_dm_all<T>(dm, [&](auto DM) { ... k_foo<DM, T> ... })           the division modes a kernel family distinguishes (below)
//
// A callable may itself return the result of an inner pick: a false from any level reaches the caller, and fs::launch (fs_launch.h) turns it into an
// error - a value nobody listed never becomes a launch that silently did not happen.  Only the listed values are instantiated: a nested pick over
// two lists instantiates their cross product, so a site whose kernel exists for some combinations only says so with explicit branches.
#pragma once
#include <type_traits>
#include <utility>

namespace fs {

template <int V> using Int = std::integral_constant<int, V>;
template <bool V> using Bool = std::integral_constant<bool, V>;

// f(tag): true unless f itself reports (as a bool) that it found nothing to call
template <typename F, typename Tag>
inline bool pick_call(F &&f, Tag tag)
{
    if constexpr (std::is_void<decltype(f(tag))>::value) { f(tag); return true; }
    else return f(tag);
}

template <int... Vs, typename F>
inline bool pick(int v, F &&f)
{
    return ((v == Vs && pick_call(f, Int<Vs>{})) || ...);
}

template <typename F>
inline bool pick_bool(bool v, F &&f)
{
    return v ? pick_call(f, Bool<true>{}) : pick_call(f, Bool<false>{});
}

// Division modes (fs_device.h DM_*: bit 0 - power-of-two dx-derived divisors, exact multiplication; bit 2 - f32 fields divide by their other loop-invariant
// divisors through one f64 multiplication; neither - IEEE division).  Which template mode a launch takes, by the kinds of divisor the kernel family has:
constexpr bool dm_is(int dm, int bits) { return (dm & 7) == bits; }
constexpr int dm_pick_const(bool f32, int dm) { return f32 && dm_is(dm, 4) ? 4 : 0; }                                     // no dx-derived divisor: 0 / 4
constexpr int dm_pick_dx(bool f32, int dm) { return (dm & 1) ? 1 : (f32 && dm_is(dm, 4) ? 4 : 0); }                        // dx-derived divisors only: 0 / 1 / 4
constexpr int dm_pick_all(bool f32, int dm) { return f32 && dm_is(dm, 5) ? 5 : (f32 && dm_is(dm, 4) ? 4 : ((dm & 1) ? 1 : 0)); }      // both kinds: 0 / 1 / 4 / 5

// f(Int<DM>{}) for the mode of the family; modes 4 and 5 exist for T = float alone (no double kernel is instantiated with them)
template <typename T, typename F>
inline bool with_dm_const(int dm, F &&f)
{
    constexpr bool f32 = std::is_same<T, float>::value;
    if constexpr (f32) return pick<0, 4>(dm_pick_const(f32, dm), f);
    else return pick<0>(dm_pick_const(f32, dm), f);
}
template <typename T, typename F>
inline bool with_dm_dx(int dm, F &&f)
{
    constexpr bool f32 = std::is_same<T, float>::value;
    if constexpr (f32) return pick<0, 1, 4>(dm_pick_dx(f32, dm), f);
    else return pick<0, 1>(dm_pick_dx(f32, dm), f);
}
template <typename T, typename F>
inline bool with_dm_all(int dm, F &&f)
{
    constexpr bool f32 = std::is_same<T, float>::value;
    if constexpr (f32) return pick<0, 1, 4, 5>(dm_pick_all(f32, dm), f);
    else return pick<0, 1>(dm_pick_all(f32, dm), f);
}

}  // namespace fs
