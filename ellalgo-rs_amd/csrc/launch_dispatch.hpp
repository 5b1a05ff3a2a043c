// launch_dispatch.hpp -- run-time values to template arguments, for the host code that picks a kernel instantiation.
//   with_bool(b, f)              calls f(std::true_type{}) or f(std::false_type{})
//   with_int(Ints<8, 16>{}, v, f)  calls f(std::integral_constant<int, V>{}) for the V of the list that equals v; false: none does
//   with_one_of(OneOf<A, B>{}, match, f)  the same over a list of empty tag types (the RW x UNR pairs): f(T{}) for the first T with
//                                match(T{}).  with_int and with_one_of DROP what f returns: an f that can fail stores its code outside
// The lists are explicit on purpose: every element of a list is a kernel in the code object, so a launcher names the forms
// that exist and nests the helpers only over arguments whose whole cross product exists.  f takes its argument BY VALUE
// (`auto np`): then `decltype(np)::value` is a constant expression inside it.  Needs nothing but <type_traits>.
#pragma once
#include <type_traits>

namespace ellhip {

template <int... Vs> struct Ints {};
template <class... Ts> struct OneOf {};

template <class F>
auto with_bool(bool b, F&& f) {
    return b ? f(std::true_type{}) : f(std::false_type{});
}

template <class... Ts, class Match, class F>
bool with_one_of(OneOf<Ts...>, Match&& match, F&& f) {
    return ((match(Ts{}) && (f(Ts{}), true)) || ...);
}

template <int... Vs, class F>
bool with_int(Ints<Vs...>, int v, F&& f) {
    return with_one_of(OneOf<std::integral_constant<int, Vs>...>{}, [v](auto c) { return c() == v; }, f);
}

}  // namespace ellhip
