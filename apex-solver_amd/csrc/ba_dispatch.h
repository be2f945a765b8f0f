// ba_dispatch.h -- host side of the bundle-adjustment launchers: the one place where their run-time choices (camera width,
// loss, a kernel's boolean forms) become template arguments.  Included only by the .hip files that launch BA kernels; each
// launcher names each kernel once, inside a generic lambda (as pg_kernels.hip does with its manifold and its view's loss).
#pragma once
#include <type_traits>

#include "pg_loss.hpp"

namespace apex {

// the one place a camera width becomes a type: f is called with std::integral_constant<int, 9> or <int, 6>
template <class F>
static inline void with_dc(int dc, F f) {
    if (dc == 9) f(std::integral_constant<int, 9>{});
    else f(std::integral_constant<int, 6>{});
}
// the one place a launcher's loss becomes a kernel's LOSS pack: f(*loss) for the general-loss instantiation, f() for the one
// that knows v.huber_delta only -- [&](auto... l) launches k<..., decltype(l)...> with l... in the kernel's loss slot
template <class F>
static inline void with_ba_loss(const PgLoss* loss, F f) {
    if (loss) f(*loss);
    else f();
}
// the one place a flag becomes a type (MASKED, WITH_SELF, REC, the queued layout): f(std::true_type) or f(std::false_type)
template <class F>
static inline void with_bool(bool b, F f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}
// No column group the factor has at this width is masked: mask_code (4 POSE + 2 LANDMARK + INTRINSIC) is 7 at d_c = 9, 6 at
// d_c = 6.  Invariant: d_c = 9 <=> the intrinsic bit of mask_code -- Solver's constructor derives dc_ from the low bit of
// mode_mask(mode) and its view carries mode_mask(mode), so a six-column handle has 6, 4 or 2 and a nine-column one 7, 5, 3 or 1.
static inline bool all_columns_free(int dc, int mask_code) { return mask_code == (dc == 9 ? 7 : 6); }

}  // namespace apex
