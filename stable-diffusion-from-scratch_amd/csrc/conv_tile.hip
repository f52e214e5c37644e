// One compile part of the conv tile kernels: the build compiles this file once per part k = 1..5
// (-DSDK_CONV_PART=k, in parallel; one monolithic object took ~10 minutes) and each object expands exactly the
// launcher of its part, so a kernel template is instantiated only in the part whose sublist
// SDK_CONV_VARIANTS_Pk (conv.h) names its row.
#include "conv_tile.h"

#if !defined(SDK_CONV_PART) || SDK_CONV_PART < 1 || SDK_CONV_PART > 5
#error "conv_tile.hip: compile with -DSDK_CONV_PART=1..5"
#endif

namespace sdk {
namespace conv {

#define SDK_LAUNCH_CASE(P, ID, FAM, CF, DBG, PER_CU, GEGLU, NAME) \
    case ID: return launch_variant<Fam::FAM, CF, DBG>(p, s);
#define SDK_PART_FN(k) SDK_PART_FN_(k)   /* k is itself a macro (SDK_CONV_PART) */
#define SDK_PART_FN_(k) SDK_PART_DECL(k) {                                                              \
    switch (v) { SDK_CONV_VARIANTS_P##k(SDK_LAUNCH_CASE, k) }                                           \
    return fail(SDK_EINVAL, "conv2d: variant " + std::to_string(v) + " is not in this launcher part");  \
  }
SDK_PART_FN(SDK_CONV_PART)

}  // namespace conv
}  // namespace sdk
