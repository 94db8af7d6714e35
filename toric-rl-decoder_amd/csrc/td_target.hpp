// The learner's TD target of one state (Learner_mp.py:146-151 after the network forward), usable from host and device
// code like the lattice algebra: the kernel (k_td_target, kernels.hpp) and the header's unit test call the same two
// functions.
//
//   m = predictMaxOptimized's reduction (util_learner.py:96-110) of the state's (cnt, 3) Q-slice
//   y = clamp(reward + (1 - terminal) * discount * m, lo, hi)
//
// f32 throughout, with the roundings of the torch expression `reward + (~terminal).float() * discount * target`:
// ((1 - t) * discount) rounded, times m rounded, plus reward rounded -- never contracted into an FMA (the device
// path names the rounded operations; host code is built with -ffp-contract=off).
#pragma once
#include "lattice.hpp"

namespace tq {

// np.amax's step: a NaN on either side gives a NaN, two numbers give fmaxf's answer bit for bit.
TQ_HD float td_max(float a, float b) { return a != a ? a : (b != b ? b : fmaxf(a, b)); }

// max_q: the maximum over the slice (anything for an empty one); largest: the longest slice of the batch.  The
// reference pads every slice with zero rows up to the longest before the argmax (:98-100), so a shorter slice gets
// max(max_q, 0), which keeps a NaN maximum a NaN; a state without perspectives (terminal) gives 0 (:74-76,108).
TQ_HD float td_next_max(float max_q, int64_t cnt, int64_t largest) {
    if (cnt == 0) return 0.f;
    return (cnt < largest && max_q <= 0.f) ? 0.f : max_q;
}

TQ_HD float td_target_value(float reward, int terminal, float discount, float m, float lo, float hi) {
    const float live = terminal ? 0.f : 1.f;
#if defined(__HIP_DEVICE_COMPILE__)
    const float y = __fadd_rn(reward, __fmul_rn(__fmul_rn(live, discount), m));
#else
    const float g = live * discount;
    const float gm = g * m;
    const float y = reward + gm;
#endif
    return y < lo ? lo : (y > hi ? hi : y);
}

}  // namespace tq
