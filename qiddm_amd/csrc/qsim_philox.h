// qsim_philox.h -- Philox4x32-10 (Salmon et al., Random123) on the device: the one counter-based generator of the
// library.  Users: the noise field of the training launch (qsim_train.h, philox_normal), the sampled read-out of the
// density-matrix engines (qsim_mixed_shots.h) and the decisions of the trajectory engine (qsim_traj.h).  A value is a pure function of (counter, key): whichever thread, kernel
// or launch needs it derives the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace qiddm {

// ten rounds on the counter (c0, c1, c2, c3) under the key (k0, k1), in place: the four output words
__device__ __forceinline__ void philox4x32_10(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3, uint32_t k0,
                                              uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

}  // namespace qiddm
