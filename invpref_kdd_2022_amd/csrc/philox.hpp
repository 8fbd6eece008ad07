// philox.hpp -- the counter-based generator of the device-side draws (invpref_rank_stats.hip's bootstrap, neg_draw.hpp's
// negatives, the doubly robust and sampled-softmax draws): the same words for the same (counter, key) on every device and in
// the tests' numpy restatement.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace invpref {

// Philox4x32-10 (Salmon et al., SC 2011; Random123's constants)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&x)[4]) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    x[0] = c0; x[1] = c1; x[2] = c2; x[3] = c3;
}

}  // namespace invpref
