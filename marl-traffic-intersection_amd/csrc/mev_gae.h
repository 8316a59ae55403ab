// mev_gae.h — one row of generalised advantage estimation (mev_gae, include/marlenv.h).
//
// The arithmetic is the header's, word for word: f32, multiply, then add, no fused operation (the
// tree is built with -ffp-contract=off and nothing here names an FMA), for one (e, i) and one t of
// the descending scan.  The device kernel (k_gae, mev_kernels.hip) and the host check
// (tests/native/gae_check.cpp) compile this text.
//
//   stop  = done | terminated;  cut = stop | truncated
//   nv    = stop ? 0 : V[t+1]
//   delta = (r + gamma * nv) - V[t]
//   adv   = cut ? delta : delta + c * adv_next            (c = gamma * lambda, rounded once by the caller)
//   masked: adv = 0, valid = 0
//   ret   = adv + V[t]
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MEV_GAE_HD __host__ __device__ __forceinline__
#else
#define MEV_GAE_HD static inline
#endif

namespace mev {

struct GaeRow {
    float adv, ret;
    uint8_t valid;
};

// r = r[t], v = V[t], v_next = V[t + 1]; done / terminated / truncated of row t (0 where the array is
// absent); masked: the MASK flag's condition for row t; adv_next: row t + 1's adv (0.0f at t = T - 1).
MEV_GAE_HD GaeRow gae_step(const float r, const float v, const float v_next, const uint8_t done, const uint8_t terminated,
                           const uint8_t truncated, const bool masked, const float gamma, const float c,
                           const float adv_next) {
    const bool stop = (done | terminated) != 0;
    const bool cut = stop || truncated != 0;
    const float nv = stop ? 0.0f : v_next;
    const float gnv = gamma * nv;
    const float target = r + gnv;
    const float delta = target - v;
    float adv = delta;
    if (!cut) {
        const float tail = c * adv_next;
        adv = delta + tail;
    }
    GaeRow o;
    o.valid = 1;
    if (masked) {
        adv = 0.0f;
        o.valid = 0;
    }
    o.adv = adv;
    o.ret = adv + v;
    return o;
}

}  // namespace mev
