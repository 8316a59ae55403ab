// mev_beams.h — what the LiDAR derives from a handle's beam offsets alone, computed once on the
// host wherever the offsets are written (mev_create, mev_set_beam_angles) and read by the kernels
// from SimParams: the offsets do not change between steps, and the two IEEE divisions and the LDS
// reads they took at the head of every step's phase 3 are not step work.
//
// Phase 3b models the offsets as rel[b] = rel0 + b * dphi (SimParams::beam_cull says whether the
// list fits the model; when it does not, every beam is resolved against every box and dphi, idphi
// and period are not used).  The expressions are the ones the kernels evaluated, operation for
// operation in single precision, and the host is built like the device code without contraction,
// and both divisions are IEEE-correct on either side, so the fields should hold the bits the device
// computed.  What checks that is the GPU parity against the oracle (tests/test_lidar_hoist_gpu.py,
// tests/test_lidar_segments_gpu.py: a different beam range shows as a different LiDAR block);
// tests/native/lidar_prepass_check.cpp only holds the host expressions to this form.
#pragma once

#include "mev_math.h"

namespace mev {

struct BeamModel {
    float rel0;    // rel[0]
    float dphi;    // (rel[R-1] - rel[0]) / (R - 1); 1 for a single beam
    float idphi;   // 1 / dphi
    float period;  // beam indices per revolution: 2 pi * idphi
    float inv_r;   // 1 / R: a beam slot's agent as an exact float quotient (load_beam)
};

MEV_HD BeamModel beam_model(const float* rel, int R) {
    BeamModel m;
    m.rel0 = rel[0];
    m.dphi = R > 1 ? (rel[R - 1] - m.rel0) / (float)(R - 1) : 1.0f;
    m.idphi = 1.0f / m.dphi;
    m.period = 6.28318531f * m.idphi;
    m.inv_r = 1.0f / (float)R;
    return m;
}

}  // namespace mev
