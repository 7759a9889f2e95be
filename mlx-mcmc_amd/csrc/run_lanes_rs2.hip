// run_lanes_rs2.hip — lane-resident HMC launches with 2 register slots per lane.
#include "run_lanes.h"

int hmc_lanes_rs2(const mc_program* p, const mc_run_config* cfg, void* state, float* samples,
                  const mc_trace* tr, void* ws, hipStream_t st) {
    return hmc_lanes_dispatch<2>(p, cfg, state, samples, tr, ws, st);
}

int hmc_dense_rs2(const mc_program* p, const mc_run_config* cfg, void* state, float* samples,
                  const mc_trace* tr, void* ws, hipStream_t st) {
    return launch_hmc_dense<2>(p, cfg, state, samples, tr, ws, st);
}

#ifdef MC_STAMPS
// the two-slot unit's accumulators: the dense 4 x 2 / 8 x 2 kernels (Large)
// and medium's one-wave kernel (scripts/stamps_lf.py)
MC_STAMPS_EXPORT(mc_debug_stamps_lanes2, mc_debug_stamps_lanes2_wg)
#endif
