// run_nuts_lr_met.h — the launch of k_nuts_lr's metric instantiations
// (nuts_lanes.h MET), compiled in run_nuts_lr_met.hip: a translation unit of
// its own so the six kernels build beside run_nuts.hip, not after it.
#pragma once
#include "launch.h"

// A k_nuts_lr workgroup (run_nuts.hip nuts_lr_launch_shape): dynamic LDS bytes
// (with the draw wave's buffers when `pw`), the draw wave, threads
struct NutsLrShape {
    size_t lds;
    bool pw;
    int threads;
};

// A register-only program (run_nuts.hip lanes_register_only) with the metric
// buffer `metric`.
int nuts_lr_met_launch(const mc_program* p, const mc_run_config* cfg, void* state, float* samples,
                       const mc_trace* tr, void* metric, int adapt, const NutsLrShape& sh,
                       hipStream_t st);
