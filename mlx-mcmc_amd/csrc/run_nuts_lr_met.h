// run_nuts_lr_met.h — the launch of k_nuts_lr's metric instantiations
// (nuts_lanes.h MET), compiled in run_nuts_lr_met.hip: a translation unit of
// its own so the six kernels build beside run_nuts.hip, not after it.
#pragma once
#include "host.h"

// A register-only program (run_nuts.hip lanes_register_only) with the metric
// buffer `metric`; `lds` dynamic LDS bytes (with the draw wave's buffers when
// `pw`), decided by mc_nuts_run_metric_lanes as launch_nuts_lr decides them.
int nuts_lr_met_launch(const mc_program* p, const mc_run_config* cfg, void* state, float* samples,
                       const mc_trace* tr, void* metric, int adapt, size_t lds, bool pw,
                       hipStream_t st);
