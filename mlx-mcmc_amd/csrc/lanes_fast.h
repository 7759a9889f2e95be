// lanes_fast.h — the lane-resident HMC kernel for "fast-form" programs
// (k_hmc_lf): the layout, exchange protocol and arithmetic of k_hmc_lr
// (lanes.h; reference hmc.py:7-206 per chain) with everything a fast-form
// program does not need compiled out.
//
// Fast form (host planner, plan_lanes.hip plan_lanes: LanePlan::fast): every slice
// holds at most one swept term — y ~ N(theta[g], scale), value data, loc the
// lane's private parameter, scale shared or constant: moment sums over the
// private parameter's elements — and at most one direct term — theta ~
// N(loc, scale), one element per parameter — and every scalar term is the
// "own" prior of one shared parameter.  The hierarchical models of BASELINE
// configs[2]/[3] and the isotropic / diagonal Gaussians of configs[1]/[4] are
// of this form.
//
// FORM (template): -1 reads the form from the terms at run time; FORM >= 0
// fixes it at compile time (bits LF_*; the planner sets LanePlan::form when
// every slice has the same terms and the shared roles are distinct
// parameters).  A compile-time form keys the record's cotangent items by
// *role* (swept scale, direct loc, direct scale) instead of by shared
// ordinal: no selects between them, and the lane that holds a role's total
// after the exchange holds that role's parameter.
//
// What differs from k_hmc_lr:
//   * the terms' fields, the lanes holding their shared operands and the
//     runs' data pointers are read once per launch;
//   * both chains' per-step arithmetic runs packed (v_pk_*_f32: the same
//     IEEE operations per chain, two chains per instruction), the per-launch
//     uniform values pinned in VGPRs (no SGPR spills reloaded per step);
//   * no step reads an observation: both moment sums of a run are closed
//     forms in the position about the run's centre c — sum (x - th) =
//     R + n (c - th), sum (x - th)^2 = Q + 2 (c - th) R + n (c - th)^2 — and
//     the data's share (c, R = sum (x - c), Q = sum (x - c)^2, n) is a table
//     the planner forms once per program (plan_lanes.hip lane_moments: float64
//     sums in element order, rounded once; lf_moments below): a regrouping of
//     the same sums, with a handful of roundings where a serial sum has one
//     per element, so the slice block is neither copied to LDS nor read;
//   * with nothing to sweep, a chain pair's slices need not be workgroups:
//     the dense launch (DN below) runs them as the waves of one workgroup;
//   * the wave totals of the record are reduce-scattered (permlane32 /
//     permlane16 swaps + one 16-lane DPP row sum) so that pair P's total is
//     in row perm[P % 4] of register P / 4 — no readlanes, no publish select;
//     the poll uses the same pair -> row map, so after the slice sums the
//     lane that holds shared slot (k, c) finds its cotangent total in its own
//     register (lane 16 perm[P % 4] + P / 4, P = 2 (k + 1) + c);
//   * the shared parameters' own priors enter slice 0's log-p record (one
//     add in the lane that holds the parameter, instead of a per-step
//     readlane sum over the shared parameters after the exchange);
//   * the kinetic-energy items K0 / K1 travel only on the first / last step;
//   * log p is evaluated, exchanged and summed on the last step only: a
//     leapfrog step needs the gradient alone, and the Hamiltonian of the
//     proposal (hmc.py:139-153) reads log p at the end of the trajectory, so
//     the intermediate steps' log-p items (their terms' log / normaliser
//     work, the records' lp pairs and their polls) were never used;
//   * the intermediate steps run two per loop trip (record-line parity 0 then
//     1, fixed publish / poll addresses, no copies of the carried state at
//     the latch), and the launch constants of the common layout are compiled
//     in (SPEC).
// Results equal k_hmc_lr's up to fp32 summation order; runs are
// bit-reproducible and independent of how chains are split over launches.
#pragma once
#include <type_traits>

#include "lanes.h"

namespace mc {

// compile-time term forms (FORM bits)
constexpr int LF_SW = 1;    // a swept term
constexpr int LF_SWS = 2;   //   its scale a shared parameter (else constant)
constexpr int LF_DIR = 4;   // a direct term
constexpr int LF_DM = 8;    //   its loc a shared parameter (else constant)
constexpr int LF_DS = 16;   //   its scale a shared parameter (else constant)
// the shared slots of a compile-time form: swept scale, direct loc, direct
// scale, in that order, for the roles present
constexpr int lf_slot_sws(int F) { return (void)F, 0; }
constexpr int lf_slot_dm(int F) { return (F & LF_SWS) ? 1 : 0; }
constexpr int lf_slot_ds(int F) { return lf_slot_dm(F) + ((F & LF_DM) ? 1 : 0); }
constexpr int lf_nroles(int F) { return lf_slot_ds(F) + ((F & LF_DS) ? 1 : 0); }
// launch constants fixed at compile time (SPEC bits; run_lanes.h resolves them)
constexpr int LFS_REP1 = 1;  // LrCtx::rep == 1: no replicated private parameter
constexpr int LFS_NOXF = 2;  // LrCtx::has_xf == 0: no transformed shared parameter

// pair P -> the row (16-lane group) that holds its total after the
// reduce-scatter / the slice sums: rows hold values 4n + {0, 2, 1, 3}
MC_DEV constexpr int lf_row(int P) { return (P & 3) == 1 ? 2 : ((P & 3) == 2 ? 1 : (P & 3)); }
// the lane that holds shared slot k of chain c
MC_DEV constexpr int lf_shlane(int k, int c) {
    return 16 * lf_row(2 * (k + 1) + c) + (2 * (k + 1) + c) / 4;
}
// Uniform (per chain) value `v` of shared slot k, chain c.
MC_DEV float lf_sh(float v, int k, int c) { return rl(v, lf_shlane(k, c)); }
// Both chains' values of shared slot k.
MC_DEV f2 lf_sh2(float v, int k) { return (f2){rl(v, lf_shlane(k, 0)), rl(v, lf_shlane(k, 1))}; }

// Keep a wave-uniform value in a VGPR: the kernel holds more uniform values
// than there are SGPRs, and a spilled SGPR costs a v_readlane at every use.
MC_DEV float vpin(float x) {
    asm volatile("" : "+v"(x));
    return x;
}
MC_DEV f2 vpin(f2 x) {
    asm volatile("" : "+v"(x));
    return x;
}
MC_DEV f2 bc2(float x) { return (f2){x, x}; }

// dpp_row (eval.h) without a seed register: every lane of a row has a source
// lane under these row controls, so the `old` operand is never read; leaving
// it unspecified spares the zero the other form materialises where the move
// is not folded into its add.
template <int CTRL>
MC_DEV float lf_dpp(float x) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), CTRL, 0xF, 0xF, true));
}

// Reduce-scatter of 8 per-lane values over the wave: returns two registers;
// row r of register n holds (in all 16 lanes) the wave total of value
// 4n + {0, 2, 1, 3}[r].  A fixed tree: the same bits in every wave / slice.
// Z01: values 0 and 1 carry nothing (an intermediate step has no log-p pair):
// v[0] and v[1] are not read, and rows 0 and 2 of x[0], where their totals
// would be, are unspecified; the three live pairs' totals are the same bits.
// (The 16-lane swap needs a partner register for w[1]: a dead one, the first
// half of the 32-lane swap that made w[1], not a zero materialised per step.)
template <bool Z01 = false>
MC_DEV void lf_rs8(const float (&v)[8], float (&x)[2]) {
    float w[4];
    uint32_t dead = 0;
#pragma unroll
    for (int m = Z01 ? 1 : 0; m < 4; ++m) {  // lanes 0-31: v[2m] sums, lanes 32-63: v[2m+1]
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[2 * m]),
                                                        __float_as_uint(v[2 * m + 1]), false, false);
        w[m] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
        if (m == 1) dead = r[0];
    }
#pragma unroll
    for (int n = 0; n < 2; ++n) {  // per 32-lane half: lanes 0-15 w[2n], 16-31 w[2n+1]
        const auto r = __builtin_amdgcn_permlane16_swap(
            (Z01 && n == 0) ? dead : __float_as_uint(w[2 * n]), __float_as_uint(w[2 * n + 1]),
            false, false);
        float t = __uint_as_float(r[0]) + __uint_as_float(r[1]);
        t += lf_dpp<0xB1>(t);
        t += lf_dpp<0x4E>(t);
        t += lf_dpp<0x141>(t);
        t += lf_dpp<0x140>(t);
        x[n] = t;
    }
}

// The moment sums of a run at the position th, from the run's constants
// (plan_lanes.hip lane_moments: LrCtx::mom, one float4 (c, R, Q, n) per slot
// and lane): about the centre c = (float) mean(x), with R = sum_e (x_e - c)
// and Q = sum_e (x_e - c)^2 (float64 sums in element order, rounded once) and
// d = c - th,
//   M1 = sum_e (x_e - th)   = R + n d           = fma(n, d, R)
//   M2 = sum_e (x_e - th)^2 = Q + 2 d R + n d^2 = fma(fma(n, d, 2 R), d, Q)
// exactly, so a step reads no observation: the constants depend on the data
// alone.  Both chains packed; the roundings are d, the fmas, and the
// constants' own.  Q and n d^2 are not negative and R is the small residual of
// the centring, so nothing cancels.  Non-finite or overflowing observations
// give non-finite constants and a non-finite log p (the proposal is rejected);
// bit equality with an element-by-element sum is not promised there.
struct LfMom {
    f2 c, R, R2, Q, n;  // (each a value broadcast to both chains; R2 = 2 R)
};
MC_DEV void lf_moments(const LfMom& m, f2 th, f2& M1, f2& M2) {
    const f2 d = m.c - th;
    M1 = pk_fma(m.n, d, m.R);
    M2 = pk_fma(pk_fma(m.n, d, m.R2), d, m.Q);
}

// The job map of the block-wide draws (k_hmc_lf draw_block): with NBk =
// ceil(D / 4) momentum blocks per chain, job t < 2 NBk is momentum block
// t % NBk of chain t / NBk, jobs 2 NBk and 2 NBk + 1 are the accept draws of
// chains 0 and 1; a thread of `lanes` takes jobs tid, tid + lanes, ...
struct LfDrawJob {
    bool acc;  // an accept draw (else a momentum block)
    int c, b;  // chain of the pair, Philox block
};
constexpr int lf_draw_jobs(int D) { return 2 * ((D + 3) / 4) + 2; }
constexpr LfDrawJob lf_draw_job(int t, int D) {
    const int NBk = (D + 3) / 4;
    const bool acc = t >= 2 * NBk;
    const int c = acc ? t - 2 * NBk : (t >= NBk ? 1 : 0);
    return {acc, c, acc ? 0 : t - (c ? NBk : 0)};
}
// every (chain, block) and both accept draws are taken exactly once
constexpr bool lf_draw_jobs_once(int D, int lanes) {
    const int NBk = (D + 3) / 4;
    int mom[2][257] = {}, acc[2] = {};
    if (NBk > 257) return false;
    for (int tid = 0; tid < lanes; ++tid)
        for (int t = tid; t < lf_draw_jobs(D); t += lanes) {
            const LfDrawJob jb = lf_draw_job(t, D);
            if (jb.c < 0 || jb.c > 1 || jb.b < 0 || jb.b >= NBk) return false;
            if (jb.acc) ++acc[jb.c];
            else ++mom[jb.c][jb.b];
        }
    for (int c = 0; c < 2; ++c) {
        if (acc[c] != 1) return false;
        for (int b = 0; b < NBk; ++b)
            if (mom[c][b] != 1) return false;
    }
    return true;
}
static_assert(lf_draw_jobs(1000) == 502 && lf_draw_jobs(1027) == 516, "Large: one trip of 512");
static_assert(lf_draw_jobs_once(4, 64) && lf_draw_jobs_once(4, 256) && lf_draw_jobs_once(4, 512) &&
              lf_draw_jobs_once(5, 64) && lf_draw_jobs_once(5, 256) && lf_draw_jobs_once(5, 512) &&
              lf_draw_jobs_once(303, 64) && lf_draw_jobs_once(303, 256) &&
              lf_draw_jobs_once(303, 512) && lf_draw_jobs_once(1000, 64) &&
              lf_draw_jobs_once(1000, 256) && lf_draw_jobs_once(1000, 512) &&
              lf_draw_jobs_once(1024, 64) && lf_draw_jobs_once(1024, 256) &&
              lf_draw_jobs_once(1024, 512) && lf_draw_jobs_once(1027, 64) &&
              lf_draw_jobs_once(1027, 256) && lf_draw_jobs_once(1027, 512),
              "the block-wide draws' job map");

// The fast-form terms of a slice, read once per launch: at most one swept
// term (y ~ N(theta[g], scale): value data, loc private, scale shared or
// constant) and one direct term (theta ~ N(loc, scale), loc / scale shared or
// constant).  Shared operands are named by their shared ordinals.
struct LfTerms {
    bool sw, dir;
    // swept term
    float sw_w, sw_c0, sw_cinv, sw_cinv2, sw_clogs;
    bool sw_shs;
    int sw_ks;           // shared ordinal of the scale (or -1)
    // direct term
    float d_w, d_c0, d_m, d_cinv, d_cinv2, d_clogs;
    bool d_shm, d_shs;
    int d_km, d_ks;      // shared ordinals of loc / scale (or -1)
};

MC_DEV LfTerms lf_terms(const MC_CONST LrTerm* tt, int nsweep, int ndirect) {
    LfTerms F;
    F.sw = nsweep > 0;
    F.dir = ndirect > 0;
    const MC_CONST LrTerm* T = tt;
    F.sw_w = F.sw ? T->weight : 0.f;
    F.sw_c0 = F.sw ? T->c0 : 0.f;
    F.sw_cinv = F.sw ? T->cinv : 0.f;
    F.sw_cinv2 = F.sw ? T->cinv2 : 0.f;
    F.sw_clogs = F.sw ? T->clogs : 0.f;
    F.sw_shs = F.sw && T->kind[2] == SK_SHARED;
    F.sw_ks = F.sw_shs ? T->jsh[2] : -1;
    const MC_CONST LrTerm* U = tt + nsweep;
    F.d_w = F.dir ? U->weight : 0.f;
    F.d_c0 = F.dir ? U->c0 : 0.f;
    F.d_m = F.dir ? U->cval[1] : 0.f;
    F.d_cinv = F.dir ? U->cinv : 0.f;
    F.d_cinv2 = F.dir ? U->cinv2 : 0.f;
    F.d_clogs = F.dir ? U->clogs : 0.f;
    F.d_shm = F.dir && U->kind[1] == SK_SHARED;
    F.d_shs = F.dir && U->kind[2] == SK_SHARED;
    F.d_km = F.d_shm ? U->jsh[1] : -1;
    F.d_ks = F.d_shs ? U->jsh[2] : -1;
    return F;
}

// NSH: shared slots of the record (FORM >= 0: lf_nroles(FORM)).
// XL: the host found every exchange group's workgroups on one XCD
// (host.h xcd_round_robin): records are published with L2-resident stores
// (sliced.h granule_store_xcd), after an in-kernel check of the placement.
// SPEC: launch constants the host resolved (LFS_* bits): their uniform
// branches, live masks and scalar registers are compiled out; 0 reads them
// all at run time.  (The own prior's kind needs no such bit: see o_m below.)
// DN > 0 — the dense launch (run_lanes.h launch_hmc_dense): a workgroup is one
// chain pair and its wave w is slice w of DN = NW slices (the plan's S).  The
// records are exchanged through LDS — a line of 16 floats per (parity, slice),
// one workgroup barrier per step — so there are no tags, spins, timeout,
// workspace or co-residency requirement: every wave of the block runs the
// same steps and iterations (dead chains are clamped, not skipped) and the
// kernel has no early return, so every barrier is reached by all waves.
template <int RS, int NSH, int NW, bool X1, int FORM, bool XL = false, int SPEC = 0, int DN = 0>
__global__ void __launch_bounds__(64 * NW)
k_hmc_lf(LrCtx P, RunArgs A, int64_t chain_base, int64_t n_groups, mc_chain_scalars* scal,
         float* st_q, float* st_g, float* samples, TraceDev tr, unsigned long long* xch,
         int* status, uint32_t ebase) {
    static_assert(NSH <= kLrMaxShared, "shared parameters");
    constexpr bool CF = FORM >= 0;      // the form is fixed at compile time
    static_assert(!CF || lf_nroles(FORM) == NSH, "record slots of a compile-time form");
    constexpr bool DENSE = DN > 0;
    static_assert(!DENSE || (DN == NW && DN >= 2 && DN <= kLrSlices && !X1 && !XL),
                  "dense: wave w is slice w, records through LDS");
    // chains per block: wave w owns chains 2w, 2w + 1 (dense: the block's one pair)
    constexpr int NB = DENSE ? 2 : 2 * NW;
    constexpr int NV = 2 * (NSH + 1);   // per-step pairs: lp and the shared cotangents
    constexpr int NPAIR = NV + 4;       // + K0 (first step) and K1 (last step)
    constexpr int NPASS = (NPAIR + 3) / 4, NPASS_V = (NV + 3) / 4;
    constexpr int NRS = (NV + 7) / 8;   // reduce-scatter calls per step
    if (!X1 && !DENSE && A.fault && blockIdx.x == gridDim.x - 1)
        return;  // test hook: never publishes
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const mc_run_config& cfg = A.cfg;
    const int tid = threadIdx.x;
    const int wave = tid >> 6, j = tid & 63;
    const int S = DENSE ? DN : P.S, D = P.D, Dsh = P.Dsh;
    int64_t grp;
    int slice;
    if constexpr (DENSE) {
        grp = blockIdx.x;
        slice = wave;
    } else {
        const int64_t w = blockIdx.x, nwg = gridDim.x;
        if (nwg % 8 == 0 && (nwg / 8) % S == 0) {  // a block's slices share an XCD (speed only)
            const int64_t x = w & 7, r = w >> 3;
            grp = x * ((nwg / 8) / S) + r / S;
            slice = (int)(r % S);
        } else {
            grp = w / S;
            slice = (int)(w % S);
        }
    }
    const int64_t C = cfg.num_chains;
    const int64_t cbase = chain_base + grp * NB;
    const int b0 = DENSE ? 0 : 2 * wave;
    int64_t cc[2];
    bool live[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        live[c] = cbase + b0 + c < C;
        cc[c] = min(cbase + b0 + c, C - 1);
    }

    // LDS: (dense: the record lines [parity][slice][16], then) the scalar
    // terms.  The slice block stays in global memory: a step reads no
    // observation (lf_moments), and the run lengths come with the constants.
    float* const xl = smem;
    const int64_t* blk = P.blocks + 4 * (int64_t)slice;
    const float* gd = P.data + blk[0];
    const int nsweep = (int)(blk[3] & 255);
    const int ndirect = (int)((blk[3] >> 8) & 255);
    LrSterm* sst = (LrSterm*)(smem + (DENSE ? 2 * DN * 16 : 0));
    for (int i = tid; i < P.n_sterms * (int)(sizeof(LrSterm) / 16); i += 64 * NW)
        ((float4*)sst)[i] = ((const float4*)P.sterms)[i];

    const MC_CONST LrTerm* tt = cptr(P.terms) + (int64_t)slice * P.n_terms;
    const LfTerms F = lf_terms(tt, nsweep, ndirect);
    // the form, folded to constants when FORM >= 0
    const bool SW = CF ? (FORM & LF_SW) != 0 : F.sw;
    const bool SWS = CF ? (FORM & LF_SWS) != 0 : F.sw_shs;
    const bool DIR = CF ? (FORM & LF_DIR) != 0 : F.dir;
    const bool DM = CF ? (FORM & LF_DM) != 0 : F.d_shm;
    const bool DS = CF ? (FORM & LF_DS) != 0 : F.d_shs;
    // the shared slot of each role: its role index (compile-time form) or its
    // shared ordinal (run-time form)
    const int ksw = CF ? lf_slot_sws(FORM) : max(F.sw_ks, 0);
    const int kdm = CF ? lf_slot_dm(FORM) : max(F.d_km, 0);
    const int kds = CF ? lf_slot_ds(FORM) : max(F.d_ks, 0);
    const int nsl = CF ? NSH : Dsh;  // shared slots
    // shared ordinal of slot k
    auto ord_of = [&](int k) {
        int o = F.d_ks;  // selects, not an indexed read of F (scratch)
        o = (DM && k == kdm) ? F.d_km : o;
        o = (SWS && k == ksw) ? F.sw_ks : o;
        return CF ? o : k;
    };
    // this lane's shared slot: (xk, xc) with lf_shlane(xk, xc) == j
    int xk = -1, xc = 0;
#pragma unroll
    for (int k = 0; k < kLrMaxShared; ++k)
#pragma unroll
        for (int c = 0; c < 2; ++c)
            if (k < nsl && lf_shlane(k, c) == j) {
                xk = k;
                xc = c;
            }
    const bool xon = xk >= 0;
    const int xo = xon ? ord_of(xk) : 0;  // its shared ordinal
    int xg = P.shl[0];
#pragma unroll
    for (int k = 1; k < kLrMaxShared; ++k) xg = (xo == k) ? P.shl[k] : xg;
    const int64_t xch_id = xc ? cc[1] : cc[0];
    const bool xlive = xon && (xc ? live[1] : live[0]);
    // lanes per private parameter (lanes.h); 1 at compile time under LFS_REP1
    const int rep = (SPEC & LFS_REP1) ? 1 : P.rep;
    const bool lead = (j & (rep - 1)) == 0;  // this lane counts its parameters
    // a transformed shared parameter (lanes.h LrCtx::shxf) and the identity
    // terms over its raw value: a uniform branch, so programs without them
    // run the same instructions as before (none of them under LFS_NOXF)
    const bool hxf = (SPEC & LFS_NOXF) ? false : P.has_xf != 0;
    int xxf = P.shxf[0];
    float xid = P.shid[0];
#pragma unroll
    for (int k = 1; k < kLrMaxShared; ++k) {
        xxf = (xo == k) ? P.shxf[k] : xxf;
        xid = (xo == k) ? P.shid[k] : xid;
    }
    xxf = xon ? xxf : MC_XF_NONE;
    xid = xon ? xid : 0.0f;

    LrPriv<RS> R0;  // (loaded as in k_hmc_lr, then packed per slot)
    int gk[RS];
    f2 q[RS], p[RS], g[RS];
#pragma unroll
    for (int r = 0; r < RS; ++r) {
        gk[r] = P.gidx[((int64_t)slice * kLrMaxSlots + r) * 64 + j];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            R0.q[r][c] = gk[r] >= 0 ? st_q[cc[c] * D + gk[r]] : 0.0f;
            R0.g[r][c] = gk[r] >= 0 ? st_g[cc[c] * D + gk[r]] : 0.0f;
        }
        q[r] = (f2){R0.q[r][0], R0.q[r][1]};
        g[r] = (f2){R0.g[r][0], R0.g[r][1]};
        p[r] = (f2){0.f, 0.f};
    }
    // the lane RNG plan (plan_lanes.hip plan_lane_rng), when the planner made one
    const bool rngp = P.rng != nullptr;
    int4 rw = {0, 0, 0, 0};
    if (rngp) rw = P.rng[(int64_t)slice * 64 + j];
    const int racc0 = __builtin_amdgcn_readfirstlane((rw.w >> 8) & 63);
    const int racc1 = __builtin_amdgcn_readfirstlane((rw.w >> 14) & 63);
    // the lane holding this lane's shared parameter's Philox block (chain xc)
    int sh_src = 0;
    if (rngp) {
        const int target = (xc + 1) | ((xg >> 2) << 3);
        for (int i = 0; i < 64; ++i)
            sh_src = (__builtin_amdgcn_readlane(rw.x, i) == target) ? i : sh_src;
    }
    LrShared sh;
    sh.q = xon ? st_q[xch_id * D + xg] : 1.0f;
    sh.g = xon ? st_g[xch_id * D + xg] : 0.0f;
    sh.p = 0.0f;
    sh.v = hxf ? xf_apply(xxf, sh.q) : sh.q;
    sh.is = sh.iv = 1.0f;
    sh.lg = 0.0f;
    double eps[2];
    f2 lp;
    int nacc[2], ntot[2], wacc[2], wtot[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        eps[c] = scal[cc[c]].step_size;
        lp[c] = scal[cc[c]].logp;
        nacc[c] = scal[cc[c]].n_accept;
        ntot[c] = scal[cc[c]].n_total;
        wacc[c] = scal[cc[c]].warmup_accept;
        wtot[c] = scal[cc[c]].warmup_total;
    }
    // Block-wide draws (LrCtx::blk_rng: a dense plan without a lane RNG plan).
    // An iteration needs NBk = ceil(D / 4) momentum blocks per chain and one
    // accept draw per chain, dealt to the threads by lf_draw_job (Large: 502
    // jobs on 512 lanes, one trip).  A job is one Philox block
    // and both Box-Muller pairs of it (mc_box_muller_log of the first
    // uniform's log: the bits of mc_box_muller, philox.h), written as one
    // float4 to z[c][4 b ..]; an accept job's first log is the accept log
    // (mc_logf_unit of the accept uniform, as mc_logf_u01).  These are the
    // counters and functions of the per-lane draws below (normal_of), so
    // every lane reads the bits it would have drawn.  LDS, after the scalar
    // terms, per iteration parity: z[2][4 NBk] and the two accept logs.  The
    // draws of iteration it + 1 are made by the last step of iteration it,
    // between its publish and its barrier, into the other parity's buffer:
    // that buffer was last read at the start of iteration it - 1, before a
    // barrier every wave has passed (with L = 1 too: that iteration's one
    // step), so no barrier is added; the launch's first iteration is drawn
    // ahead of the barrier below.
    // Compiled into the dense launches' instantiations alone (run_lanes.h
    // launch_hmc_dense), and of the one-wave kernels only the four-slot one,
    // whose plans (more than 128 parameters) never have a lane RNG plan: the
    // one-slot kernel's always have one, and the code would cost it its third
    // wave per SIMD (167 -> 182 VGPRs); the two-slot kernel (medium) lacks one
    // only at 117 .. 128 parameters, and keeps the per-lane draws there.
    constexpr bool BDRAW = (DENSE || (X1 && RS == 4)) &&
                           FORM == (LF_SW | LF_SWS | LF_DIR | LF_DM | LF_DS) &&
                           SPEC == (LFS_REP1 | LFS_NOXF);
    const bool bdraw = BDRAW && P.blk_rng != 0;
    const int NBk = (D + 3) >> 2;
    const int ZB = 8 * NBk + 4;  // floats per parity
    static_assert(sizeof(LrSterm) % 16 == 0, "the draws' float4 stores follow the scalar terms");
    float* const zl = (float*)sst + P.n_sterms * (int)(sizeof(LrSterm) / 4);
    auto draw_block = [&](int64_t itd) {
        float* const zb = zl + (int)(itd & 1) * ZB;
        for (int t = tid; t < lf_draw_jobs(D); t += 64 * NW) {
            const LfDrawJob jb = lf_draw_job(t, D);
            const bool acl = jb.acc;
            const int c = jb.c, b = jb.b;
            const mc_u32x4 rr =
                mc_draw(cfg.seed, (uint32_t)(cfg.chain_offset + (c ? cc[1] : cc[0])),
                        (uint32_t)itd, acl ? MC_RNG_TAG_ACCEPT : MC_RNG_TAG_MOMENTUM, 0,
                        acl ? 0u : (uint32_t)b);
            const float la = mc_logf_unit(acl ? mc_u01_f32(rr.x) : mc_u01_boxf(rr.x));
            const float lb = mc_logf_unit(mc_u01_boxf(rr.z));
            float4 z;
            mc_box_muller_log(la, rr.y, &z.x, &z.y);
            mc_box_muller_log(lb, rr.w, &z.z, &z.w);
            if (acl) zb[8 * NBk + c] = la;
            else *(float4*)(zb + 4 * (c * NBk + b)) = z;
        }
    };
    if constexpr (BDRAW) {
        if (bdraw && cfg.iter_count > 0) draw_block(cfg.iter_begin);
    }
    MC_STAMP_INIT
    __syncthreads();  // the scalar terms (and the first iteration's draws) are in LDS

    // the lane's own prior (lr_own_prior keys it by ordinal); it enters
    // slice 0's log-p record through this lane
    const LrOwn own = lr_own_prior(P.n_sterms, sst, xon ? 2 * xo + xc : 64, Dsh);
    const bool own_lp0 = own.on && slice == 0 && xc == 0;
    const bool own_lp1 = own.on && slice == 0 && xc == 1;
    // (a HalfNormal prior measures from 0: its loc is held as +0, and v - (+0)
    // is v bit for bit, so the step's d = v - o_m needs no select on the kind)
    const float o_m = vpin(own.hn ? 0.0f : own.m), o_cinv2 = vpin(own.cinv2),
                o_c0l = vpin(own.c0l), o_wn = vpin(own.wn);
    // the own prior's gradient at the shared parameter's value v: it depends on
    // v alone, so it is formed where v is (drift_shared), off the path from
    // the poll to the next position
    auto own_grad = [&](float v) {
        const float d = v - o_m;
        const bool out = own.hn && !(v >= 0.0f);
        return (out || !own.on) ? 0.0f : o_wn * -(d * o_cinv2);
    };
    // per slot: the swept term's run — its constants and element count
    // (LrCtx::mom) — and the direct term's presence
    int len[RS];
    f2 cnt[RS];
    LfMom mom[RS];
    bool pdir[RS];
#pragma unroll
    for (int r = 0; r < RS; ++r) {
        float4 m = {0.f, 0.f, 0.f, 0.f};
        if (SW && r < tt[0].nslot) m = P.mom[((int64_t)slice * kLrMaxSlots + r) * 64 + j];
        len[r] = (int)m.w;
        cnt[r] = bc2(m.w);
        mom[r].c = vpin(bc2(m.x));
        mom[r].R = vpin(bc2(m.y));
        mom[r].R2 = vpin(bc2(m.y + m.y));
        mom[r].Q = vpin(bc2(m.z));
        mom[r].n = cnt[r];
        pdir[r] = DIR && r < tt[nsweep].nslot &&
                  ((const int32_t*)gd)[tt[nsweep].len_off + r * 64 + j] > 0;
    }
    // the terms' constants, pinned in VGPRs
    const f2 sw_w = vpin(bc2(F.sw_w)), sw_c0 = vpin(bc2(F.sw_c0));
    const f2 sw_cinv = vpin(bc2(F.sw_cinv)), sw_cinv2 = vpin(bc2(F.sw_cinv2)),
             sw_clogs = vpin(bc2(F.sw_clogs));
    const f2 d_w = vpin(bc2(F.d_w)), d_c0 = vpin(bc2(F.d_c0)), d_m = vpin(bc2(F.d_m));
    // (one slot: the direct term's weight per lane, zero where the lane's
    // parameter has no direct term)
    const f2 d_w1 = vpin(bc2(pdir[0] ? F.d_w : 0.0f));
    const f2 d_cinv = vpin(bc2(F.d_cinv)), d_cinv2 = vpin(bc2(F.d_cinv2)),
             d_clogs = vpin(bc2(F.d_clogs));
    const f2 half = bc2(0.5f), one = bc2(1.0f);
    const float lp_const = vpin(P.lp_const);
    const int L = cfg.num_leapfrog_steps;
    uint32_t epoch = ebase;  // tags continue across launches (host.h ws_reserve)
    bool ok = true;
    // one 128-byte line per (wave, slice) record; lanes publish the pairs
    // they hold after the reduce-scatter, pass ps of the poll reads pair
    // 4 ps + perm[lane / 16] of slice lane % 16
    unsigned long long* gline[2];
#pragma unroll
    for (int par = 0; par < 2; ++par)
        gline[par] = DENSE ? nullptr
                           : xch + (((int64_t)par * n_groups + grp) * (NB / 2) + wave) * S * 16;
    const int row = j >> 4, col = j & 15;
    const bool poll_lane = col < S;
    // the poll address of pass 0 (pass ps: + 4 ps), per epoch parity
    unsigned long long* gp[2];
#pragma unroll
    for (int par = 0; par < 2; ++par)
        gp[par] = DENSE ? nullptr : gline[par] + min(col, S - 1) * 16 + lf_row(row);
    // dense: the same lines in LDS, a float per pair (no tags), [parity][slice][16]
    const int lpoll = min(col, S - 1) * 16 + lf_row(row);
    auto lput = [&](int par, int off, float v) { xl[par * (DN * 16) + off] = v; };
    // publishing: lanes 16 r + n (n < NRS * 2) hold pair 8 (n / 2) + 4 (n % 2) + perm[r]
    const int pub_pair = (col < 2 * NRS) ? 8 * (col >> 1) + 4 * (col & 1) + lf_row(row) : -1;
    const bool pub_rec = pub_pair >= 0 && pub_pair < NV;
    // an intermediate step's store: the pairs past the log-p pair, at their
    // granule of either parity's line
    const bool pub_mid = pub_rec && pub_pair >= 2;
    const int pub_x = 2 * (col >> 1) + (col & 1);
    const int pub_off = slice * 16 + max(pub_pair, 0);
    // poll passes by kind: record pairs every step, K0 / K1 pairs on the first / last
    uint32_t need_v = 0, need_lp = 0, need_k0 = 0, need_k1 = 0;
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps) {
        const int pr = 4 * ps + lf_row(row);
        if (X1 || !poll_lane || pr >= NPAIR) continue;
        if (pr < 2) need_lp |= 1u << ps;  // the log-p pairs: last step only
        else if (pr < NV) need_v |= 1u << ps;
        else if (pr < NV + 2) need_k0 |= 1u << ps;
        else need_k1 |= 1u << ps;
    }
    // XL: check that the block's slices share an XCD (sliced.h xcd_announce /
    // xcd_agree) before the first publish.  The check's granules: granule 15
    // of each slice's parity-0 line of wave 0 (record pairs use 0 .. NPAIR - 1
    // < 15); its tag ebase + 1 is never 0, the value of a freshly cleared
    // line (the steps' tags start there too, on the record granules).  Its
    // loads are issued here and completed after the first drift.
    constexpr bool xchk = XL && !X1;
    unsigned long long* const xslots = xch + ((int64_t)grp * (NB / 2)) * S * 16 + 15;
    XcdPoll xpoll = {0ull};
    if (xchk && cfg.iter_count > 0)
        xpoll = xcd_announce(xslots, S, slice, ebase + 1, wave == 0 && j == 0);
    static_assert(NPAIR <= 15, "granule 15 of a record line is the XCD handshake's");
    const int64_t it_end = cfg.iter_begin + cfg.iter_count;
    // The lane RNG plan's draws of iteration `itd` (plan_lanes.hip plan_lane_rng):
    // this lane's Philox block — a momentum block of one chain or a chain's
    // accept draw — and both Box-Muller pairs of it; the accept lanes' first
    // log is the accept log (mc_logf_unit of the same uniform transform the
    // per-lane path uses); the normals are fetched from their lanes.  They
    // depend on the counters alone, so an iteration's are drawn while the
    // last step of the iteration before waits for its exchange (nothing else
    // covers that wait: no drift follows the last step), the launch's first
    // ahead of the loop — in the kernels of the Large shape's layout
    // (DRAW_AHEAD: one slot, a compile-time form, one lane per parameter); every
    // other instantiation draws at the iteration's start, as before.
    constexpr bool DRAW_AHEAD = RS == 1 && CF && (SPEC & LFS_REP1) != 0;
    f2 nx_z[RS];
    float nx_sh = 0.0f, nx_lu[2] = {0.f, 0.f};
#pragma unroll
    for (int r = 0; r < RS; ++r) nx_z[r] = (f2){0.f, 0.f};
    auto draw_plan = [&](int64_t itd) {
        const int kind = rw.x & 7;
        const bool acl = kind >= 3;
        const int csel = (kind == 2 || kind == 4) ? 1 : 0;
        const mc_u32x4 rr =
            mc_draw(cfg.seed, (uint32_t)(cfg.chain_offset + (csel ? cc[1] : cc[0])),
                    (uint32_t)itd, acl ? MC_RNG_TAG_ACCEPT : MC_RNG_TAG_MOMENTUM, 0,
                    acl ? 0u : ((uint32_t)rw.x >> 3));
        const float la = mc_logf_unit(acl ? mc_u01_f32(rr.x) : mc_u01_boxf(rr.x));
        const float lb = mc_logf_unit(mc_u01_boxf(rr.z));
        float z[4];
        mc_box_muller_log(la, rr.y, &z[0], &z[1]);
        mc_box_muller_log(lb, rr.w, &z[2], &z[3]);
        nx_lu[0] = rl(la, racc0);
        nx_lu[1] = rl(la, racc1);
        auto fetch = [&](int src, int comp) {
            float v = __shfl(z[0], src);
            const float v1 = __shfl(z[1], src), v2 = __shfl(z[2], src), v3 = __shfl(z[3], src);
            v = comp == 1 ? v1 : v;
            v = comp == 2 ? v2 : v;
            return comp == 3 ? v3 : v;
        };
#pragma unroll
        for (int r = 0; r < RS; ++r) {
            const int word = (r < 2 ? rw.y : rw.z) >> (14 * (r & 1));
            const int comp = (word >> 12) & 3;
            nx_z[r] = (f2){fetch(word & 63, comp), fetch((word >> 6) & 63, comp)};
        }
        nx_sh = fetch(sh_src, xg & 3);
    };
    if (DRAW_AHEAD && rngp && cfg.iter_count > 0) draw_plan(cfg.iter_begin);
    for (int64_t it = cfg.iter_begin; it < it_end && ok; ++it) {
        MC_STAMP_DECL
        const bool warm = it < cfg.num_warmup;
        float hs[2], es[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (it == cfg.num_warmup) {  // hmc.py:175-180
                wacc[c] = nacc[c];
                wtot[c] = ntot[c];
                nacc[c] = 0;
                ntot[c] = 0;
            }
            hs[c] = (float)(0.5 * eps[c]);
            es[c] = (float)eps[c];
        }
        const f2 h = vpin((f2){hs[0], hs[1]}), e = vpin((f2){es[0], es[1]});
        const float xh = vpin(xc ? hs[1] : hs[0]), xe = vpin(xc ? es[1] : es[0]);
        // momentum: parameter g takes normal g % 4 of Philox block g / 4
        auto normal_of = [&](int gi, int64_t chain) {
            const mc_u32x4 rr = mc_draw(cfg.seed, (uint32_t)(cfg.chain_offset + chain),
                                        (uint32_t)it, MC_RNG_TAG_MOMENTUM, 0, (uint32_t)(gi >> 2));
            float z0, z1;
            if ((gi & 3) < 2) mc_box_muller(rr.x, rr.y, &z0, &z1);
            else mc_box_muller(rr.z, rr.w, &z0, &z1);
            return (gi & 1) ? z1 : z0;
        };
        f2 k0p = {0.f, 0.f};
        float logu_acc[2] = {0.f, 0.f};  // the chains' accept logs (lane RNG plan)
        if (rngp) {
            if constexpr (DRAW_AHEAD) {
                // this iteration's draws, made by draw_plan at the launch's
                // start or in the shadow of the last exchange of the
                // iteration before
                logu_acc[0] = nx_lu[0];
                logu_acc[1] = nx_lu[1];
#pragma unroll
                for (int r = 0; r < RS; ++r) {
                    if (gk[r] < 0) continue;  // (an empty slot's p stays 0: its g is always 0)
                    p[r] = nx_z[r];
                    if (lead) k0p += nx_z[r] * nx_z[r];
                }
                sh.p = xon ? nx_sh : 0.0f;
            } else {
                // the lane RNG plan (plan_lanes.hip plan_lane_rng): this lane's Philox
                // block — a momentum block of one chain or a chain's accept draw —
                // and both Box-Muller pairs of it; the accept lanes' first log is
                // the accept log (mc_logf_unit of the same uniform transform the
                // per-lane path uses); the normals are fetched from their lanes
                const int kind = rw.x & 7;
                const bool acl = kind >= 3;
                const int csel = (kind == 2 || kind == 4) ? 1 : 0;
                const mc_u32x4 rr =
                    mc_draw(cfg.seed, (uint32_t)(cfg.chain_offset + (csel ? cc[1] : cc[0])),
                            (uint32_t)it, acl ? MC_RNG_TAG_ACCEPT : MC_RNG_TAG_MOMENTUM, 0,
                            acl ? 0u : ((uint32_t)rw.x >> 3));
                const float la = mc_logf_unit(acl ? mc_u01_f32(rr.x) : mc_u01_boxf(rr.x));
                const float lb = mc_logf_unit(mc_u01_boxf(rr.z));
                float z[4];
                mc_box_muller_log(la, rr.y, &z[0], &z[1]);
                mc_box_muller_log(lb, rr.w, &z[2], &z[3]);
                logu_acc[0] = rl(la, racc0);
                logu_acc[1] = rl(la, racc1);
                auto fetch = [&](int src, int comp) {
                    float v = __shfl(z[0], src);
                    const float v1 = __shfl(z[1], src), v2 = __shfl(z[2], src), v3 = __shfl(z[3], src);
                    v = comp == 1 ? v1 : v;
                    v = comp == 2 ? v2 : v;
                    return comp == 3 ? v3 : v;
                };
    #pragma unroll
                for (int r = 0; r < RS; ++r) {
                    const int word = (r < 2 ? rw.y : rw.z) >> (14 * (r & 1));
                    const int comp = (word >> 12) & 3;
                    const f2 zz = {fetch(word & 63, comp), fetch((word >> 6) & 63, comp)};
                    if (gk[r] < 0) continue;  // (an empty slot's p stays 0: its g is always 0)
                    p[r] = zz;
                    if (lead) k0p += zz * zz;
                }
                const float zs = fetch(sh_src, xg & 3);
                sh.p = xon ? zs : 0.0f;
            }
        } else if (bdraw) {
            // the block-wide draws of this iteration (draw_block), published
            // by the barrier of the step that made them (one wave: this one)
            if constexpr (X1) __syncthreads();
            const float* const zb = zl + (int)(it & 1) * ZB;
            logu_acc[0] = zb[8 * NBk];
            logu_acc[1] = zb[8 * NBk + 1];
#pragma unroll
            for (int r = 0; r < RS; ++r) {
                const int gi = max(gk[r], 0);
                const f2 z = {zb[gi], zb[4 * NBk + gi]};
                if (gk[r] >= 0) {  // (an empty slot's p stays 0: its g is always 0)
                    p[r] = z;
                    if (lead) k0p += z * z;
                }
            }
            const float zs = zb[(xc ? 4 * NBk : 0) + xg];
            sh.p = xon ? zs : 0.0f;
        } else {
#pragma unroll
            for (int r = 0; r < RS; ++r) {
                if (gk[r] < 0) continue;  // (an empty slot's p stays 0: its g is always 0)
                const f2 z = {normal_of(gk[r], cc[0]), normal_of(gk[r], cc[1])};
                p[r] = z;
                if (lead) k0p += z * z;
            }
            sh.p = xon ? normal_of(xg, xch_id) : 0.0f;
        }
        const float K0w[2] = {wave_sum(k0p[0]), wave_sum(k0p[1])};
        float k0s[2] = {0.f, 0.f};  // the shared parameters' part, in slot order
        {
            const float p2 = sh.p * sh.p;
            for (int k = 0; k < nsl; ++k) {
                k0s[0] += lf_sh(p2, k, 0);
                k0s[1] += lf_sh(p2, k, 1);
            }
        }
        f2 q0[RS], g0[RS];
#pragma unroll
        for (int r = 0; r < RS; ++r) {
            q0[r] = q[r];
            g0[r] = g[r];
        }
        const float q0s = sh.q, g0s = sh.g;
        f2 lpn = lp;
        float K0[2] = {0.f, 0.f}, K1[2] = {0.f, 0.f};
        MC_STAMP(5);
        // (the two half kicks of consecutive steps stay separate roundings, as
        // the reference's; their common product h * g is formed once)
        auto drift_private = [&](bool second_half) {
#pragma unroll
            for (int r = 0; r < RS; ++r) {
                const f2 hg = h * g[r];
                f2 pj = p[r];
                if (second_half) pj = pj + hg;  // end of the previous step
                pj = pj + hg;
                p[r] = pj;
                q[r] = q[r] + e * pj;
            }
        };
        float gown = 0.0f;  // the own prior's gradient at sh.v
        auto drift_shared = [&](bool second_half) {
            const float hg = xh * sh.g;
            float pj = sh.p;
            if (second_half) pj = pj + hg;
            pj = pj + hg;
            sh.p = pj;
            sh.q = sh.q + xe * pj;
            sh.v = sh.q;
            if (hxf) sh.v = xf_apply(xxf, sh.q);  // (mx.exp(log_sigma) ...: the terms' value)
            // the shared scale's reciprocals (moment form): hardware v_rcp_f32
            // (<= 1 ulp) instead of the IEEE division — one dependent chain of
            // ~40 VALU on every step's critical path becomes 2; the same bits in
            // every slice, so the replicas stay identical.  Its log (v_log_f32)
            // is taken on the last step only, where log p is formed.
            sh.is = __builtin_amdgcn_rcpf(sh.v);
            sh.iv = sh.is * sh.is;
            gown = vpin(own_grad(sh.v));  // for the step at this position
        };
        drift_private(false);
        drift_shared(false);
        if (xchk && it == cfg.iter_begin) {  // (before the launch's first publish)
            const bool same = xcd_agree(xpoll, xslots, S, ebase + 1, ok);
            // (diagnostic: blocks found on one XCD / not, counted by slice 0,
            // in the status area's words 8 / 9; mc_debug_workspace_xcd)
            if (ok && slice == 0 && wave == 0 && j == 0)  // (one per block)
                __hip_atomic_fetch_add(status + (same ? 8 : 9), 1, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
            if (!ok || !same) {
                // a timeout (1), or a placement the L2-resident stores would
                // not reach (2): nothing published, the block's chains keep
                // their state, the launch reports it (mc_workspace_status)
                __hip_atomic_store(status, ok ? 2 : 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ok = false;
                break;
            }
        }
        // one leapfrog step at the point q(l + 1), compiled per kind so that the
        // intermediate steps carry none of the first / last steps' work (K0 /
        // K1 items, log p) nor its uniform branches and their live masks:
        // 0 first (l = 0 < L - 1), 1 intermediate, 2 last (l = L - 1 > 0),
        // 3 the only step (L = 1).  Returns false on an exchange timeout.
        // ahead: called by a last step between its publish and its poll.
        // PAR: the record lines' parity when the caller knows it (an
        // intermediate step, compiled once per parity: the publish and poll
        // addresses are then fixed registers, no per-step selects), else -1
        auto step = [&](int l, auto kind, auto parc, auto& ahead) -> bool {
            constexpr int KIND = decltype(kind)::value;
            constexpr int PAR = decltype(parc)::value;
            constexpr bool FIRST = KIND == 0 || KIND == 3, LAST = KIND == 2 || KIND == 3;
            (void)l;
            // no vector-memory operation is in flight here (the last poll was
            // waited for): saying so explicitly keeps the compiler's wait-count
            // state clean at the step's entry, where the kinds' paths merge —
            // else it guards the step's first register writes with a
            // vmcnt(0) that also waits for this step's own publish store
            // (not the dense step, which issues no vector-memory operation;
            // the one-wave kernels keep it: without it and the poll's
            // skeleton below the small shape lost 6 %, 949 -> 894 M)
            if constexpr (!DENSE)
                __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) expcnt(7) lgkmcnt(15)
            if constexpr (LAST)  // the shared scales' logs, for log p (log2 v * ln 2)
                sh.lg = __builtin_amdgcn_logf(sh.v) * 0.693147180559945f;
            MC_STAMP(0);
            constexpr bool lst = LAST;  // log p: the last step only
            // finish the swept term from its moment sums, evaluate the direct
            // term (k_hmc_lr's lr_finish; same arithmetic, both chains packed):
            // log p partial (last step), complete private gradients, cotangent
            // partials of the swept scale (cs), the direct loc (cm) and scale (cd)
            // (the first contribution to each sum is assigned, not added to
            // zero: x + 0 is not folded under IEEE signed zeros)
            f2 lpp = {0.f, 0.f}, cs = {0.f, 0.f}, cm = {0.f, 0.f}, cd = {0.f, 0.f};
            bool lpp0 = true, cs0 = true, cm0 = true, cd0 = true;
            bool g0r[RS];
#pragma unroll
            for (int r = 0; r < RS; ++r) {
                g[r] = (f2){0.f, 0.f};
                g0r[r] = true;
            }
            auto acc = [](f2& s, bool& first, f2 v) {
                s = first ? v : s + v;
                first = false;
            };
            // (a shared scale's 1/s^2 is squared here from its 1/s: the
            // holding lane's sh.iv = sh.is * sh.is, the same rounding)
            f2 M2[RS];
            if (SW) {
                const f2 is = SWS ? lf_sh2(sh.is, ksw) : sw_cinv;
                const f2 iv = SWS ? is * is : sw_cinv2;
#pragma unroll
                for (int r = 0; r < RS; ++r) {
                    const bool on = len[r] != 0;
                    const f2 z = {0.f, 0.f};
                    // both moment sums at q[r] from the run's constants (the
                    // drift to the next position follows this finish); an
                    // empty lane's are zeros whatever its position is
                    f2 m1, m2;
                    lf_moments(mom[r], q[r], m1, m2);
                    const f2 M1r = on ? m1 : z;
                    M2[r] = on ? m2 : z;
                    if (RS == 1) {
                        // one slot: an empty lane's moment sums and count are
                        // zeros, so are its gradient and
                        // cotangent; its log p is selected away
                        g[r] = sw_w * (M1r * iv);
                        cs = sw_w * ((M2[r] * iv - cnt[r]) * is);
                        cs0 = g0r[r] = false;
                    } else if (on) {
                        acc(g[r], g0r[r], sw_w * (M1r * iv));
                        acc(cs, cs0, sw_w * ((M2[r] * iv - cnt[r]) * is));
                    }
                    if (lst) {
                        const f2 lg = SWS ? lf_sh2(sh.lg, ksw) : sw_clogs;
                        const f2 lpt = cnt[r] * (sw_c0 - lg) - (half * M2[r]) * iv;
                        if (RS == 1) {
                            lpp = on ? sw_w * lpt : z;
                            lpp0 = false;
                        } else if (on) {
                            acc(lpp, lpp0, sw_w * lpt);
                        }
                    }
                }
            }
            if (DIR) {
                const f2 um = DM ? lf_sh2(sh.v, kdm) : d_m;
                const f2 is = DS ? lf_sh2(sh.is, kds) : d_cinv;
                const f2 iv = DS ? is * is : d_cinv2;
#pragma unroll
                for (int r = 0; r < RS; ++r) {
                    // one slot: a lane without the term weighs it by zero (its
                    // cotangent items 0 * finite, its gradient g - 0) instead
                    // of branching around it under an exec mask
                    if (RS > 1 && !pdir[r]) continue;
                    const f2 dw = RS == 1 ? d_w1 : d_w;
                    const f2 d = q[r] - um;
                    const f2 s2 = d * d;
                    const f2 u = dw * (d * iv);
                    acc(g[r], g0r[r], -u);
                    acc(cm, cm0, u);
                    acc(cd, cd0, dw * ((s2 * iv - one) * is));
                    if (lst) {
                        const f2 lg = DS ? lf_sh2(sh.lg, kds) : d_clogs;
                        const f2 lpt = one * (d_c0 - lg) - (half * s2) * iv;
                        acc(lpp, lpp0, dw * lpt);
                    }
                }
            }
            // a replicated parameter's gradient: the sum of its lanes' partials
            if (rep > 1) {
#pragma unroll
                for (int r = 0; r < RS; ++r) {
                    float a = g[r][0], b = g[r][1];
                    grp_sum2(a, b, rep);
                    g[r] = (f2){a, b};
                }
            }
            // the own prior of this lane's shared parameter (moment form with
            // the constant scale's reciprocals, as the sliced terms); its log p
            // enters slice 0's record
            const float g_own = gown;  // (formed with sh.v, in drift_shared)
            {
                if (lst) {
                    const float v = sh.v;
                    const float d = v - o_m;
                    const bool out = own.hn && !(v >= 0.0f);
                    const float d2 = d * d;
                    const float lpe = out ? -__builtin_inff() : o_c0l - (0.5f * d2) * o_cinv2;
                    const float lp_own = o_wn * lpe;
                    if (own_lp0) lpp[0] += lp_own;
                    if (own_lp1) lpp[1] += lp_own;
                    // the identity terms over the raw parameter (log-Jacobians)
                    if (hxf && slice == 0 && xon) {
                        if (xc == 0) lpp[0] += xid * sh.q;
                        else lpp[1] += xid * sh.q;
                    }
                }
            }
            MC_STAMP(1);
            // wave totals, reduce-scattered: pair P = 2 slot + chain
            float xr[2 * NRS];
            {
                float v[8 * NRS];
#pragma unroll
                for (int x = 0; x < 8 * NRS; ++x) v[x] = 0.0f;
                v[0] = lpp[0];
                v[1] = lpp[1];
                if constexpr (CF) {
                    if (FORM & LF_SWS) {
                        v[2 + 2 * lf_slot_sws(FORM)] = cs[0];
                        v[3 + 2 * lf_slot_sws(FORM)] = cs[1];
                    }
                    if (FORM & LF_DM) {
                        v[2 + 2 * lf_slot_dm(FORM)] = cm[0];
                        v[3 + 2 * lf_slot_dm(FORM)] = cm[1];
                    }
                    if (FORM & LF_DS) {
                        v[2 + 2 * lf_slot_ds(FORM)] = cd[0];
                        v[3 + 2 * lf_slot_ds(FORM)] = cd[1];
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < NSH; ++k)
#pragma unroll
                        for (int c = 0; c < 2; ++c)
                            v[2 + 2 * k + c] = ((F.sw_ks == k ? cs[c] : 0.0f) +
                                                (F.d_km == k ? cm[c] : 0.0f)) +
                                               (F.d_ks == k ? cd[c] : 0.0f);
                }
#pragma unroll
                for (int qq = 0; qq < NRS; ++qq) {
                    float vv[8], xx[2];
#pragma unroll
                    for (int x = 0; x < 8; ++x) vv[x] = v[8 * qq + x];
                    if (qq == 0 && !lst) lf_rs8<true>(vv, xx);  // (no log-p pairs)
                    else lf_rs8(vv, xx);
                    xr[2 * qq] = xx[0];
                    xr[2 * qq + 1] = xx[1];
                }
            }
            // the kinetic partials of the last step (uniform)
            float k1w[2] = {0.f, 0.f};
            if constexpr (LAST) {
                f2 k1p = {0.f, 0.f};
#pragma unroll
                for (int r = 0; r < RS; ++r) {
                    const f2 pj = p[r] + h * g[r];
                    if (lead) k1p += pj * pj;
                }
                k1w[0] = wave_sum(k1p[0]);
                k1w[1] = wave_sum(k1p[1]);
            }
            ++epoch;
            const int par = PAR >= 0 ? PAR : (int)(epoch & 1);
            if constexpr (!X1 && !FIRST && !LAST) {
                // an intermediate step: the record pairs only (addresses and
                // the lane's pair fixed per launch)
                float pv = xr[0];
#pragma unroll
                for (int x = 1; x < 2 * NRS; ++x) pv = (x == pub_x) ? xr[x] : pv;
                if constexpr (DENSE) {
                    if (pub_mid) lput(par, pub_off, pv);
                } else {
                    if (pub_mid) granule_put(gline[par] + pub_off, epoch, pv, XL);
                }
            } else if (!X1) {
                // one store instruction: the record pairs, and the K items on the
                // first / last step (lanes 2, 3 of rows 0 / 1)
                int pp = -1;
                float pv = 0.0f;
                if (pub_rec && (lst || pub_pair >= 2)) {  // (log-p pairs: last step)
                    pp = pub_pair;
                    pv = xr[0];
#pragma unroll
                    for (int x = 1; x < 2 * NRS; ++x)
                        if (x == 2 * (col >> 1) + (col & 1)) pv = xr[x];
                }
                if (col == 2 * NRS || col == 2 * NRS + 1) {
                    const int c = col - 2 * NRS;
                    if (FIRST && row == 0) {
                        pp = NV + c;
                        pv = c ? K0w[1] : K0w[0];
                    }
                    if (LAST && row == 1) {
                        pp = NV + 2 + c;
                        pv = c ? k1w[1] : k1w[0];
                    }
                }
                if constexpr (DENSE) {
                    if (pp >= 0) lput(par, slice * 16 + pp, pv);
                } else {
                    if (pp >= 0) granule_put(gline[par] + slice * 16 + pp, epoch, pv, XL);
                }
            }
            MC_STAMP(2);
            // (a higher wave priority from here to the end of the poll: tuned
            // while a sweep ran here, profiles/r3/ab/ab34, and not measured
            // again since it left on the exchange kernels; the dense step runs
            // without it: Large 318.3 M without against 318.6 with, inside the
            // run-to-run spread, profiles/lf_dense_rng)
            if constexpr (!DENSE) __builtin_amdgcn_s_setprio(1);
            // poll: pass ps reads pair 4 ps + perm[row] of slice col
            constexpr bool kstep = FIRST || LAST;
            const uint32_t need =
                need_v | (FIRST ? need_k0 : 0u) | (LAST ? (need_k1 | need_lp) : 0u);
            float vals[NPASS];
#pragma unroll
            for (int ps = 0; ps < NPASS; ++ps) vals[ps] = 0.0f;
            // every pass's granules loaded at once (one round trip; lanes that
            // need none read an in-bounds line and ignore it); ready when every
            // needed tag is this step's.  A granule of this step is never
            // rewritten before this wave publishes the next one (the line
            // parity alternates per step), so the values of the last load
            // are the record's.
            unsigned long long y[NPASS];
            auto poll_issue = [&]() {
#pragma unroll
                for (int ps = 0; ps < NPASS; ++ps)
                    y[ps] = (ps < NPASS_V || kstep) ? granule_load(gp[par] + 4 * ps) : 0ull;
            };
            // while the records travel: the private parameters' next position
            // (a poll issued before the records have landed costs a second
            // round trip: A/B 83.2 vs 94.7 M steps/s, profiles/r4/ab)
            if constexpr (!LAST) drift_private(true);
            // the last step: the next iteration's draws, while the records travel
            if constexpr (LAST) ahead();
            MC_STAMP(8);
            if (!X1 && !DENSE) poll_issue();
            auto poll_eval = [&]() {
                bool ready = true;  // (bitwise: lane masks, no branches)
#pragma unroll
                for (int ps = 0; ps < NPASS; ++ps) {
                    const bool nd = ((need >> ps) & 1u) != 0u;
                    // a pass this lane does not need stays 0: the 16-lane slice
                    // sums run over every column (S < 16 leaves columns idle)
                    vals[ps] = nd ? __uint_as_float((uint32_t)y[ps]) : 0.0f;
                    ready = ready & (!nd | ((uint32_t)(y[ps] >> 32) == epoch));
                }
                return ready;
            };
            if constexpr (DENSE) {
                // the block's records are in the line after one barrier; a
                // wave writes this parity's line again two steps on, past the
                // next step's barrier, which every wave reaches only after
                // these reads
                __syncthreads();
#pragma unroll
                for (int ps = 0; ps < NPASS; ++ps) {
                    const bool nd = ((need >> ps) & 1u) != 0u;
                    const float v = (ps < NPASS_V || kstep) ? xl[par * (DN * 16) + lpoll + 4 * ps] : 0.0f;
                    vals[ps] = nd ? v : 0.0f;
                }
            }
            // (dense: nothing to wait for, no timeout — none of the poll, its
            // spin counter or the early return is compiled)
            if constexpr (!DENSE) {
                bool ready = X1 ? true : poll_eval();
                MC_STAMP(7);
                uint32_t spins = 0;
                while (__ballot(!ready)) {
                    if (++spins > kSpinLimit) {
                        ok = false;
                        break;
                    }
                    // (no s_sleep between polls: the round trip paces them; A/B
                    // medium 186.0 -> 188.8 M steps/s, large +0.3 %, profiles/r4/ab)
                    poll_issue();
                    ready = poll_eval();
                }
                // (a timeout is reported once, after the trajectory's steps: the
                // store's operands are not reloaded inside the step loop)
                if (__builtin_expect(!ok, 0)) return false;
            } else {
                MC_STAMP(7);
            }
            MC_STAMP(3);
            if constexpr (!DENSE) __builtin_amdgcn_s_setprio(0);
            // slice sums: a fixed 16-lane DPP tree per pass; pair 4 ps + perm[r]
            // in row r of tot[ps]
            float tot[NPASS];
            if constexpr (X1) {
#pragma unroll
                for (int ps = 0; ps < NPASS; ++ps) tot[ps] = ps < 2 * NRS ? xr[ps] : 0.0f;
            } else {
#pragma unroll
                for (int ps = 0; ps < NPASS; ++ps) {
                    float t = vals[ps];
                    if (ps < NPASS_V || kstep) {
                        t += lf_dpp<0xB1>(t);
                        t += lf_dpp<0x4E>(t);
                        t += lf_dpp<0x141>(t);
                        t += lf_dpp<0x140>(t);
                    }
                    tot[ps] = t;
                }
            }
            // totals: the slice sum (the own priors are in slice 0's record)
            if constexpr (LAST) {
                lpn[0] = rl(tot[0], 0) + lp_const;
                lpn[1] = rl(tot[0], 16 * lf_row(1)) + lp_const;
            }
            {
                float gx = 0.0f;
#pragma unroll
                for (int ps = 0; ps < NPASS_V; ++ps)
                    if (col == ps) gx = tot[ps];  // lane 16 row + P / 4 holds pair P
                float gt = gx + g_own;
                // the value's cotangent through the transform's VJP, plus the
                // raw identity terms (eval.h xf_chain: the tape's arithmetic)
                if (hxf) gt = xf_chain(xxf, gt, sh.q, sh.v) + xid;
                sh.g = xon ? gt : 0.0f;
            }
            if constexpr (FIRST) {
                constexpr int p0 = NV, p1 = NV + 1;
                if constexpr (X1) {
                    K0[0] = K0w[0];
                    K0[1] = K0w[1];
                } else {
                    K0[0] = rl(tot[p0 / 4], 16 * lf_row(p0));
                    K0[1] = rl(tot[p1 / 4], 16 * lf_row(p1));
                }
            }
            if constexpr (LAST) {
                constexpr int p0 = NV + 2, p1 = NV + 3;
                if constexpr (X1) {
                    K1[0] = k1w[0];
                    K1[1] = k1w[1];
                } else {
                    K1[0] = rl(tot[p0 / 4], 16 * lf_row(p0));
                    K1[1] = rl(tot[p1 / 4], 16 * lf_row(p1));
                }
            }
            if constexpr (!LAST) drift_shared(true);  // the shared parameters' next position
            MC_STAMP(4);
            return true;
        };
        // (handed to the step, not captured by it: a capture the other
        // instantiations never use still changed their register allocation)
        auto draw_next = [&]() {
            if constexpr (DRAW_AHEAD) {
                if (rngp && it + 1 < it_end) draw_plan(it + 1);
            }
            if constexpr (BDRAW) {
                if (bdraw && it + 1 < it_end) draw_block(it + 1);
            }
        };
        const std::integral_constant<int, -1> rtpar;
        if (L == 1) {
            ok = step(0, std::integral_constant<int, 3>(), rtpar, draw_next);
        } else {
            ok = step(0, std::integral_constant<int, 0>(), rtpar, draw_next);
            const std::integral_constant<int, 1> mid;
            if (X1) {
                for (int l = 1; ok && l < L - 1; ++l) ok = step(l, mid, rtpar, draw_next);
            } else {
                // the intermediate steps, two per loop trip: line parity 0 then
                // parity 1, straight-line, so every loop-carried value is in
                // the same register at the head and at the latch (no dispatch
                // on the parity, no copies between the two bodies' registers).
                // One aligning step first when the tags start on the other
                // parity, one trailing step when the count is odd.
                const std::integral_constant<int, 0> par0;
                const std::integral_constant<int, 1> par1;
                int n = L - 2;
                if (n > 0 && !(epoch & 1)) {  // (the next tag is odd: parity 1)
                    ok = step(1, mid, par1, draw_next);
                    --n;
                }
                for (; __builtin_expect(ok, 1) && n >= 2; n -= 2) {
                    ok = step(1, mid, par0, draw_next);
                    if (__builtin_expect(ok, 1)) ok = step(1, mid, par1, draw_next);
                }
                if (ok && n == 1) ok = step(1, mid, par0, draw_next);
            }
            if (ok) ok = step(L - 1, std::integral_constant<int, 2>(), rtpar, draw_next);
        }
        if (!ok) {  // an exchange timeout in one of the steps
            __hip_atomic_store(status, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
        }
        // ---- accept / adapt (identical in every slice of the block) ------------
        float k1s[2] = {0.f, 0.f};
        {
            const float p1 = sh.p + xh * sh.g;
            const float p2 = p1 * p1;
            for (int k = 0; k < nsl; ++k) {
                k1s[0] += lf_sh(p2, k, 0);
                k1s[1] += lf_sh(p2, k, 1);
            }
        }
        bool acc[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const float H0 = -lp[c] + 0.5f * (K0[c] + k0s[c]);
            const float H1 = -lpn[c] + 0.5f * (K1[c] + k1s[c]);
            const float ratio = -(H1 - H0);
            float logu = logu_acc[c];
            if (!rngp && !bdraw) {
                const mc_u32x4 ru = mc_draw(cfg.seed, (uint32_t)(cfg.chain_offset + cc[c]),
                                            (uint32_t)it, MC_RNG_TAG_ACCEPT, 0, 0);
                logu = mc_logf_u01(mc_u01_f32(ru.x));
            }
            const bool accepted = logu < ratio;
            acc[c] = accepted;
            nacc[c] += accepted ? 1 : 0;
            ntot[c] += 1;
            const double eps_used = eps[c];
            if (warm && cfg.adapt_step_size && it > 10) {
                const double rate = (double)nacc[c] / (double)ntot[c];
                eps[c] = (rate < cfg.target_accept) ? eps_used * 0.95 : eps_used * 1.05;
            }
            if (accepted) lp[c] = lpn[c];
            if (slice == 0 && j == 0 && live[c]) {
                const int64_t ti = it - tr.iter_begin;
                if (ti >= 0 && ti < tr.capacity) {
                    const int64_t o = cc[c] * tr.capacity + ti;
                    if (tr.accepted) tr.accepted[o] = accepted ? 1 : 0;
                    if (tr.accept_stat) tr.accept_stat[o] = ratio;
                    if (tr.step_size) tr.step_size[o] = eps_used;
                    if (tr.energy) tr.energy[o] = H0;
                    if (tr.tree_depth) tr.tree_depth[o] = L;
                    if (tr.n_leapfrog) tr.n_leapfrog[o] = L;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < RS; ++r) {
            q[r] = (f2){acc[0] ? q[r][0] : q0[r][0], acc[1] ? q[r][1] : q0[r][1]};
            g[r] = (f2){acc[0] ? g[r][0] : g0[r][0], acc[1] ? g[r][1] : g0[r][1]};
        }
        if (!(xc ? acc[1] : acc[0])) {
            sh.q = q0s;
            sh.g = g0s;
        }
        if (!warm && samples != nullptr) {
            const int64_t s = it - cfg.num_warmup - cfg.sample_begin;
            if (s >= 0 && s < cfg.sample_capacity) {
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    if (!live[c]) continue;
                    float* out = samples + (cc[c] * cfg.sample_capacity + s) * (int64_t)D;
#pragma unroll
                    for (int r = 0; r < RS; ++r)
                        if (gk[r] >= 0 && lead) out[gk[r]] = q[r][c];
                }
                if (slice == 0 && xlive)
                    samples[(xch_id * cfg.sample_capacity + s) * (int64_t)D + xg] = sh.q;
            }
        }
        MC_STAMP(6);
    }

    // ---- launch epilogue: state back to HBM ---------------------------------------
    MC_STAMP_FLUSH
    if (!ok) return;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        if (!live[c]) continue;
#pragma unroll
        for (int r = 0; r < RS; ++r) {
            if (gk[r] >= 0 && lead) {
                st_q[cc[c] * D + gk[r]] = q[r][c];
                st_g[cc[c] * D + gk[r]] = g[r][c];
            }
        }
        if (slice == 0 && j == 0) {
            mc_chain_scalars& sc = scal[cc[c]];
            sc.logp = lp[c];
            sc.step_size = eps[c];
            sc.n_accept = nacc[c];
            sc.n_total = ntot[c];
            sc.warmup_accept = wacc[c];
            sc.warmup_total = wtot[c];
            sc.n_grad += cfg.iter_count * (int64_t)L;
        }
    }
    if (slice == 0 && xlive) {
        st_q[xch_id * D + xg] = sh.q;
        st_g[xch_id * D + xg] = sh.g;
    }
}

}  // namespace mc
